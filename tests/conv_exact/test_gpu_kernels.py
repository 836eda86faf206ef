"""-m gpu: the fp32 conv kernels, bit-exact on integer operands (tests/conv_exact/cases.py), through
loans_amd.ops on every tile.  Every product and every partial sum of these cases is an integer below 2^24 in any order, so the
output of every tile, split-K slice count, fine-tail plan, class launch and position-major tile IS the float64 reference:
the comparison is torch.equal by value, no tolerance.  A lost, doubled or misplaced product, a border tap read one pixel
off, an epilogue applied in another order shows as a mismatch at a named (b, y, x, c).

Profiles: WIDE for the integer outputs and the exact sums of LOANS_F_STATS, SMALL for the exact sums of squares.  Cells are
(geometry, tile); references are made once per geometry.  Cells the dispatch refuses are handled as the existing test of the
family handles them.

The file's stem is its key in the -m gpu suite order (tests/conftest.py): fp32 kernels against the oracle, rank 1."""
import pytest
import torch

from tests.conv_exact import cases as X

pytestmark = pytest.mark.gpu

G = X.geometries()
CONV_TILES = (0, 1, 2, 3, 4, 5, 6, 17, 18, 19, 20, 22)         # 5: a weight-gradient tile; + 16 = LOANS_TILE_DMA
DGRAD_TILES = (0, 1, 2, 3, 4, 6, 17, 18, 19, 20, 22)
CLASS_TILES = (1, 2, 3, 4, 17, 18, 19, 20)
WGRAD_TILES = (0, 1, 3, 5)
BNSUMS_TILES = (0, 1, 2, 3, 4, 6, 17, 18, 19, 20)


def cells(geoms, tiles):
    return [pytest.param(g, t, id='%s-tile%d' % (X.gid(g), t)) for g in geoms for t in tiles]


def pad4(cin):
    return (cin + 3) // 4 * 4


@pytest.mark.parametrize("geom,tile", cells(G['conv32'], CONV_TILES))
def test_conv_fprop_dgrad_wgrad_exact(geom, tile):
    """test_gpu_kernels.py::test_conv_fprop_dgrad_wgrad's calls, every epilogue, plus the class launch of the strided data
    gradients, on WIDE: each output equals the integer reference"""
    from loans_amd import ops
    c = X.case(geom)
    cp = pad4(geom[1])
    geo, d = X.geometry(ops, c, cp), X.device(c, False, cp)
    what = 'conv32 %s tile %d' % (X.gid(geom), tile)
    X.run_fprop(ops, c, d, geo, tile if tile != 5 else 0, what)
    if tile in DGRAD_TILES:
        X.run_dgrad(ops, c, d, geo, tile, what)
    if tile in CLASS_TILES and geom[6] > 1 and len(geo.dgrad) <= 4:         # LOANS_MAX_CLASSES
        X.run_dgrad(ops, c, d, geo, tile | ops.TILE_CLASSES, what + ' class launch')
    if tile in WGRAD_TILES:
        for splits in (0, 3):
            X.run_wgrad(ops, c, d, geo, tile, splits, what, direct=False)
        X.run_wgrad(ops, c, d, geo, tile, 0, what, relu_in=True, direct=False)


@pytest.mark.parametrize("geom,tile", cells(G['conv32'], [t for t in CONV_TILES if t != 5]))
def test_conv_fprop_sums_of_squares_exact(geom, tile):
    from loans_amd import ops
    c = X.case(geom, 'SMALL')
    cp = pad4(geom[1])
    X.run_fprop_small(ops, c, X.device(c, False, cp), X.geometry(ops, c, cp), tile, 'conv32 SMALL %s tile %d' % (X.gid(geom), tile))


@pytest.mark.parametrize("geom,tile", cells(G['bnsums'], BNSUMS_TILES))
def test_data_gradient_bn_sums_exact(geom, tile):
    """LOANS_F_BNSUMS on fp32 tensors: the two sums of the BN backward are integer sums of the stored gradient"""
    from loans_amd import ops
    c = X.case(geom)
    X.run_bn_sums(ops, c, X.device(c, False), X.geometry(ops, c), tile, 'bnsums32 %s tile %d' % (X.gid(geom), tile))


@pytest.mark.parametrize("geom,splits", [pytest.param(g, s, id='%s-splits%d' % (X.gid(g), s)) for g in G['splitk32'] for s in (2, 4, 16)])
def test_conv_split_k_exact(geom, splits):
    """LOANS_TILE_SPLITK + loans_igemm_finalize_f32: atomic sums of exact integers in any order; the finalize pass's bias /
    statistics / mask / addend, the aliased addend and the in-place accumulation of test_conv_split_k"""
    from loans_amd import ops
    c = X.case(geom)
    geo, d = X.geometry(ops, c), X.device(c, False)
    tile = 3 | (splits << 8)
    what = 'splitk32 %s splits %d' % (X.gid(geom), splits)
    X.run_fprop(ops, c, d, geo, tile, what)
    acc = d['add_y'].clone()
    ops.conv_fprop(d['x'], d['w'], geo, out=acc, relu_in=True, addend=acc, tile=tile)          # in place: out = conv(relu(x)) + out
    X.assert_out(c, acc, 'relu_add', what + ' in place')
    X.run_dgrad(ops, c, d, geo, tile, what)
    cs = X.case(geom, 'SMALL')
    X.run_fprop_small(ops, cs, X.device(cs, False), geo, tile, what + ' SMALL')


@pytest.mark.parametrize("dma", [0, 16])
def test_conv_fine_tail_exact(dma):
    """LOANS_TILE_FINETAIL at test_conv_tap_loop_fine_tail's geometry, with that test's assertion that the sliced path is taken"""
    from loans_amd import ops
    geom = G['finetail32'][0]
    B, Cin, H, W, Cout, k, s, p = geom
    rows_head, slices = ops._finetail_plan(B * H * W, Cout, k * k * Cin // 32, torch.device('cuda', 0))
    assert 0 < rows_head < B * H * W and slices >= 2, 'the case must take the sliced path on this machine'
    tile = ops.TILE_FINETAIL | dma
    for profile in ('WIDE', 'SMALL'):
        c = X.case(geom, profile)
        geo, d = X.geometry(ops, c), X.device(c, False)
        st = ops.stats_buffer(Cout, 'cuda')
        what = 'finetail32 %s tile %d' % (profile, tile)
        X.assert_out(c, ops.conv_fprop(d['x'], d['w'], geo, bias=d['bias'], stats=st, tile=tile), 'bias', what)
        X.assert_stats(c, st, what)
        X.assert_out(c, ops.conv_fprop(d['x'], d['w'], geo, bias=d['bias'], relu_in=True, tile=tile), 'relu_bias', what)


@pytest.mark.parametrize("name,tile", [pytest.param(n, t, id='%s-tile%d' % (n, t)) for n in X.posmajor_cases() for t in (3 | 128, 19 | 128)])
def test_conv_posmajor_exact(name, tile):
    """LOANS_TILE_POSMAJOR at the posmajor package's geometries, each with the flags its case names: a tile that leaves the taps
    outside the frame out of its K loop gives the same integers (the sign of an exact zero may differ: compared by value)"""
    from loans_amd import ops
    geom, direction, flags = X.posmajor_cases()[name][:8], X.posmajor_cases()[name][8], X.posmajor_cases()[name][9]
    c = X.case(geom)
    geo, d = X.geometry(ops, c), X.device(c, False)
    assert ops.posmajor_ok(geo.fwd if direction == 'fwd' else geo.dgrad[0][0], geom[0]), name
    what = 'posmajor32 %s tile %d' % (name, tile)
    if direction == 'fwd':
        X.run_fprop(ops, c, d, geo, tile, what)
        X.assert_out(c, ops.conv_fprop(d['x'], d['w'], geo, relu_in=True, tile=tile), 'relu', what)
        cs = X.case(geom, 'SMALL')
        X.run_fprop_small(ops, cs, X.device(cs, False), geo, tile, what + ' SMALL')
    elif 'BNSUMS' in flags:
        X.run_bn_sums(ops, c, d, geo, tile, what)
    else:
        X.run_dgrad(ops, c, d, geo, tile, what)


@pytest.mark.parametrize("geom,tile", cells(G['pair32'], (0, 1, 2, 3, 4, 17, 18, 19)))
def test_conv_fprop_pair_exact(geom, tile):
    """loans_igemm_pair_f32: both outputs and both statistics are the integer references"""
    from loans_amd import ops
    for profile in ('WIDE', 'SMALL'):
        a, b = X.pair_cases(geom, profile)
        ga, gb = X.geometry(ops, a), X.geometry(ops, b)
        x, wa, wb = X.up(X.nhwc(a.x)), X.up(X.nhwc(a.w)), X.up(X.nhwc(b.w))
        assert ops.fprop_pair_ok(x, ga, gb)
        sa, sb = ops.stats_buffer(ga.Cout, 'cuda'), ops.stats_buffer(gb.Cout, 'cuda')
        ya, yb = ops.conv_fprop_pair(x, wa, wb, ga, gb, sa, sb, tile=tile)
        what = 'pair32 %s %s tile %d' % (X.gid(geom), profile, tile)
        X.assert_out(a, ya, 'plain', what + ' first')
        X.assert_out(b, yb, 'plain', what + ' second')
        X.assert_stats(a, sa, what + ' first', kind='plain')
        X.assert_stats(b, sb, what + ' second', kind='plain')


@pytest.mark.parametrize("geom,tile", cells(G['dense32'], (0, 1, 2, 3, 4, 5, 17, 18, 19, 20)))
def test_conv_dense_rows_exact(geom, tile):
    """LOANS_F_DENSE: the RGB stem on packed rows of a zero-padded frame, forward with bias and statistics and the weight gradient"""
    from loans_amd import ops
    B, Cin, H, W, Cout, k, s, p = geom
    geo = ops.ConvGeometry(B, H, W, 3, Cout, k, s, p, dense=True)
    what = 'dense32 %s tile %d' % (X.gid(geom), tile)
    for profile in ('WIDE', 'SMALL'):
        c = X.case(geom, profile)
        d = X.dense_device(ops, c, geo)
        st = ops.stats_buffer(Cout, 'cuda')
        X.assert_out(c, ops.conv_fprop(d['x'], d['w'], geo, bias=d['bias'], stats=st, tile=tile if tile != 5 else 0), 'bias', what)
        X.assert_stats(c, st, what + ' ' + profile)
    if tile in WGRAD_TILES:
        c = X.case(geom)
        d = X.dense_device(ops, c, geo)
        gy = X.up(X.nhwc(c.gy))
        for splits in (0, 3):
            dw = d['dw0'].clone()
            ops.conv_wgrad(d['x'], gy, dw, geo, splits=splits, tile=tile)
            ops.join_side_stream()
            X.assert_dense_dw(c, dw, c.gw() + c.dw0, what + ' wgrad splits %d' % splits)


@pytest.mark.parametrize("geom", G['stem32'], ids=X.gid)
def test_conv_stem_direct_exact(geom):
    """LOANS_TILE_STEM (csrc/stem.hip): conv1 as a direct convolution, with bias and statistics and without"""
    from loans_amd import ops
    B, Cin, H, W, Cout, k, s, p = geom
    geo = ops.ConvGeometry(B, H, W, 3, Cout, k, s, p, dense=True)
    assert ops.stem_tile_rows(geo) > 0
    for profile in ('WIDE', 'SMALL'):
        c = X.case(geom, profile)
        d = X.dense_device(ops, c, geo)
        what = 'stem32 %s %s' % (X.gid(geom), profile)
        st = ops.stats_buffer(Cout, 'cuda')
        X.assert_out(c, ops.conv_fprop(d['x'], d['w'], geo, bias=d['bias'], stats=st, tile=ops.TILE_STEM), 'bias', what)
        X.assert_stats(c, st, what)
        X.assert_out(c, ops.conv_fprop(d['x'], d['w'], geo, tile=ops.TILE_STEM), 'plain', what + ' no bias')


@pytest.mark.parametrize("geom", G['stem_wgrad32'], ids=X.gid)
def test_stem_wgrad_direct_exact(geom):
    """LOANS_TILE_STEM of loans_wgrad_f32: accumulates into a non-zero dw, leaves the window-padding columns untouched"""
    from loans_amd import ops
    B, Cin, H, W, Cout, k, s, p = geom
    geo = ops.ConvGeometry(B, H, W, 3, Cout, k, s, p, dense=True)
    assert ops.stem_wgrad_ok(geo)
    c = X.case(geom, X.wgrad_profile(geom))
    d = X.dense_device(ops, c, geo)
    gy = X.up(X.nhwc(c.gy))
    dw = d['dw0'].clone()
    dw[:, :, k:] = 77.0
    ops._conv_wgrad(d['x'], gy, dw, geo, False, 0, ops.TILE_STEM)
    X.assert_dense_dw(c, dw, c.gw() + c.dw0, 'stem_wgrad32 %s' % X.gid(geom), pad_want=77.0)


@pytest.mark.parametrize("geom,splits", [pytest.param(g, s, id='%s-splits%d' % (X.gid(g), s)) for g in G['wghalo32'] for s in (0, 1, 2, 3, 64)])
def test_wgrad_halo_f32_exact(geom, splits):
    """LOANS_TILE_WGHALO_64 of loans_wgrad_f32 (csrc/wgrad_halo_f32.hip) at its package's geometries and block counts"""
    from loans_amd import ops
    c = X.case(geom)
    geo, d = X.geometry(ops, c), X.device(c, False)
    assert ops.TILE_WGHALO_64 in ops.wghalo_tiles(geo, True)
    what = 'wghalo32 %s' % X.gid(geom)
    X.run_wgrad(ops, c, d, geo, ops.TILE_WGHALO_64, splits, what)
    X.run_wgrad(ops, c, d, geo, ops.TILE_WGHALO_64, splits, what, relu_in=True)


@pytest.mark.parametrize("shape", G['crop32'], ids=X.gid)
@pytest.mark.parametrize("g16", [False, True])
def test_crop_dgrad_exact(shape, g16):
    """loans_crop_dgrad: the gradient w.r.t. the 4-channel crops through the 3x3 / 1 and the 4x4 / 2 convolution in one launch;
    fp32 output from fp32 or bf16 gradient tensors (integer weights are their own bf16 roundings)"""
    from loans_amd import ops
    a, b = X.family_cases('crop32', shape, 'WIDE')
    ga, gb = X.geometry(ops, a, 4), X.geometry(ops, b, 4)
    assert ops.crop_dgrad_ok(ga, gb)
    cast = (lambda t: t.to(torch.bfloat16)) if g16 else (lambda t: t)
    gya, gyb = cast(X.up(X.nhwc(a.gy))), cast(X.up(X.nhwc(b.gy)))
    wa, wb = X.up(X.nhwc(a.w, 4)), X.up(X.nhwc(b.w, 4))
    out = ops.crop_dgrad(gya, wa, ga, gyb, wb, gb)
    assert out.dtype == torch.float32 and not out[..., 3].any()
    what = 'crop32 %s g16=%d' % (X.gid(shape), g16)
    X.assert_same(out, a.gx() + b.gx(), what, channels=3)
    one = ops.crop_dgrad(gyb, wb, gb, addend=X.up(X.nhwc(b.add_x, 4)))
    X.assert_same(one, b.exact('gx_add'), what + ' single + addend', channels=3)


@pytest.mark.parametrize("geom,tile", cells(G['compute16'], (0, 1, 2, 3, 4)))
def test_conv_bf16_compute_round_in_exact(geom, tile):
    """The bf16-COMPUTE arm on fp32 tensors: operands rounded to bf16 (RNE) while staged.  ROUND_IN: |x| in [256, 1024), where
    bf16 holds every second / fourth integer, so the operand rounding itself -- ties included -- decides every product; the
    reference contracts round_bf16(x) and round_bf16(w)."""
    from loans_amd import ops
    c = X.case(geom, 'WIDE', round_in=True)
    B, Cin, H, W, Cout, k, s, p = geom
    cp = pad4(Cin)
    geo = X.geometry(ops, c, cp)
    x, w = X.up(X.nhwc(c.x_raw, cp)), X.up(X.nhwc(c.w, cp))
    what = 'compute16 %s tile %d' % (X.gid(geom), tile)
    ops.set_compute_dtype('bf16')
    try:
        st = ops.stats_buffer(Cout, 'cuda')
        X.assert_out(c, ops.conv_fprop(x, w, geo, stats=st, tile=tile), 'plain', what)
        X.assert_stats(c, st, what, kind='plain', sumsq_rtol=1e-4)
        if Cin >= 32:
            gx = ops.conv_dgrad(X.up(X.nhwc(c.gy_raw)), w, geo, tile=tile)
            X.assert_same(gx, c.gx(gy=X.O.round_bf16(c.gy_raw)), what + ' dgrad', channels=Cin)
        if tile in (0, 1, 3):
            dw = X.up(X.nhwc(c.dw0, cp))
            ops._conv_wgrad(x, X.up(X.nhwc(c.gy)), dw, geo, False, 0, tile)
            X.assert_same(dw, c.gw() + c.dw0, what + ' wgrad', channels=Cin)
    finally:
        ops.set_compute_dtype('f32')
