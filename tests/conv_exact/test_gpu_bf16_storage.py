"""-m gpu: the bf16-STORAGE conv kernels, bit-exact on integer operands (tests/conv_exact/cases.py).

The fp32 accumulator of every kernel holds the exact integer on these cases, so a bf16 output is round_bf16(exact epilogue
value) -- ONE round-to-nearest-even, after bias, mask and addend -- and nothing else: truncation, round-half-away and a
second rounding (after the bias, again after the addend) all show, at a named (b, y, x, c), with the tie flag of the wanted
value.  This is where "a bf16 result is the fp32 result rounded once" of tests/test_gpu_bf16_storage.py is enforced.

  LOANS_F_STATS   WIDE: the sum is the EXACT sum -- in most channels not the sum of the stored bf16 values, which separates
                  "from the fp32 accumulators" from "from the rounded output"; SMALL: the sum of squares is exact too.
  LOANS_F_BNSUMS  the sums of the ROUNDED g (include/loans_hip.h), which differ from those of the exact g.
  bit identity    every tile equals the one reference, so LOANS_TILE_256x256PP16 (44) and the halo tiles with several chunks
                  per tap equal tiles 9 and 1 bit for bit on exact operands -- stronger than "to the position of rare roundings".
  weight gradient fp32, the exact integer plus the integer start value: slabs on and off, every split count.

Cells the dispatch refuses are skipped under the conditions of the family's existing test and no others.
The file's stem is its key in the -m gpu suite order (tests/conftest.py): bf16 kernels, rank 6."""
import pytest
import torch

from tests.conv_exact import cases as X

pytestmark = pytest.mark.gpu

G = X.geometries()
CONV_TILES = (0, 1, 2, 3, 4, 7, 9, 43, 44, 33, 34, 35, 5)          # 5: a weight-gradient tile
WGRAD_TILES = (0, 1, 3, 5, 9)
HALO_TILES = (11, 12, 13, 14, 15, 36, 37, 42)
BNSUMS_TILES = (0, 1, 2, 3, 4, 7, 9, 43, 44, 33, 34, 35, 11, 12, 13, 14, 36, 37, 42)
STATS_RTOL = 1e-4               # tests/test_gpu_bf16_storage.py's bound on the sum of squares


# SLAB_CASES (geometry + tile), then every geometry of it once more with tile 0
SLAB_ENTRIES = list(G['slab16']) + [g + (0,) for g in dict.fromkeys(e[:8] for e in G['slab16'])]


def cells(geoms, tiles):
    return [pytest.param(g, t, id='%s-tile%d' % (X.gid(g), t)) for g in geoms for t in tiles]


@pytest.fixture
def bf16_arm():
    from loans_amd import ops
    old = (ops.COMPUTE, ops.STORAGE)
    ops.set_compute_dtype('bf16')
    ops.set_storage_dtype('bf16')
    yield ops
    ops.set_compute_dtype(old[0])            # ('f32' resets the storage type with it)
    ops.set_storage_dtype(old[1])


@pytest.mark.parametrize("geom,tile", cells(G['conv16'], CONV_TILES))
def test_conv_bf16_storage_exact(geom, tile):
    """test_gpu_bf16_storage.py::test_conv_bf16_storage's calls and every epilogue on WIDE: forward, data gradient, weight gradient"""
    from loans_amd import ops
    c = X.case(geom)
    geo, d = X.geometry(ops, c), X.device(c, True)
    what = 'conv16 %s tile %d' % (X.gid(geom), tile)
    wtile, tile = tile, (tile if tile != 5 else 0)
    X.run_fprop(ops, c, d, geo, tile, what, sumsq_rtol=STATS_RTOL)
    X.run_dgrad(ops, c, d, geo, tile, what, in_place=False)
    if wtile in WGRAD_TILES:
        for splits in (0, 3):
            X.run_wgrad(ops, c, d, geo, wtile, splits, what)
        X.run_wgrad(ops, c, d, geo, wtile, 0, what, relu_in=True)


@pytest.mark.parametrize("geom,tile", cells(G['conv16'], [t for t in CONV_TILES if t != 5]))
def test_conv_bf16_storage_sums_exact(geom, tile):
    from loans_amd import ops
    c = X.case(geom, 'SMALL')
    X.run_fprop_small(ops, c, X.device(c, True), X.geometry(ops, c), tile, 'conv16 SMALL %s tile %d' % (X.gid(geom), tile))


@pytest.mark.parametrize("geom", G['conv16'], ids=X.gid)
def test_pingpong_16x16x32_tile_equals_the_256x256_and_128x128_tiles_bit_for_bit(geom):
    """stated directly, beside following from the reference: on exact operands tile 44 == tile 9 == tile 1, forward and data gradient"""
    from loans_amd import ops
    c = X.case(geom)
    geo, d = X.geometry(ops, c), X.device(c, True)
    outs = [(ops.conv_fprop(d['x'], d['w'], geo, bias=d['bias'], tile=t), ops.conv_dgrad(d['gy'], d['w'], geo, tile=t)) for t in (44, 9, 1)]
    for y, gx in outs[1:]:
        assert torch.equal(outs[0][0], y) and torch.equal(outs[0][1], gx)


@pytest.mark.parametrize("geom,tile", cells(G['halo16'], HALO_TILES))
def test_conv_halo_tiles_exact(geom, tile):
    """LOANS_TILE_HALO_* / WS64 / WSW64 over HALO_CASES with the skips of test_conv_halo_tiles_bf16_storage; the forms with several
    chunks per tap (Cin > 64) equal the implicit-GEMM tile BIT FOR BIT here, like the one-chunk forms"""
    from loans_amd import ops
    B, Cin, H, W, Cout, k, s, p = geom
    if tile in (12, 14, 15, 37) and Cin != 64:
        pytest.skip('one-chunk (Cin = 64) forms')
    if tile in (15, 37) and (Cout > 64 or k != 3):
        pytest.skip('LOANS_TILE_WS64 / LOANS_TILE_WSW64: 3x3, Cin = 64, Cout <= 64')
    c = X.case(geom)
    geo, d = X.geometry(ops, c), X.device(c, True)
    what = 'halo16 %s tile %d' % (X.gid(geom), tile)
    relu_in = tile not in (15, 37)                        # the weight-stationary kernels have no pre-activation form
    X.run_fprop(ops, c, d, geo, tile, what, sumsq_rtol=STATS_RTOL, relu_in=relu_in)
    y = ops.conv_fprop(d['x'], d['w'], geo, bias=d['bias'], tile=tile)
    for t in (1, 9):
        assert torch.equal(y, ops.conv_fprop(d['x'], d['w'], geo, bias=d['bias'], tile=t)), t
    cs = X.case(geom, 'SMALL')
    X.run_fprop_small(ops, cs, X.device(cs, True), geo, tile, what + ' SMALL')
    # data gradient: the gathered tensor is gy (Cout channels), the "output channels" are Cin
    if Cout % 64 or (tile in (12, 14, 15, 37) and Cout != 64):
        return
    X.run_dgrad(ops, c, d, geo, tile, what, in_place=False)
    gx = ops.conv_dgrad(d['gy'], d['w'], geo, tile=tile)
    for t in (1, 9):
        assert torch.equal(gx, ops.conv_dgrad(d['gy'], d['w'], geo, tile=t)), t


@pytest.mark.parametrize("geom", G['pw16'], ids=X.gid)
def test_conv_pointwise_tile_exact(geom):
    """LOANS_TILE_PW: with and without statistics; nothing written past the last pixel"""
    from loans_amd import ops
    for profile in ('WIDE', 'SMALL'):
        c = X.case(geom, profile)
        geo, d = X.geometry(ops, c), X.device(c, True)
        assert ops._pw_tiles(geo, True) == (ops.TILE_PW,) and ops._pw_tiles(geo, False) == ()
        what = 'pw16 %s %s' % (X.gid(geom), profile)
        n = geo.rows * geo.Cout
        sentinel = torch.full((n + 64,), 7.0, device='cuda', dtype=torch.bfloat16)
        st = ops.stats_buffer(geo.Cout, 'cuda')
        y = ops.conv_fprop(d['x'], d['w'], geo, out=sentinel[:n].view(geo.out_shape), stats=st, tile=ops.TILE_PW)
        X.assert_out(c, y, 'plain', what)
        assert bool((sentinel[n:] == 7.0).all())
        X.assert_stats(c, st, what, kind='plain', sumsq_rtol=STATS_RTOL)
        X.assert_out(c, ops.conv_fprop(d['x'], d['w'], geo, tile=ops.TILE_PW), 'plain', what + ' no statistics')


@pytest.mark.parametrize("geom", G['affine16'], ids=X.gid)
def test_bn_relu_on_load_exact(geom):
    """LOANS_F_AFFINE_IN: the operand is round_bf16(relu(x * scale + shift)) with scale in {0.5, 1, 2, -1} and integer shift -- exact
    whether or not the compiler contracts it; the table is written directly.  Forward (LOANS_TILE_PW) with and without
    statistics, weight gradient on every GEMM tile with `in_affine`, splits 0 and 3.  (With these tables the affine value is
    always a bf16 value, cases.affine_case: the operand's rounding on load is in the reference but not exercised here.)"""
    from loans_amd import ops
    base, c, scale, shift = X.affine_case(geom)
    geo = X.geometry(ops, c)
    x, w = X.up(X.nhwc(base.x), True), X.up(X.nhwc(c.w))
    st = X.bn_state(ops, geom[1], 0 * shift, 0 * shift + 1, scale, shift)
    assert ops.affine_in_ok(geo, x)
    what = 'affine16 %s' % X.gid(geom)
    stats = ops.stats_buffer(geo.Cout, 'cuda')
    X.assert_out(c, ops.conv_fprop_affine(x, st, w, geo, stats=stats), 'plain', what)
    X.assert_stats(c, stats, what, kind='plain', sumsq_rtol=STATS_RTOL)
    X.assert_out(c, ops.conv_fprop_affine(x, st, w, geo), 'plain', what + ' no statistics')
    assert c.bound_wgrad() < X.TWO24
    d = dict(x=x, gy=X.up(X.nhwc(c.gy), True), dw0=X.up(X.nhwc(c.dw0)))
    for tile in [1, 3, 5] + ([9] if geo.Cout % 256 == 0 else []):
        for splits in (0, 3):
            X.run_wgrad(ops, c, d, geo, tile, splits, what + ' tile %d' % tile, in_affine=st)


@pytest.mark.parametrize("geom,tile", cells(G['splitk16'], (3 | (2 << 8), 3 | (4 << 8), 2 | (8 << 8))))
def test_conv_split_k_bf16_storage_exact(geom, tile):
    """loans_igemm_bf16s_splitk + loans_igemm_finalize_bf16: raw fp32 partial tiles, ONE rounding in the finalize pass"""
    from loans_amd import ops
    c = X.case(geom)
    geo, d = X.geometry(ops, c), X.device(c, True)
    what = 'splitk16 %s tile %d' % (X.gid(geom), tile)
    X.run_fprop(ops, c, d, geo, tile, what, sumsq_rtol=STATS_RTOL)
    X.run_dgrad(ops, c, d, geo, tile, what, in_place=False)
    cs = X.case(geom, 'SMALL')
    X.run_fprop_small(ops, cs, X.device(cs, True), geo, tile, what + ' SMALL')


@pytest.mark.parametrize("geom", G['stem16'], ids=X.gid)
def test_stem_direct_bf16_exact(geom):
    """LOANS_TILE_STEM on the bf16 MFMA and the implicit-GEMM tile 3: fp32 frames in, bf16 out (loans_igemm_bf16_f32 +
    LOANS_F_OUT_BF16) and bf16 frames (loans_igemm_bf16s) -- one rounding of the exact integer + bias, exact statistics"""
    from loans_amd import ops
    B, Cin, H, W, Cout, k, s, p = geom
    geo = ops.ConvGeometry(B, H, W, 3, Cout, k, s, p, dense=True)
    assert ops.stem16_tile_rows(geo) > 0
    ops.set_compute_dtype('bf16')
    try:
        for profile in ('WIDE', 'SMALL'):
            c = X.case(geom, profile)
            d32 = X.dense_device(ops, c, geo)
            d16 = dict(d32, x=d32['x'].to(torch.bfloat16), w=d32['w'].to(torch.bfloat16))
            for name, d, kw in (('fp32 frames', d32, dict(out_bf16=True)), ('bf16 frames', d16, {})):
                for tile in (ops.TILE_STEM, 3):
                    what = 'stem16 %s %s %s tile %d' % (X.gid(geom), profile, name, tile)
                    st = ops.stats_buffer(Cout, 'cuda')
                    y = ops.conv_fprop(d['x'], d['w'], geo, bias=d['bias'], stats=st, tile=tile, **kw)
                    assert y.dtype == torch.bfloat16
                    X.assert_out(c, y, 'bias', what)
                    X.assert_stats(c, st, what, sumsq_rtol=2e-5)          # test_stem_direct_bf16's bound on the sum of squares
            X.assert_out(c, ops.conv_fprop(d16['x'], d16['w'], geo, tile=ops.TILE_STEM), 'plain', 'stem16 %s no bias' % X.gid(geom))
    finally:
        ops.set_compute_dtype('f32')


@pytest.mark.parametrize("geom,tile", cells(G['pair16'], (0, 1, 2, 3, 7, 9, 43, 44, 33, 35)))
def test_conv_pair_bf16_storage_exact(geom, tile):
    """loans_igemm_pair_bf16s: both outputs one rounding of the integer reference, both statistics exact; with and without statistics"""
    from loans_amd import ops
    for profile in ('WIDE', 'SMALL'):
        a, b = X.pair_cases(geom, profile)
        ga, gb = X.geometry(ops, a), X.geometry(ops, b)
        x, wa, wb = X.up(X.nhwc(a.x), True), X.up(X.nhwc(a.w)), X.up(X.nhwc(b.w))
        assert ops.fprop_pair_ok(x, ga, gb)
        sa, sb = ops.stats_buffer(ga.Cout, 'cuda'), ops.stats_buffer(gb.Cout, 'cuda')
        ya, yb = ops.conv_fprop_pair(x, wa, wb, ga, gb, sa, sb, tile=tile)
        what = 'pair16 %s %s tile %d' % (X.gid(geom), profile, tile)
        X.assert_out(a, ya, 'plain', what + ' first')
        X.assert_out(b, yb, 'plain', what + ' second')
        X.assert_stats(a, sa, what + ' first', kind='plain', sumsq_rtol=STATS_RTOL)
        X.assert_stats(b, sb, what + ' second', kind='plain', sumsq_rtol=STATS_RTOL)
        y2a, y2b = ops.conv_fprop_pair(x, wa, wb, ga, gb, tile=tile)
        assert torch.equal(y2a, ya) and torch.equal(y2b, yb)


@pytest.mark.parametrize("slabs", [True, False], ids=['slabs', 'atomics'])
@pytest.mark.parametrize("splits", [0, 1, 7])
@pytest.mark.parametrize("entry", SLAB_ENTRIES, ids=X.gid)
def test_weight_gradient_exact_slabs_and_atomics(entry, splits, slabs, monkeypatch):
    """_conv_wgrad on the tiles of test_weight_gradient_slabs_are_deterministic_and_equal_the_atomic_form (1, 3, 5, 9, 38, 39) and,
    at each of its geometries, on tile 0 (the fixed pick of the tuner): the workspace slabs with their fold and the atomic form
    give the same integers, into a non-zero dw"""
    from loans_amd import ops
    geom, tile = entry[:8], entry[8]
    c = X.case(geom)
    geo, d = X.geometry(ops, c), X.device(c, True)
    assert ops.WGRAD_SLABS
    monkeypatch.setattr(ops, 'WGRAD_SLABS', slabs)
    X.run_wgrad(ops, c, d, geo, tile, splits, 'slab16 %s tile %d slabs=%d' % (X.gid(geom), tile, slabs))


@pytest.mark.parametrize("geom,tile", cells(G['wghalo16'], (38, 39)))
def test_weight_gradient_halo_tiles_exact(geom, tile):
    """LOANS_TILE_WGHALO_64 / _128 with the skip and the guard of test_weight_gradient_halo_tiles; explicit block counts, relu(x)"""
    from loans_amd import ops
    B, Cin, H, W, Cout = geom[:5]
    if tile == 39 and Cout % 128:
        pytest.skip('128 output channels per block')
    c = X.case(geom)
    geo, d = X.geometry(ops, c), X.device(c, True)
    assert tile in ops.wghalo_tiles(geo) or min(H, W) < 12
    what = 'wghalo16 %s tile %d' % (X.gid(geom), tile)
    for splits in (0, 1, 5):
        X.run_wgrad(ops, c, d, geo, tile, splits, what)
    X.run_wgrad(ops, c, d, geo, tile, 0, what, relu_in=True)


@pytest.mark.parametrize("slabs", [True, False], ids=['slabs', 'atomics'])
@pytest.mark.parametrize("geom", G['stem_wgrad16'], ids=X.gid)
def test_stem_weight_gradient_direct_bf16_exact(geom, slabs, monkeypatch, bf16_arm):
    """LOANS_TILE_STEM of loans_wgrad_bf16s: bf16 frames and a bf16 gradient, accumulating into a non-zero dw whose window-padding
    columns stay as they were; WIDE where its exactness bound holds, SMALL on the 300-image case"""
    ops = bf16_arm
    B, Cin, H, W, Cout, k, s, p = geom
    geo = ops.ConvGeometry(B, H, W, 3, Cout, k, s, p, dense=True)
    assert ops.stem16_wgrad_ok(geo)
    c = X.case(geom, X.wgrad_profile(geom))
    d = X.dense_device(ops, c, geo, bf16_frames=True)
    gy = X.up(X.nhwc(c.gy), True)
    monkeypatch.setattr(ops, 'WGRAD_SLABS', slabs)
    what = 'stem_wgrad16 %s slabs=%d' % (X.gid(geom), slabs)
    dw = d['dw0'].clone()
    dw[:, :, k:] = 77.0
    ops._conv_wgrad(d['x'], gy, dw, geo, False, 0, ops.TILE_STEM)
    X.assert_dense_dw(c, dw, c.gw() + c.dw0, what, pad_want=77.0)


@pytest.mark.parametrize("geom,tile", cells(G['bnsums'], BNSUMS_TILES))
def test_data_gradient_bn_sums_bf16_exact(geom, tile, bf16_arm):
    """LOANS_F_BNSUMS on bf16 tensors, the cells of test_data_gradient_takes_the_bn_backward_sums (its two skip conditions): the sums
    are those of the ROUNDED g -- on WIDE they differ from the sums of the exact g in most channels"""
    ops = bf16_arm
    c = X.case(geom)
    geo = X.geometry(ops, c)
    if tile in (11, 12, 13, 14, 36, 37, 42) and tile not in ops._halo_tiles(geo, geo.Cout, geo.Cin, (geo.H, geo.W)):
        pytest.skip('the halo tile does not cover this geometry')
    if tile in (9, 43, 44) and geom[1] % 256:
        pytest.skip('256 columns per block')
    X.run_bn_sums(ops, c, X.device(c, True), geo, tile, 'bnsums16 %s tile %d' % (X.gid(geom), tile))
