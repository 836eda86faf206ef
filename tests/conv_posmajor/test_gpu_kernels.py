"""-m gpu: the image-strided row tiles of the fp32 implicit-GEMM kernel (LOANS_TILE_POSMAJOR = 128 OR-ed onto the 64x64 tile, register-
staged and LDS-DMA: ids 131 and 147 of loans_igemm_f32) against the plain tiles 3 and 19 on the same operands, straight through the C ABI.

Such a tile holds one grid position of 64 consecutive images and leaves the taps outside the frame out of its K loop: the plain
tile's sums in the plain tile's order minus products with a gathered zero, so for the finite operands used here the outputs are
EQUAL (np.array_equal; the sign of an exact zero may differ).  LOANS_F_STATS / LOANS_F_BNSUMS sum a tile's rows in fp32 before their
fp64 atomics, another row grouping moves those by a rounding: 1e-5 relative L2, the bound tests/test_gpu_tune_tables.py sets between
any two tiles.

The smallest shapes that can go wrong: frames 1 x 1 (eight of nine taps left out), 2 x 2 (every position a corner), 3 x 3, 4 x 5,
7 x 7; 64, 65 (a second image group with one real row) and 130 images; Cin 32 (a tap change behind every chunk) and 64; Cout 64 and
96 (a ragged column tile); a 3 x 3 / 2 forward and a 1 x 1 / pad 1 convolution (positions with no tap inside).

The file's stem is its key in the -m gpu suite order (tests/conftest.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PM = 128                          # LOANS_TILE_POSMAJOR
PAIRS = ((3, 3 | PM), (19, 19 | PM))
LOANS_EINVAL = -1

CASES = {
    # name: (B, Cin, H, W, Cout, k, stride, pad, direction, flags)
    'f_1x1_stats':   (64, 32, 1, 1, 64, 3, 1, 1, 'fwd', ('STATS', 'BIAS')),
    'f_2x2_stats':   (65, 64, 2, 2, 96, 3, 1, 1, 'fwd', ('STATS', 'BIAS')),
    'f_3x3_stats':   (130, 32, 3, 3, 96, 3, 1, 1, 'fwd', ('STATS', 'BIAS')),
    'f_4x5_stats':   (65, 32, 4, 5, 64, 3, 1, 1, 'fwd', ('STATS', 'BIAS')),
    'f_7x7_stats':   (130, 64, 7, 7, 96, 3, 1, 1, 'fwd', ('STATS', 'BIAS')),
    'f_3x3_relu':    (65, 32, 3, 3, 96, 3, 1, 1, 'fwd', ('RELU_IN',)),
    'f_7x7_relu':    (64, 64, 7, 7, 64, 3, 1, 1, 'fwd', ('RELU_IN',)),
    'f_s2':          (65, 32, 7, 7, 64, 3, 2, 1, 'fwd', ('STATS',)),
    'f_k1p1':        (65, 32, 3, 3, 64, 1, 1, 1, 'fwd', ('BIAS',)),
    'd_1x1_mask':    (65, 32, 1, 1, 64, 3, 1, 1, 'dgrad', ('MASK', 'ADDEND')),
    'd_2x2_mask':    (130, 96, 2, 2, 32, 3, 1, 1, 'dgrad', ('MASK', 'ADDEND')),
    'd_4x5_mask':    (64, 64, 4, 5, 64, 3, 1, 1, 'dgrad', ('MASK', 'ADDEND')),
    'd_3x3_addmask': (65, 96, 3, 3, 64, 3, 1, 1, 'dgrad', ('ADDEND', 'ADDEND_MASK')),
    'd_7x7_addmask': (130, 64, 7, 7, 32, 3, 1, 1, 'dgrad', ('ADDEND', 'ADDEND_MASK')),
    'd_3x3_bnsums':  (130, 96, 3, 3, 32, 3, 1, 1, 'dgrad', ('BNSUMS',)),
    'd_7x7_bnsums':  (65, 64, 7, 7, 64, 3, 1, 1, 'dgrad', ('BNSUMS',)),
}
# (forward: the gathered tensor has Cin channels and the output Cout; data gradient: the gradient with Cout channels is gathered --
# Cout is 32 or 64 there -- and the output has Cin of them, 64 or 96)

_cache = {}


def _l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / (b.norm() + 1e-300))


def _case(name):
    """descriptor and seeded operands of one case, made once"""
    if name in _cache:
        return _cache[name]
    from loans_amd import _lib, ops
    B, Cin, H, W, Cout, k, s, p, direction, fl = CASES[name]
    geo = ops.ConvGeometry(B, H, W, Cin, Cout, k, s, p)
    d = _lib.IgemmDesc()
    C.memmove(C.byref(d), C.byref(geo.fwd if direction == 'fwd' else geo.dgrad[0][0]), C.sizeof(d))
    flags = 0
    for f in fl:
        flags |= getattr(_lib, 'F_' + f)
    gen = torch.Generator(device='cuda').manual_seed(3000 + sorted(CASES).index(name))
    rnd = lambda *sh: torch.randn(*sh, device='cuda', generator=gen)       # noqa: E731
    t = {'in': rnd(d.B, d.inH, d.inW, d.Cin), 'w': rnd(d.Cout, d.ntaps, d.Cin) * 0.1}
    oshape = (d.B, d.outH, d.outW, d.Cout)
    if 'BIAS' in fl:
        t['bias'] = rnd(d.Cout)
    if 'BNSUMS' in fl:
        t['bias'] = rnd(4, d.Cout)                    # the BN's [mean | rstd | scale | shift]
        t['ref'] = rnd(*oshape)
    if 'MASK' in fl or 'ADDEND_MASK' in fl:
        t['ref'] = rnd(*oshape)
    if 'ADDEND' in fl:
        t['addend'] = rnd(*oshape)
    _cache[name] = (d, flags, oshape, t)
    return _cache[name]


def _launch(d, flags, tile, t, out, stats):
    from loans_amd import _lib, ops
    d.flags, d.tile = flags, tile
    ptr = lambda k: t[k].data_ptr() if k in t else 0      # noqa: E731
    rc = _lib.load().loans_igemm_f32(ptr('in'), ptr('w'), out.data_ptr(), ptr('bias'), stats.data_ptr() if stats is not None else 0,
                                     ptr('ref'), ptr('addend'), C.byref(d), ops._stream())
    torch.cuda.synchronize()
    return rc


def _run(name, tile):
    from loans_amd import _lib, ops
    d, flags, oshape, t = _case(name)
    out = torch.full(oshape, 12345.5, device='cuda')
    stats = ops.stats_buffer(d.Cout, 'cuda') if flags & (_lib.F_STATS | _lib.F_BNSUMS) else None
    assert _launch(d, flags, tile, t, out, stats) == 0, (name, tile)
    return out, stats


@pytest.mark.parametrize("name", list(CASES))
def test_posmajor_equals_the_plain_tile(name):
    for plain, pm in PAIRS:
        want, wstats = _run(name, plain)
        got, gstats = _run(name, pm)
        assert not bool((want == 12345.5).any()), 'the plain tile writes every output element'
        assert np.array_equal(got.cpu().numpy(), want.cpu().numpy()), (name, pm, float((got - want).abs().max()))
        if wstats is not None:
            err = _l2(gstats.sum(0), wstats.sum(0))
            print('%s tile %d: statistics rel L2 %.3g' % (name, pm, err))
            assert err < 1e-5, (name, pm, err)


REFUSED = {
    # name: (B, Cin, H, W, Cout, what)
    'b63':     (63, 32, 3, 3, 64, 'plain'),
    'cin48':   (64, 48, 3, 3, 64, 'plain'),
    'dense':   (64, 32, 3, 3, 64, 'dense'),
    'splitk':  (64, 32, 3, 3, 64, 'splitk'),
    'pair':    (64, 32, 3, 3, 64, 'pair'),
}


@pytest.mark.parametrize("name", list(REFUSED))
def test_posmajor_refusals(name):
    """argument checks on the host side of the launcher: LOANS_EINVAL, no kernel runs, a poisoned output stays as it was"""
    from loans_amd import _lib, ops
    B, Cin, H, W, Cout, what = REFUSED[name]
    geo = ops.ConvGeometry(B, H, W, Cin, Cout, 3, 1, 1)
    d = _lib.IgemmDesc()
    C.memmove(C.byref(d), C.byref(geo.fwd), C.sizeof(d))
    gen = torch.Generator(device='cuda').manual_seed(17)
    # (dense: inW counts floats of rows the caller padded; a frame wide enough for every window, so that only the tile is refused)
    x = torch.randn(B, H + 2, (W + 2) * Cin, device='cuda', generator=gen)
    w = torch.randn(Cout, 9, Cin, device='cuda', generator=gen)
    w2 = torch.randn(Cout, 9, Cin, device='cuda', generator=gen)
    poison = torch.full((B, H, W, Cout), 12345.5, device='cuda')
    for pm in (3 | PM, 19 | PM):
        out, out2 = poison.clone(), poison.clone()
        d.flags, d.tile = 0, pm
        if what == 'dense':
            d.flags = _lib.F_DENSE
            d.inH, d.inW, d.isx = H + 2, (W + 2) * Cin, Cin
            for t in range(9):
                d.dy[t], d.dx[t] = t // 3, (t % 3) * Cin
        if what == 'splitk':
            d.tile = pm | (2 << 8)
        lib = _lib.load()
        if what == 'pair':
            rc = lib.loans_igemm_pair_f32(x.data_ptr(), w.data_ptr(), out.data_ptr(), 0, w2.data_ptr(), out2.data_ptr(), 0, Cout,
                                          C.byref(d), ops._stream())
        else:
            rc = lib.loans_igemm_f32(x.data_ptr(), w.data_ptr(), out.data_ptr(), 0, 0, 0, 0, C.byref(d), ops._stream())
        torch.cuda.synchronize()
        assert rc == LOANS_EINVAL, (name, pm, rc)
        assert torch.equal(out, poison) and torch.equal(out2, poison)
        if what in ('dense', 'splitk', 'pair'):       # the plain tile takes the same call: the refusal is the tile's
            d.tile = (pm & ~PM) | (d.tile & ~0xFF)
            if what == 'pair':
                rc = lib.loans_igemm_pair_f32(x.data_ptr(), w.data_ptr(), out.data_ptr(), 0, w2.data_ptr(), out2.data_ptr(), 0, Cout,
                                              C.byref(d), ops._stream())
            else:
                rc = lib.loans_igemm_f32(x.data_ptr(), w.data_ptr(), out.data_ptr(), 0, 0, 0, 0, C.byref(d), ops._stream())
            torch.cuda.synchronize()
            assert rc == 0, (name, d.tile, rc)


def test_posmajor_python_rule_mirror():
    """ops.posmajor_ok agrees with the library on the shapes above (the tuner offers a tile only where the launcher takes it)"""
    from loans_amd import ops
    for name in CASES:
        d = _case(name)[0]
        assert ops.posmajor_ok(d, d.B), name
    for name, (B, Cin, H, W, Cout, what) in REFUSED.items():
        if what == 'plain':
            assert not ops.posmajor_ok(ops.ConvGeometry(B, H, W, Cin, Cout, 3, 1, 1).fwd, B), name
    g = ops.ConvGeometry(64, 3, 3, 32, 64, 3, 1, 1)
    assert not ops.posmajor_ok(g.fwd, 64, dense=True)
