"""-m gpu: the operand loaders of the fp32 implicit-GEMM kernel (csrc/igemm.hip, igemm_kernel) on the smallest
geometries at which their offsets can go wrong -- forward and data gradient with an explicit tile.

With Cin % 32 == 0 (and no LOANS_F_DENSE) a 32-deep K chunk lies inside one tap, and the kernel takes its per-tap loader:
the per-lane A offsets (row base + tap, or the all-ones mask where the tap leaves the image) are made once per tap, the
B offsets once per launch, and the walk along K is a wave-uniform byte count in the buffer loads' scalar offset.  What
can go wrong: a masked lane that reads data once the scalar offset is non-zero, a tap change one chunk early or late, a
K slice (split-K, fine tail) that starts in the middle of a tap, the tap order of a stride-parity class, tile rows
behind the last image and tile columns behind Cout.  The cases: one, two, three (Cin = 96: no power of two) and four
chunks per tap, 3 x 3 borders on images smaller than a tile, the assessor's 4 x 4 / 2 with 16 taps, 3 x 3 / 2 on an odd
input (data gradient per class and as one class launch, 1 / 2 / 2 / 4 taps), a 1 x 1 with 16 chunks and no tap change,
Cout = 32, relu(in), a pair launch, split-K and the fine-tail tile; Cin = 4 / 16 / 48 stay on the general loader.  Every
case on the 128x128, 128x64, 64x64 and 256x64 tiles, register-staged and with LOANS_TILE_DMA.

Bounds: every case against the fp64 oracle with the 2e-6 of test_gpu_kernels.py::test_conv_fprop_dgrad_wgrad for the
same call; the deterministic launches (one K slice, no fine tail, no statistics) additionally bit for bit against
tests/golden/conv_f32_tap_loop_bits.npz, which tests/golden/make_conv_tap_loop_golden.py recorded with the kernel as it
was before the per-tap loader.  Every tile shape contracts K in the same order, so the file holds one array per case and
launch kind, and an array per tile only where the recording kernel's tiles disagreed.

The file's stem is its key in the -m gpu suite order (tests/conftest.py): fp32 kernel tests against the oracle, rank 1."""
import os

import numpy as np
import pytest
import torch

from oracle import chainer_ops as O
from tests.gpu_util import dev, rel_err

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'golden', 'conv_f32_tap_loop_bits.npz')

GEOMS = {
    # name: B, Cin, H, W, Cout, k, stride, pad
    'c32_5':  (3, 32, 5, 5, 64, 3, 1, 1),      # M 75: one chunk per tap (a tap change every chunk), a border on every tap
    'c32_7':  (3, 32, 7, 7, 64, 3, 1, 1),      # M 147: tiles span images, ragged last tile
    'c64':    (3, 64, 7, 7, 64, 3, 1, 1),      # two chunks per tap
    'c96':    (2, 96, 7, 7, 64, 3, 1, 1),      # three chunks per tap
    'k4s2':   (2, 128, 11, 11, 64, 4, 2, 1),   # 16 taps x 4 chunks: the assessor's 4 x 4 / 2 in small; data gradient in 4 classes of 4 taps
    's2':     (3, 64, 9, 9, 64, 3, 2, 1),      # 3 x 3 / 2 on an odd input; data gradient classes of 1 / 2 / 2 / 4 taps
    'pw512':  (3, 512, 5, 5, 64, 1, 1, 0),     # one tap, 16 chunks, never a tap change
    'pw576':  (2, 576, 5, 5, 64, 1, 1, 0),     # one tap, 18 chunks: three K slices start inside it
    'co32':   (3, 64, 7, 7, 32, 3, 1, 1),      # tile columns behind Cout; the data gradient gathers 32 channels (one chunk per tap)
    'cin4':   (3, 4, 7, 7, 64, 3, 1, 1),       # the general loader: Ktot 36, a K tail
    'cin16':  (3, 16, 7, 7, 64, 3, 1, 1),      # the general loader: chunks span taps
    'cin48':  (2, 48, 7, 7, 64, 3, 1, 1),      # the general loader: Cin % 32 = 16
}
RELU = ('c32_5', 'c64', 'k4s2', 'cin16')       # geometries that also run with LOANS_F_RELU_IN
NO_DGRAD = ('pw512', 'pw576', 'cin4')
TILES = (1, 2, 3, 4, 17, 18, 19, 20)           # 128x128, 128x64, 64x64, 256x64; + 16 = LOANS_TILE_DMA
BOUND = 2e-6

FINE_TAIL_GEOM = (3, 96, 11, 11, 3072, 3, 1, 1)     # B, Cin, H, W, Cout, k, stride, pad of test_conv_tap_loop_fine_tail

_cache = {}


def _nhwc(a):
    return np.ascontiguousarray(np.transpose(a, (0, 2, 3, 1)))


def _nchw(t):
    return t.detach().cpu().numpy().transpose(0, 3, 1, 2)


def _case(name):
    """Seeded inputs, device tensors and the fp64 references of one geometry, made once and never changed."""
    if name in _cache:
        return _cache[name]
    from loans_amd import ops
    B, Cin, H, W, Cout, k, s, p = GEOMS[name]
    rng = np.random.RandomState(2000 + sorted(GEOMS).index(name))
    x = rng.standard_normal((B, Cin, H, W)).astype(np.float32)
    w = (rng.standard_normal((Cout, Cin, k, k)) / np.sqrt(Cin * k * k)).astype(np.float32)
    geo = ops.ConvGeometry(B, H, W, Cin, Cout, k, s, p)
    gy = rng.standard_normal((B, Cout, geo.Ho, geo.Wo)).astype(np.float32)
    w64 = w.astype(np.float64)
    y_ref, col = O.conv2d_fwd(x.astype(np.float64), w64, None, s, p)
    y_relu_ref, _ = O.conv2d_fwd(np.maximum(x, 0).astype(np.float64), w64, None, s, p)
    gx_ref, _, _ = O.conv2d_bwd(x.shape, col, w64, gy.astype(np.float64), s, p, False)
    _cache[name] = dict(geo=geo, x=dev(_nhwc(x)), w=dev(_nhwc(w)), gy=dev(_nhwc(gy)),
                        y_ref=y_ref, y_relu_ref=y_relu_ref, gx_ref=gx_ref)
    return _cache[name]


def run(name, kind, tile):
    """One deterministic launch kind of a geometry on one tile -> (device result, fp64 reference, both NCHW-comparable)."""
    from loans_amd import ops
    c = _case(name)
    geo = c['geo']
    if kind == 'fprop':
        return ops.conv_fprop(c['x'], c['w'], geo, tile=tile), c['y_ref']
    if kind == 'fprop_relu':
        return ops.conv_fprop(c['x'], c['w'], geo, relu_in=True, tile=tile), c['y_relu_ref']
    if kind == 'dgrad':             # strided: one launch per stride-parity class
        return ops.conv_dgrad(c['gy'], c['w'], geo, tile=tile), c['gx_ref']
    if kind == 'dgrad_classes':     # strided: every class in one launch (loans_igemm_classes_f32)
        return ops.conv_dgrad(c['gy'], c['w'], geo, tile=tile | ops.TILE_CLASSES), c['gx_ref']
    raise KeyError(kind)


def kinds(name):
    """The deterministic launch kinds of a geometry.  No data gradient where it says nothing about this kernel: a 1 x 1 gathers
    Cout = 64 channels (two chunks), Cin = 4 has a kernel of its own."""
    ks = ['fprop'] + (['fprop_relu'] if name in RELU else [])
    if name not in NO_DGRAD:
        ks.append('dgrad')
        if GEOMS[name][6] > 1:
            ks.append('dgrad_classes')
    return ks


def golden_key(name, kind, tile=None):
    return '%s_%s' % (name, kind) if tile is None else '%s_%s_tile%d' % (name, kind, tile)


def golden_array(g, name, kind, tile):
    """The recorded bits of a launch: per tile where the recording kernel's tiles disagreed, else the one array of the kind; a
    class launch that reproduced the per-class launches bit for bit shares their array."""
    keys = [golden_key(name, kind, tile), golden_key(name, kind)]
    if kind == 'dgrad_classes':
        keys += [golden_key(name, 'dgrad', tile), golden_key(name, 'dgrad')]
    for key in keys:
        if key in g.files:
            return g[key]
    raise KeyError((name, kind, tile))


def bit_cases():
    return [(n, k) for n in GEOMS for k in kinds(n)]


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("name", list(GEOMS))
def test_conv_tap_loop_oracle_and_bits(name, tile):
    with np.load(GOLDEN) as g:
        want = {k: golden_array(g, name, k, tile) for k in kinds(name)}
    for kind in kinds(name):
        got, ref = run(name, kind, tile)
        err = rel_err(_nchw(got), ref)
        w_ = torch.from_numpy(want[kind])
        diff = (got.cpu() != w_).sum().item()
        print('%s %s tile=%d rel_err=%.3g differing elements=%d of %d' % (name, kind, tile, err, diff, w_.numel()))
        assert err < BOUND, (name, kind, tile, err)
        assert got.shape == w_.shape and torch.equal(got.cpu(), w_), (name, kind, tile, diff)


@pytest.mark.parametrize("tile", TILES)
def test_conv_tap_loop_pair_launch(tile):
    """loans_igemm_pair_f32: the blocks behind the first convolution's tiles take the second one's weights and Cout (64 and
    32 here: the second has tile columns behind Cout on every tile).  Each output is the single launch's, bit for bit."""
    from loans_amd import ops
    a, b = _case('c64'), _case('co32')
    assert ops.fprop_pair_ok(a['x'], a['geo'], b['geo'])
    ya, yb = ops.conv_fprop_pair(a['x'], a['w'], b['w'], a['geo'], b['geo'], tile=tile)
    y_b_ref, _ = O.conv2d_fwd(_nchw(a['x']).astype(np.float64), _nchw(b['w']).astype(np.float64), None, 1, 1)
    ea, eb = rel_err(_nchw(ya), a['y_ref']), rel_err(_nchw(yb), y_b_ref)
    print('pair tile=%d rel_err=%.3g %.3g' % (tile, ea, eb))
    assert ea < BOUND and eb < BOUND
    with np.load(GOLDEN) as g:
        assert torch.equal(ya.cpu(), torch.from_numpy(g[golden_key('c64', 'fprop')]))
        assert torch.equal(yb.cpu(), torch.from_numpy(g['pair_second']))


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("name,splits", [('pw576', 3), ('c64', 4), ('c96', 2), ('k4s2', 7)])
def test_conv_tap_loop_split_k(name, splits, tile):
    """LOANS_TILE_SPLITK: a block starts at chunk split * ceil(nchunks / splits).  pw576: 18 chunks in 3 slices, chunks 6
    and 12 of the one tap; c64: 18 chunks in slices of 5, three starts on the second chunk of a tap or the first; c96: 27
    in slices of 14, the second starts on the last chunk of tap 4; k4s2: 64 in slices of 10.  (Atomic sums: no bit test.)"""
    from loans_amd import ops
    c = _case(name)
    y = ops.conv_fprop(c['x'], c['w'], c['geo'], tile=tile | (splits << 8))
    err = rel_err(_nchw(y), c['y_ref'])
    gx = ops.conv_dgrad(c['gy'], c['w'], c['geo'], tile=tile | (2 << 8))
    errg = rel_err(_nchw(gx), c['gx_ref'])
    print('%s splits=%d tile=%d rel_err=%.3g dgrad(2 slices) %.3g' % (name, splits, tile, err, errg))
    assert err < BOUND and errg < BOUND


def test_conv_tap_loop_fine_tail():
    """LOANS_TILE_FINETAIL (64x64 tiles, register-staged and LDS-DMA): the tiles behind the whole rounds of the machine run as
    K slices.  363 rows x 3072 channels are 288 tiles: on 256 CUs 240 at full K and 48 in slices of 27 chunks' fifth or
    sixth, which start inside a tap of three chunks.  With bias and statistics, as the tuned forward launches it."""
    from loans_amd import ops
    B, Cin, H, W, Cout, k, s, p = FINE_TAIL_GEOM
    rng = np.random.RandomState(77)
    x = rng.standard_normal((B, Cin, H, W)).astype(np.float32)
    w = (rng.standard_normal((Cout, Cin, k, k)) / np.sqrt(Cin * k * k)).astype(np.float32)
    bias = rng.standard_normal(Cout).astype(np.float32)
    geo = ops.ConvGeometry(B, H, W, Cin, Cout, k, s, p)
    rows_head, slices = ops._finetail_plan(B * H * W, Cout, k * k * Cin // 32, torch.device('cuda', 0))
    assert 0 < rows_head < B * H * W and slices >= 2, 'the case must take the sliced path on this machine'
    y_ref, _ = O.conv2d_fwd(x.astype(np.float64), w.astype(np.float64), bias.astype(np.float64), s, p)
    xd, wd, bd = dev(_nhwc(x)), dev(_nhwc(w)), dev(bias)
    for tile in (ops.TILE_FINETAIL, ops.TILE_FINETAIL | 16):
        st = ops.stats_buffer(Cout, 'cuda')
        y = ops.conv_fprop(xd, wd, geo, bias=bd, stats=st, tile=tile)
        err = rel_err(_nchw(y), y_ref)
        print('fine tail tile=%d rows at full K=%d slices=%d rel_err=%.3g' % (tile, rows_head, slices, err))
        assert err < BOUND, tile
        stats = st.sum(dim=0)
        np.testing.assert_allclose(stats[0].cpu().numpy(), y_ref.sum(axis=(0, 2, 3)), rtol=1e-5, atol=1e-2)      # test_conv_fine_tail_tile's
        np.testing.assert_allclose(stats[1].cpu().numpy(), (y_ref ** 2).sum(axis=(0, 2, 3)), rtol=1e-5)
