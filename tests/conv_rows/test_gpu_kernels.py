"""-m gpu: the per-row prologue of the implicit-GEMM convolution kernels (csrc/conv_rows.h: row walk, base offsets, tap
masks, output offsets), through whole convolutions on the smallest geometries at which it can go wrong -- bf16 storage
(igemm16_kernel and the ping-pong tile of igemm16_pp.h) and fp32 storage (igemm_kernel), forward and data gradient
with an explicit tile.

The arithmetic itself is checked on the CPU (tests/conv_rows/test_rows_cpu.py).  What is left for the GPU: that every
kernel passes the right values into it -- element size, rows per pass (32, or 64 on the 512-thread tiles), the 32- or
64-bit mask, the first row of a launch, the class's own grid and phase in a data gradient.

Bounds: every output against the fp64 oracle (on the bf16-rounded operands for bf16 storage) with the bound of the
sibling tests for the same call: 2e-6 (test_gpu_kernels.py) and BF16_EPS (test_gpu_bf16_storage.py); and bit for bit
against tests/golden/conv_rows_bits.npz, which tests/golden/make_conv_rows_golden.py recorded with the kernels as they
were while each carried its own copy of the prologue.  All launches are deterministic: one K slice, no statistics, no
atomics.  The file holds one array per storage, geometry and launch kind, and an array per tile (its XOR with the former)
only where the recording kernels' tiles disagreed (tile 44 contracts 32 k values per MFMA).

The file's stem is its key in the -m gpu suite order (tests/conftest.py): kernel tests against the oracle, rank 1."""
import os

import numpy as np
import pytest
import torch

from oracle import chainer_ops as O
from tests.gpu_util import dev, rel_err

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'golden', 'conv_rows_bits.npz')

GEOMS = {
    # name: B, Cin, H, W, Cout, k, stride, pad
    'b7':    (3, 64, 7, 7, 64, 3, 1, 1),       # borders on every tap, tiles span images, rows behind M in every tile
    'b5':    (12, 64, 5, 5, 64, 3, 1, 1),      # M 300, 25-pixel images: a 64-row advance crosses two images and more, and every
                                               # staged row of a 256-row tile is live
    's2':    (3, 64, 9, 9, 64, 3, 2, 1),       # strided on an odd input; data gradient classes of 1 / 2 / 2 / 4 taps with phases
    'k4s2':  (2, 64, 11, 11, 64, 4, 2, 1),     # 16 taps
    'wide':  (2, 64, 3, 40, 64, 3, 1, 1),      # gridW larger than the row step
    'pw':    (3, 64, 7, 7, 64, 1, 1, 0),       # one tap: nx = ny = 1
    'cin8':  (2, 8, 11, 11, 16, 3, 1, 1),      # one 16-byte unit per tap, K tail, tile columns behind Cout
}
RELU = ('b7', 'k4s2')                          # geometries that also run with LOANS_F_RELU_IN
NO_DGRAD = ('pw', 'cin8')
TILES16 = (1, 2, 3, 4, 7, 9, 43, 44, 33, 34, 35)       # 7, 9: 512 threads; 43 / 44: ping-pong K loop; + 32: deep ring
TILES32 = (1, 2, 3, 4, 17, 18, 19, 20)                 # 128x128, 128x64, 64x64, 256x64; + 16 = LOANS_TILE_DMA
GEOMS32 = ('b7', 'b5', 's2', 'k4s2', 'wide')           # fp32 storage: these, with Cin = 32 (one chunk per tap)
TILE_SPLIT = 6                                         # LOANS_TILE_SPLIT: the only launch with a first row other than 0
BOUND32 = 2e-6
BF16_EPS = 2.0 ** -8

_cache = {}


def _nhwc(a):
    return np.ascontiguousarray(np.transpose(a, (0, 2, 3, 1)))


def _nchw(t):
    return t.detach().float().cpu().numpy().transpose(0, 3, 1, 2)


def _r(a):
    """round an fp32 array to bf16 (RNE) and return it as fp32"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).float().numpy()


def geometry(storage, name):
    B, Cin, H, W, Cout, k, s, p = GEOMS[name]
    return (B, 32 if storage == 'f32' else Cin, H, W, Cout, k, s, p)


def _case(storage, name):
    """Seeded inputs, device tensors and the fp64 references of one geometry, made once and never changed."""
    if (storage, name) in _cache:
        return _cache[storage, name]
    from loans_amd import ops
    B, Cin, H, W, Cout, k, s, p = geometry(storage, name)
    rng = np.random.RandomState(3000 + sorted(GEOMS).index(name))
    geo = ops.ConvGeometry(B, H, W, Cin, Cout, k, s, p)
    x = rng.standard_normal((B, Cin, H, W)).astype(np.float32)
    w = (rng.standard_normal((Cout, Cin, k, k)) / np.sqrt(Cin * k * k)).astype(np.float32)
    gy = rng.standard_normal((B, Cout, geo.Ho, geo.Wo)).astype(np.float32)
    wq = w
    if storage == 'bf16':           # operands are bf16 tensors (the weights fp32 masters, cast by the call)
        x, wq, gy = _r(x), _r(w), _r(gy)
    w64 = wq.astype(np.float64)
    y_ref, col = O.conv2d_fwd(x.astype(np.float64), w64, None, s, p)
    y_relu_ref, _ = O.conv2d_fwd(np.maximum(x, 0).astype(np.float64), w64, None, s, p)
    gx_ref, _, _ = O.conv2d_bwd(x.shape, col, w64, gy.astype(np.float64), s, p, False)
    to = (lambda a: dev(a).to(torch.bfloat16).contiguous()) if storage == 'bf16' else dev
    _cache[storage, name] = dict(geo=geo, x=to(_nhwc(x)), w=dev(_nhwc(w)), gy=to(_nhwc(gy)),
                                 y_ref=y_ref, y_relu_ref=y_relu_ref, gx_ref=gx_ref)
    return _cache[storage, name]


def run(storage, name, kind, tile):
    """One deterministic launch kind of a geometry on one tile -> (device result, fp64 reference)."""
    from loans_amd import ops
    c = _case(storage, name)
    geo = c['geo']
    if kind == 'fprop':
        return ops.conv_fprop(c['x'], c['w'], geo, tile=tile), c['y_ref']
    if kind == 'fprop_relu':
        return ops.conv_fprop(c['x'], c['w'], geo, relu_in=True, tile=tile), c['y_relu_ref']
    if kind == 'dgrad':             # strided: one launch per stride-parity class
        return ops.conv_dgrad(c['gy'], c['w'], geo, tile=tile), c['gx_ref']
    if kind == 'dgrad_classes':     # fp32, strided: every class in one launch, each block on its class's own grid and taps
        return ops.conv_dgrad(c['gy'], c['w'], geo, tile=tile | ops.TILE_CLASSES), c['gx_ref']
    raise KeyError(kind)


def kinds(storage, name):
    """The launch kinds of a geometry.  No data gradient of the 1 x 1 (it is the forward kernel on other operands) and of
    Cin = 8 (it gathers Cout = 16 channels: nothing the forward case does not reach)."""
    ks = ['fprop'] + (['fprop_relu'] if name in RELU else [])
    if name not in NO_DGRAD:
        ks.append('dgrad')
        if storage == 'f32' and GEOMS[name][6] > 1:
            ks.append('dgrad_classes')
    return ks


def bits(t):
    """a result as an integer array (.npz holds no bf16)"""
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).numpy()


def golden_key(storage, name, kind, tile=None):
    key = '%s_%s_%s' % (storage, name, kind)
    return key if tile is None else '%s_tile%d' % (key, tile)


def golden_array(g, storage, name, kind, tile):
    """The recorded bits of a launch: the one array of the kind, XOR-ed with the tile's own array where the recording kernels'
    tiles disagreed (a few roundings: the difference is nearly all zeros and costs the file next to nothing); a class launch
    that reproduced the per-class launches bit for bit shares their arrays."""
    for kd in ((kind, 'dgrad') if kind == 'dgrad_classes' else (kind,)):
        base, own = golden_key(storage, name, kd), golden_key(storage, name, kd, tile)
        if own in g.files:
            return g[base] ^ g[own]
        if base in g.files:
            return g[base]
    raise KeyError((storage, name, kind, tile))


def cases():
    return [('bf16', n, t) for n in GEOMS for t in TILES16] + [('f32', n, t) for n in GEOMS32 for t in TILES32]


def _check(storage, name, kind, tile, want):
    got, ref = run(storage, name, kind, tile)
    err = rel_err(_nchw(got), ref)
    diff = int((bits(got) != want).sum()) if bits(got).shape == want.shape else -1
    print('%s %s %s tile=%d rel_err=%.3g differing elements=%d of %d' % (storage, name, kind, tile, err, diff, want.size))
    assert err < (BF16_EPS if storage == 'bf16' else BOUND32), (storage, name, kind, tile, err)
    assert diff == 0, (storage, name, kind, tile, diff)


@pytest.mark.parametrize("storage,name,tile", cases())
def test_conv_rows_oracle_and_bits(storage, name, tile):
    with np.load(GOLDEN) as g:
        want = {k: golden_array(g, storage, name, k, tile) for k in kinds(storage, name)}
    for kind in kinds(storage, name):
        _check(storage, name, kind, tile, want[kind])


def test_conv_rows_split_tile():
    """LOANS_TILE_SPLIT on the 300-row geometry: fewer big tiles than the machine has slots, so the whole problem is the
    second launch (64x64 tiles from row 0) and its result is the 64x64 tile's, bit for bit."""
    from loans_amd import ops
    c = _case('f32', 'b5')
    geo = c['geo']
    assert ops._igemm_launches(geo.rows, geo.Cout, TILE_SPLIT, c['x'].device) == 1
    with np.load(GOLDEN) as g:
        want = {k: golden_array(g, 'f32', 'b5', k, 3) for k in ('fprop', 'dgrad')}
    for kind in ('fprop', 'dgrad'):
        _check('f32', 'b5', kind, TILE_SPLIT, want[kind])
