"""-m gpu: the row loader of the fp32 weight-gradient kernel (csrc/igemm.hip, wgrad_kernel) on the smallest
geometries at which its running pixel offsets can go wrong -- straight through the C ABI (loans_wgrad_f32).

The loader keeps, per chunk row, byte offsets into gy and x and the tap-shifted input coordinates, and advances
them by 32 pixels per chunk with carries (row end, image end) instead of recomputing them from (b, y, x).  The
cases wrap several grid rows and cross images inside one chunk (grid width < 32 that does not divide 32), end in a
ragged chunk with rows behind the last image, stride over odd inputs, put tile columns behind Ktot (Cin = 4) and
tile rows behind Cout (Cout = 32), on every tile and with 1 / ragged / more-than-chunks K slices.

Bounds: every case against the fp64 oracle with the call and the 5e-6 of test_gpu_kernels.py::
test_conv_fprop_dgrad_wgrad; at splits = 1 (one block per output tile adds once into a zeroed dw: deterministic)
additionally bit for bit against tests/golden/wgrad_f32_loader_bits.npz, which tests/golden/
make_wgrad_loader_golden.py recorded with the kernel as it was before the loader changed.

The file's stem is its key in the -m gpu suite order (tests/conftest.py: SUITE_ORDER ranks files by stem and
test_host_cpu.py::test_gpu_suite_is_collected_in_order_of_importance admits no stem outside it): these are fp32 kernel
tests against the oracle, rank 1, so they run right beside tests/test_gpu_kernels.py."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import chainer_ops as O
from tests.gpu_util import dev, rel_err

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'golden', 'wgrad_f32_loader_bits.npz')

GEOMS = {
    # name: B, Cin, H, W, Cout, k, stride, pad                 M = B * Ho * Wo, chunks of 32 rows
    'w7':    (3, 64, 7, 7, 64, 3, 1, 1),      # M 147: grid width 7, 4.6 grid rows and an image border per chunk, ragged end
    'w9':    (3, 64, 5, 9, 64, 3, 1, 1),      # M 135: grid 5 x 9, ragged end
    's2':    (5, 16, 15, 15, 64, 3, 2, 1),    # M 320: 3 x 3 / 2 on an odd input, grid 8 x 8, whole chunks only
    'k4s2':  (3, 16, 11, 11, 64, 4, 2, 1),    # M 75: the assessor's 4 x 4 / 2 (75 -> 37) in small, grid 5 x 5
    'cin4':  (3, 4, 9, 9, 128, 3, 1, 1),      # M 243: Ktot 36, tile columns behind Ktot
    'co32':  (3, 16, 7, 7, 32, 3, 1, 1),      # M 147: gradient rows of the 64- and 128-row tiles do not exist
}
TILES = (1, 3, 5)                 # 128 x 128, 64 x 64, 64 x 128
SPLITS = (1, 2, 3, 64)            # one slice; 2 or 3 leave every geometry (3, 5, 8 or 10 chunks) a shorter last slice; more slices than chunks
BIT_TILES = (1, 3)
BIT_RELU = {'cin4', 'co32'}       # geometries whose LOANS_F_RELU_IN result is in the golden file too (file size)

_cache = {}


def _case(name):
    """Seeded inputs, device tensors and the fp64 reference (plain and relu'd input) of one geometry, made once."""
    if name in _cache:
        return _cache[name]
    from loans_amd import ops
    B, Cin, H, W, Cout, k, s, p = GEOMS[name]
    rng = np.random.RandomState(1000 + sorted(GEOMS).index(name))
    x = rng.standard_normal((B, Cin, H, W)).astype(np.float32)
    geo = ops.ConvGeometry(B, H, W, Cin, Cout, k, s, p)
    gy = rng.standard_normal((B, Cout, geo.Ho, geo.Wo)).astype(np.float32)
    w64 = np.zeros((Cout, Cin, k, k), np.float64)
    refs = []
    for relu in (False, True):
        xin = np.maximum(x, 0) if relu else x
        _, col = O.conv2d_fwd(xin.astype(np.float64), w64, None, s, p)
        _, gw, _ = O.conv2d_bwd(x.shape, col, w64, gy.astype(np.float64), s, p, False, need_gx=False)
        refs.append(gw)
    xd = dev(np.transpose(x, (0, 2, 3, 1)))
    gyd = dev(np.transpose(gy, (0, 2, 3, 1)))
    _cache[name] = (geo, xd, gyd, refs)
    return _cache[name]


def run_wgrad(name, relu, tile, splits):
    """dw (Cout, k, k, Cin) of one loans_wgrad_f32 launch into a zeroed buffer."""
    from loans_amd import _lib, ops
    lib = _lib.load()
    geo, xd, gyd, _ = _case(name)
    B, Cin, H, W, Cout, k, s, p = GEOMS[name]
    dw = torch.zeros(Cout, k, k, Cin, device='cuda')
    d = _lib.IgemmDesc()
    C.memmove(C.byref(d), C.byref(geo.fwd), C.sizeof(d))
    d.flags = _lib.F_RELU_IN if relu else 0
    d.tile = tile
    _lib.check(lib.loans_wgrad_f32(xd.data_ptr(), gyd.data_ptr(), dw.data_ptr(), C.byref(d), splits, ops._stream()),
               'loans_wgrad_f32')
    torch.cuda.synchronize()
    return dw


def golden_key(name, relu, tile):
    return '%s_relu%d_tile%d' % (name, int(relu), tile)


def golden_cases():
    return [(n, r, t) for n in GEOMS for r in (False, True) for t in BIT_TILES if not r or n in BIT_RELU]


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("name", list(GEOMS))
def test_wgrad_loader_oracle(name, relu, tile):
    Cin = GEOMS[name][1]
    ref = _case(name)[3][int(relu)]
    for splits in SPLITS:
        dw = run_wgrad(name, relu, tile, splits)
        got = dw.cpu().numpy().transpose(0, 3, 1, 2)
        err = rel_err(got, ref)
        print('%s relu=%d tile=%d splits=%d rel_err=%.3g' % (name, relu, tile, splits, err))
        assert got.shape == ref.shape and Cin == got.shape[1]
        assert err < 5e-6, (name, relu, tile, splits, err)


@pytest.mark.parametrize("name,relu,tile", golden_cases())
def test_wgrad_loader_bits(name, relu, tile):
    with np.load(GOLDEN) as g:
        want = torch.from_numpy(g[golden_key(name, relu, tile)])
    dw = run_wgrad(name, relu, tile, 1).cpu()
    diff = (dw != want).sum().item()
    print('%s relu=%d tile=%d differing elements=%d of %d' % (name, relu, tile, diff, want.numel()))
    assert dw.shape == want.shape and dw.dtype == want.dtype
    assert torch.equal(dw, want)
