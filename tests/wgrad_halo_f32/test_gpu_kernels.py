"""-m gpu: the nine-tap fp32 weight-gradient kernel (csrc/wgrad_halo_f32.hip, LOANS_TILE_WGHALO_64 of loans_wgrad_f32)
on the smallest geometries at which its pixel tiles can go wrong -- straight through the C ABI.

A block owns 64 x 64 channels x nine taps and walks pixel tiles (7 x 14, or 7 x 8 where that pads the frame less); a
k-step of the MFMA is two horizontally adjacent pixels, out-of-frame halo pixels and the pixels of ragged tiles are
zeros in LDS.  All geometries are 3 x 3 / 1 / pad 1 and ragged for any of the tile shapes 7 x 14, 8 x 14 and 8 x 16:
a frame smaller than a tile with an odd width (a k-step pairs a real pixel with a padded one) over three images (a
block's tile range crosses image ends); one or two rows and columns more than a tile (2 x 2 tiles per image, ragged
right and bottom); res5's 7 x 7 frame with 2 x 2 channel-tile pairs; whole 7 x 14 tiles with two output-channel tiles.
Every case runs with 1, 2 and 3 blocks per channel-tile pair and with more blocks than pixel tiles.

Bounds: every run against the fp64 oracle with the 5e-6 of test_gpu_kernels.py::test_conv_fprop_dgrad_wgrad, the
project's fp32 weight-gradient bound (at most 600 pixels per sum: the order of the sums cannot come near it).

The file's stem is its key in the -m gpu suite order (tests/conftest.py): fp32 kernels against the oracle, rank 1."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import chainer_ops as O
from tests.gpu_util import dev, rel_err

pytestmark = pytest.mark.gpu

TILE = 38                         # LOANS_TILE_WGHALO_64
LOANS_EINVAL = -1

GEOMS = {
    # name: B, Cin, H, W, Cout (3 x 3 / 1 / pad 1)
    'small':  (3, 64, 5, 9, 64),      # frame < tile, odd width, three images
    'ragged': (2, 64, 9, 17, 64),     # 2 x 2 tiles per image, ragged right and bottom tiles
    'res5':   (3, 128, 7, 7, 128),    # res5's frame, 2 x 2 channel-tile pairs
    'whole':  (1, 64, 14, 28, 128),   # whole 7 x 14 tiles, two output-channel tiles
}
SPLITS = (1, 2, 3, 64)            # blocks per channel-tile pair; 64 > pixel tiles of every geometry (3, 12, 3, 4)
RELU_GEOMS = ('small', 'res5')

_cache = {}


def _case(name):
    """Seeded inputs, device tensors and the fp64 reference (plain and relu'd input) of one geometry, made once."""
    if name in _cache:
        return _cache[name]
    from loans_amd import ops
    B, Cin, H, W, Cout = GEOMS[name]
    rng = np.random.RandomState(2000 + sorted(GEOMS).index(name))
    x = rng.standard_normal((B, Cin, H, W)).astype(np.float32)
    geo = ops.ConvGeometry(B, H, W, Cin, Cout, 3, 1, 1)
    gy = rng.standard_normal((B, Cout, H, W)).astype(np.float32)
    w64 = np.zeros((Cout, Cin, 3, 3), np.float64)
    refs = []
    for relu in (False, True):
        xin = np.maximum(x, 0) if relu else x
        _, col = O.conv2d_fwd(xin.astype(np.float64), w64, None, 1, 1)
        _, gw, _ = O.conv2d_bwd(x.shape, col, w64, gy.astype(np.float64), 1, 1, False, need_gx=False)
        refs.append(gw)
    xd = dev(np.transpose(x, (0, 2, 3, 1)))
    gyd = dev(np.transpose(gy, (0, 2, 3, 1)))
    _cache[name] = (geo, xd, gyd, refs)
    return _cache[name]


def _launch(geo, xd, gyd, dw, relu, splits, tile=TILE):
    """return code of one loans_wgrad_f32 launch accumulating into dw"""
    from loans_amd import _lib, ops
    d = _lib.IgemmDesc()
    C.memmove(C.byref(d), C.byref(geo.fwd), C.sizeof(d))
    d.flags = _lib.F_RELU_IN if relu else 0
    d.tile = tile
    rc = _lib.load().loans_wgrad_f32(xd.data_ptr(), gyd.data_ptr(), dw.data_ptr(), C.byref(d), splits, ops._stream())
    torch.cuda.synchronize()
    return rc


def run_wgrad(name, relu, splits, dw=None):
    geo, xd, gyd, _ = _case(name)
    B, Cin, H, W, Cout = GEOMS[name]
    if dw is None:
        dw = torch.zeros(Cout, 3, 3, Cin, device='cuda')
    assert _launch(geo, xd, gyd, dw, relu, splits) == 0
    return dw


def _nchw(dw):
    return dw.cpu().numpy().transpose(0, 3, 1, 2)


@pytest.mark.parametrize("name", list(GEOMS))
def test_wgrad_halo_f32_oracle(name):
    ref = _case(name)[3][0]
    for splits in SPLITS:
        got = _nchw(run_wgrad(name, False, splits))
        err = rel_err(got, ref)
        print('%s splits=%d rel_err=%.3g' % (name, splits, err))
        assert got.shape == ref.shape
        assert err < 5e-6, (name, splits, err)


@pytest.mark.parametrize("name", RELU_GEOMS)
def test_wgrad_halo_f32_relu_in(name):
    ref = _case(name)[3][1]
    for splits in SPLITS:
        err = rel_err(_nchw(run_wgrad(name, True, splits)), ref)
        print('%s relu splits=%d rel_err=%.3g' % (name, splits, err))
        assert err < 5e-6, (name, splits, err)


@pytest.mark.parametrize("name", list(GEOMS))
def test_wgrad_halo_f32_accumulates(name):
    """dw pre-filled with a seeded pattern: the result is the pattern plus the gradient"""
    B, Cin, H, W, Cout = GEOMS[name]
    ref = _case(name)[3][0]
    pat = np.random.RandomState(7).standard_normal((Cout, 3, 3, Cin)).astype(np.float32)
    got = _nchw(run_wgrad(name, False, 2, dw=dev(pat)))
    want = pat.astype(np.float64).transpose(0, 3, 1, 2) + ref
    err = float(np.abs(got - want).max() / (np.abs(ref).max() + 1e-30))     # relative to the gradient, not to the sum
    print('%s accumulate rel_err=%.3g' % (name, err))
    assert err < 5e-6, (name, err)


@pytest.mark.parametrize("name", list(GEOMS))
def test_wgrad_halo_f32_deterministic(name):
    """one block per pair adds once into a zeroed dw: two launches agree bit for bit"""
    assert torch.equal(run_wgrad(name, False, 1), run_wgrad(name, False, 1))


REJECTED = {
    # name: B, Cin, H, W, Cout, k, stride, pad
    's2':   (5, 64, 15, 15, 64, 3, 2, 1),
    'k4s2': (3, 64, 11, 11, 64, 4, 2, 1),
    'cin4': (3, 4, 9, 9, 64, 3, 1, 1),
    'co32': (3, 64, 7, 7, 32, 3, 1, 1),
    'k1':   (3, 64, 9, 9, 64, 1, 1, 0),
}


@pytest.mark.parametrize("name", list(REJECTED))
def test_wgrad_halo_f32_rejects(name):
    """argument checks on the host side of the launcher: LOANS_EINVAL, no kernel runs, a poisoned dw stays as it was"""
    from loans_amd import ops
    B, Cin, H, W, Cout, k, s, p = REJECTED[name]
    geo = ops.ConvGeometry(B, H, W, Cin, Cout, k, s, p)
    gen = torch.Generator(device='cuda').manual_seed(11)
    xd = torch.randn(B, H, W, Cin, device='cuda', generator=gen)
    gyd = torch.randn(B, geo.Ho, geo.Wo, Cout, device='cuda', generator=gen)
    poison = torch.full((Cout, k, k, Cin), 12345.5, device='cuda')
    dw = poison.clone()
    assert _launch(geo, xd, gyd, dw, False, 0) == LOANS_EINVAL
    assert torch.equal(dw, poison)
