"""-m gpu: ``ops.bn_eval_coeffs`` (csrc/bn_pool.hip: bn_eval_coeffs_kernel), the only producer of a test-mode BN state, over the
coefficient grid of tests/eval_mode/cases.py within the bounds derived there, and every consumer the test-mode forward runs on such
a state -- ``bn_apply(want_bits=False)``, ``bn_relu_maxpool`` without ``want_sel``, ``blur_pool(x, st)``, ``se_excite`` /
``bn_apply_gate`` -- against float64 within max(5 |fp32 restatement - fp64|, 5e-4 |ref|, 1e-5) (tests/imagenet_droppath/reference.py:
tol); bf16 tensors against the same reference on the bf16-rounded inputs, the restatement rounding what the kernel stores.  The
states are built from running statistics far from the batch statistics of ``x`` (cases.far_state); their fp32 vectors are the
references' exact inputs, as in the other kernel tests."""
import json

import numpy as np
import pytest
import torch

from loans_amd import _lib, ops
from oracle import chainer_ops as C
from tests.eval_mode import cases as K
from tests.gpu_util import dev
from tests.imagenet_droppath.reference import tol
from tests.imagenet_droppath.test_gpu_kernels import _np, _t
from tests.imagenet_se import reference as S

pytestmark = pytest.mark.gpu
VECTORS = ('mean', 'rstd', 'scale', 'shift')
BF = [False, True]
bf_id = lambda b: 'bf16' if b else 'f32'        # noqa: E731


def _eval_state(d):
    """(BNState, its fp32 vectors, the device inputs) of ops.bn_eval_coeffs on a dict of gamma, beta, rm, rv"""
    t = {k: dev(d[k]) for k in ('gamma', 'beta', 'rm', 'rv')}
    st = ops.bn_eval_coeffs(t['gamma'], t['beta'], t['rm'], t['rv'])
    return st, {k: _np(getattr(st, k)) for k in VECTORS}, t


def _far(x, seed):
    st, s, _ = _eval_state(K.far_state(x, seed))
    return st, s


def _within(name, got, r32, r64):
    err, bound = np.abs(np.asarray(got, np.float64) - r64), tol(r32, r64)
    worst = float((err / bound).max())
    print('%s: worst error / bound %.3g (max error %.3g)' % (name, worst, float(err.max())))
    assert worst <= 1.0, name


def _data(shape, seed, bf16):
    rng = np.random.RandomState(seed)
    q = C.round_bf16 if bf16 else (lambda a: a)
    return [q((rng.standard_normal(shape) * s + m).astype(np.float32)) for s, m in ((2, 0.5), (1, 0), (1, 0))]


@pytest.mark.parametrize('C_', K.COEFF_C)
def test_coefficients_over_the_grid(C_):
    assert ops.BN_EPS == C.BN_EPS
    ratios = {}
    for rot in K.rotations(C_):
        d = K.make_coeffs(C_, rot)
        st, got, t = _eval_state(d)
        assert all(getattr(st, k).dtype == torch.float32 and getattr(st, k).numel() == C_ for k in VECTORS)
        K.check_coeffs(got, d, ratios)
        for key, name in (('gamma', 'gamma'), ('beta', 'beta'), ('rm', 'running mean'), ('rv', 'running variance')):
            assert _np(t[key]).tobytes() == d[key].tobytes(), name + ' was written'
        again = ops.bn_eval_coeffs(t['gamma'], t['beta'], t['rm'], t['rv'])
        assert all(torch.equal(getattr(st, k), getattr(again, k)) for k in VECTORS)
    print('EVAL_RATIOS C%d %s' % (C_, json.dumps(ratios, sort_keys=True)))


def test_coefficients_refuse_a_missing_argument_and_an_empty_vector():
    lib = _lib.load()
    buf = torch.zeros(1 << 12, device='cuda')
    p = buf.data_ptr()
    f = lib.loans_bn_eval_coeffs_f32
    for missing in range(8):            # gamma, beta, running mean, running variance, mean, rstd, scale, shift
        args = [p] * 8
        args[missing] = 0
        assert f(64, ops.BN_EPS, *args, 0) == -1, missing          # LOANS_EINVAL
    assert f(0, ops.BN_EPS, *([p] * 8), 0) == -1
    assert f(-4, ops.BN_EPS, *([p] * 8), 0) == -1
    torch.cuda.synchronize()
    assert not buf.any()
    with pytest.raises(_lib.HipKernelError, match='LOANS_EINVAL'):
        ops.check(f(0, ops.BN_EPS, *([p] * 8), 0), 'loans_bn_eval_coeffs_f32')


# (rows as B x H x W, C): one row; the older tests' shape on the 16-byte-unit kernels and on the fall-back (96: neither type tiles
# it); an odd size at the channel count only bf16 tiles
APPLY = [((1, 1, 1), 4), ((3, 9, 7), 64), ((3, 9, 7), 96), ((5, 33, 31), 2048)]


@pytest.mark.parametrize('bf16', BF, ids=bf_id)
@pytest.mark.parametrize('case', APPLY, ids=lambda c: '%dx%dx%d-C%d' % (c[0] + (c[1],)))
def test_bn_apply_without_sign_bits_on_a_running_state(case, bf16):
    (b, h, w), C_ = case
    rows = b * h * w
    x, x2, res = _data((rows, C_), 31 * C_ + rows, bf16)
    (st, s), (st2, s2) = _far(x, 1), _far(x2, 2)
    if rows > 1:        # the state is far from the batch statistics: the output is not a normalised tensor
        z = K.apply_ref(x, s, np.float64, relu=False)['y']
        assert np.abs(z.mean(0)).min() > 0.2 and (np.abs(z.std(0) - 1) > 0.02).mean() > 0.9
    for mode, kw, rkw in (('plain', {}, {}), ('residual', dict(residual=_t(res, bf16)), dict(residual=res)),
                          ('second', dict(x2=_t(x2, bf16), st2=st2), dict(x2=x2, st2=s2))):
        for relu in (False, True):
            y = ops.bn_apply(_t(x, bf16), st, relu=relu, want_bits=False, **kw)
            assert getattr(y, 'relu_bits', None) is None and y.dtype == (torch.bfloat16 if bf16 else torch.float32)
            r64 = K.apply_ref(x, s, np.float64, relu=relu, **rkw)['y']
            r32 = K.apply_ref(x, s, np.float32, relu=relu, bf16=bf16, **rkw)['y']
            _within('%s relu=%d' % (mode, relu), _np(y), r32, r64)


POOL = [(s, c) for s in ((2, 3, 3), (2, 8, 7), (3, 13, 11)) for c in (4, 64, 96)]


@pytest.mark.parametrize('bf16', BF, ids=bf_id)
@pytest.mark.parametrize('case', POOL, ids=lambda c: '%dx%dx%d-C%d' % (c[0] + (c[1],)))
def test_bn_relu_maxpool_without_the_selected_values(case, bf16):
    shape, C_ = case[0] + (case[1],), case[1]
    x = _data(shape, 17 * C_ + shape[1], bf16)[0]
    st, s = _far(x, 3)
    y, idx = ops.bn_relu_maxpool(_t(x, bf16), st)
    r64, r32 = K.pool_ref(x, s, np.float64), K.pool_ref(x, s, np.float32, bf16=bf16)
    assert tuple(y.shape) == r64['y'].shape and idx.dtype == torch.uint8
    _within('y', _np(y), r32['y'], r64['y'])
    got = idx.cpu().numpy().astype(np.int64)
    bound = tol(r32['y'], r64['y'])
    picked = np.take_along_axis(r64['win'], got[:, :, :, None, :], axis=3)[:, :, :, 0, :]
    assert got.max() <= 8 and np.isfinite(picked).all(), 'argmax points into the overhang'
    assert (r64['y'] - picked <= 2 * bound).all(), 'argmax does not hold the maximum'
    top = np.sort(r64['win'], axis=3)
    sure = top[:, :, :, -1, :] - top[:, :, :, -2, :] > 2 * bound         # the winner leads by more than both may be off
    assert sure.mean() > 0.2 and np.array_equal(got[sure], r64['idx'][sure])
    assert (r64['y'] > 0).mean() > 0.2


BLUR = [(2, 2, 2, 64, False), (3, 3, 5, 64, False), (3, 3, 5, 64, True), (2, 7, 6, 128, True)]


@pytest.mark.parametrize('case', BLUR, ids=lambda c: '%dx%dx%dx%d-%s' % (c[:4] + (bf_id(c[4]),)))
def test_blur_pool_on_a_running_state(case):
    shape, bf16 = case[:4], case[4]
    x = _data(shape, 1000 * shape[3] + shape[1], bf16)[0]
    st, s = _far(x, 4)
    y = ops.blur_pool(_t(x, bf16), st)
    r64, r32 = K.blur_ref(x, s, np.float64), K.blur_ref(x, s, np.float32, bf16=bf16)
    assert tuple(y.shape) == r64['y'].shape and y.dtype == (torch.bfloat16 if bf16 else torch.float32)
    _within('y', _np(y), r32['y'], r64['y'])
    assert (r64['pre'] > 0).mean() > 0.1 and (r64['pre'] < 0).mean() > 0.1


GATE = [(5, (7, 5), 64, 16, False), (5, (7, 5), 64, 16, True), (3, (9, 9), 128, 4, True)]


@pytest.mark.parametrize('mode', ['residual', 'second'])
@pytest.mark.parametrize('case', GATE, ids=lambda c: '%dx%dx%d-C%d-R%d-%s' % ((c[0],) + c[1] + c[2:4] + (bf_id(c[4]),)))
def test_the_gated_junction_on_a_running_state(case, mode):
    B, (H, W), C_, R, bf16 = case
    hid = C_ // R
    x, x2, res = _data((B, H * W, C_), 1000 * C_ + 10 * B + H, bf16)
    rng = np.random.RandomState(C_ + R)
    se = [a.astype(np.float32) for a in (rng.standard_normal((hid, C_)) * np.sqrt(2.0 / C_), 0.3 * rng.standard_normal(hid),
                                         rng.standard_normal((C_, hid)) * 0.5 / np.sqrt(hid), rng.uniform(-1.7, 1.7, C_))]
    (st, s), (st2, s2) = _far(x, 5), _far(x2, 6)
    d4 = lambda a: _t(a.reshape(B, H, W, C_), bf16)        # noqa: E731
    gate = ops.se_excite(d4(x), st, *(dev(a) for a in se))
    if mode == 'residual':
        y = ops.bn_apply_gate(d4(x), st, gate.s, residual=d4(res))
        second, sec = res, None
    else:
        y = ops.bn_apply_gate(d4(x), st, gate.s, x2=d4(x2), st2=st2)
        second, sec = x2, s2
    f64 = S.junction_fwd(x, s, se, second, sec)
    f32 = S.junction_fwd(x, s, se, second, sec, dtype=np.float32, bf16=bf16)
    assert f64['s'].min() < 0.3 and f64['s'].max() > 0.7            # gates on both sides
    _within('s', _np(gate.s), f32['s'], f64['s'])
    _within('y', _np(y).reshape(B, H * W, C_), f32['out'], f64['out'])


@pytest.mark.parametrize('bf16', BF, ids=bf_id)
@pytest.mark.parametrize('C_', [64, 96])
def test_the_two_instantiations_agree(C_, bf16):
    """the training forward's kernels (sign bits, values at the argmaxes) and the test forward's write the same output"""
    x, x2, res = _data((3, 9, 7, C_), C_, bf16)
    (st, _), (st2, _) = _far(x, 7), _far(x2, 8)
    for kw in ({}, dict(residual=_t(res, bf16)), dict(x2=_t(x2, bf16), st2=st2)):
        a = ops.bn_apply(_t(x, bf16), st, relu=True, want_bits=True, **kw)
        b = ops.bn_apply(_t(x, bf16), st, relu=True, want_bits=False, **kw)
        assert a.relu_bits is not None and torch.equal(a, b)
    with_sel, without = ops.bn_relu_maxpool(_t(x, bf16), st, want_sel=True), ops.bn_relu_maxpool(_t(x, bf16), st)
    assert torch.equal(with_sel[0], without[0]) and torch.equal(with_sel[1], without[1])
    assert (with_sel[2] is not None) == (C_ == 64)
