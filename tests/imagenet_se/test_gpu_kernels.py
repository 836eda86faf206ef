"""-m gpu: the squeeze-and-excitation junction (csrc/se.hip through ops.se_excite / bn_apply_gate / bn_backward_gate) against the
float64 formulas of tests/imagenet_se/reference.py within max(5 |fp32 restatement - fp64|, 5e-4 |ref|, 1e-5); bf16 tensors
against the same reference on the bf16-rounded inputs, the restatement rounding what the kernel stores.

Shapes: 5 x (7 x 5) x 64 (hidden width 4, the smallest; 35 x 16 units per sample are no multiple of 256), 5 x (7 x 5) x 2048 fp32
(the channel count the 16-byte-unit layout does not tile: the row walk), 3 x (9 x 9) x 128 bf16 at R = 4, 2 x (56 x 56) x 64 (a
sample spans many blocks: partial records are folded), 1 x (7 x 7) x 512 (one sample, one block)."""
import numpy as np
import pytest
import torch

from loans_amd import ops
from oracle import chainer_ops as C
from tests.gpu_util import dev
from tests.imagenet_droppath import reference as D
from tests.imagenet_droppath.test_gpu_kernels import _np, _state, _t
from tests.imagenet_se import reference as S

pytestmark = pytest.mark.gpu

CASES = [  # B, positions (H, W), C, R, bf16
    (5, (7, 5), 64, 16, False), (5, (7, 5), 64, 16, True), (5, (7, 5), 2048, 16, False), (3, (9, 9), 128, 4, True),
    (2, (56, 56), 64, 16, False), (2, (56, 56), 64, 16, True), (1, (7, 7), 512, 16, False),
]
GRADS = ('ggamma', 'gbeta', 'gW1', 'gb1', 'gW2', 'gb2', 'ggamma2', 'gbeta2')


def _id(case):
    B, (H, W), C_, R, bf16 = case
    return '%dx%dx%d-C%d-R%d-%s' % (B, H, W, C_, R, 'bf16' if bf16 else 'f32')


class _Data:
    def __init__(self, case):
        B, (H, W), C_, R, bf16 = case
        rng = np.random.RandomState(1000 * C_ + 10 * B + H + int(bf16) + 3)
        q = C.round_bf16 if bf16 else (lambda a: a)
        mk = lambda: q(rng.standard_normal((B, H * W, C_)).astype(np.float32))      # noqa: E731
        self.B, self.P, self.C, self.bf16, self.shape, hid = B, H * W, C_, bf16, (B, H, W, C_), C_ // R
        self.x, self.x2, self.res, self.gy = q((mk() * 2 + 0.5).astype(np.float32)), mk(), mk(), mk()
        self.gamma, self.gamma2 = ((1 + 0.1 * rng.standard_normal(C_)).astype(np.float32) for _ in range(2))
        self.beta, self.beta2 = ((0.1 * rng.standard_normal(C_)).astype(np.float32) for _ in range(2))
        # gates spread over (0.1, 0.9): the output bias carries the spread, the hidden layer has units on both sides of its ReLU
        self.se = [a.astype(np.float32) for a in (
            rng.standard_normal((hid, C_)) * np.sqrt(2.0 / C_), 0.3 * rng.standard_normal(hid),
            rng.standard_normal((C_, hid)) * 0.5 / np.sqrt(hid), rng.uniform(-1.7, 1.7, C_))]
        self.st, self.s = _state(self.x, self.gamma, self.beta)
        self.st2, self.s2 = _state(self.x2, self.gamma2, self.beta2)
        # non-zero accumulators, so that `=` for `+=` cannot hide (tests/bn_cases.py: prefill)
        sizes = dict(ggamma=C_, gbeta=C_, gW1=(hid, C_), gb1=hid, gW2=(C_, hid), gb2=C_, ggamma2=C_, gbeta2=C_)
        self.pre = {k: ((1 + np.abs(rng.standard_normal(n))) * np.where(rng.random_sample(n) < 0.5, -1, 1)).astype(np.float32)
                    for k, n in sizes.items()}

    def dev4(self, a):
        return _t(a.reshape(self.shape), self.bf16)


def _run(d, mode):
    """the junction forward and backward on the device: (y, gate record, gx, gx2, the accumulators)"""
    W1, b1, W2, b2 = (dev(a) for a in d.se)
    x = d.dev4(d.x)
    gate = ops.se_excite(x, d.st, W1, b1, W2, b2)
    acc = {k: dev(v.copy()) for k, v in d.pre.items()}
    kw = {}
    if mode == 1:
        y = ops.bn_apply_gate(x, d.st, gate.s, residual=d.dev4(d.res))
    else:
        y = ops.bn_apply_gate(x, d.st, gate.s, x2=d.dev4(d.x2), st2=d.st2)
        kw = dict(x2=d.dev4(d.x2), st2=d.st2, gamma2=dev(d.gamma2), ggamma2=acc['ggamma2'], gbeta2=acc['gbeta2'])
    out = ops.bn_backward_gate(d.dev4(d.gy), y, gate, x, d.st, dev(d.gamma), acc['ggamma'], acc['gbeta'], W1, W2,
                               acc['gW1'], acc['gb1'], acc['gW2'], acc['gb2'], **kw)
    gx, gx2 = out if mode == 2 else (out, None)
    return y, gate, gx, gx2, acc


def _within(name, got, r32, r64):
    err, bound = np.abs(np.asarray(got, np.float64) - r64), D.tol(r32, r64)
    worst = float((err / bound).max())
    print('%s: worst error / bound %.3g (max error %.3g)' % (name, worst, float(err.max())))
    assert worst <= 1.0, name


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_forward_and_backward_against_the_reference(case, mode):
    d = _Data(case)
    y, gate, gx, gx2, acc = _run(d, mode)
    shape3 = (d.B, d.P, d.C)
    second, s2 = (d.res, None) if mode == 1 else (d.x2, d.s2)
    f64 = S.junction_fwd(d.x, d.s, d.se, second, s2)
    f32 = S.junction_fwd(d.x, d.s, d.se, second, s2, dtype=np.float32, bf16=d.bf16)
    # a condition on the inputs: no mask tie decides the case
    assert np.abs(f64['pre']).min() >= 1e-6 and np.abs(f64['a1']).min() >= 1e-6
    assert 0.1 < f64['s'].min() < 0.3 and 0.7 < f64['s'].max() < 0.9
    got = _np(y).reshape(shape3)
    assert y.dtype == (torch.bfloat16 if d.bf16 else torch.float32) and tuple(y.shape) == d.shape
    _within('s', _np(gate.s), f32['s'], f64['s'])
    _within('y', got, f32['out'], f64['out'])
    bits = y.relu_bits.cpu().numpy()
    assert bits.size == got.size // 4 and np.array_equal(bits, D.bits_of(got))
    # backward on the device's own mask
    mask = D.mask_of(bits, shape3)
    rkw = dict(x2=d.x2, st2=d.s2, gamma2=d.gamma2) if mode == 2 else {}
    b64 = S.junction_bwd(d.gy, mask, f64, d.x, d.s, d.se, d.gamma, d.pre, **rkw)
    b32 = S.junction_bwd(d.gy, mask, f32, d.x, d.s, d.se, d.gamma, d.pre, dtype=np.float32, bf16=d.bf16, **rkw)
    _within('gx', _np(gx).reshape(shape3), b32['gx'], b64['gx'])
    if mode == 2:
        _within('gx2', _np(gx2).reshape(shape3), b32['gx2'], b64['gx2'])
    for key in GRADS:
        if key in b64:
            _within(key, _np(acc[key]), b32[key], b64[key])
            assert not np.array_equal(_np(acc[key]), d.pre[key]), key
        else:
            assert np.array_equal(_np(acc[key]), d.pre[key]), key
    # no atomics: a second run gives the same bits
    again = _run(d, mode)
    for a, b in zip((y, gate.s, gx, gx2) + tuple(acc[k] for k in GRADS),
                    (again[0], again[1].s, again[2], again[3]) + tuple(again[4][k] for k in GRADS)):
        assert a is None or torch.equal(a, b)


def test_refusals_are_errors_not_fall_backs():
    from loans_amd._lib import HipKernelError
    x = _t(np.ones((2, 3, 3, 96), np.float32), False)           # 24 units per row: neither walk covers them
    with pytest.raises(HipKernelError, match='LOANS_EINVAL'):
        ops.se_squeeze(x)
    x = _t(np.ones((2, 3, 3, 64), np.float32), False)
    st = ops.BNState(64, x.device)
    with pytest.raises(HipKernelError, match='LOANS_EINVAL'):    # hidden width 2
        ops.se_excite(x, st, dev(np.ones((2, 64), np.float32)), dev(np.ones(2, np.float32)), dev(np.ones((64, 2), np.float32)),
                      dev(np.ones(64, np.float32)))
