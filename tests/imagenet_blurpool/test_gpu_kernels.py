"""-m gpu: csrc/blur.hip through ops.blur_pool / blur_pool_bn_backward / blur_pool_backward against torch.float64 on the CPU (reflect
padding, a depthwise binomial convolution at stride 2, BN with batch statistics and ReLU written out, autograd) within
max(5 |fp32 restatement - fp64|, 5e-4 |ref|, 1e-5); bf16: the reference on the bf16-rounded inputs, the restatement rounding what
the kernel stores.  A condition on the inputs: |scale x + shift| >= 1e-6 in the reference, so that no mask tie decides a case."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from loans_amd import ops
from oracle import chainer_ops as C
from tests.gpu_util import dev
from tests.imagenet_droppath.reference import tol
from tests.imagenet_droppath.test_gpu_kernels import _np, _state, _t

pytestmark = pytest.mark.gpu

CASES = [  # B, H, W, C, bf16
    (2, 2, 2, 64, False),           # the smallest legal map: every tap but the centre is a reflection
    (3, 3, 5, 64, False), (3, 3, 5, 64, True),      # odd sizes: top and bottom reflections land on the same row
    (2, 7, 6, 128, True),           # mixed parity
    (1, 14, 14, 2048, False),       # the widest channel count: a block walks channel chunks
    (2, 57, 31, 64, False), (2, 57, 31, 64, True),  # several tiles per sample in both directions, ragged last tiles
]


class _Data:
    def __init__(self, case):
        B, H, W, C_, bf16 = case
        rng = np.random.RandomState(1000 * C_ + 10 * B + H + int(bf16) + 7)
        q = C.round_bf16 if bf16 else (lambda a: a)
        self.shape, self.small, self.bf16 = (B, H, W, C_), (B, (H + 1) // 2, (W + 1) // 2, C_), bf16
        self.x = q((rng.standard_normal(self.shape) * 2 + 0.5).astype(np.float32))
        self.gy = q(rng.standard_normal(self.small).astype(np.float32))
        self.addend = q(rng.standard_normal(self.shape).astype(np.float32))
        self.gamma = (1 + 0.1 * rng.standard_normal(C_)).astype(np.float32)
        self.beta = (0.1 * rng.standard_normal(C_)).astype(np.float32)
        # non-zero accumulators, so that `=` for `+=` cannot hide
        self.pre = {k: ((1 + np.abs(rng.standard_normal(C_))) * np.where(rng.random_sample(C_) < 0.5, -1, 1)).astype(np.float32)
                    for k in ('ggamma', 'gbeta')}


def _blur(a):
    """NCHW: reflect padding of one, the depthwise 3 x 3 binomial filter at stride 2"""
    k = torch.tensor([1.0, 2.0, 1.0], dtype=a.dtype)
    k = (k[:, None] * k[None, :] / 16).expand(a.shape[1], 1, 3, 3)
    return F.conv2d(F.pad(a, (1, 1, 1, 1), mode='reflect'), k, stride=2, groups=a.shape[1])


def reference(d, fused, dtype):
    """dict(y, gx[, ggamma, gbeta, a]) as NHWC arrays in ``dtype``; float32 is the restatement (bf16: stored tensors rounded once)"""
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype)       # noqa: E731
    rnd = (lambda a: a.to(torch.bfloat16).to(dtype)) if d.bf16 and dtype == torch.float32 else (lambda a: a)
    x = t(d.x).requires_grad_()
    h = x.permute(0, 3, 1, 2)
    out = {}
    if fused:
        gamma, beta = t(d.gamma).requires_grad_(), t(d.beta).requires_grad_()
        mean, var = h.mean((0, 2, 3), keepdim=True), h.var((0, 2, 3), unbiased=False, keepdim=True)
        a = (h - mean) * torch.rsqrt(var + ops.BN_EPS) * gamma[None, :, None, None] + beta[None, :, None, None]
        h = torch.relu(a)
        out['a'] = a.detach().numpy()
    y = _blur(h).permute(0, 2, 3, 1)
    y.backward(t(d.gy))
    out['y'] = rnd(y.detach()).numpy()
    if fused:
        out.update(gx=rnd(x.grad).numpy(), ggamma=(t(d.pre['ggamma']) + gamma.grad).numpy(), gbeta=(t(d.pre['gbeta']) + beta.grad).numpy())
    else:
        out['gx'] = rnd(t(d.addend) + x.grad).numpy()
    return out


def _run(d, fused):
    x, gy = _t(d.x, d.bf16), _t(d.gy, d.bf16)
    if not fused:
        return dict(y=ops.blur_pool(x), gx=ops.blur_pool_backward(gy, d.shape, addend=_t(d.addend, d.bf16)))
    st, _ = _state(d.x.reshape(d.shape[0], -1, d.shape[-1]), d.gamma, d.beta)
    acc = {k: dev(v.copy()) for k, v in d.pre.items()}
    y = ops.blur_pool(x, st)
    gx = ops.blur_pool_bn_backward(gy, x, st, dev(d.gamma), acc['ggamma'], acc['gbeta'])
    return dict(y=y, gx=gx, **acc)


@pytest.mark.parametrize("fused", [True, False], ids=['bn_relu', 'plain'])
@pytest.mark.parametrize("case", CASES, ids=lambda c: '%dx%dx%dx%d-%s' % (c[:4] + ('bf16' if c[4] else 'f32',)))
def test_forward_and_backward_against_float64(case, fused):
    d = _Data(case)
    r64, r32 = reference(d, fused, torch.float64), reference(d, fused, torch.float32)
    assert not fused or np.abs(r64['a']).min() >= 1e-6          # the condition on the inputs
    got = _run(d, fused)
    assert got['y'].dtype == got['gx'].dtype == (torch.bfloat16 if d.bf16 else torch.float32)
    assert tuple(got['y'].shape) == d.small and tuple(got['gx'].shape) == d.shape
    for key, value in got.items():
        err, bound = np.abs(_np(value).astype(np.float64) - r64[key]), tol(r32[key], r64[key])
        print('%s: worst error / bound %.3g (max error %.3g)' % (key, float((err / bound).max()), float(err.max())))
        assert (err <= bound).all(), key
    again = _run(d, fused)          # no atomics: a second run gives the same bits
    assert all(torch.equal(v, again[k]) for k, v in got.items())
