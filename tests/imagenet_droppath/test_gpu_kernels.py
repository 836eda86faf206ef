"""-m gpu: ``ops.bn_apply_rows`` / ``ops.bn_backward_rows`` (csrc/bn_pool.hip: loans_bn_*_rows_*) against the float64 junction of
tests/imagenet_droppath/reference.py, within max(5 |fp32 restatement - fp64|, 5e-4 |ref|, 1e-5); bf16 tensors against the same
reference on the bf16-rounded inputs, the restatement rounding what the kernel stores.

Shapes: 5 x (7 x 5) at 64 and 2048 channels (2048 in fp32 is the channel count the 16-byte-unit layout does not tile; 64 x 35
units per sample are no multiple of 256: sample boundaries fall inside a block's slab), 3 x (9 x 9) at 128 bf16 / 1024 fp32 with
all samples kept and all dropped, 2 x (56 x 56) at 64 channels (a sample spans many blocks, the unrolled slab loop runs)."""
import numpy as np
import pytest
import torch

from loans_amd import ops
from oracle import chainer_ops as C
from tests.gpu_util import dev
from tests.imagenet_droppath import reference as D

pytestmark = pytest.mark.gpu
KEEP = float(D.keep_factor(0.3))

CASES = [  # B, positions (H, W), C, bf16, keep pattern
    (5, (7, 5), 64, False, (1, 0, 1, 1, 0)), (5, (7, 5), 64, True, (1, 0, 1, 1, 0)),
    (5, (7, 5), 2048, False, (1, 0, 1, 1, 0)), (5, (7, 5), 2048, True, (1, 0, 1, 1, 0)),
    (3, (9, 9), 128, True, (1, 1, 1)), (3, (9, 9), 128, True, (0, 0, 0)), (3, (9, 9), 128, True, (0, 1, 0)),
    (3, (9, 9), 1024, False, (1, 1, 1)), (3, (9, 9), 1024, False, (0, 0, 0)), (3, (9, 9), 1024, False, (1, 0, 1)),
    (2, (56, 56), 64, False, (0, 1)), (2, (56, 56), 64, True, (0, 1)),
]


def _id(case):
    B, (H, W), C_, bf16, keep = case
    return '%dx%dx%d-C%d-%s-%s' % (B, H, W, C_, 'bf16' if bf16 else 'f32', ''.join(map(str, keep)))


def _t(a, bf16):
    t = dev(np.ascontiguousarray(a, dtype=np.float32))
    return t.to(torch.bfloat16).contiguous() if bf16 else t


def _np(t):
    return t.detach().float().cpu().numpy()


def _state(a, gamma, beta):
    """the BN state of the [B][P][C] tensor ``a`` from ops.bn_finalize, and its fp32 vectors as the reference's exact inputs"""
    C_ = a.shape[-1]
    flat = torch.from_numpy(a.reshape(-1, C_).astype(np.float64)).cuda()
    stats = torch.zeros((ops.STATS_REPLICAS, 2, C_), device='cuda', dtype=torch.float64)
    stats[0, 0], stats[0, 1] = flat.sum(0), (flat * flat).sum(0)
    st = ops.bn_finalize(stats, flat.shape[0], dev(gamma), dev(beta), dev(np.zeros(C_, np.float32)), dev(np.ones(C_, np.float32)))
    return st, {k: _np(getattr(st, k)) for k in ('mean', 'rstd', 'scale', 'shift')}


class _Data:
    def __init__(self, case):
        B, (H, W), C_, bf16, keep = case
        rng = np.random.RandomState(1000 * C_ + 10 * B + H + int(bf16))
        q = C.round_bf16 if bf16 else (lambda a: a)
        mk = lambda: q(rng.standard_normal((B, H * W, C_)).astype(np.float32))      # noqa: E731
        self.B, self.P, self.C, self.bf16, self.shape = B, H * W, C_, bf16, (B, H, W, C_)
        self.x, self.x2, self.res, self.gy = mk() * 2 + 0.5, mk(), mk(), mk()
        self.x = q(self.x.astype(np.float32))
        self.r = (np.array(keep, np.float32) * np.float32(KEEP)).astype(np.float32)
        self.gamma, self.gamma2 = ((1 + 0.1 * rng.standard_normal(C_)).astype(np.float32) for _ in range(2))
        self.beta, self.beta2 = ((0.1 * rng.standard_normal(C_)).astype(np.float32) for _ in range(2))
        self.st, self.s = _state(self.x, self.gamma, self.beta)
        self.st2, self.s2 = _state(self.x2, self.gamma2, self.beta2)
        # non-zero accumulators of the gradients' own size, so that `=` for `+=` cannot hide (tests/bn_cases.py: prefill)
        m = B * H * W
        self.pre = [((1 + np.abs(rng.standard_normal(C_))) * np.sqrt(m) * np.where(rng.random_sample(C_) < 0.5, -1, 1)).astype(np.float32)
                    for _ in range(4)]

    def dev4(self, a):
        return _t(a.reshape(self.shape), self.bf16)


def _forward(d, mode, r=None):
    r = d.r if r is None else r
    if mode == 1:
        return ops.bn_apply_rows(d.dev4(d.x), d.st, dev(r), residual=d.dev4(d.res))
    return ops.bn_apply_rows(d.dev4(d.x), d.st, dev(r), x2=d.dev4(d.x2), st2=d.st2)


def _within(name, got, r32, r64):
    err, bound = np.abs(np.asarray(got, np.float64) - r64), D.tol(r32, r64)
    worst = float((err / bound).max())
    print('%s: worst error / bound %.3g (max error %.3g)' % (name, worst, float(err.max())))
    assert worst <= 1.0, name


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_forward_and_backward_against_the_reference(case, mode):
    d = _Data(case)
    y = _forward(d, mode)
    got = _np(y).reshape(d.B, d.P, d.C)
    assert y.dtype == (torch.bfloat16 if d.bf16 else torch.float32) and tuple(y.shape) == d.shape
    second, s2 = (d.res, None) if mode == 1 else (d.x2, d.s2)
    r64 = D.junction_fwd(d.x, d.s, d.r, second, s2)
    r32 = D.junction_fwd(d.x, d.s, d.r, second, s2, dtype=np.float32, bf16=d.bf16)
    _within('forward', got, r32, r64)
    # exact properties: the bits are the device output's signs; a dropped sample of mode 1 is relu(residual) to the bit
    bits = y.relu_bits.cpu().numpy()
    assert bits.dtype == np.uint8 and bits.size == got.size // 4 and np.array_equal(bits, D.bits_of(got))
    if mode == 1:
        dropped = np.flatnonzero(d.r == 0)
        want = torch.relu(d.dev4(d.res))
        for b in dropped:
            assert torch.equal(y[b], want[b]), 'dropped sample %d is not relu(residual)' % b
    # backward on the device's own mask
    mask = D.mask_of(bits, got.shape)
    gg, gb, gg2, gb2 = (dev(p.copy()) for p in d.pre)
    kw, rkw = {}, {}
    if mode == 2:
        kw = dict(x2=d.dev4(d.x2), st2=d.st2, gamma2=dev(d.gamma2), ggamma2=gg2, gbeta2=gb2)
        rkw = dict(x2=d.x2, st2=d.s2, gamma2=d.gamma2, gg20=d.pre[2], gb20=d.pre[3])
    out = ops.bn_backward_rows(d.dev4(d.gy), y, dev(d.r), d.dev4(d.x), d.st, dev(d.gamma), gg, gb, **kw)
    b64 = D.junction_bwd(d.gy, mask, d.r, d.x, d.s, d.gamma, d.pre[0], d.pre[1], **rkw)
    b32 = D.junction_bwd(d.gy, mask, d.r, d.x, d.s, d.gamma, d.pre[0], d.pre[1], dtype=np.float32, bf16=d.bf16, **rkw)
    gx = out[0] if mode == 2 else out
    _within('gx', _np(gx).reshape(got.shape), b32['gx'], b64['gx'])
    _within('ggamma', _np(gg), b32['ggamma'], b64['ggamma'])
    _within('gbeta', _np(gb), b32['gbeta'], b64['gbeta'])
    assert not np.array_equal(_np(gg), d.pre[0]) or not d.r.any()
    if mode == 2:
        _within('gx2', _np(out[1]).reshape(got.shape), b32['gx2'], b64['gx2'])
        _within('ggamma2', _np(gg2), b32['ggamma2'], b64['ggamma2'])
        _within('gbeta2', _np(gb2), b32['gbeta2'], b64['gbeta2'])
    else:
        assert np.array_equal(_np(gg2), d.pre[2]) and np.array_equal(_np(gb2), d.pre[3])


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("case", [CASES[0], CASES[1], CASES[2], CASES[4], CASES[7], CASES[10]], ids=_id)
def test_all_ones_is_the_existing_junction_within_the_bound(case, mode):
    """r = 1 for every sample: the forward differs from ops.bn_apply's and the backward from ops.bn_backward's by no more than
    the bound (not bit for bit: the two kernels may contract their multiply-adds differently)"""
    d = _Data(case)
    ones = np.ones(d.B, np.float32)
    y = _forward(d, mode, ones)
    if mode == 1:
        y0 = ops.bn_apply(d.dev4(d.x), d.st, relu=True, residual=d.dev4(d.res), want_bits=True)
        second, s2 = d.res, None
    else:
        y0 = ops.bn_apply(d.dev4(d.x), d.st, relu=True, x2=d.dev4(d.x2), st2=d.st2, want_bits=True)
        second, s2 = d.x2, d.s2
    shape3 = (d.B, d.P, d.C)
    r64 = D.junction_fwd(d.x, d.s, ones, second, s2)
    r32 = D.junction_fwd(d.x, d.s, ones, second, s2, dtype=np.float32, bf16=d.bf16)
    bound = D.tol(r32, r64)
    assert (np.abs(_np(y).astype(np.float64) - _np(y0)).reshape(shape3) <= bound).all()
    y0.relu_bits = y.relu_bits          # one mask for both backward passes: the comparison is of the passes
    mask = D.mask_of(y.relu_bits.cpu().numpy(), shape3)
    acc = [[dev(p.copy()) for p in d.pre] for _ in range(2)]
    kws = [{}, {}]
    rkw = {}
    if mode == 2:
        kws = [dict(x2=d.dev4(d.x2), st2=d.st2, gamma2=dev(d.gamma2), ggamma2=a[2], gbeta2=a[3]) for a in acc]
        rkw = dict(x2=d.x2, st2=d.s2, gamma2=d.gamma2, gg20=d.pre[2], gb20=d.pre[3])
    got = ops.bn_backward_rows(d.dev4(d.gy), y, dev(ones), d.dev4(d.x), d.st, dev(d.gamma), acc[0][0], acc[0][1], **kws[0])
    old = ops.bn_backward(d.dev4(d.gy), y0, d.dev4(d.x), d.st, dev(d.gamma), acc[1][0], acc[1][1], **kws[1])
    b64 = D.junction_bwd(d.gy, mask, ones, d.x, d.s, d.gamma, d.pre[0], d.pre[1], **rkw)
    b32 = D.junction_bwd(d.gy, mask, ones, d.x, d.s, d.gamma, d.pre[0], d.pre[1], dtype=np.float32, bf16=d.bf16, **rkw)
    pairs = [('gx', got[0] if mode == 2 else got, old[0] if mode == 2 else old), ('ggamma', acc[0][0], acc[1][0]),
             ('gbeta', acc[0][1], acc[1][1])]
    if mode == 2:
        pairs += [('gx2', got[1], old[1]), ('ggamma2', acc[0][2], acc[1][2]), ('gbeta2', acc[0][3], acc[1][3])]
    for name, a, b in pairs:
        diff = np.abs(_np(a).astype(np.float64) - _np(b)).reshape(b64[name].shape)
        assert (diff <= D.tol(b32[name], b64[name])).all(), name


def test_channel_counts_of_the_models_and_refusals():
    """every channel count of the models, in both storage types, goes through (known answers: a dropped sample is its residual,
    a kept one 3 (1 - 2) + 1 < 0); a count neither walk covers is an error, not a fall-back"""
    from loans_amd._lib import HipKernelError
    for bf16 in (False, True):
        for C_ in (64, 128, 256, 512, 1024, 2048):
            x = _t(np.ones((2, 3, 3, C_), np.float32), bf16)
            st = ops.BNState(C_, x.device)
            st.scale.fill_(1.0), st.shift.fill_(-2.0)
            y = ops.bn_apply_rows(x, st, dev(np.array([0.0, 3.0], np.float32)), residual=x)
            assert torch.equal(y[0].float(), torch.ones_like(y[0].float())) and torch.equal(y[1].float(), torch.zeros_like(y[1].float()))
            assert int(y.relu_bits[:9 * C_ // 4].min()) == 15 and int(y.relu_bits[9 * C_ // 4:].max()) == 0
    x = _t(np.ones((2, 3, 3, 96), np.float32), False)
    st = ops.BNState(96, x.device)
    with pytest.raises(HipKernelError, match='LOANS_EINVAL'):
        ops.bn_apply_rows(x, st, dev(np.ones(2, np.float32)), residual=x)
