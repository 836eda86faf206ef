"""-m gpu: the distillation loss (loans_amd/csrc/classify.hip, loans_softmax_distill_fwd_f32) through ``ops`` against float64 NumPy,
held to the bound tests/imagenet_distill/reference.py derives and the CPU test establishes on the fp32 restatement.  The two halves
of a case's reference (``Hard``: student, labels, weights, eps; ``Soft``: student, teacher, T) are computed once on the host and kept
on the device in float64; ``D.combine`` joins them there per alpha, so a case costs a launch and a handful of small device ops."""
import types

import numpy as np
import pytest
import torch

import loans_amd
from loans_amd import _lib, ops
from loans_amd.functions import ops_small
from loans_amd.mixed_labels import MixedLabels
from tests.gpu_util import dev
from tests.imagenet import reference as R
from tests.imagenet_distill import reference as D
from tests.imagenet_mix import reference as X

pytestmark = pytest.mark.gpu
K = 2
NAMES = ('row_loss', 'row_kl', 'gz', 'batch')


def _dev64(obj, names):
    return types.SimpleNamespace(**{n: torch.from_numpy(np.ascontiguousarray(getattr(obj, n), np.float64)).cuda() for n in names})


def hard_on_device(hard):
    d = _dev64(hard, ('v', 'loss', 'E_loss', 'h', 'E_h'))
    d.count, d.valid = hard.count, hard.valid
    return d


def soft_on_device(soft):
    assert np.all(np.isfinite(soft.kl)) and np.all(np.isfinite(soft.f))
    return _dev64(soft, ('f', 'E_f', 'kl', 'E_kl'))


def _ratio(got, want, bound):
    """max |got - want| / bound; where the bound is zero (a row that does not count) anything but the exact value is 'infinite'"""
    err = (got.double() - want).abs()
    return (err / torch.where(bound > 0, bound, torch.full_like(bound, 1e-300))).max()


def ratios(got, ref):
    """the four worst error / bound ratios of a launch against the device reference, a (4,) device tensor: NAMES"""
    out, gz, rl, _, _, rkl, _ = got
    batch = torch.maximum(_ratio(out[0], ref['loss'], ref['bb']), _ratio(out[3], ref['kl'], ref['bkl']))
    return torch.stack([_ratio(rl, ref['row_loss'], ref['lb']), _ratio(rkl, ref['row_kl'], ref['kb']), _ratio(gz, ref['gz'], ref['gb']), batch])


def _same(a, b, tag):
    for x, y in zip(a, b):
        assert torch.equal(x, y), tag


def _hit_tensors(hard, soft):
    return [dev(x.astype(np.float32)) for x in D.hits(hard, soft)]


_built = {}


def _pupils(N, B):
    """every student of (N, B) with its ``Hard`` halves on the device: built once per (N, B), kept until the next one"""
    if _built.get('key') != (N, B):
        _built.clear()
        pupils = []
        for sname, c, t, expect in D.students(N, B):
            hards = []
            for kind in X.PAIRS:
                ta, tb = X.label_pair(kind, t, N)
                tad, tbd = dev(ta), dev(tb)
                for lam in X.LAMS:
                    wa, wb = X.weights(lam)
                    for eps in D.DISTILL_EPS:
                        hard = D.Hard(c, ta, tb, wa, wb, eps, K)
                        hards.append(((kind, lam, eps), hard, hard_on_device(hard), tad, tbd, wa, wb, eps))
            pupils.append((sname, c, dev(c.z32), t, expect, hards))
        _built.update(key=(N, B), pupils=pupils, masters=[(tname, ct, dev(ct.z32)) for tname, ct in D.teachers(N, B)])
    return _built['pupils'], _built['masters']


@pytest.mark.parametrize('T', D.TEMPERATURES)
@pytest.mark.parametrize('B', D.DISTILL_B)
@pytest.mark.parametrize('N', D.DISTILL_N)
def test_distill_over_the_case_grid(N, B, T):
    """one case per (N, B), cut in three along the temperature to keep each short"""
    worst = torch.zeros(4, dtype=torch.float64, device='cuda')
    ignored = dev(np.full(B, -1, np.int32))
    garbage = torch.full((B, N), float('nan'), device='cuda')
    pupils, masters = _pupils(N, B)
    first = T == D.TEMPERATURES[0]
    seen = 0
    for sname, c, zd, t, expect, hards in pupils:
        for key, hard, hardd, tad, tbd, wa, wb, eps in hards if first else ():
            # alpha == 0: the mix entry's bits, the teacher not read (None, or NaNs), zeros for the teacher's outputs
            mix = ops.softmax_xent_mix_fwd(zd, tad, tbd, wa, wb, eps, K)
            for zt in (None, garbage):
                zero = ops.softmax_distill_fwd(zd, zt, tad, tbd, wa, wb, eps, K, 0.0, 4.0)
                assert torch.equal(zero[0][:3], mix[0]) and not zero[0][3:].any(), (sname,) + key
                _same(zero[1:5], mix[1:], (sname,) + key)
                assert not zero[5].any() and not zero[6].any()
        for tname, ct, ztd in masters:
            soft = D.Soft(c, ct, T)
            softd = soft_on_device(soft)
            here = torch.zeros(4, dtype=torch.float64, device='cuda')
            flags = torch.zeros((), dtype=torch.int64, device='cuda')
            for key, hard, hardd, tad, tbd, wa, wb, eps in hards:
                hit, hitk, thit = _hit_tensors(hard, soft)
                want = torch.stack([hit.sum() / B, hitk.sum() / B, thit.sum() / B])
                for alpha in D.ALPHAS:
                    got = ops.softmax_distill_fwd(zd, ztd, tad, tbd, wa, wb, eps, K, alpha, T)
                    here = torch.maximum(here, torch.nan_to_num(ratios(got, D.combine(hardd, softd, alpha, T)), nan=float('inf')))
                    # hits are exact, and so are the accuracies: sums of 0 / 1 in fp32, one division
                    flags += (got[3] != hit).sum() + (got[4] != hitk).sum() + (got[6] != thit).sum() + (got[0][[1, 2, 4]] != want).sum()
                    seen += 1
                # two launches, the same bits (the last alpha's)
                _same(got, ops.softmax_distill_fwd(zd, ztd, tad, tbd, wa, wb, eps, K, alpha, T), (sname, tname, T) + key)
                if first:
                    # the one-label weights: the array of weight zero is not read and does not decide which rows count
                    if wb == 0.0:
                        _same(got, ops.softmax_distill_fwd(zd, ztd, tad, tad, wa, wb, eps, K, alpha, T), key)
                        _same(got, ops.softmax_distill_fwd(zd, ztd, tad, ignored, wa, wb, eps, K, alpha, T), key)
                    if wa == 0.0:
                        _same(got, ops.softmax_distill_fwd(zd, ztd, tbd, tbd, wa, wb, eps, K, alpha, T), key)
                        _same(got, ops.softmax_distill_fwd(zd, ztd, ignored, tbd, wa, wb, eps, K, alpha, T), key)
                    if not hard.valid.all():       # rows that do not count: zeros, exactly, in every per-row output
                        dead = dev(~hard.valid)
                        assert not any(x[dead].any() for x in got[1:]), key
                    if expect is not None and np.array_equal(_dominant(hard, X.label_pair(key[0], t, N), wa, wb), t):
                        np.testing.assert_array_equal(got[3].cpu().numpy() != 0, expect & hard.valid, err_msg=str(key))
            assert int(flags) == 0, (sname, tname, T)
            assert bool((here < 1.0).all()), (sname, tname, T, dict(zip(NAMES, here.tolist())))
            worst = torch.maximum(worst, here)
    assert seen == D.profiles(N) ** 2 * len(X.PAIRS) * len(X.LAMS) * len(D.DISTILL_EPS) * len(D.ALPHAS)
    worst = worst.tolist()
    assert max(worst) < 1.0
    print('N=%d B=%d T=%g worst error / bound: row loss %.3f, row kl %.3f, gz %.3f, batch %.3f' % ((N, B, T) + tuple(worst)))


def _dominant(hard, pair, wa, wb):
    return pair[0] if wa >= wb else pair[1]


def test_distill_at_the_lds_limit():
    c, ct, ta, tb = D.lds_limit_case()
    zd, ztd, tad, tbd = dev(c.z32), dev(ct.z32), dev(ta), dev(tb)
    wa, wb = X.weights(np.float32(0.3))
    hard = D.Hard(c, ta, tb, wa, wb, 0.1, K)
    hardd = hard_on_device(hard)
    worst = torch.zeros(4, dtype=torch.float64, device='cuda')
    for T in D.TEMPERATURES:
        soft = D.Soft(c, ct, T)
        softd = soft_on_device(soft)
        for alpha in D.ALPHAS:
            got = ops.softmax_distill_fwd(zd, ztd, tad, tbd, wa, wb, 0.1, K, alpha, T)
            worst = torch.maximum(worst, torch.nan_to_num(ratios(got, D.combine(hardd, softd, alpha, T)), nan=float('inf')))
            for x, want in zip((got[3], got[4], got[6]), D.hits(hard, soft)):
                np.testing.assert_array_equal(x.cpu().numpy(), want.astype(np.float32))
    print('N=8192 worst error / bound: row loss %.3f, row kl %.3f, gz %.3f, batch %.3f' % tuple(worst.tolist()))
    assert float(worst.max()) < 1.0
    with pytest.raises(_lib.HipKernelError):
        ops.softmax_distill_fwd(torch.zeros(2, 8193, device='cuda'), torch.zeros(2, 8193, device='cuda'), tad, tbd, wa, wb, 0.1, K, 0.5, 1.0)


def test_every_refused_argument_returns_its_error_and_launches_nothing():
    B, N = 4, 8
    f = _lib.load().loans_softmax_distill_fwd_f32
    z = torch.randn(B, N, device='cuda')
    zt = torch.randn(B, N, device='cuda')
    ta = torch.zeros(B, dtype=torch.int32, device='cuda')
    outs = [torch.full((B, N), 7.0, device='cuda')] + [torch.full((B,), 7.0, device='cuda') for _ in range(5)] + [torch.full((5,), 7.0, device='cuda')]
    stream = torch.cuda.current_stream().cuda_stream
    inf, nan = float('inf'), float('nan')

    def call(zt_ptr=zt.data_ptr(), lam=0.5, oml=0.5, B=B, N=N, eps=0.1, k=1, alpha=0.5, T=1.0, drop=None):
        ptrs = [x.data_ptr() for x in outs]
        if drop is not None:
            ptrs[drop] = 0
        return f(z.data_ptr(), zt_ptr, ta.data_ptr(), ta.data_ptr(), lam, oml, *ptrs, B, N, eps, k, alpha, T, stream)

    assert call(zt_ptr=0) == -1 and call(zt_ptr=0, alpha=1.0) == -1
    for drop in range(7):
        assert call(drop=drop) == -1 and call(drop=drop, alpha=0.0) == -1
    for kw in (dict(alpha=-0.1), dict(alpha=1.5), dict(alpha=nan), dict(alpha=inf), dict(T=0.0), dict(T=2.0 ** -7), dict(T=65.0), dict(T=nan),
               dict(T=inf), dict(T=-1.0), dict(lam=nan), dict(oml=inf), dict(eps=1.0), dict(eps=-0.1), dict(eps=nan), dict(k=0), dict(B=0),
               dict(N=0), dict(B=-1)):
        assert call(**kw) == -1, kw
        if 'alpha' not in kw:
            assert call(alpha=0.0, **kw) == -1, kw
    assert call(N=8193) == -2 and call(B=65537) == -2 and call(N=8193, alpha=0.0) == -2
    torch.cuda.synchronize()
    assert all(bool((x == 7.0).all()) for x in outs)
    # ... and the limits themselves are taken
    assert call(T=2.0 ** -6) == 0 and call(T=64.0) == 0 and call(alpha=1.0) == 0 and call(zt_ptr=0, alpha=0.0) == 0
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(x).all()) for x in outs)
    with pytest.raises(AssertionError):
        ops.softmax_distill_fwd(z, zt[:, :4].contiguous(), ta, ta, 0.5, 0.5, 0.0, 1, 0.5, 1.0)
    with pytest.raises(_lib.HipKernelError):
        ops.softmax_distill_fwd(z, None, ta, ta, 0.5, 0.5, 0.0, 1, 0.5, 1.0)


def test_the_function_with_its_backward_on_plain_and_mixed_labels():
    N, B = 257, 5
    _, c, t, _ = next(x for x in D.students(N, B) if x[0] == 'normal')
    ct = next(x for x in D.teachers(N, B) if x[0] == 'dominant')[1]
    ta, tb = X.label_pair('different', t, N)
    zd, ztd = dev(c.z32), dev(ct.z32)
    mixed = MixedLabels(dev(ta), dev(tb), 0.3)
    assert (mixed.lam32, mixed.oml32) == X.weights(0.3)
    for labels, args in ((mixed, (ta, tb) + X.weights(0.3)), (dev(ta), (ta, ta, 1.0, 0.0)), (ta, (ta, ta, 1.0, 0.0))):
        for alpha, T in ((0.5, 4.0), (1.0, 0.5)):
            ref = D.distill_ref(c, ct, *args, 0.1, K, alpha, T)
            for g in (1.0, 0.5):
                zv, ztv = loans_amd.Variable(zd), loans_amd.Variable(ztd)           # a teacher Variable that would take a gradient
                lv, av, akv, dv, tv = ops_small.softmax_cross_entropy_distilled(zv, ztv, labels, label_smoothing=0.1, topk=K, alpha=alpha,
                                                                                temperature=T)
                assert abs(float(lv.data) - ref['loss']) <= ref['bb'] and abs(float(dv.data) - ref['distill_loss']) <= ref['bkl']
                assert float(av.data) == float(np.float32(ref['accuracy'])) and float(akv.data) == float(np.float32(ref['accuracy_topk']))
                assert float(tv.data) == float(np.float32(ref['teacher_accuracy']))
                gz = ops.softmax_distill_fwd(zd, ztd, dev(args[0]), dev(args[1]), args[2], args[3], 0.1, K, alpha, T)[1]
                lv.grad = torch.full((), g, device='cuda')
                lv.backward()
                assert ztv.grad is None                                             # the teacher's logits are a constant
                got = zv.grad.cpu().numpy().astype(np.float64)
                # the stored gz times the upstream gradient: one rounding (none at 0.5, short of the subnormals)
                want = gz.cpu().numpy().astype(np.float64) * g
                assert np.all(np.abs(got - want) <= R.U * np.abs(want) + D.TINY)
                assert np.all(np.abs(got - ref['gz'] * g) <= ref['gb'] * g + R.U * np.abs(ref['gz'] * g) * R.SLACK + D.TINY)
    with pytest.raises(ValueError):
        ops_small.softmax_cross_entropy_distilled(loans_amd.Variable(zd), ztd, dev(ta), alpha=1.5)
