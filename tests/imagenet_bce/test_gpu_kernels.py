"""-m gpu: the sigmoid binary cross-entropy (loans_amd/csrc/classify.hip, loans_sigmoid_bce_fwd_f32) through ``ops`` against
float64 NumPy, held to the bound tests/imagenet_bce/reference.py derives and the CPU test establishes on the fp32 restatement."""
import numpy as np
import pytest
import torch

import loans_amd
from loans_amd import ops
from loans_amd.functions import ops_small
from loans_amd.mixed_labels import MixedLabels
from tests.gpu_util import dev
from tests.imagenet import reference as R
from tests.imagenet_bce import reference as Q
from tests.imagenet_mix import reference as X

pytestmark = pytest.mark.gpu
K = 2


def _inside(got, ref, bounds, tag, limit=None, worst=None):
    out, gzd, rl, rh, rhk = got
    loss, acc, acck, gz, row_loss, hit, hitk = ref
    lb, gb, bb = bounds
    got_rows, got_gz = rl.cpu().numpy(), gzd.cpu().numpy()
    err = np.abs(got_rows.astype(np.float64) - row_loss)
    gerr = np.abs(got_gz.astype(np.float64) - gz)
    got_loss = float(out[0])
    assert np.all(err <= lb), tag + (float((err - lb).max()),)
    assert np.all(gerr <= gb), tag + (float((gerr - gb).max()),)
    assert abs(got_loss - loss) <= bb, tag + (got_loss, loss, bb)
    np.testing.assert_array_equal(rh.cpu().numpy(), hit.astype(np.float32), err_msg=str(tag))
    np.testing.assert_array_equal(rhk.cpu().numpy(), hitk.astype(np.float32), err_msg=str(tag))
    assert float(out[1]) == float(np.float32(acc)) and float(out[2]) == float(np.float32(acck)), tag
    valid = lb > 0
    # ignored rows are zero, exactly, and the denominator counts the others only (the bounds above are the reference's count's)
    assert not got_rows[~valid].any() and not got_gz[~valid].any(), tag
    if limit is not None:       # the extremes: finite, and no |gz| beyond fl(1 / denom)
        assert np.all(np.isfinite(got_rows)) and np.isfinite(got_loss) and np.all(np.abs(got_gz) <= np.float32(limit)), tag
    if not valid.any():
        assert got_loss == 0.0 and not rh.any() and not rhk.any(), tag
    elif worst is not None:
        worst['loss'] = max(worst['loss'], float((err[valid] / lb[valid]).max()))
        worst['gz'] = max(worst['gz'], float((gerr[valid] / gb[valid]).max()))
        worst['batch'] = max(worst['batch'], abs(got_loss - loss) / bb)


def _same(a, b, tag):
    for x, y in zip(a, b):
        assert torch.equal(x, y), tag


@pytest.mark.parametrize('thresh', Q.THRESH)
@pytest.mark.parametrize('eps', Q.BCE_EPS)
@pytest.mark.parametrize('B', Q.BCE_B)
@pytest.mark.parametrize('N', Q.BCE_N)
def test_bce_over_the_case_grid(N, B, eps, thresh):
    worst = {'loss': 0.0, 'gz': 0.0, 'batch': 0.0}
    seen = 0
    ignored = dev(np.full(B, -1, np.int32))
    for name, c, ta, tb, t, expect, extremes in Q.bce_cases(N, batches=(B,)):
        zd, tad, tbd = dev(c.z32), dev(ta), dev(tb)
        for lam in X.LAMS:
            wa, wb = X.weights(lam)
            assert not Q.threshold_ambiguous(N, ta, tb, wa, wb, eps, thresh)
            for sum_classes in (False, True):
                tag = (name, lam, eps, thresh, sum_classes)
                ref = Q.bce_ref(c, ta, tb, wa, wb, eps, K, thresh, sum_classes)
                bounds = Q.bce_bounds(c, ta, tb, wa, wb, eps, thresh, sum_classes)
                count = max(int((bounds[0] > 0).sum()), 1)
                got = ops.sigmoid_bce_fwd(zd, tad, tbd, wa, wb, eps, K, thresh, sum_classes)
                _inside(got, ref, bounds, tag, Q.gz_limit(count, N, sum_classes) if extremes else None, worst)
                _same(got, ops.sigmoid_bce_fwd(zd, tad, tbd, wa, wb, eps, K, thresh, sum_classes), tag)        # two launches, the same bits
                if wb == 0.0:       # the one-label call's bits, whatever the second array holds
                    one = ops.sigmoid_bce_fwd(zd, tad, None, 1.0, 0.0, eps, K, thresh, sum_classes)
                    _same(got, one, tag)
                    _same(ops.sigmoid_bce_fwd(zd, tad, ignored, wa, wb, eps, K, thresh, sum_classes), one, tag)
                if wa == 0.0:       # the one-label call on tb, whatever the first array holds
                    one = ops.sigmoid_bce_fwd(zd, tbd, None, 1.0, 0.0, eps, K, thresh, sum_classes)
                    _same(got, one, tag)
                    _same(ops.sigmoid_bce_fwd(zd, ignored, tbd, wa, wb, eps, K, thresh, sum_classes), one, tag)
                if expect is not None and np.array_equal(ta if wa >= wb else tb, t):
                    # the tie profile against the dominant label: the first of two equal maxima is the hit, the second is rank 1
                    valid = bounds[0] > 0
                    np.testing.assert_array_equal(got[3].cpu().numpy() != 0, expect & valid, err_msg=str(tag))
                    np.testing.assert_array_equal(got[4].cpu().numpy() != 0, valid, err_msg=str(tag))
                seen += 1
    assert seen == Q.profiles(N) * len(X.PAIRS) * len(X.LAMS) * 2
    print('N=%d B=%d eps=%g thresh=%s worst error / bound: row loss %.3f, gz %.3f, batch loss %.3f'
          % (N, B, eps, thresh, worst['loss'], worst['gz'], worst['batch']))


def test_bce_at_the_lds_limit():
    c, ta, tb = Q.lds_limit_case()
    zd, tad, tbd = dev(c.z32), dev(ta), dev(tb)
    wa, wb = X.weights(np.float32(0.3))
    for thresh in Q.THRESH:
        for sum_classes in (False, True):
            got = ops.sigmoid_bce_fwd(zd, tad, tbd, wa, wb, 0.1, K, thresh, sum_classes)
            _inside(got, Q.bce_ref(c, ta, tb, wa, wb, 0.1, K, thresh, sum_classes),
                    Q.bce_bounds(c, ta, tb, wa, wb, 0.1, thresh, sum_classes), ('lds', thresh, sum_classes))
    with pytest.raises(loans_amd._lib.HipKernelError):
        ops.sigmoid_bce_fwd(torch.zeros(2, 8193, device='cuda'), tad, tbd, wa, wb, 0.1, K)


def test_the_function_with_its_backward_on_plain_and_mixed_labels():
    N, B = 257, 5
    name, c, ta, tb, t, _, _ = next(x for x in Q.bce_cases(N, batches=(B,)) if x[0].startswith('normal') and x[0].endswith('different'))
    zd = dev(c.z32)
    mixed = MixedLabels(dev(ta), dev(tb), 0.3)
    assert (mixed.lam32, mixed.oml32) == X.weights(0.3)
    for labels, args in ((mixed, (ta, tb) + X.weights(0.3)), (dev(ta), (ta, ta, 1.0, 0.0)), (ta, (ta, ta, 1.0, 0.0))):
        for thresh, sum_classes in ((None, False), (0.2, False), (0.2, True)):
            ref = Q.bce_ref(c, *args, 0.1, K, thresh, sum_classes)
            lb, gb, bb = Q.bce_bounds(c, *args, 0.1, thresh, sum_classes)
            for g in (1.0, 0.5):
                zv = loans_amd.Variable(zd)
                lv, av, akv = ops_small.sigmoid_binary_cross_entropy(zv, labels, label_smoothing=0.1, topk=K, target_threshold=thresh,
                                                                     sum_classes=sum_classes)
                assert abs(float(lv.data) - ref[0]) <= bb
                assert float(av.data) == float(np.float32(ref[1])) and float(akv.data) == float(np.float32(ref[2]))
                gz = ops.sigmoid_bce_fwd(zd, dev(args[0]), dev(args[1]), args[2], args[3], 0.1, K, thresh, sum_classes)[1]
                lv.grad = torch.full((), g, device='cuda')
                lv.backward()
                got = zv.grad.cpu().numpy().astype(np.float64)
                # the stored gz times the upstream gradient: one rounding (none at 0.5, short of the subnormals)
                want = gz.cpu().numpy().astype(np.float64) * g
                assert np.all(np.abs(got - want) <= R.U * np.abs(want) + Q.TINY)
                assert np.all(np.abs(got - ref[3] * g) <= gb * g + R.U * np.abs(ref[3] * g) * R.SLACK + Q.TINY)
    with pytest.raises(AssertionError):
        ops.sigmoid_bce_fwd(zd, dev(ta), dev(tb)[:3], 0.5, 0.5, 0.0, 1)
    with pytest.raises(loans_amd._lib.HipKernelError):
        ops.sigmoid_bce_fwd(zd, dev(ta), dev(tb), 0.5, 0.5, 0.0, 1, thresh=1.0)
