"""-m gpu: the evaluation-mode softmax cross-entropy (loans_softmax_xent_eval_f32, loans_amd/csrc/classify.hip) through ``ops``
against the float64 reference of tests/imagenet_sgd/reference.py over its whole case grid: counts exactly, the loss sum within
the derived per-row bounds, the accumulator as a running sum, and nothing else touched."""
import numpy as np
import pytest
import torch

from loans_amd import _lib, ops
from tests.gpu_util import dev
from tests.imagenet import reference as R
from tests.imagenet_sgd import reference as S

pytestmark = pytest.mark.gpu

SENTINELS = (-7.25, 1e300, float('inf'))


def _fresh():
    """five zeroed sums and three sentinel doubles behind them"""
    return torch.tensor((0.0,) * 5 + SENTINELS, dtype=torch.float64, device='cuda')


def _single(z, t, k):
    acc = _fresh()
    ops.softmax_xent_eval(dev(z), dev(t), acc, k)
    return acc


@pytest.mark.parametrize("N", R.XENT_N)
def test_eval_sums_over_the_case_grid(N):
    worst, cases = 0.0, 0
    for name, z, t in S.ls_cases(N):
        assert R.argmax_margin_ok(z) and S.rank_margin_ok(z, t), name
        B = len(t)
        valid = (t >= 0) & (t < N)
        lb = S.ls_bounds(z, t, 0)[0]
        zd, td = dev(z), dev(t)
        z0, t0 = zd.clone(), td.clone()
        for k in S.TOPK:                                    # 5 > N at the small sizes: every valid row hits
            _, _, _, _, row_loss, hit, hitk = S.softmax_xent_ls_ref(z, t, 0, k)
            acc = _fresh()
            ops.softmax_xent_eval(zd, td, acc, k)
            again = _fresh()
            ops.softmax_xent_eval(zd, td, again, k)
            assert torch.equal(acc, again), (name, k)                                    # two runs, the same bits
            got = acc.cpu().numpy()
            assert got[1] == hit.sum() and got[2] == hitk.sum() and got[3] == valid.sum() and got[4] == B, (name, k, got[:5])
            bound = lb.sum() * (1 + 1e-6)
            err = abs(got[0] - row_loss.sum())
            assert err <= bound, (name, k, got[0], row_loss.sum(), bound)
            assert tuple(got[5:]) == SENTINELS, (name, k)                               # nothing behind acc[4] is written
            if not valid.any():
                assert tuple(got[:4]) == (0.0, 0.0, 0.0, 0.0), (name, k)                # an all-ignored batch counts its rows only
            elif bound > 0:
                worst = max(worst, err / bound)
            if k == 1:
                assert got[1] == got[2], name
        assert torch.equal(zd, z0) and torch.equal(td, t0), name                         # the inputs are read only
        cases += 1
    assert cases >= 60
    print('N=%d: %d cases, worst loss-sum error / bound %.3f' % (N, cases, worst))


def test_accumulator_is_a_running_sum_in_a_fixed_order():
    picks = []
    for N, want in ((1000, 'normal-first_last-B257'), (65, 'pm80-third_ignored-B5'), (2, 'dominant-one_out_of_range-B64')):
        picks.append(next((z, t) for name, z, t in S.ls_cases(N) if name.startswith(want)))
    singles = [_single(z, t, 2) for z, t in picks]
    assert len({float(s[0]) for s in singles}) == 3 and all(float(s[3]) > 0 for s in singles)
    acc = _fresh()
    for z, t in picks:
        ops.softmax_xent_eval(dev(z), dev(t), acc, 2)
    want = torch.zeros(5, dtype=torch.float64)
    for s in singles:
        want = want + s[:5].cpu()                          # ((0 + S1) + S2) + S3 in double
    assert torch.equal(acc[:5].cpu(), want)
    assert tuple(acc[5:].tolist()) == SENTINELS

    # an all-ignored batch on top changes acc[4] alone
    before = acc.clone()
    z = np.random.RandomState(0).standard_normal((7, 33)).astype(np.float32)
    ops.softmax_xent_eval(dev(z), dev(np.full(7, -1, np.int32)), acc, 2)
    assert torch.equal(acc[:4], before[:4]) and float(acc[4]) == float(before[4]) + 7 and torch.equal(acc[5:], before[5:])


def test_eval_equals_the_loss_kernels_rows_and_refuses_bad_arguments():
    name, z, t = next(c for c in S.ls_cases(1001) if c[0].startswith('normal-third_ignored-B257'))
    zd, td = dev(z), dev(t)
    _, _, rl, rh, rhk = ops.softmax_xent_ls_fwd(zd, td, 0.0, 5)
    acc = _single(z, t, 5).cpu().numpy()
    # the same row code: the loss sum is the double sum of the loss kernel's fp32 rows, up to the order of a double sum
    assert abs(acc[0] - rl.double().sum().item()) <= 1e-12 * acc[0]
    assert acc[1] == rh.sum().item() and acc[2] == rhk.sum().item()

    lib = _lib.load()
    buf = torch.zeros(1 << 12, device='cuda')
    p = buf.data_ptr()
    f = lib.loans_softmax_xent_eval_f32
    assert f(p, p, p, p, 4, 8, 0, 0) == -1 and f(p, p, p, 0, 4, 8, 1, 0) == -1
    assert f(p, p, p, p, 4, 8193, 1, 0) == -2 and f(p, p, p, p, 65537, 8, 1, 0) == -2
    torch.cuda.synchronize()
    assert not buf.any()
    with pytest.raises(AssertionError):
        ops.softmax_xent_eval(zd, td, torch.zeros(5, device='cuda'), 1)                  # a float32 accumulator
