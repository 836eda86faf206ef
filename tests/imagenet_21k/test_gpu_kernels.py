"""-m gpu: the split-row softmax loss (loans_softmax_xent_split_fwd_f32 / _eval_f32, csrc/classify.hip) against float64 in NumPy at
one ragged chunk, exactly one chunk, a second chunk of one element, two full chunks, a ragged third chunk and the maximum.
The bound: an fp32 NumPy restatement of the kernels' own order of operations (strided per-thread sums, xor butterfly, (w0 + w1)
+ (w2 + w3), per-chunk shift, fold in chunk order) run on the CPU against the reference below on exactly these inputs gave at
most 1.26e-6 in row_loss, 1.28e-6 in out[0] (losses 0.7 .. 13) and 7.5e-8 in gz (entries up to 0.5); times 4 for the device's
expf / logf against the host's: LOSS_TOL = 5.2e-6, GZ_TOL = 3.0e-7.  Nothing here was taken from the kernels' output."""
import numpy as np
import pytest
import torch

from loans_amd import ops
from tests.gpu_util import dev

pytestmark = pytest.mark.gpu
NS = (100, 8192, 8193, 16384, 21841, 65536)
LOSS_TOL, GZ_TOL = 5.2e-6, 3.0e-7
LAM = float(np.float32(0.3))
OML = float(np.float32(1) - np.float32(0.3))


def make_logits(N):
    """row 0: the maximum tied at 8191 and 8192; row 1: ties with the label min(8192, N - 1) on both sides of it, across the chunk
    boundary, under two larger logits in other chunks (4 ahead by the j < t rule, 6 by a wrong one); row 2: the maximum far off"""
    z = np.random.RandomState(N).standard_normal((3, N)).astype(np.float32)
    hi = min(8192, N - 1)
    z[0, [hi - 1, hi]] = 12.0
    z[1, [j for j in range(hi - 2, hi + 3) if j < N]] = 6.0
    z[1, [5, N - 3]] = 7.0
    z[2, N - 2] = 8.0
    return z


def make_calls(N):
    """(ta, tb, lam, oml): labels at 0, 8191, 8192, N - 1 and -1, ta == tb, and the weights (1, 0) with a tb that must not be read"""
    lo, hi = min(8191, N - 1), min(8192, N - 1)
    i32 = lambda *v: np.array(v, np.int32)
    return [(i32(0, lo, -1), i32(N - 1, hi, 5), LAM, OML),              # dominant tb
            (i32(hi, 7, N - 1), i32(hi, 0, lo), OML, LAM),              # dominant ta; row 0: ta == tb
            (i32(lo, hi, -1), i32(N, -5, 1 << 30), 1.0, 0.0)]          # one label


def reference(z, ta, tb, lam, oml, eps, k):
    """float64: (row_loss, row_hit, row_hitk, out[3], gz)"""
    B, N = z.shape
    z = z.astype(np.float64)
    if (lam, oml) == (1.0, 0.0):
        tb = ta
    valid = (ta >= 0) & (ta < N) & (tb >= 0) & (tb < N)
    count = max(int(valid.sum()), 1)
    dom = ta if lam >= oml else tb
    loss, hit, hitk, gz = np.zeros(B), np.zeros(B), np.zeros(B), np.zeros((B, N))
    for b in np.flatnonzero(valid):
        m = z[b].max()
        lse = m + np.log(np.exp(z[b] - m).sum())
        q = np.full(N, eps / N)
        q[ta[b]] += (1 - eps) * lam
        q[tb[b]] += (1 - eps) * oml
        loss[b] = lse - (q * z[b]).sum()
        gz[b] = (np.exp(z[b] - lse) - q) / count
        zt = z[b, dom[b]]
        hit[b] = np.argmax(z[b]) == dom[b]                       # the first index that holds the maximum
        hitk[b] = ((z[b] > zt) | ((z[b] == zt) & (np.arange(N) < dom[b]))).sum() < k
    return loss, hit, hitk, np.array([loss.sum() / count, hit.sum() / B, hitk.sum() / B]), gz


@pytest.mark.parametrize('k', [1, 5])
@pytest.mark.parametrize('eps', [0.0, 0.1])
@pytest.mark.parametrize('N', NS)
def test_split_forward_against_float64(N, eps, k):
    z = make_logits(N)
    for ta, tb, lam, oml in make_calls(N):
        got, again = ([a.cpu().numpy() for a in ops.softmax_xent_split_fwd(dev(z), dev(ta), dev(tb), lam, oml, eps, k)] for _ in 'ab')
        out, gz, row_loss, row_hit, row_hitk = got
        want_loss, want_hit, want_hitk, want_out, want_gz = reference(z, ta, tb, lam, oml, eps, k)
        errs = np.abs(row_loss - want_loss).max(), abs(out[0] - want_out[0]), np.abs(gz - want_gz).max()
        print('N %d eps %g k %d: row_loss %.3g  out[0] %.3g  gz %.3g' % ((N, eps, k) + errs))
        assert np.array_equal(row_hit, want_hit) and np.array_equal(row_hitk, want_hitk)
        assert out[1] == np.float32(want_hit.sum()) / np.float32(3) and out[2] == np.float32(want_hitk.sum()) / np.float32(3)
        ignored = want_loss == 0
        assert not row_loss[ignored].any() and not gz[ignored].any()
        assert errs[0] <= LOSS_TOL and errs[1] <= LOSS_TOL and errs[2] <= GZ_TOL
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))
    if N > 8192:
        assert row_hit[0] == 1          # the last call: the label 8191 ties the maximum with 8192 and is the argmax


@pytest.mark.parametrize('N', [8193, 21841])
def test_split_eval_accumulates_the_five_sums(N):
    z = make_logits(N)
    acc = torch.zeros(5, device='cuda', dtype=torch.float64)
    want = np.zeros(5)
    for ta, _, _, _ in make_calls(N)[1:]:
        ops.softmax_xent_split_eval(dev(z), dev(ta), acc, 5)
        loss, hit, hitk, _, _ = reference(z, ta, ta, 1.0, 0.0, 0.0, 5)
        want += [loss.sum(), hit.sum(), hitk.sum(), (loss != 0).sum(), 3]
    got = acc.cpu().numpy()
    assert np.array_equal(got[1:], want[1:]) and abs(got[0] - want[0]) <= want[3] * LOSS_TOL
