"""-m gpu: the momentum-SGD kernel (loans_amd/csrc/sgd.hip) and the label-smoothed loss with top-k accuracy
(loans_amd/csrc/classify.hip) through ``ops`` against float64 NumPy, held to the bounds tests/imagenet_sgd/reference.py derives
and the CPU test establishes on the fp32 restatements."""
import numpy as np
import pytest
import torch

import loans_amd
from loans_amd import _lib, ops
from loans_amd.functions import ops_small
from tests.gpu_util import dev
from tests.imagenet import reference as R
from tests.imagenet_sgd import reference as S
from tests.imagenet_sgd.test_reference_cpu import SGD_HYPER, SGD_N, sgd_inputs

pytestmark = pytest.mark.gpu

GRID_CAP = 256 * 8                              # grid_for's max_blocks (csrc/common.h): beyond it a thread takes a second trip
SGD_SIZES = SGD_N + (4 * 256 * GRID_CAP + 6,)
LR = 0.05


@pytest.mark.parametrize("n", SGD_SIZES)
def test_momentum_sgd_against_the_rule(n):
    p, g, v = sgd_inputs(n)
    worst = 0.0
    for mom, wd, gs in SGD_HYPER:
        p64, v64 = S.momentum_sgd_ref(p, g, v, LR, mom, wd, gs)
        bp, bv = S.momentum_sgd_bound(p, g, v, LR, mom, wd, gs)
        pd, gd, vd = dev(p), dev(g), dev(v)
        ops.momentum_sgd(pd, gd, vd, LR, mom, wd, gs)
        got_p, got_v = pd.cpu().numpy().astype(np.float64), vd.cpu().numpy().astype(np.float64)
        ep, ev = np.abs(got_p - p64), np.abs(got_v - v64)
        assert np.all(ep <= bp) and np.all(ev <= bv), (n, mom, wd, gs, float((ep / bp).max()), float((ev / bv).max()))
        for i in range(n - (n & 3), n):         # the tail block 0 handles, element by element
            assert ep[i] <= bp[i] and ev[i] <= bv[i], (n, i)
            assert got_v[i] != v[i], (n, i)                                             # it was written
        assert torch.equal(gd, dev(g))                                                # the gradient is read only
        worst = max(worst, float((ep / bp).max()), float((ev / bv).max()))

        # two launches, the same bits; the device-side rate, the same bits as the host-side one
        p2, v2 = dev(p), dev(v)
        ops.momentum_sgd(p2, gd, v2, LR, mom, wd, gs)
        assert torch.equal(p2, pd) and torch.equal(v2, vd)
        p3, v3 = dev(p), dev(v)
        ops.momentum_sgd(p3, gd, v3, torch.full((1,), LR, device='cuda', dtype=torch.float32), mom, wd, gs)
        assert torch.equal(p3, pd) and torch.equal(v3, vd)
    print('n=%d worst error / bound %.3f' % (n, worst))


def test_momentum_sgd_three_steps_and_argument_checks():
    n = 1027
    p, g, v = sgd_inputs(n)
    pd, vd = dev(p), dev(v)
    p64, v64, ep, ev = p, v, 0.0, 0.0
    for step in range(3):
        gk = np.roll(g, step)
        ep, ev = S.momentum_sgd_bound(p64, gk, v64, LR, 0.9, 5e-4, 1.0, ep, ev)
        p64, v64 = S.momentum_sgd_ref(p64, gk, v64, LR, 0.9, 5e-4)
        ops.momentum_sgd(pd, dev(gk), vd, LR, 0.9, 5e-4)
        assert np.all(np.abs(pd.cpu().numpy() - p64) <= ep) and np.all(np.abs(vd.cpu().numpy() - v64) <= ev), step
    # a zero gradient and no decay: the parameters move by the decayed momentum alone, to the bit
    before_p, before_v = pd.clone(), vd.clone()
    ops.momentum_sgd(pd, torch.zeros(n, device='cuda'), vd, LR, 0.9, 0.0)
    want_v = before_v * torch.tensor(0.9, dtype=torch.float32)
    assert torch.equal(vd, want_v) and torch.equal(pd, before_p + want_v)

    lib = _lib.load()
    buf = torch.zeros(64, device='cuda')
    a = buf.data_ptr()
    for args in ((0, a, a, 16), (a, 0, a, 16), (a, a, 0, 16), (a, a, a, 0), (a, a, a, -4)):
        assert lib.loans_momentum_sgd_f32(args[0], args[1], args[2], args[3], 0.1, 0, 0.9, 0.0, 1.0, 0) == -1, args
    torch.cuda.synchronize()
    assert not buf.any()
    with pytest.raises(_lib.HipKernelError):
        ops.momentum_sgd(buf[:0], buf[:0], buf[:0], 0.1, 0.9, 0.0)


def _check_case(name, z, t, eps, ref_by_k, lb, gb, bb, plain, worst):
    """one (case, eps): the kernel at every k against the references computed once for the case"""
    N = z.shape[1]
    zd, td = dev(z), dev(t)
    valid = (t >= 0) & (t < N)
    for k in S.TOPK:
        loss, acc, acck, gz, row_loss, hit, hitk = ref_by_k[k]
        out, gzd, rl, rh, rhk = ops.softmax_xent_ls_fwd(zd, td, eps, k)
        out2, gzd2, rl2, rh2, rhk2 = ops.softmax_xent_ls_fwd(zd, td, eps, k)
        for a, b in ((out, out2), (gzd, gzd2), (rl, rl2), (rh, rh2), (rhk, rhk2)):
            assert torch.equal(a, b), (name, eps, k)                                    # two launches, the same bits
        got_loss = float(out[0])
        err = np.abs(rl.cpu().numpy().astype(np.float64) - row_loss)
        gerr = np.abs(gzd.cpu().numpy().astype(np.float64) - gz)
        assert np.all(err <= lb), (name, eps, k, float((err - lb).max()))
        assert np.all(gerr <= gb), (name, eps, k, float((gerr - gb).max()))
        assert abs(got_loss - loss) <= bb, (name, eps, k, got_loss, loss, bb)
        np.testing.assert_array_equal(rh.cpu().numpy(), hit.astype(np.float32), err_msg=name)
        np.testing.assert_array_equal(rhk.cpu().numpy(), hitk.astype(np.float32), err_msg='%s k=%d' % (name, k))
        assert float(out[1]) == float(np.float32(acc)) and float(out[2]) == float(np.float32(acck)), (name, eps, k)
        if k == 1:
            assert torch.equal(rh, rhk) and torch.equal(out[1], out[2]), name
        if eps == 0:        # the existing arithmetic, bit for bit
            p_out, p_gz, p_rl, p_rh = plain
            assert torch.equal(out[:2], p_out) and torch.equal(gzd, p_gz) and torch.equal(rl, p_rl) and torch.equal(rh, p_rh), (name, k)
        if valid.any():
            worst['loss'] = max(worst['loss'], float((err[valid] / lb[valid]).max()))
            worst['gz'] = max(worst['gz'], float((gerr[valid] / gb[valid]).max()))
            worst['batch'] = max(worst['batch'], abs(got_loss - loss) / bb)
        else:
            assert got_loss == 0.0 and not gzd.any() and not rhk.any(), name          # exact
    return zd, td


@pytest.mark.parametrize("eps", S.EPS)
@pytest.mark.parametrize("N", R.XENT_N)
def test_smoothed_loss_and_topk_over_the_case_grid(N, eps):
    worst = {'loss': 0.0, 'gz': 0.0, 'batch': 0.0}
    g_rng = np.random.RandomState(N)
    for name, z, t in S.ls_cases(N):
        assert R.argmax_margin_ok(z) and S.rank_margin_ok(z, t), name        # no case is left out of the exact hit comparison
        ref_by_k = {k: S.softmax_xent_ls_ref(z, t, eps, k) for k in S.TOPK}
        lb, gb, bb = S.ls_bounds(z, t, eps)
        plain = ops.softmax_xent_fwd(dev(z), dev(t)) if eps == 0 else None
        zd, td = _check_case(name, z, t, eps, ref_by_k, lb, gb, bb, plain, worst)

        # through the Function: upstream gradient 1 and a seeded non-unit one
        loss, acc, acck, gz = ref_by_k[2][:4]
        for g in (1.0, float(np.float32(0.25 + g_rng.rand()))):
            zv = loans_amd.Variable(zd)
            lv, av, akv = ops_small.softmax_cross_entropy_with_topk_accuracy(zv, td, label_smoothing=eps, topk=2)
            assert abs(float(lv.data) - loss) <= bb and float(av.data) == float(np.float32(acc)), (name, eps)
            assert float(akv.data) == float(np.float32(acck)), (name, eps)
            lv.grad = torch.full((), g, device='cuda')
            lv.backward()
            ref = gz * g
            bound = gb * abs(g) + R.U * np.abs(ref) * R.SLACK
            assert np.all(np.abs(zv.grad.cpu().numpy().astype(np.float64) - ref) <= bound), (name, eps, g)
    print('N=%d eps=%g worst error / bound: row loss %.3f, gz %.3f, batch loss %.3f' % (N, eps, worst['loss'], worst['gz'], worst['batch']))


def test_topk_tie_and_k_beyond_the_classes():
    z, t = S.topk_tie_case()
    zd, td = dev(z), dev(t)
    for k, want in ((1, 0.0), (2, 1.0), (3, 1.0)):
        out, _, _, rh, rhk = ops.softmax_xent_ls_fwd(zd, td, 0.1, k)
        assert not rh.any() and float(out[1]) == 0.0             # the first tied column is the argmax, not the label
        assert float(out[2]) == want and bool(rhk.all()) == bool(want) and bool(rhk.any()) == bool(want), k
    # k larger than N: every valid row hits, an ignored one never does
    t2 = t.copy()
    t2[1] = -1
    out, _, _, _, rhk = ops.softmax_xent_ls_fwd(zd, dev(t2), 0.0, z.shape[1] + 7)
    np.testing.assert_array_equal(rhk.cpu().numpy(), (t2 >= 0).astype(np.float32))
    assert float(out[2]) == float(np.float32(np.float32(len(t) - 1) / np.float32(len(t))))


def test_smoothed_loss_refuses_what_is_out_of_range():
    lib = _lib.load()
    buf = torch.zeros(1 << 16, device='cuda')
    p = buf.data_ptr()
    f = lib.loans_softmax_xent_ls_fwd_f32
    assert f(p, p, p, p, p, p, p, 4, 8, 1.0, 1, 0) == -1            # eps = 1
    assert f(p, p, p, p, p, p, p, 4, 8, -0.1, 1, 0) == -1           # eps < 0
    assert f(p, p, p, p, p, p, p, 4, 8, float('nan'), 1, 0) == -1
    assert f(p, p, p, p, p, p, p, 4, 8, 0.1, 0, 0) == -1            # k = 0
    assert f(p, p, p, p, p, p, p, 0, 8, 0.1, 1, 0) == -1
    assert f(p, p, p, p, p, 0, p, 4, 8, 0.1, 1, 0) == -1            # row_hitk missing
    assert f(p, p, p, p, p, p, p, 4, 1 << 14, 0.1, 1, 0) == -2      # beyond one row of LDS
    assert f(p, p, p, p, p, p, p, (1 << 16) + 1, 8, 0.1, 1, 0) == -2
    torch.cuda.synchronize()
    assert not buf.any()
