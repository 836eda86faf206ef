"""-m gpu: the kernels of the ImageNet head (loans_amd/csrc/classify.hip) through ``ops`` against float64 NumPy: the wide
Linear layer in its three directions, and softmax cross-entropy with accuracy over the case grid of tests/imagenet/reference.py,
held to the bound the CPU test establishes there."""
import numpy as np
import pytest
import torch

import loans_amd
from loans_amd import _lib, ops
from loans_amd.functions import ops_small
from tests.gpu_util import dev, rel_err
from tests.imagenet import reference as R

pytestmark = pytest.mark.gpu

# B in {1, 3, 33, 65} x N in {9, 10, 1000, 1001} x K in {4, 36, 512, 2048}, pruned: every value of every axis with every value
# of the others' extremes; one row, ragged tiles in all three dimensions, a K shorter than one chunk of 16
LINEAR_CASES = [(B, N, K) for B in (1, 3, 33, 65) for N in (9, 10, 1000, 1001) for K in (4, 36, 512, 2048)
                if (B in (1, 65) and N in (9, 1001)) or (N in (10, 1000) and K in (36, 512) and B in (3, 33))
                or (B, N, K) in ((3, 9, 4), (33, 1001, 2048), (65, 1000, 36), (1, 10, 512), (33, 9, 2048), (3, 1001, 4))]


@pytest.mark.parametrize("case", LINEAR_CASES, ids=lambda c: 'B%d-N%d-K%d' % c)
def test_wide_linear_three_directions(case):
    B, N, K = case
    rng = np.random.RandomState(B * 7 + N * 3 + K)
    x = rng.standard_normal((B, K)).astype(np.float32)
    W = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    gy = rng.standard_normal((B, N)).astype(np.float32)
    x64, W64, gy64 = x.astype(np.float64), W.astype(np.float64), gy.astype(np.float64)
    xd, Wd, bd, gyd = dev(x), dev(W), dev(b), dev(gy)

    # the sums are no longer than test_conv_fprop_dgrad_wgrad's: its fp32 bounds (2e-6 forward / data gradient, 5e-6 weight gradient)
    y = ops.linear_wide_fwd(xd, Wd, bd)
    assert rel_err(y.cpu().numpy(), x64 @ W64.T + b) < 2e-6
    y0 = ops.linear_wide_fwd(xd, Wd, None)
    assert rel_err(y0.cpu().numpy(), x64 @ W64.T) < 2e-6
    assert torch.equal(ops.linear_wide_fwd(xd, Wd, bd), y)                  # two launches, the same bits

    gW0 = rng.standard_normal((N, K)).astype(np.float32)
    gb0 = rng.standard_normal(N).astype(np.float32)
    gW, gb = dev(gW0), dev(gb0)
    gx = ops.linear_wide_bwd(xd, Wd, gyd, gW=gW, gb=gb)
    assert rel_err(gx.cpu().numpy(), gy64 @ W64) < 2e-6
    assert rel_err(gW.cpu().numpy(), gW0 + gy64.T @ x64) < 5e-6             # accumulated onto non-zero starting values
    assert rel_err(gb.cpu().numpy(), gb0 + gy64.sum(axis=0)) < 5e-6
    gW2, gb2 = dev(gW0), dev(gb0)
    gx2 = ops.linear_wide_bwd(xd, Wd, gyd, gW=gW2, gb=gb2)
    assert torch.equal(gx2, gx) and torch.equal(gW2, gW) and torch.equal(gb2, gb)

    # each of gx / gW / gb absent: the others are what they were
    only_w = dev(gW0)
    assert ops.linear_wide_bwd(xd, Wd, gyd, gW=only_w, gb=None, need_gx=False) is None and torch.equal(only_w, gW)
    only_b = dev(gb0)
    assert ops.linear_wide_bwd(xd, Wd, gyd, gW=None, gb=only_b, need_gx=False) is None and torch.equal(only_b, gb)
    assert torch.equal(ops.linear_wide_bwd(xd, Wd, gyd, gW=None, gb=None, need_gx=True), gx)


def test_linear_dispatch_keeps_the_small_kernel_and_refuses_other_shapes():
    rng = np.random.RandomState(0)
    B, K = 5, 512
    x, gy = dev(rng.standard_normal((B, K)).astype(np.float32)), dev(rng.standard_normal((B, 6)).astype(np.float32))
    W6 = loans_amd.Parameter(rng.standard_normal((6, K)).astype(np.float32), (6, K))
    b6 = loans_amd.Parameter(rng.standard_normal(6).astype(np.float32), (6,))
    for p in (W6, b6):
        p.bind(dev(p.host), torch.zeros(p.physical_shape, device='cuda'))
    # N = 6: the bits of the existing kernel, recorded from it in this run
    want_y = ops.linear_fwd(x, W6.data, b6.data)
    want_gW, want_gb = torch.zeros_like(W6.data), torch.zeros_like(b6.data)
    want_gx = ops.linear_bwd(x, W6.data, want_y, gy, gW=want_gW, gb=want_gb)
    xv = loans_amd.Variable(x)
    y = ops_small.linear(xv, W6, b6)
    assert torch.equal(y.data, want_y)
    y.grad = gy
    y.backward()
    assert torch.equal(xv.grad, want_gx) and torch.equal(W6.grad_view, want_gW) and torch.equal(b6.grad_view, want_gb)
    # N = 9 goes to the wide kernels
    W9 = loans_amd.Parameter(rng.standard_normal((9, K)).astype(np.float32), (9, K))
    W9.bind(dev(W9.host), torch.zeros((9, K), device='cuda'))
    y9 = ops_small.linear(loans_amd.Variable(x), W9)
    assert torch.equal(y9.data, ops.linear_wide_fwd(x, W9.data, None))

    # outside the stated limits: refused by return code, nothing launched
    lib = _lib.load()
    buf = torch.zeros(1 << 16, device='cuda')
    p = buf.data_ptr()
    assert lib.loans_linear_wide_fwd_f32(p, p, p, p, 4, 6, 16, 0) == -1            # K % 4 != 0
    assert lib.loans_linear_wide_fwd_f32(p, p, p, p, 4, 8, 0, 0) == -1             # N = 0
    assert lib.loans_linear_wide_fwd_f32(p, p, p, p, 4, 8, 8, 0) == -1             # N <= 8 is the small kernel's
    assert lib.loans_linear_wide_bwd_f32(p, p, p, p, p, p, 4, 6, 16, 0) == -1
    assert lib.loans_linear_wide_bwd_f32(p, p, p, p, p, p, 4, 8, 0, 0) == -1
    assert lib.loans_linear_wide_fwd_f32(p, p, p, p, 4, 8, 1 << 20, 0) == -2       # beyond the launcher's range
    assert lib.loans_softmax_xent_fwd_f32(p, p, p, p, p, p, 4, 1 << 14, 0) == -2
    assert lib.loans_softmax_xent_fwd_f32(p, p, p, p, p, p, 0, 8, 0) == -1
    torch.cuda.synchronize()
    assert not buf.any()


@pytest.mark.parametrize("N", R.XENT_N)
def test_softmax_cross_entropy_and_accuracy_over_the_case_grid(N):
    worst = {'loss': 0.0, 'gz': 0.0, 'batch': 0.0}
    g_rng = np.random.RandomState(N)
    for name, z, t, expect in R.xent_cases(N):
        loss, acc, gz, row_loss, am = R.softmax_xent_ref(z, t)
        lb, gb, bb = R.row_bounds(z, t)
        zd, td = dev(z), dev(t)
        out, gzd, rl, hit = ops.softmax_xent_fwd(zd, td)
        out2, gzd2, _, _ = ops.softmax_xent_fwd(zd, td)
        assert torch.equal(out, out2) and torch.equal(gzd, gzd2), name          # two launches, the same bits
        got_loss, got_acc = float(out[0]), float(out[1])
        err = np.abs(rl.cpu().numpy().astype(np.float64) - row_loss)
        gerr = np.abs(gzd.cpu().numpy().astype(np.float64) - gz)
        valid = (t >= 0) & (t < N)
        print('%s: loss %.9g (ref %.9g, bound %.3g)  worst row %.3g  worst gz %.3g' % (
            name, got_loss, loss, bb, float((err - lb).max()), float((gerr - gb).max())))
        assert np.all(err <= lb), name
        assert np.all(gerr <= gb), name
        assert abs(got_loss - loss) <= bb, (name, got_loss, loss, bb)
        # no case is left out of the argmax comparison (the CPU test checks the margin of every row)
        np.testing.assert_array_equal(hit.cpu().numpy(), (am == t).astype(np.float32), err_msg=name)
        assert got_acc == float(np.float32(acc)), (name, got_acc, acc)
        if expect is not None:
            np.testing.assert_array_equal(hit.cpu().numpy() == 1, expect, err_msg=name)
        if valid.any():
            worst['loss'] = max(worst['loss'], float((err[valid] / lb[valid]).max()))
            worst['gz'] = max(worst['gz'], float((gerr[valid] / gb[valid]).max()))
            worst['batch'] = max(worst['batch'], abs(got_loss - loss) / bb)
        else:
            assert got_loss == 0.0 and not gzd.any(), name                      # exact

        # through the Function: upstream gradient 1 and a seeded non-unit one
        for g in (1.0, float(np.float32(0.25 + g_rng.rand()))):
            zv = loans_amd.Variable(zd)
            lv = ops_small.softmax_cross_entropy(zv, td)
            assert float(lv.data) == got_loss
            lv.grad = torch.full((), g, device='cuda')
            lv.backward()
            ref = gz * g
            bound = gb * abs(g) + R.U * np.abs(ref) * R.SLACK
            assert np.all(np.abs(zv.grad.cpu().numpy().astype(np.float64) - ref) <= bound), (name, g)
        assert float(ops_small.accuracy(loans_amd.Variable(zd), td).data) == got_acc
    print('N=%d worst error / bound: row loss %.3f, gz %.3f, batch loss %.3f' % (N, worst['loss'], worst['gz'], worst['batch']))
