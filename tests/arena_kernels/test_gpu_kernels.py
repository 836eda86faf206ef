"""-m gpu: what the sharing in loans_amd/csrc/arena.h rests on.  lars_partials_kernel, lamb_moments_kernel and grad_sumsq_kernel
sum a unit's squares in ONE order -- a thread's elements float4 by float4, the xor butterfly, waves 0..3 --, so the per-unit fp64
partials they leave for the same buffer are the same bits; and the segmented momentum SGD kernel with a ratio table of ones is the
one without a table (fl(lr * 1) = lr).  Sizes: scalars only, one full unit, full units and a ragged end, and one unit more than
grid_for's 2048 blocks, which gives every walker a second trip; a buffer is at most 33.6 MB."""
import numpy as np
import pytest
import torch

from tests.imagenet_lamb import cases as L
from tests.imagenet_lars import cases as A

pytestmark = pytest.mark.gpu

SIZES = (5, A.UNIT, 2 * A.UNIT + 3, (A.GRID_CAP + 1) * A.UNIT + 1)


def _bits64(t):
    return t.cpu().numpy().view(np.int64)


@pytest.mark.parametrize('n', SIZES)
def test_the_three_unit_walks_sum_in_one_order(n):
    from loans_amd import ops
    device = torch.device('cuda', torch.cuda.current_device())
    rng = np.random.RandomState([n % 65521, 3])
    p = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(device)
    g = torch.from_numpy((1e-3 * rng.standard_normal(n)).astype(np.float32)).to(device)
    units = -(-n // A.UNIT)
    table = ops.LarsTable([n], [0], device)
    assert table.workspace.numel() == 2 * units
    table.workspace.fill_(float('nan'))
    ops.lars_ratios(p, g, 5e-5, A.ETA, A.EPS, table, 1.0)
    lars = table.workspace.clone()
    assert not torch.isnan(lars).any() and (lars > 0).all()

    state = ops.GradClipState(n, device)
    assert state.workspace.numel() == units
    state.workspace.fill_(float('nan'))
    ops.grad_norm(g, float('inf'), state, 1.0)
    assert np.array_equal(_bits64(lars[1::2]), _bits64(state.workspace))           # the sums of g^2

    m, v = torch.zeros_like(p), torch.zeros_like(p)
    c1, c2 = L.corrections(1)
    table.workspace.fill_(float('nan'))
    ops.lamb_moments(p, g, m, v, L.BETA1, L.BETA2, c1, c2, L.EPS, 5e-5, table, 1.0)
    assert np.array_equal(_bits64(lars[0::2]), _bits64(table.workspace[0::2]))      # the sums of p^2
    assert not torch.isnan(table.workspace).any()


@pytest.mark.parametrize('lr_dev', [False, True], ids=['host-rate', 'device-rate'])
def test_a_ratio_table_of_ones_is_no_ratio_table(lr_dev):
    from loans_amd import ops
    device = torch.device('cuda', torch.cuda.current_device())
    n, ends, flags = A.TABLES['kinds']
    h = A.UPDATE_HYPER
    values = A.make('kinds')
    table = ops.LarsTable(ends, flags, device)
    table.ratios.fill_(1.0)
    out = []
    for update in (ops.lars_update, ops.momentum_sgd_seg):
        p, g, v = (torch.from_numpy(a).to(device) for a in values)
        lr = torch.full((1,), h['lr'], device=device, dtype=torch.float32) if lr_dev else h['lr']
        update(p[:n], g[:n], v[:n], lr, h['momentum'], 5e-5, table, 0.5)
        out.append((p.cpu().numpy().view(np.int32), v.cpu().numpy().view(np.int32)))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    assert not np.array_equal(out[0][0][:n], values[0].view(np.int32)[:n])            # something moved
    assert np.array_equal(out[0][0][n:], values[0].view(np.int32)[n:]) and np.array_equal(out[0][1][n:], values[2].view(np.int32)[n:])
