"""No GPU: the fp32 NumPy restatement of the misc / insight kernels (tests/misc_kernels/cases.py: NumpyImpl) stays inside the
derived bounds on EVERY generated case, the share of elements left out of a comparison is 0, the generators' tie / gap assertions
hold, and the regime table of cases.py is what the kernels' constants give.  The largest ratios are the restatement column of
DESIGN 3, item 12."""
import json

import numpy as np
import pytest

from tests.misc_kernels import cases as M

WORST = {}


def _run(fn, *args):
    M.merge(WORST, M.report('restatement', fn, _impl(), *args))


def _impl():
    return M.NumpyImpl()


def test_regime_table_is_what_the_constants_give():
    """1024 elements per trip, LU = 8, slabs of 16, 2048 x 256: a later change of the grid cannot silently empty a cell"""
    assert (M.LIN_TRIP, M.LIN_LU, M.LIN_SLAB, M.LIN_NMAX, M.BLOCK, M.GRID_CAP, M.TRIP) == (1024, 8, 16, 8, 256, 2048, 524288)
    assert set(M.REGIMES['linear_K']) == set(M.LIN_K) and set(M.REGIMES['linear_B']) == set(M.LIN_B)
    assert set(M.REGIMES['gap_HW']) == set(M.GAP_HW) and set(M.REGIMES['gap_C']) == set(M.GAP_C)
    for K, want in M.REGIMES['linear_K'].items():
        assert M.linear_fwd_regime(K) == want, K
    for B, want in M.REGIMES['linear_B'].items():
        slabs = -(-B // M.LIN_SLAB)
        assert (slabs, B - (slabs - 1) * M.LIN_SLAB, -(-B // M.BLOCK)) == want, B
    for HW, want in M.REGIMES['gap_HW'].items():
        assert M.gap_fwd_regime(HW, 4)[:4] == want, HW
    for C_, want in M.REGIMES['gap_C'].items():
        assert M.gap_fwd_regime(1, C_)[4:] == want, C_
    for items, want in M.REGIMES['stride'].items():
        assert M.stride_trips(items) == want, items
    for items, want in M.REGIMES['block'].items():
        assert -(-items // M.BLOCK) == want, items
    # the shapes of the grid are the table's
    b, hw, c = M.GAP_BWD_BIG
    assert b * hw * c // 4 in M.REGIMES['stride'] and M.ST_BIG[0] * M.ST_BIG[1] * M.ST_BIG[2] in M.REGIMES['stride']
    assert M.SAMPLER_BIG[0] * M.SAMPLER_BIG[3] * M.SAMPLER_BIG[4] in M.REGIMES['stride']
    assert (M.ADAM_BIG + 3) // 4 in M.REGIMES['stride'] and M.ADAM_BIG & 3 == 2 and M.GLUE_N[-1] in M.REGIMES['stride']
    bb, hh, ww = M.NHWC4_SHAPES[-1]
    assert bb * hh * ww in M.REGIMES['stride']
    for n in M.MSE_N + M.REG_B + tuple(th * tw for th, tw in M.ST_SIZES if th * tw > 1):
        assert n in M.REGIMES['block'] or n < M.BLOCK, n
    # every regime the kernels have is met by some shape
    lin = list(M.REGIMES['linear_K'].values())
    assert any(r[0] == 0 and r[1] == 7 for r in lin) and any(r[0] == 1 and r[2] == 0 for r in lin) and any(r[0] > 1 for r in lin)
    assert any(r[3] == 0 for r in lin)                                 # a thread with nothing to do
    gap = list(M.REGIMES['gap_HW'].values())
    assert any(r[0] == 1 and r[2] == 0 for r in gap) and any(r[:2] == (1, 0) and r[2:] == (1, 0) for r in gap)
    assert any(r[0] and r[1] for r in gap) and any(r[3] == 0 and r[2] == 0 for r in gap)
    assert any(s > 1 and last == 1 for s, last, _ in M.REGIMES['linear_B'].values())
    assert any(t > 1 for _, _, t in M.REGIMES['linear_B'].values())


def test_linear_case_list_meets_what_the_grid_promises():
    cases = M.linear_cases()
    seen = {(c['K'], c['N']) for c in cases}
    for K in M.LIN_K:
        assert (K, 1) in seen and (K, 6) in seen
    for B in M.LIN_B:
        assert {c['K'] for c in cases if c['B'] == B} >= {1028, 8196}
    assert sum(1 for c in cases if c['B'] == 257 and c['K'] == 41472) == 1
    assert {c['N'] for c in cases} == set(M.LIN_N)
    combos = {(c['act_in'], c['act_out'], c['bias']) for c in cases if (c['K'], c['N'], c['B']) == (1028, 6, 17)}
    assert len(combos) == 8
    assert {c['mode'] for c in cases} == {'all', 'no_gx', 'gW', 'gb'}
    assert len({M.linear_id(c) for c in cases}) == len(cases)


def test_tie_products_are_inexact_with_the_signs_the_grid_relies_on():
    for t, size in M.TIES_NEG:
        assert M.tie_residual(t, size) < 0, (t, size)
    for t, size in M.TIES_POS:
        assert M.tie_residual(t, size) > 0, (t, size)
    # what a kernel that fused `a * size - round(b * size)` would compute at such a tie: the residual, not 0
    t, size = M.TIES_NEG[0]
    s = np.float32((np.float32(t) + np.float32(1)) / np.float32(2))
    assert float(s) * size - float(np.float32(s * np.float32(size))) < 0 <= float(np.float32(s * np.float32(size)) - np.float32(s * np.float32(size)))


def test_hand_written_sampler_grid_hits_the_borders():
    H, W = 5, 3
    u = (M.HAND_GX + np.float32(1)) * np.float32(W - 1) / np.float32(2) + np.float32(1)
    v = (M.HAND_GY + np.float32(1)) * np.float32(H - 1) / np.float32(2) + np.float32(1)
    assert np.array_equal(u, M.HAND_U) and np.array_equal(v, M.HAND_V)
    assert {0, W + 1, 1, W}.issubset(set(u.tolist())) and {0, H + 1, 1, H}.issubset(set(v.tolist()))


@pytest.mark.parametrize("HW", M.GAP_HW)
def test_gap(HW):
    _run(M.run_gap, HW)


def test_gap_backward_second_trip():
    _run(M.run_gap_big)


@pytest.mark.parametrize("case", M.linear_cases(), ids=M.linear_id)
def test_linear(case):
    _run(M.check_linear, case)


@pytest.mark.parametrize("size", M.ST_SIZES, ids=lambda s: '%dx%d' % s)
def test_st_grid(size):
    _run(M.run_st_grid, size)


def test_st_grid_second_trip():
    _run(M.run_st_grid_big)


@pytest.mark.parametrize("frame", M.SAMPLER_FRAMES, ids=lambda s: '%dx%d' % s)
def test_sampler(frame):
    _run(M.run_sampler, frame)


def test_sampler_second_trip():
    _run(M.run_sampler_big)


def test_mse():
    _run(M.run_mse)


@pytest.mark.parametrize("B", M.REG_B)
def test_regularisers(B):
    _run(M.run_regularisers, B)


def test_regulariser_ties():
    _run(M.check_regulariser_ties)


@pytest.mark.parametrize("n", M.ADAM_N + (M.ADAM_BIG,))
def test_adam(n):
    _run(M.check_adam, n)


def test_glue():
    _run(M.run_glue)


def test_insight():
    _run(M.run_insight)


def test_zz_restatement_ratios_are_at_most_one():
    """(runs last in this file) every ratio of the restatement is <= 1 on every generated case and nothing was left out"""
    print('MISC_RATIOS_WORST %s' % json.dumps({k: round(v, 4) for k, v in WORST.items() if not k.startswith('exact:')}, sort_keys=True))
    ratios = [v for k, v in WORST.items() if not k.startswith(('share:', 'exact:'))]
    assert max(ratios + [0.0]) <= 1.0
    assert max([v for k, v in WORST.items() if k.startswith('share:')] + [0.0]) == 0.0
