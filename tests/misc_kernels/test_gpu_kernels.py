"""-m gpu: the kernels of csrc/misc.hip and csrc/insight.hip that are neither a convolution nor a BN, through ``ops`` (and
``_lib.load()`` where ``ops`` hides an argument) against float64 NumPy, held to the bounds tests/misc_kernels/cases.py derives and
tests/misc_kernels/test_cases_cpu.py establishes on the fp32 restatement."""
import json

import pytest
import torch

from loans_amd import _lib
from tests.misc_kernels import cases as M

pytestmark = pytest.mark.gpu

WORST = {}


@pytest.fixture(scope='module')
def impl():
    return M.HipImpl()


def _run(impl, fn, *args):
    M.merge(WORST, M.report('kernel', fn, impl, *args))


@pytest.mark.parametrize("HW", M.GAP_HW)
def test_gap(impl, HW):
    _run(impl, M.run_gap, HW)


def test_gap_backward_second_trip(impl):
    _run(impl, M.run_gap_big)


@pytest.mark.parametrize("case", M.linear_cases(), ids=M.linear_id)
def test_linear(impl, case):
    _run(impl, M.check_linear, case)


def test_linear_refuses_by_return_code_and_launches_nothing():
    lib = _lib.load()
    buf = torch.zeros(4096, device='cuda')
    p = buf.data_ptr()
    fwd, bwd = lib.loans_linear_fwd_f32, lib.loans_linear_bwd_f32
    fwd16, bwd16 = lib.loans_linear_fwd_bf16, lib.loans_linear_bwd_bf16
    for f in (fwd, fwd16):
        assert f(p, p, p, p, 2, 8, 9, 0, 0, 0) == -1                    # N = 9
        assert f(p, p, p, p, 2, 6, 2, 0, 0, 0) == -1                    # K = 6: no multiple of four
        assert f(p, p, p, p, 0, 8, 2, 0, 0, 0) == -1 and f(p, p, p, p, 2, 0, 2, 0, 0, 0) == -1 and f(p, p, p, p, 2, 8, 0, 0, 0, 0) == -1
        assert f(0, p, p, p, 2, 8, 2, 0, 0, 0) == -1 and f(p, 0, p, p, 2, 8, 2, 0, 0, 0) == -1 and f(p, p, p, 0, 2, 8, 2, 0, 0, 0) == -1
    for f in (bwd, bwd16):
        assert f(p, p, p, p, p, p, p, 2, 8, 9, 0, 0, 0) == -1
        assert f(p, p, p, p, p, p, p, 2, 6, 2, 0, 0, 0) == -1
        assert f(p, p, 0, p, p, p, p, 2, 8, 2, 0, 1, 0) == -1           # act_out without y
        assert f(0, p, p, p, p, p, p, 2, 8, 2, 0, 0, 0) == -1 and f(p, 0, p, p, p, p, p, 2, 8, 2, 0, 0, 0) == -1
        assert f(p, p, p, 0, p, p, p, 2, 8, 2, 0, 0, 0) == -1           # gy missing
    torch.cuda.synchronize()
    assert not buf.any()


@pytest.mark.parametrize("size", M.ST_SIZES, ids=lambda s: '%dx%d' % s)
def test_st_grid(impl, size):
    _run(impl, M.run_st_grid, size)


def test_st_grid_second_trip(impl):
    _run(impl, M.run_st_grid_big)


@pytest.mark.parametrize("frame", M.SAMPLER_FRAMES, ids=lambda s: '%dx%d' % s)
def test_sampler(impl, frame):
    """with the bounds: st_sampler_fwd equals the float32 oracle bit for bit (unfused products)"""
    _run(impl, M.run_sampler, frame)


def test_sampler_second_trip(impl):
    _run(impl, M.run_sampler_big)


def test_mse(impl):
    _run(impl, M.run_mse)


@pytest.mark.parametrize("B", M.REG_B)
def test_regularisers(impl, B):
    _run(impl, M.run_regularisers, B)


def test_regulariser_ties(impl):
    _run(impl, M.check_regulariser_ties)


@pytest.mark.parametrize("n", M.ADAM_N + (M.ADAM_BIG,))
def test_adam(impl, n):
    _run(impl, M.check_adam, n)


def test_adam_refuses_by_return_code_and_launches_nothing():
    lib = _lib.load()
    buf = torch.zeros(64, device='cuda')
    a = buf.data_ptr()
    hyper = (0.9, 0.999, 1e-8, 1.0, 0.0, 1.0, 0)
    for bad in range(5):                                                # each of p, g, m, v, vhat missing
        ptrs = [0 if i == bad else a for i in range(5)]
        assert lib.loans_adam_amsgrad_f32(*ptrs, 16, 1e-3, *hyper) == -1, bad
        assert lib.loans_adam_amsgrad_devlr_f32(*ptrs, 16, a, *hyper) == -1, bad
        if bad < 4:
            assert lib.loans_adam_f32(*ptrs[:4], 16, 1e-3, 0, *hyper) == -1, bad
    assert lib.loans_adam_amsgrad_devlr_f32(a, a, a, a, a, 16, 0, *hyper) == -1                 # the device-side rate missing
    for n in (0, -4):
        assert lib.loans_adam_amsgrad_f32(a, a, a, a, a, n, 1e-3, *hyper) == -1
        assert lib.loans_adam_amsgrad_devlr_f32(a, a, a, a, a, n, a, *hyper) == -1
        assert lib.loans_adam_f32(a, a, a, a, n, 1e-3, 0, *hyper) == -1
    torch.cuda.synchronize()
    assert not buf.any()


def test_glue(impl):
    _run(impl, M.run_glue)


def test_insight(impl):
    _run(impl, M.run_insight)


def test_zz_kernel_ratios_are_at_most_one():
    """(runs last in this file) the kernel column of DESIGN 3, item 12"""
    print('MISC_RATIOS_WORST kernel %s' % json.dumps({k: round(v, 4) for k, v in WORST.items() if not k.startswith('exact:')}, sort_keys=True))
    ratios = [v for k, v in WORST.items() if not k.startswith(('share:', 'exact:'))]
    assert max(ratios + [0.0]) <= 1.0
    assert max([v for k, v in WORST.items() if k.startswith('share:')] + [0.0]) == 0.0
