"""No GPU: the case grid of tests/grad_clip/cases.py covers the regimes it claims, the NumPy restatement of the kernels lies inside the
derived bounds on every case before any GPU run, wrong implementations fall outside, the reference is the rule worked by hand; the
hook class against a stub optimiser, the C ABI's declarations and host-side checks, and the trainer's new option."""
import ctypes
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest

from tests.grad_clip import cases as A

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


# ---- the grid ---------------------------------------------------------------------------------------------------------------------
def test_grid_covers_the_regimes_it_claims():
    from loans_amd import _lib
    assert A.UNIT == _lib.LARS_UNIT == 4096
    for n, want in A.REGIMES.items():
        assert A.regime(n) == want, n
    assert set(A.REGIMES) == {1, 3, 4, 5, 64, A.UNIT - 1, A.UNIT, A.UNIT + 1, 2 * A.UNIT + 3}
    assert A.units_of(A.N_LANE2) == A.LANES + 2 and A.regime(A.N_LANE2) == (65, 0, 1)      # a fold lane takes a second partial
    assert A.units_of(A.N_TRIP2) == A.GRID_CAP + 1 and A.regime(A.N_TRIP2) == (A.GRID_CAP, 1, 1)      # a block takes a second trip
    assert {n for _, n, _, _, _ in A.GRID} == set(A.SIZES)
    assert {kind for _, _, kind, _, _ in A.GRID} == set(A.KINDS + A.EDGES + A.BROKEN)
    assert {(gs, c) for _, _, kind, gs, c in A.GRID if kind == 'unit'} >= {(gs, c) for gs in A.GRAD_SCALES for c in A.THRESHOLDS}
    assert len(set(A.IDS)) == len(A.GRID)
    clipped = not_clipped = 0
    for name, n, kind, gs, c in A.GRID:
        g = A.make(n, kind, gs)
        assert len(g) == n + A.GUARD and np.isnan(g[n:]).all(), name
        N, k, _ = A.clip_ref(g, n, gs, c)
        with np.errstate(all='ignore'):
            s32 = np.sum(np.square(g[:n]), dtype=np.float32)
        if kind == 'tiny':
            assert s32 == 0 and 0 < N < 1e-20, name       # the squares vanish in fp32, not in fp64
        elif kind == 'huge':
            assert np.isinf(s32) and 1e24 < N < A.ABOVE, name
        elif kind == 'zero':
            assert N == 0.0 and k == 1.0, name
        elif kind in A.EDGES:
            assert N == 5.0 and (k == 1.0) == (kind in ('below', 'exact')), name
            assert np.float32(k) == (np.float32(1 - 2.0 ** -20) if kind == 'above20' else 1.0), name
        elif kind in A.BROKEN:
            assert not np.isfinite(N) and k == 1.0 and (np.isnan(N) if kind == 'nan' else np.isinf(N)), name
        else:
            assert np.isfinite(N) and N < A.ABOVE, name
        if c in (A.ABOVE, math.inf):
            assert k == 1.0, name
        clipped += k < 1.0
        not_clipped += k == 1.0
    assert clipped >= 15 and not_clipped >= 15


# ---- the restatement inside the bounds, on the whole grid -----------------------------------------------------------------------------
@pytest.mark.parametrize('name,n,kind,gs,c', A.GRID, ids=A.IDS)
def test_restatement_sits_inside_the_bounds(name, n, kind, gs, c):
    g = A.make(n, kind, gs)
    N32, k32 = A.record_numpy(g, n, gs, c)
    out = A.apply_numpy(g, n, k32)
    worst = A.check(N32, k32, out, g, n, gs, c)
    assert worst <= 1.0, worst
    want_k = A.clip_ref(g, n, gs, c)[1]
    if np.float32(want_k) != 1.0:
        assert not np.array_equal(out[:n], g[:n])
        with np.errstate(all='ignore'):
            after = abs(gs) * np.sqrt(np.sum(np.square(out[:n].astype(np.longdouble))))
        assert after <= A.clipped_norm_bound(n, c), (after, c)


def test_the_summation_order_is_a_function_of_n_alone():
    """the partial of unit u covers floats [UNIT u, ..) whichever block sums it: the first GRID_CAP partials of the two-trip size are
    those of its first GRID_CAP units taken alone"""
    g = A.make(A.N_TRIP2, 'unit')
    whole = A.partials_numpy(g, A.N_TRIP2)
    head = A.partials_numpy(g, A.GRID_CAP * A.UNIT)
    assert len(whole) == A.GRID_CAP + 1 and np.array_equal(whole[:A.GRID_CAP], head)
    a, b, c, d, e = (float(x) ** 2 for x in g[A.N_TRIP2 - 5:A.N_TRIP2])       # the last unit: thread 0's float4, then its scalar
    assert whole[-1] == (((a + b) + c) + d) + e
    # lanes: partial 64 goes to lane 0, behind partial 0
    parts = np.arange(1.0, 67.0)
    assert A.fold_numpy(parts) == parts.sum()


# ---- wrong implementations fall outside -------------------------------------------------------------------------------------------------
def _outside(n, kind, gs, c, record, apply=A.apply_numpy):
    g = A.make(n, kind, gs)
    right = A.check(*A.record_numpy(g, n, gs, c), A.apply_numpy(g, n, A.record_numpy(g, n, gs, c)[1]), g, n, gs, c)
    N32, k32 = record(g, n, gs, c)
    wrong = A.check(N32, k32, apply(g, n, k32), g, n, gs, c)
    assert right <= 1.0 < wrong, (right, wrong)


def test_wrong_implementations_fall_outside():
    F32 = np.float32

    def S64(g, n):
        return np.sum(np.square(g[:n].astype(np.float64)))

    def k_of(N, c):
        return c / N if np.isfinite(N) and N > c else 1.0

    def no_grad_scale(g, n, gs, c):
        N = np.sqrt(S64(g, n))
        return F32(N), F32(k_of(N, c))

    def always_scaling(g, n, gs, c):
        N = abs(gs) * np.sqrt(S64(g, n))
        return F32(N), F32(c / N)

    def over_the_square(g, n, gs, c):
        N = abs(gs) * np.sqrt(S64(g, n))
        return F32(N), F32(c / (N * N) if N > c else 1.0)

    def l1_norm(g, n, gs, c):
        N = abs(gs) * np.sum(np.abs(g[:n].astype(np.float64)))
        return F32(N), F32(k_of(N, c))

    def fp32_sums(g, n, gs, c):
        with np.errstate(all='ignore'):
            N = float(F32(abs(gs)) * np.sqrt(np.sum(np.square(g[:n]), dtype=np.float32)))
        return F32(N), F32(k_of(N, c))

    def clipped_at_equality(g, n, gs, c):
        N = abs(gs) * np.sqrt(S64(g, n))
        return F32(N), F32(c / N * (1 - 2.0 ** -20) if N >= c else 1.0)

    def per_parameter(g, n, k32):
        """each half clipped to c by its own norm (the record holds the global norm)"""
        out = g.copy()
        half = n // 2
        for lo, hi in ((0, half), (half, n)):
            N = np.sqrt(S64(g[lo:hi], hi - lo))
            out[lo:hi] = g[lo:hi] * F32(k_of(N, 1.0))
        return out

    def nan_written(g, n, k32):
        """Chainer's arithmetic on a non-finite norm: the whole gradient is multiplied by c / N"""
        out = g.copy()
        with np.errstate(all='ignore'):
            out[:n] = g[:n] * F32(0.0)
        return out

    n = A.N_KINDS
    _outside(n, 'unit', 0.5, 1.0, no_grad_scale)
    _outside(n, 'unit', 1.0, A.ABOVE, always_scaling)
    _outside(n, 'unit', 1.0, 1.0, over_the_square)
    _outside(n, 'unit', 1.0, 1.0, l1_norm)
    _outside(n, 'unit', 1.0, 1.0, A.record_numpy, per_parameter)
    _outside(n, 'huge', 1.0, 1.0, fp32_sums)
    _outside(n, 'tiny', 1.0, 1e-26, fp32_sums)
    _outside(n, 'exact', 1.0, 5.0, clipped_at_equality)
    _outside(n, 'inf', 1.0, 1.0, A.record_numpy, nan_written)


def test_reference_is_the_rule_by_hand():
    """g = (3, 4): |g| = 5"""
    g = np.array([3, 4, np.nan], np.float32)
    for gs, c, N, k in ((1.0, 1.0, 5.0, 0.2), (1.0, 2.5, 5.0, 0.5), (0.5, 1.0, 2.5, 0.4), (-0.5, 1.0, 2.5, 0.4), (1.0, 5.0, 5.0, 1.0),
                        (1.0, 6.0, 5.0, 1.0), (0.125, 1.0, 0.625, 1.0), (1.0, math.inf, 5.0, 1.0)):
        got_N, got_k, got_g = A.clip_ref(g, 2, gs, c)
        assert (got_N, got_k) == (N, pytest.approx(k, rel=1e-15)) and np.allclose(got_g, np.array([3.0, 4.0]) * k, rtol=1e-15, atol=0)
        N32, k32 = A.record_numpy(g, 2, gs, c)
        assert (N32, k32) == (np.float32(N), np.float32(k))
        assert np.array_equal(A.apply_numpy(g, 2, k32)[:2], g[:2] * np.float32(k))
    z = np.zeros(4, np.float32)
    assert A.clip_ref(z, 4, 1.0, 1.0)[:2] == (0.0, 1.0) and A.record_numpy(z, 4, 1.0, 1.0) == (0.0, 1.0)
    bad = np.array([3, np.inf, 4, np.nan], np.float32)
    assert A.clip_ref(bad, 3, 1.0, 1.0)[:2] == (math.inf, 1.0) and math.isnan(A.clip_ref(bad, 4, 1.0, 1.0)[0])
    assert A.additions(1) == 16 + 6 + 3 + 1 + 6 and A.additions(A.N_LANE2) == 16 + 6 + 3 + 2 + 6
    assert A.additions(6300 * A.UNIT) == 16 + 6 + 3 + 99 + 6


# ---- the hook, without a GPU -----------------------------------------------------------------------------------------------------------
def test_hook_class_against_a_stub_optimiser(monkeypatch):
    import torch
    import loans_amd
    from loans_amd import ops
    from loans_amd.runtime import optimizers
    assert loans_amd.GradientClipping is optimizers.GradientClipping and loans_amd.GradientClipping.name == 'GradientClipping'
    for bad in (0, 0.0, -1, float('nan'), -math.inf):
        with pytest.raises(ValueError, match='must be positive'):
            loans_amd.GradientClipping(bad)
    with pytest.raises(RuntimeError, match='no step'):
        loans_amd.GradientClipping(1.0).last_norm()
    calls = []

    class State:
        def __init__(self, numel, device):
            calls.append(('state', numel, str(device)))
            self.record = torch.tensor([2.5, 0.4])

    monkeypatch.setattr(ops, 'GradClipState', State)
    monkeypatch.setattr(ops, 'grad_norm', lambda g, c, state, gs=1.0: calls.append(('norm', g.data_ptr(), g.numel(), c, type(state), gs)))
    monkeypatch.setattr(ops, 'grad_clip_apply', lambda g, state: calls.append(('apply', g.data_ptr(), g.numel(), type(state))))
    grad = torch.zeros(24)
    arena = SimpleNamespace(grad=grad, numel=24, active_numel=16, device=torch.device('cpu'))
    opt = SimpleNamespace(target=SimpleNamespace(arena=arena), grad_scale=0.5)
    hook = loans_amd.GradientClipping(2)
    assert hook.threshold == 2.0 and isinstance(hook.threshold, float)
    hook(opt)
    hook(opt)
    step = [('norm', grad.data_ptr(), 16, 2.0, State, 0.5), ('apply', grad.data_ptr(), 16, State)]
    assert calls == [('state', 24, 'cpu')] + step + step            # allocated once, over the whole arena; the active prefix is clipped
    assert (hook.last_norm(), hook.last_coefficient()) == (2.5, pytest.approx(0.4))
    del calls[:]
    measure = loans_amd.GradientClipping(math.inf)
    measure(SimpleNamespace(target=SimpleNamespace(arena=arena)))           # (an optimiser that was never stepped has no grad_scale)
    assert calls == [('state', 24, 'cpu'), ('norm', grad.data_ptr(), 16, math.inf, State, 1.0)]       # measure only: no third launch
    # Chainer's surface: add_hook takes the object under its name, once
    real = loans_amd.MomentumSGD(lr=0.1)
    real.add_hook(hook)
    assert list(real._hooks) == ['GradientClipping'] and real._hooks['GradientClipping'] is hook
    with pytest.raises(KeyError):
        real.add_hook(loans_amd.GradientClipping(1.0))
    real.remove_hook('GradientClipping')
    assert not real._hooks
    for words in ('Synchronise', 'departure from Chainer', 'captured step'):
        assert words in loans_amd.GradientClipping.__doc__ + loans_amd.GradientClipping.last_norm.__doc__
    assert 'no gradient clipping' not in loans_amd.LAMB.__doc__


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_and_registered():
    from loans_amd import _lib
    with open(os.path.join(ROOT, 'include', 'loans_hip.h')) as f:
        header = f.read()
    for proto in ('int64_t loans_grad_clip_workspace_bytes(int64_t n);', 'int loans_grad_norm_f32(const float* g, int64_t n, double grad_scale, double max_norm,',
                  'int loans_grad_clip_apply_f32(float* g, int64_t n, const float* record_dev, void* stream);'):
        assert proto in header, proto
    p, i64, f64 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_double
    assert _lib.SIGNATURES['loans_grad_clip_workspace_bytes'] == [i64] and _lib.RESTYPES['loans_grad_clip_workspace_bytes'] is i64
    assert _lib.SIGNATURES['loans_grad_norm_f32'] == [p, i64, f64, f64, p, i64, p, p]
    assert _lib.SIGNATURES['loans_grad_clip_apply_f32'] == [p, i64, p, p]
    with open(os.path.join(ROOT, 'loans_amd', 'csrc', 'Makefile')) as f:
        assert ' clip.hip ' in f.read()


def test_host_side_checks_refuse_before_any_launch():
    """no GPU here: an entry that got as far as a launch would return a hipError_t, not LOANS_EINVAL / LOANS_ERANGE"""
    from loans_amd import _lib
    lib = _lib.load()
    EINVAL, ERANGE = -1, -2
    size = lib.loans_grad_clip_workspace_bytes
    assert [size(n) for n in (1, 4096, 4097, 3 * 4096, A.N_LANE2)] == [8, 8, 16, 24, 66 * 8]
    assert size(0) == EINVAL and size(-5) == EINVAL and size(2 ** 42) == 2 ** 30 * 8 and size(2 ** 42 + 1) == ERANGE
    g, ws, rec = 0x1000, 0x2000, 0x3000         # never dereferenced on the host

    def norm(g_=g, n=8, gs=1.0, c=1.0, ws_=ws, nbytes=8, rec_=rec):
        return lib.loans_grad_norm_f32(g_, n, gs, c, ws_, nbytes, rec_, 0)

    assert norm(g_=0) == EINVAL and norm(ws_=0) == EINVAL and norm(rec_=0) == EINVAL
    assert norm(g_=g + 4) == EINVAL and norm(g_=g + 8) == EINVAL and norm(ws_=ws + 8) == EINVAL and norm(rec_=rec + 4) == EINVAL
    assert norm(n=0) == EINVAL and norm(n=-8) == EINVAL
    assert norm(nbytes=7) == EINVAL and norm(n=4097, nbytes=8) == EINVAL
    assert norm(c=0.0) == EINVAL and norm(c=-1.0) == EINVAL and norm(c=float('nan')) == EINVAL
    assert norm(gs=math.inf) == EINVAL and norm(gs=-math.inf) == EINVAL and norm(gs=float('nan')) == EINVAL
    assert norm(n=2 ** 42 + 1, nbytes=2 ** 40) == ERANGE
    apply = lib.loans_grad_clip_apply_f32
    assert apply(0, 8, rec, 0) == EINVAL and apply(g, 8, 0, 0) == EINVAL and apply(g + 4, 8, rec, 0) == EINVAL
    assert apply(g, 8, rec + 4, 0) == EINVAL and apply(g, 0, rec, 0) == EINVAL and apply(g, 2 ** 42 + 1, rec, 0) == ERANGE


# ---- the trainer's option ---------------------------------------------------------------------------------------------------------------
def test_parser_takes_and_refuses(capsys):
    import train_imagenet as T
    assert T.parse_args(['--clip-grad-norm', '1.0']).clip_grad_norm == 1.0
    assert T.parse_args(['--optimizer', 'lamb', '--clip-grad-norm', 'inf']).clip_grad_norm == math.inf
    assert T.parse_args(['--optimizer', 'sgd', '--clip-grad-norm', '0.25', '--ema-decay', '0.9']).clip_grad_norm == 0.25
    plain = T.parse_args([])
    assert plain.clip_grad_norm is None and 'clip_grad_norm' not in vars(plain)
    assert 'clip_grad_norm' not in vars(T.parse_args(['--optimizer', 'lamb']))
    for bad in ('0', '-1', 'nan', '-inf'):
        with pytest.raises(SystemExit):
            T.parse_args(['--clip-grad-norm=' + bad])
        assert '--clip-grad-norm is the largest gradient norm a step is taken with: it must be positive' in capsys.readouterr().err, bad
    with pytest.raises(ValueError, match='must be positive'):
        T.check_clip_arguments(T.argparse.Namespace(clip_grad_norm=0.0))
    for words in ('--clip-grad-norm C', '``--lamb-eps``, ``--clip-grad-norm``', '--ema-decay 0.9999 --clip-grad-norm 1.0'):
        assert words in T.__doc__, words


def test_resume_table_holds_the_new_default():
    import train_imagenet as T
    from loans_amd.runtime import checkpoint
    assert T.RESUME_DEFAULTS_CLIP == {'clip_grad_norm': None}
    assert T.RESUME_DEFAULTS_WITH_CLIP == dict(T.RESUME_DEFAULTS_WITH_LAMB, **T.RESUME_DEFAULTS_CLIP)
    assert 'clip_grad_norm' not in T.RESUME_FIXED
    fixed = [k for k in T.RESUME_FIXED if k != 'gpus']
    # a checkpoint from before the option existed resumes, with and without the option
    args = T.parse_args(['--optimizer', 'lamb'])
    saved = {k: v for k, v in checkpoint.plain_arguments(args).items() if k not in T.Arguments._CLIP}
    assert checkpoint.check_arguments(saved, args, fixed, checkpoint.SILENT, T.RESUME_DEFAULTS_WITH_CLIP) == []
    later = T.parse_args(['--optimizer', 'lamb', '--clip-grad-norm', '1.0'])
    lines = checkpoint.check_arguments(saved, later, fixed, checkpoint.SILENT, T.RESUME_DEFAULTS_WITH_CLIP)
    assert [l.split()[1] for l in lines] == ['clip_grad_norm']
    # the threshold may change on resume, inf included: reported, not refused
    saved = checkpoint.plain_arguments(later)
    assert saved['clip_grad_norm'] == 1.0
    for argv in (['--clip-grad-norm', '2'], ['--clip-grad-norm', 'inf'], []):
        lines = checkpoint.check_arguments(saved, T.parse_args(['--optimizer', 'lamb'] + argv), fixed, checkpoint.SILENT, T.RESUME_DEFAULTS_WITH_CLIP)
        assert [l.split()[1] for l in lines] == ['clip_grad_norm'], argv
