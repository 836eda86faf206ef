"""-m gpu: loans_grad_norm_f32 and loans_grad_clip_apply_f32 against float64 inside the derived bounds on the case grid of
tests/grad_clip/cases.py; exactness where the rule is exact, repeatability, independence of the launch grid, the product's bits, the
guards, an index beyond 2^31 and the argument checks.  Every case is three launches over at most 34 MB (one over 8.6 GB of zeros)."""
import math

import numpy as np
import pytest
import torch

from tests.grad_clip import cases as A

pytestmark = pytest.mark.gpu

_SHARED = {}


def _values(n, kind, gs):
    key = (n, kind, gs if kind in A.EDGES else None)
    if key not in _SHARED:
        _SHARED[key] = A.make(n, kind, gs)
        _SHARED[key].setflags(write=False)
    return _SHARED[key]


def _bits(t):
    return (t.cpu().numpy() if torch.is_tensor(t) else t).view(np.int32)


def _run(g_h, n, gs, c, apply=True):
    """(N, k, g after) of the entries on a device copy of g_h; the record starts out as NaN"""
    from loans_amd import ops
    g = torch.from_numpy(np.array(g_h)).cuda()
    state = ops.GradClipState(n, g.device)
    state.record.fill_(float('nan'))
    ops.grad_norm(g[:n], c, state, gs)
    if apply:
        ops.grad_clip_apply(g[:n], state)
    N, k = state.record.cpu().numpy()
    return N, k, g.cpu().numpy()


@pytest.mark.parametrize('name,n,kind,gs,c', A.GRID, ids=A.IDS)
def test_record_and_gradient_against_float64(name, n, kind, gs, c):
    g_h = _values(n, kind, gs)
    N, k, got = _run(g_h, n, gs, c)
    worst = A.check(N, k, got, g_h, n, gs, c)
    print('%s: N %r k %r, error / bound %.3f' % (name, N, k, worst))
    assert worst <= 1.0, worst
    want_N, want_k, _ = A.clip_ref(g_h, n, gs, c)
    if kind in A.BROKEN:
        assert not np.isfinite(N) and k == 1.0 and np.array_equal(_bits(got), _bits(g_h))
    elif np.float32(want_k) == 1.0:
        assert k == 1.0 and np.array_equal(_bits(got), _bits(g_h))          # exact cases are exact: not a bit of g moved
        if kind in A.EDGES:
            assert N == 5.0
    else:
        # the bits are torch.mul's of g by the recorded k: one fp32 product per element
        want = torch.mul(torch.from_numpy(np.array(g_h[:n])).cuda(), torch.tensor(k, dtype=torch.float32, device='cuda'))
        assert np.array_equal(_bits(got[:n]), _bits(want))
        with np.errstate(all='ignore'):
            after = abs(gs) * np.sqrt(np.sum(np.square(got[:n].astype(np.longdouble))))
        assert after <= A.clipped_norm_bound(n, c), (after, c)
    assert np.array_equal(_bits(got[n:]), _bits(g_h[n:]))                  # the guards are intact


def test_k_of_one_leaves_every_bit_of_g():
    """-0.0, NaN payloads, subnormals and infinities survive a step that does not clip and one whose norm is not finite; the norm
    pass alone writes nothing to g"""
    from loans_amd import ops
    n = A.UNIT + 7
    g_h = np.zeros(n + A.GUARD, np.float32)
    g_h[n:] = np.nan
    odd = np.array([0x80000000, 0x00000001, 0x807fffff, 0x3f800000, 0xbf800001], np.uint32).view(np.float32)
    g_h[[0, 5, A.UNIT - 1, A.UNIT, n - 1]] = odd
    N, k, got = _run(g_h, n, 1.0, 2.0)
    assert k == 1.0 and N == np.float32(np.sqrt(np.sum(np.square(g_h[:n].astype(np.float64))))) and np.array_equal(_bits(got), _bits(g_h))
    payload = g_h.copy()
    payload.view(np.uint32)[[3, n - 2]] = [0x7fc12345, 0xff800000]       # a NaN with a payload and -inf
    N, k, got = _run(payload, n, 1.0, 1e-3)
    assert math.isnan(N) and k == 1.0 and np.array_equal(_bits(got), _bits(payload))
    N, k, got = _run(A.make(A.N_KINDS, 'unit'), A.N_KINDS, 1.0, 1.0, apply=False)
    assert k < 1.0 and np.array_equal(_bits(got), _bits(A.make(A.N_KINDS, 'unit')))
    # measure only: the host issues no third launch (ops.grad_clip_apply would return at k == 1 anyway)
    N, k, got = _run(A.make(A.N_KINDS, 'unit'), A.N_KINDS, 1.0, math.inf)
    assert k == 1.0 and N > 1.0


@pytest.mark.parametrize('n', [A.N_KINDS, A.N_LANE2, A.N_TRIP2])
def test_two_runs_give_the_same_bits(n):
    g_h = _values(n, 'unit', 1.0)
    a, b = _run(g_h, n, 0.5, 1.0), _run(g_h, n, 0.5, 1.0)
    assert a[1] < 1.0
    for x, y in zip(a, b):
        assert np.array_equal(_bits(np.asarray(x)), _bits(np.asarray(y)))


def test_the_result_does_not_depend_on_the_launch_grid():
    """the two-trip buffer (GRID_CAP + 1 units: block 0 sums units 0 and GRID_CAP) against the same buffer summed in two launches of
    one trip each: the per-unit partials are the same bits, and so are N, k and g'"""
    from loans_amd import ops
    n, head = A.N_TRIP2, A.GRID_CAP * A.UNIT
    g_h = _values(n, 'unit', 1.0)
    g = torch.from_numpy(np.array(g_h)).cuda()
    whole = ops.GradClipState(n, g.device)
    ops.grad_norm(g[:n], 1.0, whole, 0.5)
    # the first GRID_CAP units alone (every block one trip), then the last unit alone, into one workspace
    parts = ops.GradClipState(n, g.device)
    scratch = ops.GradClipState(n, g.device)
    ops.grad_norm(g[:head], 1.0, parts, 0.5)
    ops.grad_norm(g[head:n], 1.0, scratch, 0.5)
    parts.workspace[A.GRID_CAP:].copy_(scratch.workspace[:1])
    assert np.array_equal(_bits(whole.workspace.view(torch.float32)), _bits(parts.workspace.view(torch.float32)))
    want = A.partials_numpy(g_h, n)
    assert np.all(np.abs(whole.workspace.cpu().numpy() - want) <= 25 * A.U64 * want)
    # the record is a function of the partials alone (one wave, whatever the grid of the first launch was): it is the
    # restatement's fold of these partials, rounded to fp32 once (one ulp of fp32 covers a last-bit difference in the root)
    N32, k32 = A.record_numpy(g_h, n, 0.5, 1.0)
    N, k = whole.record.cpu().numpy()
    assert abs(float(N) - float(N32)) <= 2 * A.U32 * float(N32) and abs(float(k) - float(k32)) <= 2 * A.U32 * float(k32)
    # g' of the whole buffer in one launch (grid capped, a grid stride) = g' of its two pieces in two launches
    a, b = g.clone(), g.clone()
    ops.grad_clip_apply(a[:n], whole)
    ops.grad_clip_apply(b[:head], whole)
    ops.grad_clip_apply(b[head:n], whole)
    assert torch.equal(a[:n], b[:n]) and not torch.equal(a[:n], g[:n])
    assert np.array_equal(_bits(a[n:]), _bits(g_h[n:]))


def test_an_index_beyond_two_to_the_31():
    """2^31 + UNIT + 3 floats, all zero but a 3 and a 4 behind index 2^31: N is exactly 5, and with c = 2.5 the two become 1.5 and 2"""
    from loans_amd import ops
    n = 2 ** 31 + A.UNIT + 3
    g = torch.zeros(n + A.GUARD, device='cuda', dtype=torch.float32)
    g[n:] = float('nan')
    g[2 ** 31 + 5] = 3.0
    g[n - 1] = -4.0
    state = ops.GradClipState(n, g.device)
    ops.grad_norm(g[:n], 2.5, state, 1.0)
    assert state.record.cpu().tolist() == [5.0, 0.5]
    ops.grad_clip_apply(g[:n], state)
    assert g[2 ** 31 + 5].item() == 1.5 and g[n - 1].item() == -2.0 and int(torch.count_nonzero(g[:n])) == 2
    assert torch.isnan(g[n:]).all()
    del g, state
    torch.cuda.empty_cache()


def test_argument_checks_launch_nothing():
    from loans_amd import _lib, ops
    lib = _lib.load()
    EINVAL, ERANGE = -1, -2
    n = 40
    g_h = np.random.RandomState(7).standard_normal(n).astype(np.float32)
    g = torch.from_numpy(g_h).cuda()
    state = ops.GradClipState(n, g.device)
    state.record.fill_(7.0)
    state.workspace.fill_(7.0)
    assert state.workspace.numel() * 8 == lib.loans_grad_clip_workspace_bytes(n) == 8
    with pytest.raises(_lib.HipKernelError, match='LOANS_EINVAL'):
        ops.GradClipState(0, g.device)
    with pytest.raises(ValueError, match='was given'):
        ops.grad_norm(torch.zeros(4200, device='cuda'), 1.0, state)

    def norm(g_=None, n_=n, gs=1.0, c=1.0, ws=None, nbytes=8, rec=None):
        return lib.loans_grad_norm_f32(g.data_ptr() if g_ is None else g_, n_, gs, c, state.workspace.data_ptr() if ws is None else ws, nbytes,
                                       state.record.data_ptr() if rec is None else rec, ops._stream())

    def apply(g_=None, n_=n, rec=None):
        return lib.loans_grad_clip_apply_f32(g.data_ptr() if g_ is None else g_, n_, state.record.data_ptr() if rec is None else rec, ops._stream())

    assert norm(g_=0) == EINVAL and norm(ws=0) == EINVAL and norm(rec=0) == EINVAL                     # null pointers
    assert norm(g_=g.data_ptr() + 4) == EINVAL and norm(ws=state.workspace.data_ptr() + 8) == EINVAL    # misaligned
    assert norm(rec=state.record.data_ptr() + 4) == EINVAL
    assert norm(n_=0) == EINVAL and norm(n_=-4) == EINVAL and norm(n_=2 ** 42 + 4) == ERANGE
    assert norm(nbytes=7) == EINVAL and norm(nbytes=0) == EINVAL                                        # a workspace that is too small
    assert norm(c=0.0) == EINVAL and norm(c=-1.0) == EINVAL and norm(c=float('nan')) == EINVAL
    assert norm(gs=math.inf) == EINVAL and norm(gs=float('nan')) == EINVAL
    assert apply(g_=0) == EINVAL and apply(rec=0) == EINVAL and apply(g_=g.data_ptr() + 8) == EINVAL
    assert apply(rec=state.record.data_ptr() + 4) == EINVAL and apply(n_=0) == EINVAL and apply(n_=2 ** 42 + 4) == ERANGE
    torch.cuda.synchronize()
    assert np.array_equal(_bits(g), _bits(g_h)) and (state.record == 7.0).all() and (state.workspace == 7.0).all()
    # ... and sane arguments are taken: a negative grad_scale counts by its magnitude, inf is a threshold
    assert norm(gs=-0.5, c=math.inf) == 0 and apply() == 0
    torch.cuda.synchronize()
    N, k = state.record.cpu().numpy()
    assert k == 1.0 and abs(N - 0.5 * np.sqrt(np.sum(g_h.astype(np.float64) ** 2))) <= 2 * A.U32 * N and np.array_equal(_bits(g), _bits(g_h))
