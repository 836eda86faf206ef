"""Case grid, float64 reference, derived bounds and NumPy restatements for the LAMB kernels (csrc/lamb.hip: lamb_moments_kernel,
lamb_fold_kernel, lamb_update_kernel); not collected by pytest.  The same functions run on the restatement (test_cases_cpu.py, before
any GPU run) and on the kernels (test_gpu_kernels.py, test_gpu_model.py).  The sizes, the tables, the guard convention and the
summation order of the norms are tests/imagenet_lars/cases.py's: the two optimisers cut the arena the same way.

THE RULE.  Step t (1-based), gs = grad_scale; segment s has flag byte f (bit 0 = no weight decay, bit 1 = no adaptation):
    g^  = g * gs
    m'  = m + (1 - beta1) (g^ - m)
    v'  = v + (1 - beta2) (g^ g^ - v)
    c1  = 1 / (1 - beta1^t)      c2 = 1 / (1 - beta2^t)
    a   = (m' c1) / (sqrt(v' c2) + eps)
    wd_s = (f & 1) ? 0 : wd
    u   = a + wd_s p
    W   = |p|_2 over the segment     U = |u|_2 over the segment
    r   = (f & 2) or W == 0 or U == 0 ?  1  :  W / U
    p'  = p - (lr r) u
No case has |g gs| above 1e15: v = g^2 overflowing fp32 (beyond ~1e19) is the rule's own limit, not the kernel's.

THE ELEMENTWISE BOUNDS (u = 2^-24; UF = 2^-126 wherever an fp32 result can underflow and the float64 one cannot; sqrtf and the
division are budgeted at 2 ulp = 4 u each, as tests/misc_kernels/cases.py: adam_ref budgets Adam's).  The kernel is
    g^ = fl(g fl(gs));  m' = fmaf(omb1, fl(g^ - m), m);  v' = fmaf(omb2, fmaf(g^, g^, -v), v)
    a = fl(fl(m' c1) / fl(fl(sqrt(fl(v' c2))) + eps));  u = fmaf(wd_s, p, a);  p' = fmaf(-fl(lr32 r32), u, p)
with every scalar rounded to fp32 once.  An fmaf rounds once.  Counting roundings, with incoming errors e_m, e_v, e_p (zero for
a step from given fp32 state):
    e_g   = 2 u |g^| + UF                                           fl(gs), the product
    e_m'  = beta1 e_m + omb1 e_g    + 2 u |omb1 d| + u |m'| + UF    d = g^ - m: its rounding, fl(omb1); the fmaf's result
    e_dv  = 4 u g^2 + u |dv| + UF                                   dv = g^2 - v: 2 |g^| e_g = 4 u g^2, the inner fmaf's result
    e_v'  = beta2 e_v + omb2 e_dv    + u |omb2 dv| + u |v'| + UF    fl(omb2); the outer fmaf's result
    e_num = c1 e_m' + 2 u |m' c1| + UF                              fl(c1), the product
    e_x   = c2 e_v' + 2 u x + UF                                    x = v' c2
    e_sq  = min(e_x / (2 sqrt x), sqrt e_x) + 4 u sqrt x            |sqrt(x + e) - sqrt x| <= both; sqrtf
    e_den = e_sq + u eps + u den                                    fl(eps); the sum
    e_a   = e_num / den + |a| e_den / den + 4 u |a| + UF            the division
    e_u   = e_a + wd_s e_p + u |wd_s p| + u |u| + UF                fl(wd); the fmaf's result
THE RATIO BOUND.  tests/imagenet_lars/cases.py derives (u32 + C T u64) for a quotient of two such norms rounded to fp32 once (T
additions per term, C = 2): W / U is that quotient without LARS's denominator sum, T + 3 <= 2 T.  The kernel's U^ is the norm of the
COMPUTED u: | |u^| - |u| | <= |e_u|_2, so rel_r gains |e_u|_2 / U, and from the second step on |e_p|_2 / W in the same way:
    rel_r = u32 + C T u64 + |e_u|_2 / U + |e_p|_2 / W
A ratio the rule makes exactly 1 (flag bit 1, W = 0, U = 0) is compared exactly: u = 0 in float64 means a = 0 and wd_s p = 0
elementwise, which fp32 reproduces exactly.
THE STEP BOUND.
    e_p'  = e_p + lr r e_u + (u32 + rel_r) |lr r u| + u |p'| + UF   the product fl(lr32 r32) and r's own error; the fmaf's result
and one more u |lr r u| where lr is no fp32 number (fl(lr); the grid's LR = 2^-6 is one).  Everything is multiplied by
SLACK = 1.01 for the second-order terms, as in tests/imagenet_lars/cases.py.  Nothing here was read off a kernel's output; no element
and no segment is excluded.

A CONSEQUENCE: wherever a segment adapts (r != 1 by the rule), |p' - p|_2 = lr r U = lr W, at every step and whatever the gradient."""
import numpy as np

from tests.imagenet_lars import cases as L
from tests.imagenet_lars.cases import (UNIT, GRID_CAP, MAX_SEGMENTS, GUARD, REGIMES, TABLES, KINDS, PREFIX_FULL, PREFIX_N, RESNET_SHAPES,  # noqa: F401
                                       first_units, additions, kinds_of, regime, arena_layout, table_of, _unit_sums, _segment_sum)

U32, U64, SLACK, C, F32 = L.U32, L.U64, L.SLACK, L.C, L.F32
UF = 2.0 ** -126
ULP2 = 4 * U32
S_GUARD = L.V_GUARD            # the sentinel behind n in the state buffers m and v

BETA1, BETA2, EPS = 0.9, 0.999, 1e-6
LR = 2.0 ** -6
STEPS = (1, 2, 1000)
GRAD_SCALES = L.GRAD_SCALES
DECAYS = L.DECAYS

# (table, t, grad_scale, weight decay, warm): every table at step 2 from non-zero moments; every step, scale, decay and both kinds of
# incoming state on the table that holds every kind of values under every flag byte; the ResNet-like table once more from zeros
GRID = [(name, 2, 1.0, 5e-5, True) for name in TABLES] + \
       [('kinds', t, gs, wd, warm) for t in STEPS for gs in GRAD_SCALES for wd in DECAYS for warm in (False, True)
        if (t, gs, wd, warm) != (2, 1.0, 5e-5, True)] + [('resnet', 1, 0.125, 0.0, False), ('prefix', 1000, 0.5, 0.0, False)]
IDS = ['%s-t%d-gs%g-wd%g-%s' % (c[0], c[1], c[2], c[3], 'warm' if c[4] else 'cold') for c in GRID]


def corrections(t, beta1=BETA1, beta2=BETA2):
    """(c1, c2) in double, as the optimiser forms them"""
    return 1.0 / (1.0 - beta1 ** t), 1.0 / (1.0 - beta2 ** t)


def make(name, warm=True, seed=0):
    """(p, g, m, v) fp32 of n + GUARD floats for table ``name``: unit-scale weights, gradients 1e-3 of them, moments of the
    gradients' scale (v >= 0; all zero unless ``warm``), and per kinds_of() a segment of zero weights, of zero gradients with zero
    moments, of magnitudes 1e-25 (squares vanish in fp32, not in fp64), of weights of 1e25 with unit-scale gradients (the norm's
    squares overflow fp32, not fp64).  NaNs behind n in p and g, S_GUARD in m and v."""
    n, ends, flags = TABLES[name]
    rng = np.random.RandomState([seed, n % 65521, len(ends), 77])
    p = rng.standard_normal(n + GUARD).astype(F32)
    g = (1e-3 * rng.standard_normal(n + GUARD)).astype(F32)
    m = (3e-4 * rng.standard_normal(n + GUARD)).astype(F32)
    v = (1e-6 * rng.uniform(0.1, 2.0, n + GUARD)).astype(F32)
    if not warm:
        m[:], v[:] = 0, 0
    lo = 0
    for hi, kind in zip(ends, kinds_of(len(ends), name)):
        if kind == 'zero_w':
            p[lo:hi] = 0
        elif kind == 'zero_g':
            g[lo:hi] = m[lo:hi] = v[lo:hi] = 0
        elif kind == 'tiny':
            p[lo:hi] *= F32(1e-25)
            g[lo:hi] *= F32(1e-25)
            m[lo:hi] *= F32(1e-25)
            v[lo:hi] = 0                    # (1e-50 of it is no fp32 number)
        elif kind == 'huge':
            p[lo:hi] *= F32(1e25)
            g[lo:hi] *= F32(1e3)
            m[lo:hi] *= F32(1e3)
            v[lo:hi] *= F32(1e6)
        lo = hi
    p[n:], g[n:], m[n:], v[n:] = np.nan, np.nan, S_GUARD, S_GUARD
    return p, g, m, v


def _per_element(ends, values):
    return np.repeat(np.asarray(values), np.diff(np.asarray(ends), prepend=0))


# ---- float64 reference ------------------------------------------------------------------------------------------------------------
def _norm(x):
    return float(np.sqrt(np.sum(np.square(x.astype(np.longdouble)))))


def lamb_ref(p, g, m, v, ends, flags, t, lr, wd, gs, beta1=BETA1, beta2=BETA2, eps=EPS):
    """one step of the rule in float64, the norms summed in np.longdouble -> dict(p, m, v, u, r, W, U); r, W, U per segment"""
    n = ends[-1]
    p64, g64, m64, v64 = (np.asarray(a[:n], np.float64) for a in (p, g, m, v))
    c1, c2 = corrections(t, beta1, beta2)
    gh = g64 * gs
    m1 = m64 + (1 - beta1) * (gh - m64)
    v1 = v64 + (1 - beta2) * (gh * gh - v64)
    a = (m1 * c1) / (np.sqrt(v1 * c2) + eps)
    wd_e = _per_element(ends, [0.0 if f & 1 else wd for f in flags])
    u = a + wd_e * p64
    r, Ws, Us = [], [], []
    lo = 0
    for hi, f in zip(ends, flags):
        W, U = _norm(p64[lo:hi]), _norm(u[lo:hi])
        r.append(1.0 if f & 2 or W == 0 or U == 0 else W / U); Ws.append(W); Us.append(U)
        lo = hi
    r, Ws, Us = np.asarray(r), np.asarray(Ws), np.asarray(Us)
    p1 = p64 - lr * _per_element(ends, r) * u
    return dict(p=p1, m=m1, v=v1, u=u, r=r, W=Ws, U=Us)


def lamb_bounds(p, g, m, v, ends, flags, t, lr, wd, gs, beta1=BETA1, beta2=BETA2, eps=EPS, ep=0.0, em=0.0, ev=0.0, T=None):
    """the bounds of the module docstring around lamb_ref's values -> dict(p, m, v, u (per element), rel_r, W, U (per segment)).
    ``ep``, ``em``, ``ev``: bounds on the incoming state's own error; ``T``: the additions per segment where the kernel's segment
    is longer than ``ends`` says (an arena pads a parameter with zeros)"""
    n = ends[-1]
    ref = lamb_ref(p, g, m, v, ends, flags, t, lr, wd, gs, beta1, beta2, eps)
    p64, g64, m64, v64 = (np.asarray(a[:n], np.float64) for a in (p, g, m, v))
    ep, em, ev = (np.broadcast_to(np.asarray(e, np.float64), (n,)) for e in (ep, em, ev))
    c1, c2 = corrections(t, beta1, beta2)
    a1, b1 = 1 - beta1, 1 - beta2
    u_ = U32
    with np.errstate(all='ignore'):
        gh = g64 * gs
        e_g = 2 * u_ * np.abs(gh) + UF
        d = gh - m64
        e_m = beta1 * em + a1 * e_g + 2 * u_ * np.abs(a1 * d) + u_ * np.abs(ref['m']) + UF
        dv = gh * gh - v64
        e_dv = 4 * u_ * gh * gh + u_ * np.abs(dv) + UF
        e_v = beta2 * ev + b1 * e_dv + u_ * np.abs(b1 * dv) + u_ * np.abs(ref['v']) + UF
        num = ref['m'] * c1
        e_num = c1 * e_m + 2 * u_ * np.abs(num) + UF
        x = ref['v'] * c2
        e_x = c2 * e_v + 2 * u_ * x + UF
        sq = np.sqrt(x)
        e_sq = np.minimum(np.where(sq > 0, e_x / (2 * sq), np.inf), np.sqrt(e_x)) + ULP2 * sq
        den = sq + eps
        e_den = e_sq + u_ * eps + u_ * den
        a = num / den
        e_a = e_num / den + np.abs(a) * e_den / den + ULP2 * np.abs(a) + UF
        wd_e = _per_element(ends, [0.0 if f & 1 else wd for f in flags])
        e_u = e_a + wd_e * ep + u_ * np.abs(wd_e * p64) + u_ * np.abs(ref['u']) + UF
        T = additions(ends) if T is None else np.asarray(T, np.float64)
        rel_r, bW, bU = [], [], []
        lo = 0
        for hi, f, W, U, Ts in zip(ends, flags, ref['W'], ref['U'], T):
            nu, npn = _norm(e_u[lo:hi]), _norm(ep[lo:hi])
            fold = C * Ts * U64
            bW.append((fold * W + npn) * SLACK); bU.append((fold * U + nu) * SLACK)
            rel_r.append(0.0 if (f & 2 or W == 0 or U == 0) else U32 + fold + nu / U + npn / W)
            lo = hi
        rel_r = np.asarray(rel_r)
        rate = lr * _per_element(ends, ref['r'])
        step = np.abs(rate * ref['u'])
        lr_round = 0.0 if float(F32(lr)) == lr else U32
        e_p = ep + rate * e_u + (U32 + lr_round + _per_element(ends, rel_r)) * step + u_ * np.abs(ref['p']) + UF
    return dict(ref=ref, p=e_p * SLACK, m=e_m * SLACK, v=e_v * SLACK, u=e_u * SLACK, rel_r=rel_r * SLACK, W=np.asarray(bW), U=np.asarray(bU))


def check(got, p, g, m, v, ends, flags, t, lr, wd, gs, **kw):
    """``got``: dict with any of p, m, v, u (fp32 arrays of >= n floats), r (fp32 per segment), norms ((nseg, 2) float64).  ->
    {name: the largest error / bound over ALL elements or segments} (<= 1 passes); ratios that the rule makes exactly 1 must be
    exactly 1"""
    n = ends[-1]
    b = lamb_bounds(p, g, m, v, ends, flags, t, lr, wd, gs, **kw)
    ref = b['ref']
    worst = {}
    for name in ('p', 'm', 'v', 'u'):
        if name in got:
            have = np.asarray(got[name][:n], np.float64)
            assert np.isfinite(have).all(), name + ' is not finite'
            worst[name] = float((np.abs(have - ref[name]) / b[name]).max())
    if 'r' in got:
        have = np.asarray(got['r'], np.float64)
        assert have.shape == ref['r'].shape and np.isfinite(have).all(), 'a ratio is not finite'
        one = b['rel_r'] == 0.0
        assert np.array_equal(have[one], np.ones(int(one.sum()))), 'a ratio that the rule makes 1 is not exactly 1'
        worst['r'] = float((np.abs(have - ref['r'])[~one] / (b['rel_r'] * ref['r'])[~one]).max()) if (~one).any() else 0.0
    if 'norms' in got:
        have = np.asarray(got['norms'], np.float64).reshape(-1, 2)
        with np.errstate(all='ignore'):
            for k, name in enumerate('WU'):
                err, bound = np.abs(have[:, k] - ref[name]), b[name]
                assert np.array_equal(have[bound == 0, k], ref[name][bound == 0]), name
                worst[name] = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    return worst


def adapting(ref, flags):
    """the segments whose ratio the rule does not make 1"""
    return np.asarray([not (f & 2 or W == 0 or U == 0) for f, W, U in zip(flags, ref['W'], ref['U'])])


def identity_check(got_p, p, g, m, v, ends, flags, t, lr, wd, gs, **kw):
    """for every adapting segment | |p' - p|_2 / (lr |p|_2) - 1 | over its tolerance, the 2-norm of the p' bound over lr W
    (| |x^| - |x| | <= |x^ - x|_2); the largest (<= 1 passes), and the number of segments it covers"""
    b = lamb_bounds(p, g, m, v, ends, flags, t, lr, wd, gs, **kw)
    worst, count, lo = 0.0, 0, 0
    for hi, on, W in zip(ends, adapting(b['ref'], flags), b['ref']['W']):
        if on:
            moved = _norm(np.asarray(got_p[lo:hi], np.float64) - np.asarray(p[lo:hi], np.float64))
            worst = max(worst, abs(moved / (lr * W) - 1.0) / (_norm(b['p'][lo:hi]) / (lr * W)))
            count += 1
        lo = hi
    return worst, count


# ---- the kernels' arithmetic in NumPy ---------------------------------------------------------------------------------------------
def _fma(a, b, c):
    """fmaf: the product of two fp32 numbers is exact in float64; the sum rounds there first (a double rounding in rare ties, a
    relative 2^-53 that SLACK covers)"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


VARIANTS = ('eps_inside_root', 'no_bias_correction', 'ratio_inverted', 'coupled_decay', 'one_d_adapts')


def lamb_numpy(p, g, m, v, ends, flags, t, lr, wd, gs, beta1=BETA1, beta2=BETA2, eps=EPS, wrong=None):
    """the three passes in fp32, operation for operation, the norms in the kernels' summation order -> dict(p, m, v, u, r, norms).
    ``wrong``: one of VARIANTS, a mistake the bounds have to catch"""
    n = ends[-1]
    p, g, m, v = (np.asarray(a[:n], F32) for a in (p, g, m, v))
    c1, c2 = corrections(t, beta1, beta2)
    if wrong == 'no_bias_correction':
        c1 = c2 = 1.0
    omb1, omb2, c1, c2, eps32, gs32 = F32(1.0 - beta1), F32(1.0 - beta2), F32(c1), F32(c2), F32(eps), F32(gs)
    wd_e = _per_element(ends, [F32(0.0 if f & 1 else wd) for f in flags]).astype(F32)
    with np.errstate(all='ignore'):
        gh = g * gs32
        if wrong == 'coupled_decay':
            gh = gh + wd_e * p
        m1 = _fma(omb1, gh - m, m)
        v1 = _fma(omb2, _fma(gh, gh, -v), v)
        if wrong == 'eps_inside_root':
            a = (m1 * c1) / np.sqrt(v1 * c2 + eps32)
        else:
            a = (m1 * c1) / (np.sqrt(v1 * c2) + eps32)
        u = a if wrong == 'coupled_decay' else _fma(wd_e, p, a)
        r32, norms = np.empty(len(ends), F32), np.empty((len(ends), 2))
        lo = 0
        for s, (hi, f) in enumerate(zip(ends, flags)):
            W, U = np.sqrt(_segment_sum(p[lo:hi])), np.sqrt(_segment_sum(u[lo:hi]))
            r = 1.0
            if (wrong == 'one_d_adapts' or not f & 2) and W > 0.0 and U > 0.0:
                r = U / W if wrong == 'ratio_inverted' else W / U
            r32[s], norms[s] = F32(r), (W, U)
            lo = hi
        rate = F32(lr) * r32                                  # ONE fp32 product per segment
        p1 = _fma(-_per_element(ends, rate).astype(F32), u, p)
    return dict(p=p1, m=m1, v=v1, u=u, r=r32, norms=norms)
