"""Case grid, float64 reference, derived bounds and NumPy restatements for the LARS kernels (csrc/sgd.hip: lars_partials_kernel,
lars_fold_kernel, momentum_sgd_seg_kernel<true>); not collected by pytest.  The same functions run on the restatement (test_cases_cpu.py, before
any GPU run) and on the kernels (test_gpu_kernels.py, test_gpu_model.py).

THE RULE, per segment s of the flat buffer with flag byte f:
    W = sqrt(sum p_i^2)     G = |gs| sqrt(sum g_i^2)     wd_s = (f & 1) ? 0 : wd
    r = (f & 2) ? 1 : (W > 0 and G > 0 ? eta W / (G + wd_s W + eps) : 1)
    g' = g gs + wd_s p;   v' = mom v - (lr r) g';   p' = p + v'

THE RATIO BOUND.  u64 = 2^-53, u32 = 2^-24.  The kernel converts every fp32 element to double and squares it: exact (24 + 24 bits
in 53).  Only additions round.  A term passes at most T of them:
    16      a thread's own elements (four float4 of a full unit)
     6      the xor butterfly of the wave
     3      waves 0..3 through LDS
    units   the fold, a segment's partials in ascending unit order (units = ceil(length / UNIT))
All terms are non-negative, so the computed sum of squares S^ has |S^ - S| <= T u64 S at first order.  From there, relative errors:
    W^ = sqrt(S_p^)            T/2 + 1      (the root halves the error and rounds once)
    G^ = |gs| sqrt(S_g^)       T/2 + 2
    wd W^                      T/2 + 2
    G^ + wd W^ + eps           T/2 + 4      (positive terms: the sum's relative error is at most the largest term's, + 1 per addition)
    eta W^                     T/2 + 2
    the quotient               T + 7        (numerator + denominator + 1)
in units of u64, and T + 7 <= 2 T because T >= 25.  Then ONE rounding to fp32.  So
    |r^ - r| <= (u32 + C T u64) |r| SLACK,       C = 2
Only the u32 matters at first order.  SLACK = 1.01 covers the second-order terms, as in tests/imagenet/reference.py.  The
reference sums in np.longdouble (64-bit mantissa): its own error is below 2^-60 and is not in the bound.  No element and no
segment is excluded; a ratio of exactly 1 (flag bit 1, or a zero norm) is compared exactly.

THE STEP BOUND.  The update is momentum SGD with lr r in place of lr.  tests/imagenet_sgd/reference.py: momentum_sgd_bound holds a
kernel whose rate is the double rounded to fp32 once (relative u32).  Here the rate is fl(fl(lr) r^): two roundings and the error of
r^, so beside momentum_sgd_bound(p, g, v, lr r, ...) the term d = lr r g' carries (u32 + rel_r) |d| more, with rel_r the relative
error of r^ -- the ratio bound above plus, from the second step on, the effect of the incoming error e_p of p on W:
| |p^| - |p| | <= |e_p|_2, and r grows no faster than W (d ln r / d ln W <= 1), so rel_r += |e_p|_2 / W.
Nothing here was read off a kernel's output."""
import numpy as np

from tests.imagenet_sgd import reference as S

U32 = 2.0 ** -24
U64 = 2.0 ** -53
SLACK = 1.01
C = 2
F32 = np.float32

# ---- constants of the kernels that the grid mirrors -------------------------------------------------------------------------------
UNIT = 4096             # LOANS_LARS_UNIT: floats per unit of work, one block per unit and trip (256 threads x 4 float4)
GRID_CAP = 2048         # grid_for's max_blocks: beyond GRID_CAP units a block takes a second trip
MAX_SEGMENTS = 1024     # LOANS_LARS_MAX_SEGMENTS
GUARD = 8               # floats behind n: NaN in p and g, V_GUARD in v
V_GUARD = F32(-54321.0)

ETA, EPS = 0.001, 1e-8
GRAD_SCALES = (1.0, 0.5, 0.125)
DECAYS = (0.0, 5e-5)
UPDATE_HYPER = dict(lr=0.4, momentum=0.9)


def first_units(ends):
    """(first unit per segment, units)"""
    per = [-(-(e - s) // UNIT) for s, e in zip([0] + list(ends[:-1]), ends)]
    return [sum(per[:i]) for i in range(len(per))], sum(per)


def regime(n):
    """(full units, float4 of the short last unit, single floats behind them) of a single segment of n floats"""
    full, rest = divmod(n, UNIT)
    return full, rest // 4, rest % 4


# n of a single segment -> the regime it reaches; test_cases_cpu.py recomputes every entry
REGIMES = {
    1: (0, 0, 1),               # one thread, one scalar
    3: (0, 0, 3),               # scalars only
    4: (0, 1, 0),               # one float4, no tail
    5: (0, 1, 1),               # a float4 and a scalar
    64: (0, 16, 0),             # a BN scale
    UNIT - 1: (0, 1023, 3),     # the short path at its longest: a thread takes float4 k, k + 1024 .. and three scalars follow
    UNIT: (1, 0, 0),            # the unrolled path, nothing else
    UNIT + 1: (1, 0, 1),        # a second unit of a single scalar
    2 * UNIT + 3: (2, 0, 3),    # two units + 3
}

KINDS = ('unit', 'zero_w', 'zero_g', 'tiny', 'huge')


def _resnet50_like():
    """161 parameters in ResNet-50's order and proportions at 3/16 of its widths and 1001 classes: 53 x (conv W, gamma, beta), fc W,
    fc b.  Widths of 12 and 1001 give sizes that are no multiple of 8, and one that is no multiple of 4.  -> (shapes)"""
    shapes = []

    def conv(cout, cin, k):
        shapes.extend([(cout, cin, k, k), (cout,), (cout,)])

    conv(12, 3, 7)
    cin = 12
    for mid, blocks in ((12, 3), (24, 4), (48, 6), (96, 3)):
        for b in range(blocks):
            if b == 0:
                conv(mid * 4, cin, 1)           # the projection shortcut
            conv(mid, cin, 1)
            conv(mid, mid, 3)
            conv(mid * 4, mid, 1)
            cin = mid * 4
    shapes.extend([(1001, cin), (1001,)])
    return shapes


def arena_layout(shapes):
    """(sizes, offsets, numel) as ParamArena lays parameters out: every one padded to 8 floats"""
    sizes = [int(np.prod(s)) for s in shapes]
    offsets, at = [], 0
    for n in sizes:
        offsets.append(at)
        at += (n + 7) // 8 * 8
    return sizes, offsets, at


def table_of(shapes, exempt_decay_1d=True):
    """(n, ends, flags) of the layout: 1-d parameters carry bit 1 (and bit 0 with ``exempt_decay_1d``); a parameter that adapts is
    a segment of its own, 1-d neighbours of equal flags are one"""
    sizes, offsets, numel = arena_layout(shapes)
    ends, flags = [], []
    for shape, stop in zip(shapes, offsets[1:] + [numel]):
        flag = (2 | (1 if exempt_decay_1d else 0)) if len(shape) <= 1 else 0
        if flags and flag & 2 and flags[-1] == flag:
            ends[-1] = stop
        else:
            ends.append(stop)
            flags.append(flag)
    return numel, ends, flags


def _many_units():
    """more units than the grid has blocks: 900 segments of one unit + 4 floats (two units each), 100 of two units + 4 (three)"""
    lengths = [2 * UNIT + 4 if i % 10 == 9 else UNIT + 4 for i in range(1000)]
    ends = np.cumsum(lengths).tolist()
    return ends[-1], ends, [i & 3 for i in range(1000)]


def _kinds_table():
    """every kind of values under every flag byte, sizes on both sides of a unit; the last segment ragged"""
    lengths = [68, UNIT + 8, 12, 260, 2 * UNIT, 36, 1028, 4, UNIT - 4, 132, 8, 516, 72, UNIT, 24, 2052, 40, 300, 16, 1031]
    ends = np.cumsum(lengths).tolist()
    return ends[-1], ends, [i // 5 for i in range(20)]


def kinds_of(nseg, name):
    """the kind of values of every segment"""
    if name == 'kinds':
        return [KINDS[i % 5] for i in range(nseg)]
    if name.startswith('n'):
        return ['unit'] * nseg
    return [('unit', 'unit', 'zero_w', 'unit', 'tiny', 'unit', 'zero_g', 'unit', 'unit', 'huge', 'unit')[i % 11] for i in range(nseg)]


RESNET_SHAPES = _resnet50_like()
PREFIX_FULL = (48, [16, 32, 48], [0, 3, 0])         # cut by prefix(24): inside the merged 1-d segment, at a multiple of 8
PREFIX_N = 24
# name -> (n, ends, flags)
TABLES = dict([('n%d' % n, (n, [n], [0])) for n in REGIMES],
              resnet=table_of(RESNET_SHAPES), many=_many_units(), kinds=_kinds_table(), prefix=(PREFIX_N, [16, 24], [0, 3]))
# (table, grad_scale, weight decay): every table at (1, 5e-5); every grad_scale and both decays on the tables that hold all flags
GRID = [(name, 1.0, 5e-5) for name in TABLES] + [('kinds', gs, wd) for gs in GRAD_SCALES for wd in DECAYS if (gs, wd) != (1.0, 5e-5)] + \
       [('resnet', 0.125, 0.0)]


def make(name, seed=0):
    """(p, g, v) fp32 of n + GUARD floats for table ``name``: unit-scale weights with gradients 1e-3 of them, and per kinds_of()
    a segment of zero weights, of zero gradients, of magnitudes 1e-25 (squares vanish in fp32, not in fp64), of 1e25 (squares
    overflow fp32, not fp64); the padding a parameter would have is not modelled (a segment is filled to its end)"""
    n, ends, flags = TABLES[name]
    rng = np.random.RandomState([seed, n % 65521, len(ends)])
    p = rng.standard_normal(n + GUARD).astype(F32)
    g = (1e-3 * rng.standard_normal(n + GUARD)).astype(F32)
    v = (1e-3 * rng.standard_normal(n + GUARD)).astype(F32)
    lo = 0
    for hi, kind in zip(ends, kinds_of(len(ends), name)):
        if kind == 'zero_w':
            p[lo:hi] = 0
        elif kind == 'zero_g':
            g[lo:hi] = 0
        elif kind == 'tiny':
            p[lo:hi] *= F32(1e-25)
            g[lo:hi] *= F32(1e-25)
            v[lo:hi] *= F32(1e-25)
        elif kind == 'huge':
            p[lo:hi] *= F32(1e25)
            g[lo:hi] *= F32(1e25)
            v[lo:hi] *= F32(1e25)
        lo = hi
    p[n:], g[n:], v[n:] = np.nan, np.nan, V_GUARD
    return p, g, v


# ---- float64 reference ------------------------------------------------------------------------------------------------------------
def ratio_of(W, G, flag, wd, eta=ETA, eps=EPS):
    wd_s = 0.0 if flag & 1 else wd
    if flag & 2 or not (W > 0 and G > 0):
        return 1.0
    return float(eta * W / (G + wd_s * W + eps))


def ratios_ref(p, g, ends, flags, wd, gs, eta=ETA, eps=EPS):
    """(r, W, G) per segment, float64; the sums of squares in np.longdouble"""
    r, Ws, Gs = [], [], []
    lo = 0
    for hi, flag in zip(ends, flags):
        W = float(np.sqrt(np.sum(np.square(p[lo:hi].astype(np.longdouble)))))
        G = float(abs(gs) * np.sqrt(np.sum(np.square(g[lo:hi].astype(np.longdouble)))))
        r.append(ratio_of(W, G, flag, wd, eta, eps)); Ws.append(W); Gs.append(G)
        lo = hi
    return np.asarray(r), np.asarray(Ws), np.asarray(Gs)


def additions(ends):
    """T per segment"""
    return np.asarray([16 + 6 + 3 + -(-(e - s) // UNIT) for s, e in zip([0] + list(ends[:-1]), ends)], np.float64)


def ratio_rel_bound(ends):
    return (U32 + C * additions(ends) * U64) * SLACK


def check_ratios(got, p, g, ends, flags, wd, gs, eta=ETA, eps=EPS):
    """the largest error / bound over ALL segments (<= 1 passes); ratios that the rule makes exactly 1 must be exactly 1"""
    want, W, G = ratios_ref(p, g, ends, flags, wd, gs, eta, eps)
    got = np.asarray(got, np.float64)
    assert got.shape == want.shape and np.isfinite(got).all(), 'a ratio is not finite'
    one = np.asarray([bool(f & 2) or not (w > 0 and gg > 0) for f, w, gg in zip(flags, W, G)])
    assert np.array_equal(got[one], np.ones(int(one.sum()))), 'a ratio that the rule makes 1 is not exactly 1'
    return float((np.abs(got - want) / (ratio_rel_bound(ends) * np.abs(want))).max())


def lars_ref(p, g, v, ends, flags, lr, momentum, wd, gs, eta=ETA, eps=EPS):
    """one step of the rule in float64: (p', v', r)"""
    r = ratios_ref(p, g, ends, flags, wd, gs, eta, eps)[0]
    p1, v1 = np.empty(ends[-1]), np.empty(ends[-1])
    lo = 0
    for hi, flag, rs in zip(ends, flags, r):
        p1[lo:hi], v1[lo:hi] = S.momentum_sgd_ref(p[lo:hi], g[lo:hi], v[lo:hi], lr * rs, momentum, 0.0 if flag & 1 else wd, gs)
        lo = hi
    return p1, v1, r


def lars_step_bound(p, g, v, lr, r, rel_r, momentum, wd_s, gs, ep=0.0, ev=0.0):
    """(bound on p', bound on v') of one segment for one step with the float64 ratio ``r`` whose computed value is off by at most
    ``rel_r`` (relative); see THE STEP BOUND"""
    bp, bv = S.momentum_sgd_bound(p, g, v, lr * r, momentum, wd_s, gs, ep, ev)
    p64, g64 = np.asarray(p, np.float64), np.asarray(g, np.float64)
    d = np.abs(lr * r * (g64 * gs + wd_s * p64))
    more = (U32 + rel_r) * d * SLACK
    return bp + more, bv + more


# ---- the kernels' arithmetic in NumPy ---------------------------------------------------------------------------------------------
_LANE = np.arange(64)


def _unit_sums(sq):
    """the partial sums of units of squares ``sq`` (float64, shape (units, m), m <= UNIT), in the order of lars_partials_kernel"""
    units, m = sq.shape
    m4 = m & ~3
    trips = -(-m4 // 1024) if m4 else 0
    body = np.zeros((units, trips * 1024))           # (adding +0.0 to a non-negative sum changes no bit)
    body[:, :m4] = sq[:, :m4]
    body = body.reshape(units, trips, 256, 4)
    acc = np.zeros((units, 256))
    for k in range(trips):
        for e in range(4):
            acc = acc + body[:, k, :, e]
    for t in range(m & 3):
        acc[:, t] = acc[:, t] + sq[:, m4 + t]
    w = acc.reshape(units, 4, 64)
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[:, :, _LANE ^ o]
    w = w[:, :, 0]
    return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def _segment_sum(x):
    sq = np.square(x.astype(np.float64))
    full = len(sq) // UNIT
    parts = []
    if full:
        parts.append(_unit_sums(sq[:full * UNIT].reshape(full, UNIT)))
    if len(sq) % UNIT:
        parts.append(_unit_sums(sq[None, full * UNIT:]))
    total = 0.0
    for part in np.concatenate(parts):      # the fold: ascending unit order
        total = total + part
    return total


def ratios_numpy(p, g, ends, flags, wd, gs, eta=ETA, eps=EPS):
    """lars_partials_kernel + lars_fold_kernel operation for operation: float64 throughout, one rounding to fp32"""
    out = np.empty(len(ends), F32)
    lo = 0
    with np.errstate(all='ignore'):
        for s, (hi, flag) in enumerate(zip(ends, flags)):
            W = np.sqrt(_segment_sum(p[lo:hi]))
            G = abs(gs) * np.sqrt(_segment_sum(g[lo:hi]))
            wd_s = 0.0 if flag & 1 else wd
            r = 1.0
            if not flag & 2 and W > 0.0 and G > 0.0:
                r = eta * W / (G + wd_s * W + eps)
            out[s] = F32(r)
            lo = hi
    return out


def segment_rate(lr, r32):
    """the rate momentum_sgd_seg_kernel<true> applies in a segment: ONE fp32 product of the rate as the kernel holds it"""
    return float(F32(lr) * F32(r32))


def update_numpy(p, g, v, ratios32, ends, flags, lr, momentum, wd, gs):
    """momentum_sgd_seg_kernel<true> (LARS's update) in NumPy float32, every product rounded (no contraction): (p', v')"""
    p1, v1 = p[:ends[-1]].copy(), v[:ends[-1]].copy()
    lo = 0
    with np.errstate(all='ignore'):
        for hi, flag, r in zip(ends, flags, ratios32):
            p1[lo:hi], v1[lo:hi] = S.momentum_sgd_fp32(p[lo:hi], g[lo:hi], v[lo:hi], segment_rate(lr, r), momentum, 0.0 if flag & 1 else wd, gs)
            lo = hi
    return p1, v1


def check_step(got_p, got_v, p, g, v, ends, flags, lr, momentum, wd, gs):
    """the largest error / bound of a whole step (ratios + update) against lars_ref over all floats (<= 1 passes)"""
    want_p, want_v, r = lars_ref(p, g, v, ends, flags, lr, momentum, wd, gs)
    rel = ratio_rel_bound(ends)
    worst, lo = 0.0, 0
    with np.errstate(all='ignore'):
        for hi, flag, rs, rel_s in zip(ends, flags, r, rel):
            bp, bv = lars_step_bound(p[lo:hi], g[lo:hi], v[lo:hi], lr, rs, 0.0 if rs == 1.0 else rel_s, momentum, 0.0 if flag & 1 else wd, gs)
            worst = max(worst, float((np.abs(got_p[lo:hi].astype(np.float64) - want_p[lo:hi]) / bp).max()),
                        float((np.abs(got_v[lo:hi].astype(np.float64) - want_v[lo:hi]) / bv).max()))
            lo = hi
    return worst
