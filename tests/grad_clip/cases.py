"""Case grid, float64 reference, derived bounds and a NumPy restatement for the gradient-clipping kernels (csrc/clip.hip:
grad_sumsq_kernel, grad_clip_fold_kernel, grad_scale_dev_kernel); not collected by pytest.  The same functions run on the
restatement (test_cases_cpu.py, before any GPU run) and on the kernels (test_gpu_kernels.py, test_gpu_model.py).

THE RULE, for the first n floats g of a buffer, the optimiser's grad_scale gs and the threshold c > 0:
    S    = sum g_i^2                      every g_i converted to double and squared (exact), summed in fp64 in a FIXED order
    N    = |gs| sqrt(S)                   in double
    k    = (N is finite and N > c) ? c / N : 1          in double, rounded to fp32 ONCE
    g_i' = fl32(g_i k)                    one fp32 product per element -- skipped entirely when k == 1

THE BOUNDS.  u64 = 2^-53, u32 = 2^-24.  The square of an fp32 value is exact in fp64 (24 + 24 bits in 53): only additions round.
A term passes at most T of them:
    16                  a thread's own elements (four float4 of a full unit)
     6                  the xor butterfly of the wave
     3                  waves 0..3 through LDS
    ceil(units / 64)    a lane of the fold: partials l, l + 64, .. in ascending order (units = ceil(n / UNIT))
     6                  the fold's xor butterfly
All terms are non-negative, so |S^ - S| <= T u64 S at first order.  From there, relative errors in units of u64:
    sqrt(S^)            T/2 + 1     (the root halves the error and rounds once)
    N^ = |gs| sqrt(S^)  T/2 + 2
    c / N^              T/2 + 3
and each of N^ and k^ is rounded to fp32 ONCE: + u32.  The product g_i k^ rounds once more: |g'^ - g'| <= (u32 + rel_k) |g_i k|, plus
half the spacing of fp32's subnormals, 2^-150 <= 2^-149, where the product falls below the normal range.  SLACK = 1.01 covers the
second-order terms, as in tests/imagenet_lars/cases.py.  The reference sums in np.longdouble (64-bit mantissa): its own error is
below 2^-60 and is not in the bound.  No element and no case is left out of a comparison; what the rule makes exact -- k = 1, N = 0,
an untouched gradient -- is compared exactly.  Nothing here was read off a kernel's output."""
import numpy as np

U32 = 2.0 ** -24
U64 = 2.0 ** -53
SLACK = 1.01
F32 = np.float32
SUBNORMAL = 2.0 ** -149

# ---- constants of the kernels that the grid mirrors -------------------------------------------------------------------------------
UNIT = 4096             # LOANS_LARS_UNIT: floats per unit of work, one block per unit and trip (256 threads x 4 float4)
GRID_CAP = 2048         # grid_for's max_blocks: beyond GRID_CAP units a block takes a second trip
LANES = 64              # the fold's lanes: beyond LANES units a lane takes a second partial
GUARD = 8               # floats behind n, NaN: neither read into the sum nor written

GRAD_SCALES = (1.0, 0.5, 0.125)
ABOVE = 1e30            # a threshold above every norm of the grid
THRESHOLDS = (1.0, ABOVE, float('inf'))


def regime(n):
    """(full units, float4 of the short last unit, single floats behind them)"""
    full, rest = divmod(n, UNIT)
    return full, rest // 4, rest % 4


def units_of(n):
    return -(-n // UNIT)


# n -> the regime it reaches; test_cases_cpu.py recomputes every entry
REGIMES = {
    1: (0, 0, 1),               # one thread, one scalar
    3: (0, 0, 3),               # scalars only
    4: (0, 1, 0),               # one float4, no tail
    5: (0, 1, 1),               # a float4 and a scalar
    64: (0, 16, 0),
    UNIT - 1: (0, 1023, 3),     # the short path at its longest
    UNIT: (1, 0, 0),            # the unrolled path, nothing else
    UNIT + 1: (1, 0, 1),        # a second unit of a single scalar
    2 * UNIT + 3: (2, 0, 3),    # two units + 3
}
N_LANE2 = 65 * UNIT + 1                 # 66 units: fold lanes 0 and 1 take a second partial
N_TRIP2 = GRID_CAP * UNIT + 5           # GRID_CAP + 1 units: block 0 takes a second trip, the last unit is a float4 and a scalar
SIZES = tuple(REGIMES) + (N_LANE2, N_TRIP2)
N_KINDS = 2 * UNIT + 3

KINDS = ('unit', 'tiny', 'huge', 'zero')
EDGES = ('below', 'exact', 'above', 'above20')          # N against c around N = 5, see make()
BROKEN = ('nan', 'inf')


def _grid():
    """(name, n, kind, grad_scale, threshold)"""
    grid = [('n%d' % n, n, 'unit', 1.0, 1.0) for n in SIZES]
    grid += [('n%d-gs0.5-above' % n, n, 'unit', 0.5, ABOVE) for n in (5, UNIT + 1, N_LANE2)]
    for kind in KINDS:
        for gs in GRAD_SCALES:
            for c in THRESHOLDS:
                grid.append(('%s-gs%g-c%g' % (kind, gs, c), N_KINDS, kind, gs, c))
    grid += [('huge-lane2', N_LANE2, 'huge', 0.125, 1.0), ('tiny-lane2', N_LANE2, 'tiny', 1.0, 1e-26)]
    for kind in EDGES:
        for gs in (1.0, 0.5):
            grid.append(('%s-gs%g' % (kind, gs), N_KINDS, kind, gs, edge_threshold(kind)))
    for kind in BROKEN:
        grid += [('%s-c1' % kind, N_KINDS, kind, 1.0, 1.0), ('%s-short' % kind, UNIT - 1, kind, 0.5, 1.0)]
    return grid


def edge_threshold(kind):
    """the threshold of an edge case, whose N is exactly 5"""
    return {'below': float(np.nextafter(5.0, 6.0)),          # N just below c: no clip
            'exact': 5.0,                                    # N == c: no clip
            'above': float(np.nextafter(5.0, 4.0)),          # N just above c: k < 1 in double, 1 once rounded to fp32 -- nothing moves
            'above20': 5.0 * (1.0 - 2.0 ** -20)}[kind]       # k = 1 - 2^-20, exact in fp32: every product is exact


GRID = _grid()
IDS = [c[0] for c in GRID]


def make(n, kind, gs=1.0, seed=0):
    """g, fp32, of n + GUARD floats.  unit: standard normal; tiny / huge: 1e-25 / 1e25 of that (squares vanish / overflow in fp32,
    not in fp64); zero; the edges: all zero but a 3 and a 4 (over |gs|, exact for the grid's powers of two), so that N is exactly 5;
    nan / inf: unit with one such element (in the last, short unit when there is one).  NaN behind n."""
    rng = np.random.RandomState([seed, n % 65521, KINDS.index(kind) if kind in KINDS else 7])
    g = rng.standard_normal(n + GUARD).astype(F32)
    if kind == 'tiny':
        g *= F32(1e-25)
    elif kind == 'huge':
        g *= F32(1e25)
    elif kind == 'zero':
        g[:] = 0
    elif kind in EDGES:
        g[:] = 0
        g[n // 3] = F32(-3.0 / abs(gs))
        g[n - 1] = F32(4.0 / abs(gs))
    elif kind in BROKEN:
        g[n - 2 if n > 2 else 0] = np.nan if kind == 'nan' else -np.inf
    g[n:] = np.nan
    return g


# ---- float64 reference ------------------------------------------------------------------------------------------------------------
def coefficient(N, c):
    return c / N if np.isfinite(N) and N > c else 1.0


def clip_ref(g, n, gs, c):
    """(N, k, g') in float64; the sum of squares in np.longdouble"""
    with np.errstate(all='ignore'):
        S = np.sum(np.square(g[:n].astype(np.longdouble)))
        N = float(abs(gs) * np.sqrt(S))
    k = coefficient(N, c)
    g64 = g[:n].astype(np.float64)
    return N, k, g64 if k == 1.0 else g64 * k


def additions(n):
    """T"""
    return 16 + 6 + 3 + -(-units_of(n) // LANES) + 6


def norm_rel_bound(n):
    return ((additions(n) / 2 + 2) * U64 + U32) * SLACK


def coefficient_rel_bound(n):
    return ((additions(n) / 2 + 3) * U64 + U32) * SLACK


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.int32)


def check(got_N, got_k, got_g, g, n, gs, c):
    """The largest error / bound of the record and of ALL n elements of g' (<= 1 passes; inf where something the rule makes exact is
    not: N = 0, a non-finite N, k = 1, an untouched gradient), and the guards behind n."""
    want_N, want_k, want_g = clip_ref(g, n, gs, c)
    got_N, got_k = float(got_N), float(got_k)
    if not np.array_equal(_bits(got_g[n:]), _bits(g[n:])):
        return float('inf')
    if not np.isfinite(want_N):
        ok = not np.isfinite(got_N) and got_k == 1.0 and np.array_equal(_bits(got_g[:n]), _bits(g[:n]))
        return 0.0 if ok else float('inf')
    if want_N == 0.0:
        ok = got_N == 0.0 and got_k == 1.0 and np.array_equal(_bits(got_g[:n]), _bits(g[:n]))
        return 0.0 if ok else float('inf')
    if not (np.isfinite(got_N) and np.isfinite(got_k)):
        return float('inf')
    worst = abs(got_N - want_N) / (norm_rel_bound(n) * want_N)
    rel_k = 0.0
    if want_k == 1.0:
        if got_k != 1.0:
            return float('inf')
    else:
        rel_k = coefficient_rel_bound(n)
        worst = max(worst, abs(got_k - want_k) / (rel_k * want_k))
    if got_k == 1.0 and not np.array_equal(_bits(got_g[:n]), _bits(g[:n])):        # k == 1: not a bit of g moves
        return float('inf')
    bound = (U32 + rel_k) * np.abs(want_g) * SLACK + SUBNORMAL
    err = np.abs(got_g[:n].astype(np.float64) - want_g)
    if want_k == 1.0:
        return float('inf') if err.max() != 0.0 else float(worst)
    return float(max(worst, (err / bound).max()))


def clipped_norm_bound(n, c):
    """what the float64 norm of g' gs may reach after a clip: every element is off by at most (u32 + rel_k) |g k| relative, + the
    subnormal term over sqrt(n) elements"""
    return c * (1.0 + (U32 + coefficient_rel_bound(n)) * SLACK) + SUBNORMAL * np.sqrt(n)


# ---- the kernels' arithmetic in NumPy ---------------------------------------------------------------------------------------------
_LANE = np.arange(64)


def _unit_sums(sq):
    """the partial sums of units of squares ``sq`` (float64, shape (units, m), m <= UNIT), in the order of grad_sumsq_kernel"""
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


def partials_numpy(g, n):
    """one float64 partial per unit: unit u is floats [UNIT u, min(n, UNIT (u + 1)))"""
    with np.errstate(all='ignore'):
        sq = np.square(g[:n].astype(np.float64))
        full = n // UNIT
        parts = []
        if full:
            parts.append(_unit_sums(sq[:full * UNIT].reshape(full, UNIT)))
        if n % UNIT:
            parts.append(_unit_sums(sq[None, full * UNIT:]))
        return np.concatenate(parts)


def fold_numpy(partials):
    """grad_clip_fold_kernel: lane l sums partials l, l + 64, .. in ascending order, the lanes meet in the xor butterfly"""
    with np.errstate(all='ignore'):
        rows = -(-len(partials) // LANES)
        padded = np.zeros(rows * LANES)
        padded[:len(partials)] = partials
        acc = np.zeros(LANES)
        for row in padded.reshape(rows, LANES):
            acc = acc + row
        for o in (32, 16, 8, 4, 2, 1):
            acc = acc + acc[_LANE ^ o]
        return acc[0]


def record_numpy(g, n, gs, c):
    """(N, k) as the two launches of loans_grad_norm_f32 leave them: float64 throughout, each rounded to fp32 once"""
    with np.errstate(all='ignore'):
        N = abs(gs) * np.sqrt(fold_numpy(partials_numpy(g, n)))
        k = c / N if np.isfinite(N) and N > c else 1.0
        return F32(N), F32(k)


def apply_numpy(g, n, k32):
    """grad_scale_dev_kernel: one fp32 product per element of the first n, or nothing at all"""
    out = g.copy()
    if F32(k32) != F32(1.0):
        with np.errstate(all='ignore'):
            out[:n] = g[:n] * F32(k32)
    return out
