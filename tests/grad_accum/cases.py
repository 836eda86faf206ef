"""Operand table, size grid and a NumPy fp32 restatement for the gradient accumulation kernel (csrc/accum.hip: grad_accum_kernel)
and the K-step chain ``GradientMethod.accumulate`` / ``update`` build from it; not collected by pytest.  The same functions run on
the restatement (test_cases_cpu.py, before any GPU run) and on the kernel (test_gpu_kernels.py).

THE RULE, for the first n floats of an accumulator acc and of the gradient buffer g, one call per micro-batch:
    STORE   acc_i = g_i                    g unchanged
    ADD     acc_i = fl32(acc_i + g_i)      g unchanged
    CLOSE   g_i   = fl32(acc_i + g_i)      acc unchanged
A step of K micro-batches is STORE, K - 2 times ADD, CLOSE: the closed gradient is ((g1 + g2) + g3) + .. + gK, one IEEE fp32 addition
per element and micro-batch.  K = 2 is STORE, CLOSE.

THE COMPARISON is of bits.  An fp32 addition is correctly rounded on every IEEE machine, so NumPy's float32 ``+`` and the kernel's
agree in every bit of every result that is a number, signed zeros, subnormals and infinities included.  A NaN result is a NaN on
both, but WHICH NaN is the machine's choice (x86 produces the negative default NaN for inf - inf, the GPU the positive one), so
``same_bits`` asks for NaN at the same places and equal bits everywhere else.  Against ``torch.add`` on the same device the kernel
tests ask for equal bits at every place, NaN included.  Nothing here was read off a kernel's output."""
import numpy as np

F32 = np.float32
STORE, ADD, CLOSE = 0, 1, 2
MODES = {'store': STORE, 'add': ADD, 'close': CLOSE}

# ---- constants of the kernel that the size grid mirrors ---------------------------------------------------------------------------
UNIT = 4096             # LOANS_LARS_UNIT: floats per block and trip (256 threads x 4 float4)
THREAD_TRIP = 16        # floats of one thread in a full unit: four float4
GRID_CAP = 2048         # grid_for's max_blocks: beyond GRID_CAP units a block takes a second trip
GUARD = 8               # floats behind n: neither read nor written
ARENA_ALIGN = 8         # arena offsets are multiples of 8 floats

SIZES = (1, 3, 4, 5,
         THREAD_TRIP - 1, THREAD_TRIP, THREAD_TRIP + 1,
         UNIT - 1, UNIT, UNIT + 1,
         GRID_CAP * UNIT + 1,           # one float past a whole grid round: block 0 takes a second trip, of one scalar
         3 * 1000 * 1000 + 7)           # an odd size of a few million: 732 full units, a short one of float4s and three scalars


def regime(n):
    """(full units, float4 of the short last unit, single floats behind them, trips of block 0)"""
    full, rest = divmod(n, UNIT)
    units = full + (rest > 0)
    return full, rest // 4, rest % 4, -(-units // GRID_CAP)


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def apply(mode, acc, g):
    """(acc', g') of one call; float32 arrays of equal length, neither changed in place"""
    acc, g = np.asarray(acc, F32), np.asarray(g, F32)
    with np.errstate(all='ignore'):
        if mode == STORE:
            return g.copy(), g.copy()
        if mode == ADD:
            return (acc + g).astype(F32), g.copy()
        if mode == CLOSE:
            return acc.copy(), (acc + g).astype(F32)
    raise ValueError('unknown mode %r' % (mode,))


def modes_of(K):
    """the calls of a step of K >= 2 micro-batches"""
    assert K >= 2
    return [STORE] + [ADD] * (K - 2) + [CLOSE]


def chain(gs, acc0=None):
    """(closed gradient, the accumulator it leaves) of a step over the micro-gradients ``gs`` (K >= 2 rows), from an accumulator that
    holds ``acc0`` -- anything: STORE does not read it"""
    gs = [np.asarray(g, F32) for g in gs]
    acc = np.full_like(gs[0], np.nan) if acc0 is None else np.asarray(acc0, F32)
    g = None
    for mode, gi in zip(modes_of(len(gs)), gs):
        acc, g = apply(mode, acc, gi)
    return g, acc


def sequential_sum(gs):
    """((g1 + g2) + g3) + .. in fp32, written without the modes"""
    gs = [np.asarray(g, F32) for g in gs]
    total = gs[0].copy()
    with np.errstate(all='ignore'):
        for g in gs[1:]:
            total = (total + g).astype(F32)
    return total


def bits(a):
    return np.ascontiguousarray(np.asarray(a, F32)).view(np.uint32)


def same_bits(a, b):
    """NaN at the same places, equal bits everywhere else (see the module docstring)"""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb])


# ---- implementations that are NOT the rule: each must differ from it on the table below -------------------------------------------
def wrong_fp64_once(gs):
    """accumulate in fp64, round once"""
    with np.errstate(all='ignore'):
        return np.sum(np.stack([np.asarray(g, np.float64) for g in gs]), axis=0).astype(F32)


def wrong_reversed(gs):
    """((gK + gK-1) + ..) + g1"""
    return sequential_sum(list(gs)[::-1])


def wrong_scaled_per_micro_batch(gs):
    """every micro-gradient times fl32(1 / K) before it is added, instead of ONE scale on the closed sum"""
    k = F32(1.0 / len(gs))
    with np.errstate(all='ignore'):
        return sequential_sum([(np.asarray(g, F32) * k).astype(F32) for g in gs])


def scaled_once(gs):
    """what the rule gives where the optimiser's kernel then applies fl32(1 / K): the like-for-like partner of the function above"""
    with np.errstate(all='ignore'):
        return (sequential_sum(gs) * F32(1.0 / len(gs))).astype(F32)


def wrong_close_writes_acc(acc, g):
    """CLOSE that also leaves the sum in acc"""
    _, total = apply(CLOSE, acc, g)
    return total.copy(), total


def wrong_add_for_store(gs, acc0):
    """the first call adds into whatever the accumulator held"""
    acc = np.asarray(acc0, F32)
    g = None
    for mode, gi in zip([ADD] + modes_of(len(gs))[1:], gs):
        acc, g = apply(mode, acc, gi)
    return g


# ---- the operand table: one column per case, one row per micro-batch (K = 3) -------------------------------------------------------
TINY = float(np.finfo(F32).tiny)            # 2^-126, the smallest normal
SUB = 2.0 ** -149                           # the smallest subnormal
COLUMNS = [
    # (g1, g2, g3)                          what the column is there for
    (1e8, -1e8, 1.0),                       # (a + b) + c = 1, a + (b + c) = 0: the order shows, reversed gives 0
    (1.0, 2.0 ** -24, 2.0 ** -24),          # each half-ulp ties back to 1; fp64 rounded once gives 1 + 2^-23
    (1.0, 2.0 ** -24, -(2.0 ** -25)),       # ties to even, then falls inside the ulp
    (0.1, 0.2, 0.3),                        # three roundings; a per-micro-batch 1/3 rounds elsewhere
    (1.0, 3.0, 5.0),                        # 9 / 3 exact, 1/3 + 1 + 5/3 in fp32 not
    (1.0, -1.0, 0.0),                       # cancellation to +0
    (-1.0, 1.0, -0.0),                      # +0 + -0 = +0
    (-0.0, -0.0, -0.0),                     # -0 survives
    (0.0, -0.0, -0.0),                      # +0 wins
    (1.5, -1.5, -0.0),                      # +0, not -0
    (SUB, SUB, SUB),                        # subnormals add exactly
    (TINY, -SUB, -SUB),                     # a normal falls into the subnormal range
    (TINY / 2, TINY / 2, -TINY),            # two subnormals make a normal, and cancel
    (-SUB, SUB, -SUB),                      # cancellation among subnormals: +0, then -SUB
    (np.inf, 1.0, -1.0),                    # inf stays
    (-np.inf, 1e30, 1e30),
    (np.inf, -np.inf, 1.0),                 # NaN is born and stays
    (1.0, np.inf, -np.inf),
    (np.nan, 1.0, 2.0),                     # NaN goes through
    (1.0, 2.0, np.nan),
    (1e30, 1e-30, -1e30),                   # 1e-30 vanishes beside 1e30: 0, where the reverse order agrees and fp64 gives 1e-30
    (1e-30, 1e-30, 1e30),
    (1e30, 1e30, 1e30),
    (-1e-30, 1e-30, 1e-30),
    (3e38, 3e38, -3e38),                    # overflow on the way: inf, where fp64 rounded once gives 3e38
    (3e38, -3e38, 3e38),
    (16777216.0, 1.0, 1.0),                 # 2^24 + 1 ties to 2^24 twice; the reverse order gives 2^24 + 2
    (0.75, 0.5, -1.25),
]
TABLE = np.array(COLUMNS, dtype=np.float64).T.astype(F32)         # (3, cases): row k is micro-batch k + 1
DIRTY = F32(7.0)            # what a dirty accumulator holds for wrong_add_for_store


def tiled(n, rows=3):
    """``rows`` micro-gradients of n floats: the table's columns repeated, so that every thread position and every tail of the
    kernel meets every case.  Row k of a K = 2 step is taken from the same table."""
    reps = -(-n // TABLE.shape[1])
    return [np.tile(TABLE[k], reps)[:n].copy() for k in range(rows)]


# ---- host side: the bookkeeping of StandardUpdater(accum_steps=K) ---------------------------------------------------------------------
def updater_schedule(n_examples, batch_size, K, steps):
    """per optimiser step: (epoch after it, is_new_epoch) of an in-order SerialIterator over ``n_examples`` with ``repeat``: a batch
    crosses the boundary when it consumes the epoch's last example, and a step is a new epoch where ANY of its K batches did"""
    pos = epoch = 0
    out = []
    for _ in range(steps):
        crossed = False
        for _ in range(K):
            pos += batch_size
            if pos >= n_examples:
                pos -= n_examples
                epoch += 1
                crossed = True
        out.append((epoch, crossed))
    return out
