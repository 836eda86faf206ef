"""Case grid, fp64 reference, derived bound and an fp32 NumPy restatement for the job-table kernel of the weight average
(csrc/misc.hip: average_jobs_kernel) and the case grid of the segmented momentum SGD (csrc/sgd.hip: momentum_sgd_seg_kernel); not collected by
pytest.  The same functions run on the restatement (test_cases_cpu.py, before any GPU run) and on the kernels
(test_gpu_kernels.py).

UPDATE, ``dst += omd * (src - dst)``, against float64 on float64 copies of the fp32 inputs, elementwise.  The bound is
    3 u omd |src - dst|  +  u |result|  +  UF,        u = 2^-24
one rounding each for ``omd`` as a float, the difference and the product (relative to the product), one for the sum (relative to
the result), and one smallest normal where fp32 may underflow -- gradually or flushed -- and float64 does not.  A fused
multiply-add rounds less and stays inside.  No element is excluded.  Nothing here was read off a kernel's output."""
import numpy as np

U = 2.0 ** -24
UF = 2.0 ** -126
F32 = np.float32

# ---- constants of the kernels that the grid mirrors -------------------------------------------------------------------------------
UNIT = 4096             # LOANS_AVG_UNIT: floats per unit of work, one block per unit and trip (256 threads x 4 float4)
GRID_CAP = 2048         # grid_for's max_blocks: beyond GRID_CAP units a block takes a second trip
SGD_TRIP = 2048 * 256 * 4   # floats the segmented SGD's grid covers in one trip of its float4 grid-stride loop
SGD_BLOCK = 256 * 4         # floats of one block and trip
SGD_MAX_SEGMENTS = 1024

OMDS = (9.0 / 11.0, 0.5, 1.0 - 0.9999)          # update 1 of any decay; a plain half; the long-run decay of a ResNet recipe
OMDS_EQUAL = (2.0 ** -14, 0.5, 9.0 / 11.0)      # where dst == src the output is the input, bit for bit


def average_regime(n):
    """(full units, float4 of the short last unit, single floats behind them, trips of block 0) of a single job of n floats"""
    full, rest = divmod(n, UNIT)
    units = full + (1 if rest else 0)
    return full, rest // 4, rest % 4, -(-units // min(units, GRID_CAP))


# n of a single job -> the regime it reaches; test_cases_cpu.py recomputes every entry
REGIMES = {
    1: (0, 0, 1, 1),                # one thread, one scalar
    3: (0, 0, 3, 1),                # scalars only
    4: (0, 1, 0, 1),                # one float4, no tail
    5: (0, 1, 1, 1),                # a float4 and a scalar
    64: (0, 16, 0, 1),              # the smallest BN statistics tensor
    2048: (0, 512, 0, 1),           # the largest: a thread takes two float4 of the short unit (k, k + 1024)
    UNIT - 1: (0, 1023, 3, 1),      # one unit - 1: the short path at its longest
    UNIT: (1, 0, 0, 1),             # one unit: the unrolled path, nothing else
    UNIT + 1: (1, 0, 1, 1),         # one unit + 1: a second block with a single scalar
    2 * UNIT + 3: (2, 0, 3, 1),     # two units + 3
    GRID_CAP * UNIT + UNIT + 5: (GRID_CAP + 1, 1, 1, 2),     # more units than blocks: block 0 and block 1 take a second trip
}
SINGLE_N = tuple(sorted(REGIMES))[:-1]
LONG_N = GRID_CAP * UNIT + UNIT + 5
# 1 big + 120 small jobs, as ResNet-50 gives: the arena, then avg_mean / avg_var of every BN; sizes that are no multiple of 4 among them
TABLE_N = (3 * UNIT + 7,) + tuple((64, 64, 128, 256, 255, 512, 1024, 1021, 2048, 2050, 66, 1)[i % 12] for i in range(120))

GUARD = 4               # floats between jobs, beside what alignment adds
GUARD_DST, GUARD_SRC = F32(12345.0), F32(-54321.0)


def layout(ns):
    """(offsets, total): every job 16-byte aligned inside one buffer, at least GUARD guard floats in front of, between and behind"""
    offsets, at = [], GUARD
    for n in ns:
        offsets.append(at)
        at = (at + n + GUARD + 3) // 4 * 4
    return offsets, at


def make_update(ns, seed, equal=False):
    """(dst, src) fp32 buffers of `layout(ns)`: weights of unit scale; half of every job's live values a small step away from the
    average (training), half independent of it (a fresh BN statistic); ``equal``: src == dst everywhere, zeros and denormals
    among the values"""
    rng = np.random.RandomState(seed)
    offsets, total = layout(ns)
    dst, src = np.full(total, GUARD_DST, F32), np.full(total, GUARD_SRC, F32)
    for n, o in zip(ns, offsets):
        d = rng.standard_normal(n).astype(F32)
        if equal:
            d[::7] = 0.0
            d[3::11] = F32(1e-41)           # a denormal
            s = d.copy()
        else:
            near = rng.rand(n) < 0.5
            s = np.where(near, d + F32(1e-3) * rng.standard_normal(n).astype(F32), rng.standard_normal(n).astype(F32)).astype(F32)
        dst[o:o + n], src[o:o + n] = d, s
    return dst, src


def make_swap(ns, seed):
    """(dst, src) of random BITS -- NaNs of every payload, infinities, denormals among them -- with the named specials in front"""
    rng = np.random.RandomState(seed)
    offsets, total = layout(ns)
    dst, src = np.full(total, GUARD_DST, F32), np.full(total, GUARD_SRC, F32)
    special = np.array([0x7fc00001, 0xffc12345, 0x7f800001, 0x80000000, 0x00000001, 0x807fffff, 0x7f800000, 0x00000000], np.uint32)
    for n, o in zip(ns, offsets):
        for buf in (dst, src):
            bits = rng.randint(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
            k = min(n, len(special))
            bits[:k] = special[:k] if buf is dst else special[::-1][:k]
            buf[o:o + n] = bits.view(F32)
    return dst, src


def update_reference(dst, src, omd):
    """float64, on float64 copies of the fp32 inputs; ``omd`` the host's double"""
    d, s = dst.astype(np.float64), src.astype(np.float64)
    return d + float(omd) * (s - d)


def update_bound(dst, src, omd, result):
    d, s = dst.astype(np.float64), src.astype(np.float64)
    return 3 * U * float(omd) * np.abs(s - d) + U * np.abs(result) + UF


def update_numpy(dst, src, omd):
    """the kernel's arithmetic in fp32 NumPy, unfused: every operator rounds"""
    return (dst + F32(omd) * (src - dst)).astype(F32)


def check_update(got, dst, src, omd, ns):
    """the largest error / bound over the jobs' floats (<= 1 passes); guard floats of ``got`` must be the inputs'"""
    offsets, total = layout(ns)
    inside = np.zeros(total, bool)
    for n, o in zip(ns, offsets):
        inside[o:o + n] = True
    want = update_reference(dst, src, omd)
    bound = update_bound(dst, src, omd, want)
    assert np.array_equal(got[~inside].view(np.int32), dst[~inside].view(np.int32)), 'a float outside every job was written'
    assert np.isfinite(got[inside]).all()
    return float((np.abs(got.astype(np.float64) - want)[inside] / bound[inside]).max())


# ---- segmented momentum SGD: (n, ends, flags), what each case reaches ----------------------------------------------------------------
def _alternate(ends, first=0):
    return [(first + i) & 1 for i in range(len(ends))]


SGD_CASES = {
    # one segment, not exempt: one plain call over the whole buffer; n & 3 = 3, the ragged end outside an exempt segment
    'one': (4099, [4099], [0]),
    # 300 segments of 8 floats, alternating: every float4 pair has its own flag, a thread's cursor crosses segments on every trip
    'eights': (2400, list(range(8, 2401, 8)), _alternate(range(300), 1)),
    # boundaries at 8, either side of a block's edge (256 * 4) and of the first trip's end; the last segment 1019 floats, n & 3 = 3,
    # exempt -- the ragged end inside an exempt segment
    'edges': (SGD_TRIP + SGD_BLOCK + 3,
              [8, SGD_BLOCK - 8, SGD_BLOCK, SGD_BLOCK + 8, SGD_TRIP - 8, SGD_TRIP, SGD_TRIP + 8, SGD_TRIP + SGD_BLOCK + 3],
              _alternate(range(8), 0)),
}
SGD_HYPER = dict(lr=0.05, momentum=0.9, weight_decay_rate=0.1, grad_scale=0.5)


def make_sgd(n, seed):
    rng = np.random.RandomState(seed)
    return tuple(rng.standard_normal(n).astype(F32) for _ in range(3))         # p, g, v
