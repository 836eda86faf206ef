"""Case grid, fp64 reference, derived bounds and an fp32 NumPy restatement for the kernels of csrc/misc.hip and csrc/insight.hip
that are neither a convolution nor a BN: GAP, the small Linear heads, the spatial transformer's grid and sampler, MSE, the grid
regularisers, Adam / AMSGrad, the glue kernels and the VisualBackprop / grayscale kernels (not collected by pytest; DESIGN 3,
item 12).

The same `check_*` functions run twice: on `NumpyImpl` (tests/misc_kernels/test_cases_cpu.py: the restatement must sit inside the
bounds on every generated case, before any GPU run) and on `HipImpl` (tests/misc_kernels/test_gpu_kernels.py).  The reference is
oracle/chainer_ops.py in float64 on float64 copies of the fp32 inputs; bf16 inputs are rounded to bf16 FIRST and the oracle sees
the rounded values.  What Chainer decides in float32 -- the sampler's source coordinates, their clip, floor and masks, the sign of
the regularisers' distances -- is decided in float32 in the reference too, and only the arithmetic after it is float64: no case
has an ambiguous index or mask, and every check asserts that the share of excluded elements is 0.

Every bound is elementwise, first order in u = 2^-24, and counts the roundings of the kernel's own summation tree; the counts
stand next to the code.  None was read off a kernel's output.  A fused multiply-add rounds once where the count has two, so a
contracted kernel stays inside.  `tanhf`, `sqrtf` and the division are budgeted 2 ulp = 4 u each."""
import json
import types

import numpy as np

from oracle import chainer_ops as C

U = 2.0 ** -24          # unit round-off of fp32 (round to nearest)
U16 = 2.0 ** -8         # one round-to-nearest-even of a bf16 result
ULP2 = 4 * U            # 2 ulp of an fp32 result, relative (1 ulp <= 2 u |value|)
UF = 2.0 ** -126        # absolute term where fp32 can underflow and float64 cannot: one smallest normal, gradual or flushed
F32 = np.float32

# ---- constants of the kernels that the grid mirrors (asserted against the regime table by test_cases_cpu.py) ---------------------
BLOCK = 256             # threads per block, every kernel here
GRID_CAP = 2048         # grid_for's max_blocks (csrc/common.h): beyond BLOCK * GRID_CAP items a thread takes a second trip
TRIP = BLOCK * GRID_CAP  # 524 288
LIN_TRIP = 1024         # linear_fwd_kernel: elements of K per block and trip (256 threads x 4)
LIN_LU = 8              # ... unrolled eight deep: the body runs while k + 7 * 1024 < K
LIN_SLAB = 16           # linear_bwd_w_kernel: samples per slab (blockIdx.y)
LIN_NMAX = 8
GAP_PHASES = 4          # gap_fwd_kernel: pixel phases per block; the unrolled body takes 4 pixels per phase: p + 12 < HW
GAP_LANES = 64          # ... four-channel groups per block


def depth_block(L):
    """additions on the longest path of a 256-thread strided chain over L items followed by block_sum (6 shuffle levels, then
    sh[0] + sh[1] + sh[2] + sh[3]): ceil(L / 256) + 6 + 3"""
    return -(-L // BLOCK) + 6 + 3


# ---- regimes ---------------------------------------------------------------------------------------------------------------------
def linear_fwd_regime(K):
    """(unrolled trips of thread 0, tail trips of thread 0, unrolled trips of thread 255, tail trips of thread 255)"""
    out = []
    for tid in (0, BLOCK - 1):
        k, un, tail = tid * 4, 0, 0
        while k + (LIN_LU - 1) * LIN_TRIP < K:
            un, k = un + 1, k + LIN_LU * LIN_TRIP
        while k < K:
            tail, k = tail + 1, k + LIN_TRIP
        out += [un, tail]
    return tuple(out)


def gap_fwd_regime(HW, C_):
    """(unrolled trips of phase 0, tail trips of phase 0, unrolled trips of phase 3, tail trips of phase 3, chunks, lanes
    working in the last chunk)"""
    out = []
    for part in (0, GAP_PHASES - 1):
        p, un, tail = part, 0, 0
        while p + 12 < HW:
            un, p = un + 1, p + 16
        while p < HW:
            tail, p = tail + 1, p + 4
        out += [un, tail]
    c4 = C_ // 4
    chunks = -(-c4 // GAP_LANES)
    return tuple(out) + (chunks, c4 - (chunks - 1) * GAP_LANES)


def stride_trips(items):
    """trips of the busiest thread of a grid-stride loop launched with grid_for(items, 256)"""
    blocks = min(max(-(-items // BLOCK), 1), GRID_CAP)
    return -(-items // (blocks * BLOCK))


# shape -> what it reaches, with the arithmetic; test_cases_cpu.py recomputes every entry from the constants above
REGIMES = {
    # linear_fwd_kernel, K -> (unrolled, tail) trips of thread 0 and of thread 255
    'linear_K': {
        4: (0, 1, 0, 0),            # one thread works
        1024: (0, 1, 0, 1),         # one tail trip each
        1028: (0, 2, 0, 1),         # thread 0 takes a second tail trip
        7168: (0, 7, 0, 7),         # seven tail trips, the unrolled body never: 0 + 7 * 1024 < 7168 is false
        7172: (1, 0, 0, 7),         # thread 0 alone runs the unrolled body (0 + 7168 < 7172), the others seven tail trips
        8196: (1, 1, 1, 0),         # every thread runs the unrolled body once, thread 0 one tail trip on top (8192 < 8196)
        41472: (5, 1, 5, 0),        # the assessor head: 40.5 trips -> five bodies each, threads 0 .. 127 one tail trip on top
    },
    # linear_bwd: B -> (slabs of 16 samples, samples in the last slab, trips of linear_bwd_b_kernel's thread 0)
    'linear_B': {1: (1, 1, 1), 5: (1, 5, 1), 16: (1, 16, 1), 17: (2, 1, 1), 33: (3, 1, 1), 257: (17, 1, 2)},
    # gap_fwd_kernel, HW -> (unrolled, tail) trips of phase 0 and of phase 3
    'gap_HW': {1: (0, 1, 0, 0), 3: (0, 1, 0, 0), 4: (0, 1, 0, 1), 13: (1, 0, 0, 3), 16: (1, 0, 1, 0), 17: (1, 1, 1, 0),
               49: (3, 1, 3, 0), 256: (16, 0, 16, 0)},
    # ... C -> (chunks of 64 four-channel groups, lanes working in the last chunk)
    'gap_C': {4: (1, 1), 96: (1, 24), 260: (2, 1), 512: (2, 64), 2048: (8, 64)},
    # grid-stride kernels, items -> trips of the busiest thread (2048 blocks x 256 threads = 524 288 items per trip)
    'stride': {5 * 256 * 512: 2,                # gap_bwd: B = 5, HW = 256, C = 2048 -> 655 360 four-channel groups
               94 * 75 * 75: 2,                 # st_grid_fwd: 528 750 points
               2 * 520 * 520: 2,                # st_sampler_fwd / bwd: 540 800 points
               (4 * TRIP + 6 + 3) // 4: 2,      # adam_kernel at n = 4 * 524 288 + 6: 524 290 groups of four (+ a tail of 2)
               TRIP + 3: 2,                     # mul / axpby / scale_by_scalar
               4 * 419 * 417: 2,                # nchw3_to_nhwc4: 698 892 pixels
               1003: 1},
    # single-block reductions, items -> trips of thread 0
    'block': {1: 1, 5: 1, 255: 1, 256: 1, 257: 2, 600: 3, 1542: 7, 75 * 75: 22},
}


# ---- helpers ---------------------------------------------------------------------------------------------------------------------
def bf16(a):
    return C.round_bf16(np.asarray(a, F32))


def f64(a):
    return None if a is None else np.asarray(a, np.float64)


def block_reduce32(terms):
    """fp32: thread t adds items t, t + 256, ... in order; wave_sum's xor butterfly (32, 16, .. 1); sh[0] + sh[1] + sh[2] + sh[3].
    terms (..., L) -> (...)"""
    terms = np.asarray(terms, F32)
    L = terms.shape[-1]
    T = -(-L // BLOCK)
    pad = np.zeros(terms.shape[:-1] + (T * BLOCK,), F32)
    pad[..., :L] = terms
    pad = pad.reshape(terms.shape[:-1] + (T, BLOCK))
    acc = np.zeros(terms.shape[:-1] + (BLOCK,), F32)
    for t in range(T):
        acc = acc + pad[..., t, :]
    return wave_fold32(acc)


def wave_fold32(acc):
    """(..., 256) per-thread values -> block_sum"""
    v = acc.reshape(acc.shape[:-1] + (4, 64))
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ o]
    w = v[..., 0]
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


class Worst(dict):
    """name -> largest error / bound seen; 'share:<name>' -> share of elements left out of a comparison (always 0 here)"""

    def ratio(self, name, got, ref, bound, what=''):
        got, ref, bound = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(bound, np.float64)
        assert got.shape == ref.shape == bound.shape, (name, what, got.shape, ref.shape, bound.shape)
        nan = np.isnan(ref)
        assert np.array_equal(np.isnan(got), nan), (name, what, 'NaN pattern')
        err = np.abs(np.where(nan, 0.0, got - ref))
        ok = (err <= bound) | nan
        with np.errstate(divide='ignore', invalid='ignore'):
            r = np.where(err == 0, 0.0, err / bound)
        worst = float(r.max()) if r.size else 0.0
        self[name] = max(self.get(name, 0.0), worst)
        assert ok.all(), '%s %s: error / bound %.3f at %d of %d elements' % (name, what, worst, int((~ok).sum()), ok.size)

    def exact(self, name, got, want, what=''):
        got, want = np.asarray(got), np.asarray(want)
        assert got.shape == want.shape, (name, what, got.shape, want.shape)
        if got.dtype == F32 and want.dtype == F32:                      # the same bits; +0 and -0 count as the same number
            got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
            same = (got.view(np.uint32) == want.view(np.uint32)) | ((got == 0) & (want == 0))
        else:
            same = got == want
        assert same.all(), '%s %s: %d of %d elements differ in their bits' % (name, what, int((~same).sum()), same.size)
        self['exact:' + name] = 0.0

    def share(self, name, excluded, total):
        s = float(excluded) / max(int(total), 1)
        self['share:' + name] = max(self.get('share:' + name, 0.0), s)
        assert s == 0.0, (name, excluded, total)


def report(label, fn, impl, *args):
    w = Worst()
    fn(impl, w, *args)
    print('%s %s%s %s' % (label, fn.__name__, args if len(repr(args)) < 80 else '', json.dumps({k: round(v, 3) for k, v in sorted(w.items())})))
    return w


def merge(total, w):
    for k, v in w.items():
        total[k] = max(total.get(k, 0.0), v)


# =================================================================================================================================
# GAP
# =================================================================================================================================
GAP_HW = (1, 3, 4, 13, 16, 17, 49, 256)
GAP_C = (4, 96, 260, 512, 2048)
GAP_B = (1, 3)
GAP_BWD_BIG = (5, 256, 2048)      # 655 360 four-channel groups: gap_bwd_kernel's grid-stride loop runs twice


def make_gap(B, HW, C_, seed, is16):
    """x (B, HW, C) NHWC.  Channel c has profile c % 4, so that every group of four holds all of them: 0 N(0, 1); 1 mean >> std
    (100 + N(0, 1)); 2 constant 0.75; 3 N(0, 1) * 1e-3"""
    rng = np.random.RandomState(seed)
    x = rng.standard_normal((B, HW, C_))
    p = np.arange(C_) % 4
    x[:, :, p == 1] += 100.0
    x[:, :, p == 2] = 0.75
    x[:, :, p == 3] *= 1e-3
    x = x.astype(F32)
    return bf16(x) if is16 else x


def gap_fwd_depth(HW):
    """roundings on the longest path: phase 0's accumulator takes its unrolled + tail additions, then (s0 + s1) + (s2 + s3): 2,
    the four phases: 2, and the product with fp32(1 / HW): the reciprocal's rounding and the product's: 2"""
    un, tail = gap_fwd_regime(HW, 4)[:2]
    return un + tail + 2 + 2 + 2


def check_gap_fwd(impl, w, B, HW, C_, is16):
    x = make_gap(B, HW, C_, 1000 + HW * 7 + C_, is16)
    ref = C.gap_fwd(f64(x).transpose(0, 2, 1)[..., None])
    bound = gap_fwd_depth(HW) * U * np.abs(f64(x)).mean(axis=1)
    got = impl.gap_fwd(x, is16)
    w.ratio('gap_fwd' + ('_bf16' if is16 else ''), got, ref, bound, (B, HW, C_))
    w.exact('gap_fwd twice', impl.gap_fwd(x, is16), got)
    if HW == 1 and not is16:
        w.exact('gap_fwd HW=1', got, x[:, 0])


def check_gap_bwd(impl, w, B, HW, C_, is16):
    rng = np.random.RandomState(2000 + HW * 7 + C_)
    gy = rng.standard_normal((B, C_)).astype(F32)
    ref = C.gap_bwd((B, C_, HW, 1), f64(gy))[..., 0].transpose(0, 2, 1)
    b32 = 2 * U * np.abs(ref)                                   # fp32(1 / HW): 1, the product: 1
    bound = b32 + (U16 * (np.abs(ref) + b32) if is16 else 0.0)
    got = impl.gap_bwd(gy, HW, is16)
    w.ratio('gap_bwd' + ('_bf16' if is16 else ''), got, ref, bound, (B, HW, C_))
    w.exact('gap_bwd rows', got, np.broadcast_to(got[:, :1], got.shape))        # every pixel gets the same bits


# =================================================================================================================================
# small Linear
# =================================================================================================================================
LIN_K = (4, 1024, 1028, 7168, 7172, 8196, 41472)
LIN_N = (1, 2, 6, 8)
LIN_B = (1, 5, 16, 17, 33, 257)


def linear_cases():
    """dicts; not the full product: every K meets N in {1, 6}; every B meets K in {1028, 8196}; B = 257 meets K = 41 472 once"""
    cases = []
    def add(K, N, B, act_in=False, act_out=False, bias=True, is16=False, mode='all'):
        cases.append(dict(K=K, N=N, B=B, act_in=act_in, act_out=act_out, bias=bias, is16=is16, mode=mode))
    for K in LIN_K:
        add(K, 1, 5, act_in=True, act_out=True, bias=False)           # the assessor head's form
        add(K, 6, 5)                                                  # the localizer head's form
        add(K, 6, 5, is16=True, act_in=K % 8 == 4)
    for B in LIN_B:
        add(1028, 2, B, act_out=True)                                 # n < N inside NMAX = 8 with N = 2
        add(8196, 8, B, act_in=True)
        add(1028, 1, B, is16=True, act_in=True, act_out=True, bias=False)
    add(41472, 1, 257, act_in=True, act_out=True, bias=False)
    for act_in in (False, True):
        for act_out in (False, True):
            for bias in (False, True):
                add(1028, 6, 17, act_in, act_out, bias)
    for mode in ('no_gx', 'gW', 'gb'):
        add(1028, 2, 17, act_in=True, act_out=True, mode=mode)
    return cases


def linear_id(c):
    return 'K%d-N%d-B%d%s%s%s%s%s' % (c['K'], c['N'], c['B'], '-relu' if c['act_in'] else '', '-sig' if c['act_out'] else '',
                                      '-bias' if c['bias'] else '', '-bf16' if c['is16'] else '', '' if c['mode'] == 'all' else '-' + c['mode'])


def make_linear(c):
    rng = np.random.RandomState(3000 + c['K'] + 17 * c['N'] + 131 * c['B'] + c['act_in'] + 2 * c['act_out'])
    K, N, B = c['K'], c['N'], c['B']
    x = rng.standard_normal((B, K)).astype(F32)
    x[:, ::7] = 0.0                                                    # exact zeros: relu's mask is x > 0
    if c['is16']:
        x = bf16(x)
    W = (rng.standard_normal((N, K)) / np.sqrt(K) * 2).astype(F32)
    b = rng.standard_normal(N).astype(F32) if c['bias'] else None
    gy = rng.standard_normal((B, N)).astype(F32)
    gW0 = rng.standard_normal((N, K)).astype(F32)                      # the kernels do +=: the destinations start non-zero
    gb0 = rng.standard_normal(N).astype(F32)
    return x, W, b, gy, gW0, gb0


def check_linear(impl, w, c):
    x, W, b, gy, gW0, gb0 = make_linear(c)
    K, N, B, is16 = c['K'], c['N'], c['B'], c['is16']
    tag = '_bf16' if is16 else ''
    xa = np.maximum(f64(x), 0) if c['act_in'] else f64(x)
    z = C.linear_fwd(xa, f64(W), f64(b))
    # per thread: the four products of a group summed (1 + 3), one addition per trip; block_sum: 6 + 3; the bias: 1
    trips = -(-K // LIN_TRIP)
    bz = (4 + trips + 9 + 1) * U * (np.abs(xa) @ np.abs(f64(W)).T + (np.abs(f64(b)) if b is not None else 0.0))
    if c['act_out']:
        ref = C.sigmoid(z)
        # z * 0.5 is exact; tanhf: 2 ulp; * 0.5 exact; + 0.5: 1.  The error of z passes with d sigmoid / dz = y (1 - y)
        by = bz * ref * (1 - ref) + 0.5 * ULP2 * np.abs(np.tanh(z / 2)) + U * ref
    else:
        ref, by = z, bz
    y = impl.linear_fwd(x, W, b, c['act_in'], c['act_out'], is16)
    w.ratio('linear_fwd' + tag, y, ref, by, linear_id(c))
    w.exact('linear_fwd twice', impl.linear_fwd(x, W, b, c['act_in'], c['act_out'], is16), y)

    # backward: y is an INPUT (the forward's fp32 output), the reference differentiates at it
    y64 = f64(y)
    gz = C.sigmoid_bwd(y64, f64(gy)) if c['act_out'] else f64(gy)
    kz = 3 if c['act_out'] else 0                                       # g * y: 1, 1 - y: 1, the product: 1
    mode = c['mode']
    gx, gW, gb = impl.linear_bwd(x, W, y if c['act_out'] else None, gy, None if mode == 'gb' else gW0,
                                 None if mode == 'gW' else gb0, mode == 'all', c['act_in'], c['act_out'], is16)
    gx_ref, gW_ref, gb_ref = C.linear_bwd(xa, f64(W), gz, True)
    if mode == 'all':
        if c['act_in']:
            gx_ref = gx_ref * (f64(x) > 0)
        b32 = (kz + 1 + N) * U * (np.abs(gz) @ np.abs(f64(W)))          # per term gz's roundings, the product, N additions
        if c['act_in']:
            b32 = b32 * (f64(x) > 0)
        bx = b32 + (U16 * (np.abs(gx_ref) + b32) if is16 else 0.0)
        w.ratio('linear_bwd gx' + tag, gx, gx_ref, bx, linear_id(c))
        if c['act_in']:                                                 # x is an input: its sign is nobody's rounding
            w.exact('linear_bwd relu mask', gx[x <= 0], np.zeros(int((x <= 0).sum()), F32))
            w.share('linear_bwd relu mask', 0, gx.size)
    else:
        assert gx is None
    slabs = -(-B // LIN_SLAB)
    if mode != 'gb':
        # a slab's chain: up to 16 products (1 each) and additions; the slabs and the initial value meet in atomics: slabs
        bW = (kz + 1 + min(B, LIN_SLAB) + slabs) * U * (np.abs(gz).T @ np.abs(xa) + np.abs(f64(gW0)))
        w.ratio('linear_bwd gW' + tag, gW, gW_ref + f64(gW0), bW, linear_id(c))
        if slabs == 1:                                                  # one atomic per element: the order is fixed
            gW2 = impl.linear_bwd(x, W, y if c['act_out'] else None, gy, gW0, None, False, c['act_in'], c['act_out'], is16)[1]
            w.exact('linear_bwd gW twice', gW2, gW)
    else:
        assert gW is None
    if mode != 'gW':
        bb = (kz + depth_block(B) + 1) * U * (np.abs(gz).sum(axis=0) + np.abs(f64(gb0)))
        w.ratio('linear_bwd gb', gb, gb_ref + f64(gb0), bb, linear_id(c))
        gb2 = impl.linear_bwd(x, W, y if c['act_out'] else None, gy, None, gb0, False, c['act_in'], c['act_out'], is16)[2]
        w.exact('linear_bwd gb twice', gb2, gb)
    else:
        assert gb is None


# =================================================================================================================================
# spatial transformer: grid
# =================================================================================================================================
ST_SIZES = ((1, 1), (1, 7), (7, 1), (2, 2), (16, 16), (75, 75))        # P = 256: one trip of the backward's loop; 5625: 22
ST_B = (1, 4)
ST_BIG = (94, 75, 75)                                                  # B P = 528 750 > 524 288: st_grid_fwd's second trip


def make_theta(B, kind, seed):
    rng = np.random.RandomState(seed)
    ident = np.tile(np.array([[1, 0, 0], [0, 1, 0]], F32), (B, 1, 1))
    if kind == 'identity':
        return ident
    if kind == 'random':
        return (0.8 * ident + 0.3 * rng.standard_normal((B, 2, 3))).astype(F32)
    assert kind == 'large'
    t = (ident + rng.standard_normal((B, 2, 3))).astype(F32)
    t[:, 0, 1] = 1e3
    t[:, 1, 2] = -1e3
    return t


def check_st_grid(impl, w, B, th, tw, kind):
    theta = make_theta(B, kind, 4000 + th * 100 + tw + B)
    ref, coords = C.st_grid_fwd(f64(theta), (th, tw))
    # t0 xs + t1 ys + t2: the fp32 coordinate (1), the product (1) and the two additions a term passes (2); t2 only the additions
    a = np.abs(f64(theta))
    bound = 4 * U * (a[:, :, :2] @ np.abs(coords[:2].reshape(2, -1)) + a[:, :, 2:]).reshape(ref.shape)
    got = impl.st_grid_fwd(theta, th, tw)
    w.ratio('st_grid_fwd', got, ref, bound, (B, th, tw, kind))
    w.exact('st_grid_fwd twice', impl.st_grid_fwd(theta, th, tw), got)
    if kind == 'identity':
        # the sample coordinates themselves: numpy.linspace(-1, 1, n, dtype=float32); n = 1 gives -1, the last point is exactly 1
        xs, ys = np.linspace(-1, 1, tw, dtype=F32), np.linspace(-1, 1, th, dtype=F32)
        assert xs[0] == -1 and ys[0] == -1 and (tw == 1 or xs[-1] == 1) and (th == 1 or ys[-1] == 1)
        w.exact('st_grid_fwd linspace x', got[:, 0], np.broadcast_to(xs[None, None, :], (B, th, tw)))
        w.exact('st_grid_fwd linspace y', got[:, 1], np.broadcast_to(ys[None, :, None], (B, th, tw)))
    if B * th * tw > TRIP:
        return
    rng = np.random.RandomState(4500 + th * 100 + tw + B)
    gg = rng.standard_normal((B, 2, th, tw)).astype(F32)
    gref = C.st_grid_bwd(coords, f64(gg))
    # per term: the fp32 coordinate (1) and the product (1); a 256-strided chain over P and block_sum
    bb = (2 + depth_block(th * tw)) * U * (np.abs(f64(gg)).reshape(B, 2, -1) @ np.abs(coords.reshape(3, -1)).T)
    gt = impl.st_grid_bwd(gg)
    w.ratio('st_grid_bwd', gt, gref, bb, (B, th, tw))
    w.exact('st_grid_bwd twice', impl.st_grid_bwd(gg), gt)


# =================================================================================================================================
# spatial transformer: sampler
# =================================================================================================================================
SAMPLER_FRAMES = ((2, 2), (5, 3), (20, 28), (48, 64))                  # (H, W); the launcher's minimum is 2
SAMPLER_BIG = (2, 48, 64, 520, 520)                                    # B P = 540 800 > 524 288
# on the (5, 3) frame: u = (gx + 1) (W - 1) / 2 + 1 in {0, 4 = W + 1, 1, 3, 2, -0.5, 5}, v in {0, 6 = H + 1, 1, 5, 3, -3, 7},
# exactly in float32: both clip borders, both mask borders, the first and last pixel centres, and outside
HAND_GX = np.array([-2, 2, -1, 1, 0, -2.5, 3], F32)
HAND_GY = np.array([-1.5, 1.5, -1, 1, 0, -3, 2], F32)
HAND_U = np.array([0, 4, 1, 3, 2, -0.5, 5], F32)
HAND_V = np.array([0, 6, 1, 5, 3, -3, 7], F32)


def sampler_grids(B, H, W):
    """(name, grid (B, 2, th, tw) fp32)"""
    out = []
    for kind, size in (('identity', (3, 5)), ('random', (9, 11)), ('large', (4, 4))):
        out.append((kind, C.st_grid_fwd(make_theta(B, kind, 5000 + H + W), size)[0].astype(F32)))
    rng = np.random.RandomState(5100 + H + W)
    # a tiny box: every sample inside one pixel cell (the cell of pixel (0, 0): u, v in (1, 2))
    cx, cy = 2.0 * 0.5 / (W - 1) - 1, 2.0 * 0.5 / (H - 1) - 1
    tiny = np.stack([cx + 0.2 / (W - 1) * (rng.random_sample((B, 6, 6)) - 0.5), cy + 0.2 / (H - 1) * (rng.random_sample((B, 6, 6)) - 0.5)], axis=1)
    out.append(('tiny', tiny.astype(F32)))
    far = (rng.standard_normal((B, 2, 5, 5)) * 10.0 ** rng.uniform(0, 6, (B, 2, 5, 5))).astype(F32)
    out.append(('far', np.clip(far, -1e6, 1e6)))
    if (H, W) == (5, 3):
        gx, gy = np.meshgrid(HAND_GX, HAND_GY)
        out.append(('hand', np.broadcast_to(np.stack([gx, gy])[None], (B, 2, 7, 7)).astype(F32).copy()))
    return out


def sampler_setup32(img, grid):
    """the float32 decisions of chainer's sampler (oracle._st_sampler_setup on the fp32 inputs): coordinates, clip, floor"""
    assert img.dtype == F32 and grid.dtype == F32
    x_pad, u, v, uc, vc, u0, u1, v0, v1 = C._st_sampler_setup(img, grid)
    assert u.dtype == F32 and uc.dtype == F32
    return x_pad, u, v, uc, vc, u0, u1, v0, v1


def sampler_ref(img, grid, gy=None):
    """float64 arithmetic on the float32 decisions.  int32 - float32 is float64 in NumPy, so the weights are exact differences.
    -> (rois (B, 3, th, tw), bound) or, with gy, (ggrid (B, 2, th, tw), bound)"""
    B, _, H, W = img.shape
    th, tw = grid.shape[2:]
    x_pad, u, v, uc, vc, u0, u1, v0, v1 = sampler_setup32(img, grid)
    xp = f64(x_pad)
    wu0, wu1, wv0, wv1 = f64(uc) - u0, u1 - f64(uc), f64(vc) - v0, v1 - f64(vc)
    x1, x2, x3, x4 = (C._st_gather(xp, a, b) for a, b in ((v0, u0), (v0, u1), (v1, u0), (v1, u1)))       # (B, P, 3)
    nchw = lambda a: a.reshape(B, th, tw, -1).transpose(0, 3, 1, 2)     # noqa: E731
    if gy is None:
        ws = [(wu1 * wv1)[:, :, None], (wu0 * wv1)[:, :, None], (wu1 * wv0)[:, :, None], (wu0 * wv0)[:, :, None]]
        y = sum(wi * xi for wi, xi in zip(ws, (x1, x2, x3, x4)))
        # per term: the weight's rounding to fp32 (1), the product (1), three additions (3)
        bound = 5 * U * sum(np.abs(wi * xi) for wi, xi in zip(ws, (x1, x2, x3, x4)))
        return nchw(y), nchw(bound)
    g = f64(gy).transpose(0, 2, 3, 1).reshape(B, th * tw, 3)
    a, b, c, d = wv1[:, :, None], wv0[:, :, None], wu1[:, :, None], wu0[:, :, None]
    du = -a * x1 + a * x2 - b * x3 + b * x4
    dv = -c * x1 - d * x2 + c * x3 + d * x4
    mu = (u > 0) & (u < W + 1)                                          # float32 comparisons
    mv = (v > 0) & (v < H + 1)
    gu = (du * g).sum(axis=2) / 2. * (W - 1) * mu
    gv = (dv * g).sum(axis=2) / 2. * (H - 1) * mv
    # per term: the weight's rounding to fp32 (1), its product (1), three additions inside du (3), du * g (1), the three
    # channels (3), / 2 exact, * (W - 1) (1)
    ku = 10 * U
    bu = ku * ((np.abs(a * x1) + np.abs(a * x2) + np.abs(b * x3) + np.abs(b * x4)) * np.abs(g)).sum(axis=2) / 2. * (W - 1) * mu
    bv = ku * ((np.abs(c * x1) + np.abs(d * x2) + np.abs(c * x3) + np.abs(d * x4)) * np.abs(g)).sum(axis=2) / 2. * (H - 1) * mv
    shp = (B, 1, th, tw)
    return np.concatenate([gu.reshape(shp), gv.reshape(shp)], axis=1), np.concatenate([bu.reshape(shp), bv.reshape(shp)], axis=1)


def check_sampler(impl, w, B, H, W, name, grid, backward=True):
    rng = np.random.RandomState(5200 + H * 100 + W)
    img = rng.random_sample((B, 3, H, W)).astype(F32)
    what = (B, H, W, name)
    if name == 'hand':
        _, u, v = sampler_setup32(img, grid)[:3]
        assert np.array_equal(u.reshape(B, 7, 7)[0, 0], HAND_U) and np.array_equal(v.reshape(B, 7, 7)[0, :, 0], HAND_V)
    ref, bound = sampler_ref(img, grid)
    got = impl.st_sampler_fwd(img, grid)
    w.ratio('st_sampler_fwd', got, ref, bound, what)
    w.share('st_sampler index', 0, ref.size)                            # the decisions are float32 on both sides: nothing is left out
    w.exact('st_sampler_fwd == float32 oracle', got, C.st_sampler_fwd(img, grid), what)
    w.exact('st_sampler_fwd twice', impl.st_sampler_fwd(img, grid), got)
    if not backward:
        return
    gy = rng.standard_normal(ref.shape).astype(F32)
    gref, gb = sampler_ref(img, grid, gy)
    gg = impl.st_sampler_bwd(img, grid, gy, None)
    w.ratio('st_sampler_bwd', gg, gref, gb, what)
    masked = (gref == 0) & (gb == 0)                                    # outside 0 < u < W + 1 (float32's decision): exactly 0
    w.exact('st_sampler_bwd mask', gg[masked], np.zeros(int(masked.sum()), F32), what)
    w.exact('st_sampler_bwd twice', impl.st_sampler_bwd(img, grid, gy, None), gg)
    d0 = rng.standard_normal(gref.shape).astype(F32)
    acc = impl.st_sampler_bwd(img, grid, gy, d0)                        # accumulate = 1: the destination starts non-zero
    w.ratio('st_sampler_bwd accumulate', acc, gref + f64(d0), gb + U * (np.abs(gref) + np.abs(f64(d0))), what)
    w.exact('st_sampler_bwd accumulate == d0 + g', acc, d0 + gg, what)


# =================================================================================================================================
# MSE
# =================================================================================================================================
MSE_N = (1, 5, 255, 256, 257, 1542)


def check_mse(impl, w, n, with_target):
    rng = np.random.RandomState(6000 + n)
    y = rng.random_sample(n).astype(F32)
    t = rng.random_sample(n).astype(F32) if with_target else None
    tconst = 0.0 if with_target else 1.0
    gloss = F32(0.37)
    t64 = f64(t) if with_target else np.full(n, tconst)
    d = f64(y) - t64
    ref = C.mse_fwd(f64(y), t64)
    # d: 1 rounding -> 2 u d^2; the product: 1; the chain and block_sum; the division: 2 ulp
    bound = (3 + depth_block(n)) * U * (d * d).sum() / n + ULP2 * abs(ref)
    got = impl.mse_fwd(y, t, tconst)
    w.ratio('mse_fwd', got, ref, bound, (n, with_target))
    w.exact('mse_fwd twice', impl.mse_fwd(y, t, tconst), got)
    gref = C.mse_bwd(f64(y), t64, float(gloss))
    # gloss * 2 exact; / n: 2 ulp; d: 1; the product: 1
    gg = impl.mse_bwd(y, t, tconst, gloss)
    w.ratio('mse_bwd', gg, gref, (ULP2 + 2 * U) * np.abs(gref), (n, with_target))
    w.exact('mse_bwd twice', impl.mse_bwd(y, t, tconst, gloss), gg)


# =================================================================================================================================
# grid regularisers
# =================================================================================================================================
REG_B = (1, 3, 256, 257, 600)
REG_SIZES = ((1, 1), (1, 6), (5, 1), (5, 6))
REG_IMAGES = ((48, 64), (75, 100), (224, 224))
REG_GAP = 1e-3
# ties whose scaled products are inexact: rows with tly == bly == t (and tlx == trx == t).  With s = (t + 1) / 2 in float32,
# exact(s * size) - round(s * size) is negative in TIES_NEG and positive in TIES_POS: a kernel that fused the subtraction with one
# of the two products would see a negative distance (and drop the tie's gradient) in the first group and a positive one (a
# non-zero forward term) in the second
TIES_NEG = ((0.3, 75), (0.1, 48), (-0.7, 224), (0.55, 100))
TIES_POS = ((0.3, 224), (0.1, 75), (0.55, 48))


def tie_residual(t, size):
    """exact(s * size) - fp32(s * size), s = fp32((fp32(t) + 1) / 2); float64 holds the 24 x 8 bit product exactly"""
    s = F32(F32(F32(t) + F32(1)) / F32(2))
    return float(s) * size - float(F32(s * F32(size)))


def make_reg_grid(B, th, tw, image, seed):
    """random boxes, with every distance the regularisers compare either exactly 0 or at least REG_GAP away from it (asserted):
    the sign is then the same in float32 and float64"""
    H, W = image
    rng = np.random.RandomState(seed)
    g = (0.9 * rng.standard_normal((B, 2, th, tw))).astype(F32)
    if th > 1 and tw > 1:
        for i, (t, _) in enumerate(TIES_NEG + TIES_POS):                # tie rows, as far as the batch has room
            if i < B:
                g[i, 1, 0, 0] = g[i, 1, th - 1, 0] = F32(t)
                g[i, 0, 0, 0] = g[i, 0, 0, tw - 1] = F32(t)
        if B > 8:
            g[7, 0, 0, tw - 1] = 1.0                                    # the exact ties of the out-of-image term
            g[8, 1, 0, 0] = -1.0
    for _ in range(4):                                                  # push near misses away
        corners = [g[:, 0, 0, 0], g[:, 1, 0, 0], g[:, 0, 0, tw - 1], g[:, 1, th - 1, 0]]
        for v in corners:
            for e in (-1.0, 1.0):
                near = (np.abs(v - e) < 4 * REG_GAP) & (v != e)
                v[near] += F32(16 * REG_GAP)
        d1 = (f64(g[:, 1, 0, 0]) - g[:, 1, th - 1, 0]) / 2 * H
        d2 = (f64(g[:, 0, 0, 0]) - g[:, 0, 0, tw - 1]) / 2 * W
        g[(np.abs(d1) < 4 * REG_GAP) & (d1 != 0), 1, 0, 0] += F32(0.05)
        g[(np.abs(d2) < 4 * REG_GAP) & (d2 != 0), 0, 0, 0] += F32(0.05)
    assert_reg_gaps(g, image)
    return g


def assert_reg_gaps(g, image):
    H, W = image
    th, tw = g.shape[2:]
    x = f64(g)
    d1 = (x[:, 1, 0, 0] - x[:, 1, th - 1, 0]) / 2 * H
    d2 = (x[:, 0, 0, 0] - x[:, 0, 0, tw - 1]) / 2 * W
    for d in (d1, d2):
        assert ((d == 0) | (np.abs(d) >= REG_GAP)).all()
    for v in (x[:, 0, 0, 0], x[:, 1, 0, 0], x[:, 0, 0, tw - 1], x[:, 1, th - 1, 0]):
        for e in (-1.0, 1.0):
            assert ((v == e) | (np.abs(v - e) >= REG_GAP)).all()


def check_regularisers(impl, w, B, th, tw, image, oob):
    H, W = image
    g = make_reg_grid(B, th, tw, image, 7000 + B + 10 * th + tw + H)
    x = f64(g)
    gloss = F32(0.6)
    what = (B, th, tw, image, oob)
    # ---- direction: the sign is float32's (the oracle run in float32), the arithmetic float64's
    l64, g64 = C.direction_loss(x, image)
    _, g32 = C.direction_loss(g, image)
    w.share('direction sign', int(((g32 != 0) != (g64 != 0)).sum()), g64.size)
    a1, b1 = (x[:, 1, 0, 0] + 1) / 2 * H, (x[:, 1, th - 1, 0] + 1) / 2 * H
    a2, b2 = (x[:, 0, 0, 0] + 1) / 2 * W, (x[:, 0, 0, tw - 1] + 1) / 2 * W
    # a scaled corner: g + 1 (1), / 2 exact, * size (1): 2 u |a|; the difference: 1; the sum of the two terms: 1; the chain
    # over the batch and block_sum; / B: 2 ulp
    per = sum(np.where(a - b > 0, 2 * U * (np.abs(a) + np.abs(b)) + U * np.abs(a - b), 0.0) for a, b in ((a1, b1), (a2, b2)))
    terms = np.maximum(a1 - b1, 0) + np.maximum(a2 - b2, 0)
    bound = (per.sum() + (1 + depth_block(B)) * U * terms.sum()) / B + ULP2 * abs(l64)
    got = impl.grid_loss_fwd(g, 0, H, W, 1.0)
    w.ratio('direction_fwd', got, l64, bound, what)
    w.exact('direction_fwd twice', impl.grid_loss_fwd(g, 0, H, W, 1.0), got)
    gg = impl.grid_loss_bwd(g, gloss, 0, H, W, 1.0)
    ref = g64 * float(gloss)
    w.ratio('direction_bwd', gg, ref, (ULP2 + U) * np.abs(ref), what)   # gl / B: 2 ulp; * (size / 2), itself exact: 1
    w.exact('direction_bwd mask', gg != 0, ref != 0, what)
    w.exact('direction_bwd twice', impl.grid_loss_bwd(g, gloss, 0, H, W, 1.0), gg)
    # ---- out of image
    l64, g64 = C.out_of_image_loss(x)
    _, g32 = C.out_of_image_loss(g)
    w.share('out_of_image sign', int((g32 != g64).sum()), g64.size)
    # v + 1, v - 1: 1; the eight terms of a sample: 7; the chain and block_sum; * oob_scale: 1
    bound = (1 + 7 + depth_block(B) + 1) * U * abs(l64) * oob
    got = impl.grid_loss_fwd(g, 1, 0.0, 0.0, oob)
    w.ratio('out_of_image_fwd', got, l64 * oob, bound, what)
    gg = impl.grid_loss_bwd(g, gloss, 1, 0.0, 0.0, oob)
    ref = g64 * float(gloss) * oob
    w.ratio('out_of_image_bwd', gg, ref, U * np.abs(ref), what)         # gl * oob_scale: 1; sums of +-s and 0 are exact
    w.exact('out_of_image_bwd mask', gg != 0, ref != 0, what)
    w.exact('out_of_image_bwd twice', impl.grid_loss_bwd(g, gloss, 1, 0.0, 0.0, oob), gg)


def check_regulariser_ties(impl, w):
    """every row a tie in y and in x with an inexact scaled product: the forward term is exactly 0, the gradient is written out"""
    B, th, tw = 4, 5, 6                                                 # gl / B = 0.25 and size / 2 / 4 are exact in fp32
    for t, size in TIES_NEG + TIES_POS:
        assert tie_residual(t, size) != 0
        rng = np.random.RandomState(int(1000 * abs(t)) + size)
        g = (0.5 * rng.standard_normal((B, 2, th, tw))).astype(F32)
        g[:, 1, 0, 0] = g[:, 1, th - 1, 0] = F32(t)
        g[:, 0, 0, 0] = g[:, 0, 0, tw - 1] = F32(t)
        other = {75: 100, 100: 75, 48: 64, 224: 224}[size]
        for H, W in ((size, other), (other, size)):
            w.exact('tie forward', impl.grid_loss_fwd(g, 0, H, W, 1.0), np.zeros((), F32), (t, H, W))
            want = np.zeros_like(g)
            want[:, 1, 0, 0], want[:, 1, th - 1, 0] = H / 2.0 / B, -H / 2.0 / B
            want[:, 0, 0, 0], want[:, 0, 0, tw - 1] = W / 2.0 / B, -W / 2.0 / B
            w.exact('tie gradient', impl.grid_loss_bwd(g, F32(1.0), 0, H, W, 1.0), want, (t, H, W))
            np.testing.assert_array_equal(C.direction_loss(g, (H, W))[1], want)
    # the out-of-image ties: v - 1 == 0 passes the gradient, v + 1 == 0 does not (|min(v + 1, 0)| has sign(0) = 0)
    g = np.zeros((B, 2, th, tw), F32)
    g[:, 0, 0, tw - 1] = 1.0
    g[:, 1, th - 1, 0] = 1.0
    g[:, 0, 0, 0] = -1.0
    g[:, 1, 0, 0] = -1.0
    want = np.zeros_like(g)
    want[:, 0, 0, tw - 1] = want[:, 1, th - 1, 0] = 4.0
    w.exact('tie forward', impl.grid_loss_fwd(g, 1, 0.0, 0.0, 4.0), np.zeros((), F32))
    w.exact('tie gradient', impl.grid_loss_bwd(g, F32(1.0), 1, 0.0, 0.0, 4.0), want)
    # (1, 1): all corners coincide, += and -= land on one element
    g = np.full((B, 2, 1, 1), 1.5, F32)
    w.exact('tie gradient', impl.grid_loss_bwd(g, F32(1.0), 0, 48, 64, 1.0), np.zeros_like(g), '1x1 direction')
    w.exact('tie gradient', impl.grid_loss_bwd(g, F32(1.0), 1, 0.0, 0.0, 1.0), np.full_like(g, 2.0), '1x1 out of image')


# =================================================================================================================================
# Adam / AMSGrad
# =================================================================================================================================
ADAM_N = (1, 2, 3, 4, 5, 1003, 1024)
ADAM_BIG = 4 * TRIP + 6                                                 # 524 290 groups of four: the grid-stride loop's second trip
# (beta2, eta, weight decay, gradient scale)
ADAM_HYPER = ((0.999, 1.0, 0.0, 1.0), (0.999, 0.5, 1e-2, 0.125), (0.5, 1.0, 0.0, 1.0))
ADAM_ALPHA, ADAM_BETA1, ADAM_EPS, ADAM_T = 1e-3, 0.9, 1e-8, 3


def make_adam(n, seed=8000):
    """state from earlier steps: m, v non-zero, vhat above v on some elements and below on others; gradients spanning
    1e-9 .. 1, exact zeros with m = v = vhat = 0, and a block of 1e-20 (g^2 underflows)"""
    rng = np.random.RandomState(seed + n % 9973)
    p = rng.standard_normal(n).astype(F32)
    g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-9, 0, n)).astype(F32)
    m = (0.1 * rng.standard_normal(n) * np.abs(g)).astype(F32)
    v = (np.abs(g) ** 2 * rng.uniform(0.1, 2, n)).astype(F32)
    vh = (v * np.where(rng.random_sample(n) < 0.5, 4.0, 0.25)).astype(F32)
    if n >= 64:
        z = slice(8, 24)
        g[z] = m[z] = v[z] = vh[z] = 0.0
        s = slice(24, 40)
        g[s] = 1e-20
        v[s] = vh[s] = 0.0
        m[s] = 1e-21
    return p, g, m, v, vh


def adam_ref(p, g, m, v, vh, lr, beta2, eta, wd, gs):
    """oracle.adam_amsgrad_update in float64 on the scaled gradient -> new (p, m, v, vh) and their bounds"""
    p64, g64, m64, v64 = f64(p).copy(), f64(g) * gs, f64(m).copy(), f64(v).copy()
    vh64 = None if vh is None else f64(vh).copy()
    p0, m0, v0 = p64.copy(), m64.copy(), v64.copy()
    # adam_lr(alpha, beta1, beta2, t) is what the caller hands the kernel as lr_t
    C.adam_amsgrad_update(p64, g64, m64, v64, vh64, ADAM_T, alpha=ADAM_ALPHA, beta1=ADAM_BETA1, beta2=beta2, eps=ADAM_EPS,
                          eta=eta, weight_decay_rate=wd, amsgrad=vh is not None)
    assert lr == C.adam_lr(ADAM_ALPHA, ADAM_BETA1, beta2, ADAM_T)
    a, b = 1 - ADAM_BETA1, 1 - beta2
    e_g = 2 * U * np.abs(g64)                                   # fp32(grad_scale): 1, the product: 1
    d = g64 - m0
    # m += a (g - m): the difference carries e_g and 1; fp32(a): 1, the product: 1; the sum: 1
    e_m = a * e_g + 3 * U * np.abs(a * d) + U * np.abs(m64)
    # g^2: 2 |g| e_g + 1 = 5 u g^2, and it can underflow; the difference: 1; fp32(b), the product (can underflow): 2; the sum: 1
    e_sq = 5 * U * g64 * g64 + UF
    dv = g64 * g64 - v0
    e_v = b * e_sq + 3 * U * np.abs(b * dv) + U * np.abs(v64) + UF
    if vh is None:
        den2, e_den2 = v64, e_v
        e_vh = None
    else:
        # max is 1-Lipschitz in v; where v + e_v stays below vhat the old vhat comes back bit for bit
        e_vh = np.where(v64 + e_v >= f64(vh), e_v, 0.0)
        den2, e_den2 = vh64, e_vh
    sq = np.sqrt(den2)
    # sqrtf: 2 ulp, and |sqrt(x + e) - sqrt(x)| <= min(e / (2 sqrt(x)), sqrt(e)); + fp32(eps): 1 for eps, 1 for the sum
    with np.errstate(divide='ignore', invalid='ignore'):
        e_sq_root = np.minimum(np.where(sq > 0, e_den2 / (2 * sq), np.inf), np.sqrt(e_den2)) + ULP2 * sq
    den = sq + ADAM_EPS
    e_den = e_sq_root + U * ADAM_EPS + U * den
    step = lr * m64 / den
    # fp32(lr_t): 1, lr_t * m: 1, the division: 2 ulp
    e_step = lr * e_m / den + np.abs(step) * e_den / den + (2 * U + ULP2) * np.abs(step)
    inner = step + wd * p0
    # fp32(wd), wd * p: 2; the sum: 1; fp32(eta), the product: 2; p - ...: 1
    e_p = eta * (e_step + 2 * U * np.abs(wd * p0) + U * np.abs(inner)) + 2 * U * np.abs(eta * inner) + U * np.abs(p64)
    return (p64, m64, v64, vh64), (e_p, e_m, e_v, e_vh)


def check_adam(impl, w, n):
    p, g, m, v, vh = make_adam(n)
    for beta2, eta, wd, gs in ADAM_HYPER:
        lr = C.adam_lr(ADAM_ALPHA, ADAM_BETA1, beta2, ADAM_T)
        for ams in (True, False):
            what = (n, beta2, eta, wd, gs, ams)
            refs, bounds = adam_ref(p, g, m, v, vh if ams else None, lr, beta2, eta, wd, gs)
            args = (lr, ADAM_BETA1, beta2, ADAM_EPS, eta, wd, gs)
            got = impl.adam(p, g, m, v, vh if ams else None, *args, dev_lr=False)
            for name, a, r, b in zip(('p', 'm', 'v', 'vhat'), got[:4], refs, bounds):
                if r is not None:
                    w.ratio('adam ' + name, a, r, b, what)
            for i in range(n - (n & 3), n):                             # the tail block 0 handles, element by element
                for a, r, b in zip(got[:3], refs[:3], bounds[:3]):
                    assert abs(float(a[i]) - r[i]) <= b[i], (what, i)
                assert got[1][i] != m[i], (what, i)                     # it was written
            w.exact('adam gradient read only', got[4], g, what)
            again = impl.adam(p, g, m, v, vh if ams else None, *args, dev_lr=False)
            dev = impl.adam(p, g, m, v, vh if ams else None, *args, dev_lr=True)
            for a, b2, c in zip(got[:4], again[:4], dev[:4]):
                if a is not None:
                    w.exact('adam twice', b2, a, what)
                    w.exact('adam device-side rate', c, a, what)
            if ams:
                keep = refs[2] + bounds[2] < f64(vh)
                w.exact('adam vhat kept', got[3][keep], vh[keep], what)
            if n >= 64:
                z = slice(8, 24)                                        # g = m = v = vhat = 0: only the weight decay moves p
                w.exact('adam zeros', got[1][z], np.zeros(16, F32), what)
                w.exact('adam zeros', got[2][z], np.zeros(16, F32), what)
                if wd == 0:
                    w.exact('adam zeros', got[0][z], p[z], what)


# =================================================================================================================================
# glue
# =================================================================================================================================
GLUE_N = (1, 6, 1023, TRIP + 3)
NHWC4_SHAPES = ((1, 1, 1), (2, 5, 7), (4, 419, 417))


def check_glue(impl, w, n):
    rng = np.random.RandomState(9000 + n % 9973)
    x, y = rng.standard_normal(n).astype(F32), rng.standard_normal(n).astype(F32)
    w.exact('mul', impl.mul(x, y), x * y, n)
    s = F32(0.3)
    w.exact('scale_by_scalar', impl.scale_by_scalar(x, s), x * s, n)
    a, b = F32(0.7), F32(-1.3)
    ref = float(a) * f64(x) + float(b) * f64(y)
    bound = 2 * U * (np.abs(float(a) * f64(x)) + np.abs(float(b) * f64(y)))         # each product: 1, the sum: 1
    got, x_after = impl.axpby(a, x, b, y)
    w.ratio('axpby', got, ref, bound, n)
    w.exact('axpby x read only', x_after, x, n)
    nan = np.full(n, np.nan, F32)
    w.exact('axpby b == 0 over NaN', impl.axpby(a, x, F32(0), nan)[0], a * x, n)     # what the branch is for


def check_nhwc4(impl, w, shape):
    B, H, W = shape
    x = np.random.RandomState(9100 + H).standard_normal((B, 3, H, W)).astype(F32)
    got = impl.nchw3_to_nhwc4(x)
    w.exact('nchw3_to_nhwc4 copy', got[..., :3], x.transpose(0, 2, 3, 1), shape)
    w.exact('nchw3_to_nhwc4 fourth channel', got[..., 3], np.zeros((B, H, W), F32), shape)


# =================================================================================================================================
# VisualBackprop / grayscale
# =================================================================================================================================
CM_ROWS = (1, 3, 4, 5, 1000)
CM_C = (4, 64, 260, 512, 2048)
VBP_KSP = ((7, 2, 3), (3, 2, 0), (3, 1, 1), (3, 2, 1))
MINMAX_N = (2, 255, 257, 50176)


def ones_deconv(f, H, W, s, p):
    """F.deconvolution_2d(f, ones(1, 1, kh, kw), stride s, pad p, outsize (H, W)), kh = H + 2p - s (fh - 1)  (visual_backprop.py:29-37)"""
    B, fh, fw = f.shape
    kh, kw = H + 2 * p - s * (fh - 1), W + 2 * p - s * (fw - 1)
    full = np.zeros((B, s * (fh - 1) + kh, s * (fw - 1) + kw))
    for i in range(fh):
        for j in range(fw):
            full[:, s * i:s * i + kh, s * j:s * j + kw] += f[:, i:i + 1, j:j + 1]
    return full[:, p:p + H, p:p + W]


def check_channel_mean(impl, w, rows, C_, is16, affine, cdiv=None):
    rng = np.random.RandomState(9200 + rows + C_)
    x = make_gap(1, rows, C_, 9200 + rows + C_, is16)[0]
    scale = (1 + 0.5 * rng.standard_normal(C_)).astype(F32) if affine else None
    shift = (0.5 * rng.standard_normal(C_)).astype(F32) if affine else None
    cd = cdiv or C_
    x64 = f64(x)
    if affine:
        act = np.maximum(x64 * scale + shift, 0)
        pre = 2 * U * (np.abs(x64 * scale) + np.abs(f64(shift)))        # x * scale: 1, + shift: 1; relu is 1-Lipschitz
    else:
        act, pre = x64, 0.0 * x64
    ref = act.sum(axis=1) / cd
    # a lane's trips: (x + y) + (z + w): 2 and the accumulator: 1 each; wave_sum: 6; fp32(1 / cdiv) and the product: 2
    depth = 3 * -(-C_ // 256) + 6 + 2
    bound = (pre.sum(axis=1) + depth * U * np.abs(act).sum(axis=1)) / cd
    got = impl.channel_mean(x, scale, shift, cd, is16)
    w.ratio('channel_mean' + ('_bf16' if is16 else '') + ('_affine' if affine else ''), got, ref, bound, (rows, C_, cdiv))


def check_vbp_scale(impl, w, k, s, p, H, W):
    fh, fw = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    rng = np.random.RandomState(9300 + 10 * k + s + p + H)
    B = 2
    feat = rng.random_sample((B, fh, fw)).astype(F32)
    feat[0, 0, 0] = -0.5
    avg = rng.standard_normal((B, H, W)).astype(F32)
    ref = ones_deconv(f64(feat), H, W, s, p) * f64(avg)
    cnt = (-(-(H + 2 * p - s * (fh - 1)) // s)) ** 2                    # cells under one pixel: at most ceil(kh / s)^2
    bound = (cnt + 1) * U * ones_deconv(np.abs(f64(feat)), H, W, s, p) * np.abs(f64(avg))     # the chain, and the product with avg
    got = impl.vbp_scale(feat, avg, s, p)
    w.ratio('vbp_scale', got, ref, bound, (k, s, p, H, W))


def check_minmax(impl, w, B, n):
    x = np.random.RandomState(9400 + n).standard_normal((B, n)).astype(F32)
    x64 = f64(x)
    lo, hi = x64.min(axis=1, keepdims=True), x64.max(axis=1, keepdims=True)
    ref = (x64 - lo) / (hi - lo)
    # min and max are exact; hi - lo: 1; 1 / (hi - lo): 2 ulp; x - lo: 1; the product: 1
    got = impl.minmax(x)
    w.ratio('minmax_normalize', got, ref, (3 * U + ULP2) * np.abs(ref), (B, n))
    assert (got.min(axis=1) == 0).all()
    const = np.full((B, n), 0.25, F32)                                  # 0 / 0, as the reference's
    assert np.isnan(impl.minmax(const)).all()


def check_gray(impl, w, n):
    rng = np.random.RandomState(9500 + n)
    rois = rng.standard_normal((1, n, 1, 4)).astype(F32)
    r64 = f64(rois)[0, :, 0]
    terms = np.stack([0.299 * r64[:, 2], 0.587 * r64[:, 1], 0.114 * r64[:, 0]])
    # each fp32 constant: 1, each product: 1, two additions: 2
    got = impl.gray_fwd(rois)
    w.ratio('gray_fwd', got.reshape(-1), terms.sum(axis=0), 4 * U * np.abs(terms).sum(axis=0), n)
    g = rng.standard_normal((1, n, 1)).astype(F32)
    want = np.stack([F32(0.114) * g, F32(0.587) * g, F32(0.299) * g, np.zeros_like(g)], axis=-1)
    w.exact('gray_bwd', impl.gray_bwd(g), want, n)


# =================================================================================================================================
# the two implementations
# =================================================================================================================================
class NumpyImpl:
    """fp32 NumPy restatement of each kernel's order of operations (unfused: every product and sum rounds on its own)"""

    def gap_fwd(self, x, is16):
        B, HW, C_ = x.shape
        red = []
        for part in range(GAP_PHASES):
            s = [np.zeros((B, C_), F32) for _ in range(4)]
            p = part
            while p + 12 < HW:
                for j in range(4):
                    s[j] = s[j] + x[:, p + 4 * j]
                p += 16
            while p < HW:
                s[0] = s[0] + x[:, p]
                p += 4
            red.append((s[0] + s[1]) + (s[2] + s[3]))
        return ((red[0] + red[1]) + (red[2] + red[3])) * (F32(1) / F32(HW))

    def gap_bwd(self, gy, HW, is16):
        gx = np.broadcast_to((gy * (F32(1) / F32(HW)))[:, None, :], (gy.shape[0], HW, gy.shape[1])).copy()
        return bf16(gx) if is16 else gx

    @staticmethod
    def _gz(y, gy, act_out):
        return (gy * y) * (F32(1) - y) if act_out else gy

    def linear_fwd(self, x, W, b, act_in, act_out, is16):
        B, K = x.shape
        N = W.shape[0]
        xa = np.maximum(x, F32(0)) if act_in else x
        T = -(-K // LIN_TRIP)
        xp = np.zeros((B, T * LIN_TRIP), F32)
        xp[:, :K] = xa
        xp = xp.reshape(B, T, BLOCK, 4)
        y = np.zeros((B, N), F32)
        for n in range(N):
            wp = np.zeros(T * LIN_TRIP, F32)
            wp[:K] = W[n]
            wp = wp.reshape(T, BLOCK, 4)
            acc = np.zeros((B, BLOCK), F32)
            for t in range(T):
                q = xp[:, t] * wp[t]
                acc = acc + (((q[..., 0] + q[..., 1]) + q[..., 2]) + q[..., 3])
            v = wave_fold32(acc) + (b[n] if b is not None else F32(0))
            y[:, n] = np.tanh(v * F32(0.5)) * F32(0.5) + F32(0.5) if act_out else v
        return y

    def linear_bwd(self, x, W, y, gy, gW0, gb0, need_gx, act_in, act_out, is16):
        B, K = x.shape
        N = W.shape[0]
        gz = self._gz(y, gy, act_out)
        gx = gW = gb = None
        if need_gx:
            gx = np.zeros((B, K), F32)
            for n in range(N):
                gx = gx + W[n][None, :] * gz[:, n:n + 1]
            if act_in:
                gx = np.where(x > 0, gx, F32(0))
            if is16:
                gx = bf16(gx)
        if gW0 is not None:
            xa = np.maximum(x, F32(0)) if act_in else x
            gW = gW0.copy()
            for s0 in range(0, B, LIN_SLAB):
                acc = np.zeros((N, K), F32)
                for s in range(s0, min(s0 + LIN_SLAB, B)):
                    acc = acc + gz[s][:, None] * xa[s][None, :]
                gW = gW + acc
        if gb0 is not None:
            gb = gb0 + block_reduce32(gz.T)
        return gx, gW, gb

    @staticmethod
    def _lin(n):
        return np.linspace(-1, 1, n, dtype=F32)

    def st_grid_fwd(self, theta, th, tw):
        xs, ys = np.meshgrid(self._lin(tw), self._lin(th))
        t = theta[:, :, :, None, None]
        return (t[:, :, 0] * xs + t[:, :, 1] * ys) + t[:, :, 2]

    def st_grid_bwd(self, gg):
        B, _, th, tw = gg.shape
        xs, ys = np.meshgrid(self._lin(tw), self._lin(th))
        g = gg.reshape(B, 2, 1, -1)
        coords = np.stack([xs.ravel(), ys.ravel(), np.ones(th * tw, F32)])[None, None]
        return block_reduce32(g * coords)

    def st_sampler_fwd(self, img, grid):
        return C.st_sampler_fwd(img, grid)

    def st_sampler_bwd(self, img, grid, gy, d0):
        g = C.st_sampler_bwd_grid(img, grid, gy)
        assert g.dtype == F32
        return g if d0 is None else d0 + g

    def mse_fwd(self, y, t, tconst):
        d = y - (t if t is not None else F32(tconst))
        return block_reduce32(d * d) / F32(y.size)

    def mse_bwd(self, y, t, tconst, gloss):
        return (F32(gloss) * F32(2) / F32(y.size)) * (y - (t if t is not None else F32(tconst)))

    @staticmethod
    def _corners(g):
        th, tw = g.shape[2:]
        return g[:, 0, 0, 0], g[:, 1, 0, 0], g[:, 0, 0, tw - 1], g[:, 1, th - 1, 0]

    def grid_loss_fwd(self, g, kind, H, W, oob):
        tlx, tly, trx, bly = self._corners(g)
        B = F32(g.shape[0])
        if kind == 0:
            sc = lambda v, size: (v + F32(1)) / F32(2) * F32(size)      # noqa: E731
            terms = np.maximum(sc(tly, H) - sc(bly, H), F32(0)) + np.maximum(sc(tlx, W) - sc(trx, W), F32(0))
            return block_reduce32(terms) / B
        terms = np.zeros(g.shape[0], F32)
        for v in (tlx, tly, trx, bly):
            terms = terms + (np.abs(np.minimum(v + F32(1), F32(0))) + np.maximum(v - F32(1), F32(0)))
        return block_reduce32(terms) * F32(oob)

    def grid_loss_bwd(self, g, gloss, kind, H, W, oob):
        tlx, tly, trx, bly = self._corners(g)
        th, tw = g.shape[2:]
        B = F32(g.shape[0])
        gg = np.zeros_like(g)
        gl = F32(gloss)
        if kind == 0:
            sc = lambda v, size: (v + F32(1)) / F32(2) * F32(size)      # noqa: E731
            m1 = np.where(sc(tly, H) - sc(bly, H) >= 0, gl / B * (F32(H) / F32(2)), F32(0)).astype(F32)
            m2 = np.where(sc(tlx, W) - sc(trx, W) >= 0, gl / B * (F32(W) / F32(2)), F32(0)).astype(F32)
            gg[:, 1, 0, 0] += m1
            gg[:, 1, th - 1, 0] -= m1
            gg[:, 0, 0, 0] += m2
            gg[:, 0, 0, tw - 1] -= m2
            return gg
        s = gl * F32(oob)
        d = lambda v: (np.where(v + F32(1) < 0, -s, F32(0)) + np.where(v - F32(1) >= 0, s, F32(0))).astype(F32)   # noqa: E731
        gg[:, 0, 0, 0] += d(tlx)
        gg[:, 1, 0, 0] += d(tly)
        gg[:, 0, 0, tw - 1] += d(trx)
        gg[:, 1, th - 1, 0] += d(bly)
        return gg

    def adam(self, p, g, m, v, vh, lr, beta1, beta2, eps, eta, wd, gs, dev_lr):
        lr_t, a, b = F32(lr), F32(1.0 - beta1), F32(1.0 - beta2)
        g0 = g.copy()
        g = g * F32(gs)
        m = m + a * (g - m)
        v = v + b * (g * g - v)
        vh2 = np.maximum(vh, v) if vh is not None else None
        den = np.sqrt(vh2 if vh is not None else v) + F32(eps)
        p = p - F32(eta) * (lr_t * m / den + F32(wd) * p)
        return p, m, v, vh2, g0

    def mul(self, x, y):
        return x * y

    def scale_by_scalar(self, x, s):
        return x * s

    def axpby(self, a, x, b, y):
        return (a * x if b == 0 else a * x + b * y), x.copy()

    def nchw3_to_nhwc4(self, x):
        B, _, H, W = x.shape
        out = np.zeros((B, H, W, 4), F32)
        out[..., :3] = x.transpose(0, 2, 3, 1)
        return out

    def channel_mean(self, x, scale, shift, cdiv, is16):
        rows, C_ = x.shape
        v = np.maximum(x * scale + shift, F32(0)) if scale is not None else x
        T = -(-C_ // 256)
        pad = np.zeros((rows, T * 256), F32)
        pad[:, :C_] = v
        pad = pad.reshape(rows, T, 64, 4)
        acc = np.zeros((rows, 64), F32)
        for t in range(T):
            q = pad[:, t]
            acc = acc + ((q[..., 0] + q[..., 1]) + (q[..., 2] + q[..., 3]))
        lane = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            acc = acc + acc[:, lane ^ o]
        return acc[:, 0] * (F32(1) / F32(cdiv))

    def vbp_scale(self, feat, avg, s, p):
        B, fh, fw = feat.shape
        _, H, W = avg.shape
        kh, kw = H + 2 * p - s * (fh - 1), W + 2 * p - s * (fw - 1)
        out = np.zeros((B, H, W), F32)
        for fy in range(fh):                                            # rows first, then columns: the kernel's order per pixel
            for fx in range(fw):
                y0, x0 = s * fy - p, s * fx - p
                ys, xs = slice(max(y0, 0), min(y0 + kh, H)), slice(max(x0, 0), min(x0 + kw, W))
                out[:, ys, xs] = out[:, ys, xs] + feat[:, fy:fy + 1, fx:fx + 1]
        return out * avg

    def minmax(self, x):
        lo, hi = x.min(axis=1, keepdims=True), x.max(axis=1, keepdims=True)
        with np.errstate(divide='ignore', invalid='ignore'):
            return (x - lo) * (F32(1) / (hi - lo))

    def gray_fwd(self, rois):
        return (F32(0.299) * rois[..., 2] + F32(0.587) * rois[..., 1]) + F32(0.114) * rois[..., 0]

    def gray_bwd(self, g):
        return np.stack([F32(0.114) * g, F32(0.587) * g, F32(0.299) * g, np.zeros_like(g)], axis=-1)


class HipImpl:
    """the kernels through loans_amd.ops; through _lib.load() where ops hides an argument (the sampler's `accumulate`)"""

    def __init__(self):
        import torch
        from loans_amd import _lib, ops
        self.torch, self.ops, self.lib = torch, ops, _lib.load()

    def dev(self, a, is16=False):
        if a is None:
            return None
        t = self.torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).cuda()
        return t.to(self.torch.bfloat16) if is16 else t              # exact: the values are bf16 already

    @staticmethod
    def host(t):
        return None if t is None else t.float().cpu().numpy()

    def gap_fwd(self, x, is16):
        B, HW, C_ = x.shape
        return self.host(self.ops.gap_fwd(self.dev(x, is16).view(B, HW, 1, C_)))

    def gap_bwd(self, gy, HW, is16):
        B, C_ = gy.shape
        gx = self.ops.gap_bwd(self.dev(gy), (B, HW, 1, C_), self.torch.bfloat16 if is16 else self.torch.float32)
        return self.host(gx).reshape(B, HW, C_)

    def linear_fwd(self, x, W, b, act_in, act_out, is16):
        return self.host(self.ops.linear_fwd(self.dev(x, is16), self.dev(W), self.dev(b), act_in, act_out))

    def linear_bwd(self, x, W, y, gy, gW0, gb0, need_gx, act_in, act_out, is16):
        xd, Wd, yd, gyd = self.dev(x, is16), self.dev(W), self.dev(y), self.dev(gy)
        keep = [t.clone() for t in (xd, Wd, gyd)] + ([yd.clone()] if yd is not None else [])
        gW, gb = self.dev(gW0), self.dev(gb0)
        gx = self.ops.linear_bwd(xd, Wd, yd, gyd, gW=gW, gb=gb, need_gx=need_gx, act_in=act_in, act_out=act_out)
        for a, b in zip(keep, (xd, Wd, gyd, yd)):
            assert self.torch.equal(a, b)                            # the inputs are read only
        return self.host(gx), self.host(gW), self.host(gb)

    def st_grid_fwd(self, theta, th, tw):
        return self.host(self.ops.st_grid_fwd(self.dev(theta), (th, tw)))

    def st_grid_bwd(self, gg):
        return self.host(self.ops.st_grid_bwd(self.dev(gg)))

    def st_sampler_fwd(self, img, grid):
        return self.host(self.ops.st_sampler_fwd(self.dev(img), self.dev(grid)))[..., :3].transpose(0, 3, 1, 2)

    def st_sampler_bwd(self, img, grid, gy, d0):
        B, _, H, W = img.shape
        th, tw = grid.shape[2:]
        g4 = np.zeros((B, th, tw, 4), F32)
        g4[..., :3] = gy.transpose(0, 2, 3, 1)
        imgd, gridd, gd = self.dev(img), self.dev(grid), self.dev(g4)
        if d0 is None:
            out = self.ops.st_sampler_bwd_grid(imgd, gridd, gd)
        else:
            from loans_amd._lib import check
            out = self.dev(d0)
            check(self.lib.loans_st_sampler_bwd_grid_f32(imgd.data_ptr(), gridd.data_ptr(), gd.data_ptr(), out.data_ptr(), 1,
                                                         B, H, W, th, tw, self.ops._stream()), 'loans_st_sampler_bwd_grid_f32')
        assert self.torch.equal(gridd, self.dev(grid)) and self.torch.equal(gd, self.dev(g4))
        return self.host(out)

    def mse_fwd(self, y, t, tconst):
        return self.host(self.ops.mse_fwd(self.dev(y), self.dev(t), tconst))

    def mse_bwd(self, y, t, tconst, gloss):
        return self.host(self.ops.mse_bwd(self.dev(y), self.dev(np.asarray(gloss, F32).reshape(())), self.dev(t), tconst))

    def grid_loss_fwd(self, g, kind, H, W, oob):
        return self.host(self.ops.grid_loss_fwd(self.dev(g), kind, float(H), float(W), float(oob)))

    def grid_loss_bwd(self, g, gloss, kind, H, W, oob):
        gd = self.dev(g)
        out = self.ops.grid_loss_bwd(gd, self.dev(np.asarray(gloss, F32).reshape(())), kind, float(H), float(W), float(oob))
        assert self.torch.equal(gd, self.dev(g))
        return self.host(out)

    def adam(self, p, g, m, v, vh, lr, beta1, beta2, eps, eta, wd, gs, dev_lr):
        pd, gd, md, vd, vhd = (self.dev(a) for a in (p, g, m, v, vh))
        rate = self.torch.full((1,), lr, device='cuda', dtype=self.torch.float32) if dev_lr else lr
        self.ops.adam_amsgrad(pd, gd, md, vd, vhd, rate, beta1, beta2, eps, eta, wd, gs)
        return tuple(self.host(t) for t in (pd, md, vd, vhd, gd))

    def mul(self, x, y):
        return self.host(self.ops.mul(self.dev(x), self.dev(y)))

    def scale_by_scalar(self, x, s):
        return self.host(self.ops.scale_by_scalar(self.dev(x), self.dev(np.asarray([s], F32))))

    def axpby(self, a, x, b, y):
        xd, yd = self.dev(x), self.dev(y)
        self.ops.axpby(float(a), xd, float(b), yd)
        return self.host(yd), self.host(xd)

    def nchw3_to_nhwc4(self, x):
        return self.host(self.ops.nchw3_to_nhwc4(self.dev(x)))

    def channel_mean(self, x, scale, shift, cdiv, is16):
        st = types.SimpleNamespace(scale=self.dev(scale), shift=self.dev(shift)) if scale is not None else None
        return self.host(self.ops.channel_mean(self.dev(x, is16), cdiv, st))

    def vbp_scale(self, feat, avg, s, p):
        return self.host(self.ops.vbp_scale(self.dev(feat), self.dev(avg), None, s, p))

    def minmax(self, x):
        return self.host(self.ops.minmax_normalize_(self.dev(x)))

    def gray_fwd(self, rois):
        return self.host(self.ops.gray_fwd(self.dev(rois)))

    def gray_bwd(self, g):
        return self.host(self.ops.gray_bwd(self.dev(g)))


# =================================================================================================================================
# the families as the two test files run them
# =================================================================================================================================
def run_gap(impl, w, HW):
    for C_ in GAP_C:
        for B in GAP_B:
            for is16 in (False, True):
                check_gap_fwd(impl, w, B, HW, C_, is16)
                check_gap_bwd(impl, w, B, HW, C_, is16)


def run_gap_big(impl, w):
    for is16 in (False, True):
        check_gap_bwd(impl, w, *GAP_BWD_BIG, is16)


def run_st_grid(impl, w, size):
    for B in ST_B:
        for kind in ('identity', 'random', 'large'):
            check_st_grid(impl, w, B, size[0], size[1], kind)


def run_st_grid_big(impl, w):
    for kind in ('identity', 'random'):
        check_st_grid(impl, w, *ST_BIG, kind)


def run_sampler(impl, w, frame):
    H, W = frame
    for B in (1, 3):
        for name, grid in sampler_grids(B, H, W):
            check_sampler(impl, w, B, H, W, name, grid)


def run_sampler_big(impl, w):
    B, H, W, th, tw = SAMPLER_BIG
    grid = C.st_grid_fwd(make_theta(B, 'random', 5300), (th, tw))[0].astype(F32)
    check_sampler(impl, w, B, H, W, 'big', grid)


def run_mse(impl, w):
    for n in MSE_N:
        for with_target in (True, False):
            check_mse(impl, w, n, with_target)


def run_regularisers(impl, w, B):
    for th, tw in REG_SIZES:
        for i, image in enumerate(REG_IMAGES):
            check_regularisers(impl, w, B, th, tw, image, (1.0, 4.0)[(i + th) % 2])
    check_regularisers(impl, w, B, 5, 6, (48, 64), 4.0)
    check_regularisers(impl, w, B, 5, 6, (48, 64), 1.0)


def run_glue(impl, w):
    for n in GLUE_N:
        check_glue(impl, w, n)
    for shape in NHWC4_SHAPES:
        check_nhwc4(impl, w, shape)


def run_insight(impl, w):
    for rows in CM_ROWS:
        for C_ in CM_C:
            for is16 in (False, True):
                for affine in (False, True):
                    check_channel_mean(impl, w, rows, C_, is16, affine)
    check_channel_mean(impl, w, 5, 64, False, False, cdiv=3)            # the stem's NHWC4 frames: C = 4 storage, 3 channels
    check_channel_mean(impl, w, 5, 4, False, False, cdiv=3)
    for k, s, p in VBP_KSP:
        for H, W in ((15, 17), (16, 14)):                               # odd and even map sizes
            check_vbp_scale(impl, w, k, s, p, H, W)
    for n in MINMAX_N:
        for B in (1, 3):
            check_minmax(impl, w, B, n)
    for n in (1, 255, 1000):
        check_gray(impl, w, n)
