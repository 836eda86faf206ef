"""Case grid, fp64 reference, derived bounds and an fp32 NumPy restatement for the BN / pool kernels of csrc/bn_pool.hip
(not collected by pytest).

The same `check_*` functions run twice: on `NumpyImpl` (tests/test_host_cpu.py: the restatement must sit inside the bounds on
every generated case, before any GPU run) and on `HipImpl` (the -m gpu tests at the end of tests/test_gpu_kernels.py and
tests/test_gpu_bf16_storage.py).  The reference is oracle/chainer_ops.py in float64 on the same inputs; for bf16 cases the
inputs are rounded to bf16 FIRST and the oracle sees the rounded values.  Every bound is elementwise and comes from the number
formats and the order of operations -- none was read off a kernel's output.  Tensors are NHWC, flattened to (rows, C)."""
import json

import numpy as np

from oracle import chainer_ops as C

U = 2.0 ** -24          # unit round-off of fp32 (round to nearest)
U16 = 2.0 ** -8         # one round-to-nearest-even of a bf16 result (8 significant bits)
K_BWD = 7               # k1 g + k2 x + k3 with fp32 coefficients: see backward_bounds()
# fp32 partial sums of the reductions: a thread adds at most 32 rows (bn_bwd_reduce_impl: rpt <= 32; reduce_geometry: 8 rows
# per thread until rows > 8192 RL, and the grid below never gets there), then one thread folds the RL <= 256 partial sums of
# its block through LDS; everything after that is fp64.  A chain of L fp32 additions is off by at most (L - 1) u sum |terms|.
ACC_CHAIN = 32 + 256
MAX_AMBIGUOUS_SHARE = 1e-4

# ---- the grid ------------------------------------------------------------------------------------------------------------------
# (B, H, W): one row; fewer units than one 256-thread block for every C <= 512 (rows * U <= 8 * 16 .. 128); the shape of the
# older tests; an odd mid size (5115 rows: its unit count is no multiple of 32 or 1024 for any U); and BIG.
#
# The slab kernels (bn_apply_u16_kernel, bn_bwd_apply_u16_kernel) launch slab_grid(n) = min(ceil(n / 1024), 8192) blocks and
# give each per = roundup256(ceil(n / grid)) units (slab_of).  Below 8192 * 1024 units per <= 1024 = SLAB_UNR * 256, so a thread
# runs the unrolled body AT MOST ONCE; 8 388 608 units are 128 MiB, beyond the 96 MB non-temporal switch that
# tests/test_gpu_nontemporal.py owns.  What can be reached below it, and is: full blocks that run the unrolled body once
# (ODD, BIG), a last block where threads tid < end - lo - 768 run the unrolled body and the rest only the tail (ODD at C = 64:
# 81 840 fp32 units = 79 * 1024 + 944, 40 920 bf16 units = 39 * 1024 + 984), slabs of 256 / 512 / 768 units that are tail only
# (the small shapes), and a last block with a two-step tail (BIG at C = 64, fp32: 1 058 400 = 1033 * 1024 + 608).
# The reductions do iterate: bn_bwd_reduce_u16_kernel at BIG, C = 64, fp32 has U = UB = 16, RL = 16, rpt = 8 (ceil(66150 / 128) =
# 517 >= 512 blocks), 128 rows per block = 8 per thread = two UF = 4 bodies (four UF = 2 bodies in the dual form), and 102 rows in
# the last block = one body plus a tail of 2 or 3.  The fall-back kernels' grid-stride loops (grid_for: at most 2048 blocks of 256)
# run twice or more from 524 288 four-channel groups: BIG at C = 96 has 1 587 600.
# BIG at C = 96 is 25.4 MB per fp32 tensor, 1 058 400 units at C = 64: "a few hundred thousand units", far below 96 MB.
S_ONE, S_FEW, S_OLD, S_ODD, S_BIG = (1, 1, 1), (2, 2, 2), (3, 9, 7), (5, 33, 31), (3, 150, 147)
SHAPES = (S_ONE, S_FEW, S_OLD, S_ODD, S_BIG)

# C -> (16-byte-unit kernels in fp32, in bf16): asserted against ops.bn_units_ok by the tests, so that a change of the dispatch
# cannot silently empty a cell.  C = 4 is the only count with unit kernels in fp32 and the fall-back in bf16.
PATHS = {4: (True, False), 64: (True, True), 96: (False, False), 512: (True, True), 1024: (True, True), 2048: (False, True)}
# C -> the fused pool-backward pair tiles it (ops.reduce_channels_ok(C) and C <= 1024); otherwise the three-pass form
POOL_FUSED = {4: True, 64: True, 96: False, 1024: True, 2048: False}


def bn_grid():
    """(shape, C): every path {unit, fall-back} x {fp32, bf16} meets the small, the odd and the big shape"""
    grid = [(s, c) for s in (S_ONE, S_FEW, S_OLD) for c in (4, 64, 96, 512, 1024, 2048)]
    grid += [(S_ODD, c) for c in (4, 64, 96, 512, 2048)]
    grid += [(S_BIG, c) for c in (4, 64, 96)]
    return grid


# H, W in {3 (the launchers' minimum), even, odd}: cover_all's overhanging last window occurs on either axis (even sizes)
POOL_SHAPES = ((2, 3, 3), (1, 3, 8), (2, 8, 7), (3, 13, 11), (2, 16, 16), (2, 33, 31))


def pool_grid():
    grid = [(s, c) for s in POOL_SHAPES for c in (4, 64, 96)]
    grid += [(s, c) for s in ((2, 3, 3), (2, 8, 7), (3, 13, 11)) for c in (1024, 2048)]
    return grid


def case_id(case):
    (b, h, w), c = case
    return '%dx%dx%d-C%d' % (b, h, w, c)


# ---- data ----------------------------------------------------------------------------------------------------------------------
N_PROFILES = 7


def make_bn(rows, C_, seed, bf16, rot=0):
    """x (rows, C), gamma, beta, running mean / variance (all fp32).  Channel c has profile (c + rot) % 7, so every 16-byte unit
    mixes them: 0 plain N(0.5, 2); 1 std 1e-3; 2 std 1e3; 3 mean = +-30 std; 4 gamma = 1e-3; 5 gamma < 0; 6 plain, except the
    FIRST such channel, which is constant (variance 0, rstd = 1 / sqrt(eps))."""
    rng = np.random.RandomState(seed)
    p = (np.arange(C_) + rot) % N_PROFILES
    mean = np.full(C_, 0.5)
    std = np.full(C_, 2.0)
    mean[p == 1], std[p == 1] = 0.0, 1e-3
    std[p == 2] = 1e3
    mean[p == 3] = np.where((np.arange(C_) // N_PROFILES) % 2 == 0, 60.0, -60.0)[p == 3]
    x = (rng.standard_normal((rows, C_)) * std + mean).astype(np.float32)
    const = np.flatnonzero(p == 6)[:1]
    x[:, const] = 0.75
    gamma = (1 + 0.1 * rng.standard_normal(C_)).astype(np.float32)
    gamma[p == 4] = 1e-3
    gamma[p == 5] = -np.abs(gamma[p == 5])
    beta = (0.1 * rng.standard_normal(C_)).astype(np.float32)
    rm = rng.standard_normal(C_).astype(np.float32)
    rv = (0.5 + rng.random_sample(C_)).astype(np.float32)
    if bf16:
        x = C.round_bf16(x)
    certain = np.ones(C_, bool)         # channels whose ReLU sign the reference decides (not the constant one, not rows = 1)
    certain[const] = False
    if rows == 1:
        certain[:] = False
    return dict(x=x, gamma=gamma, beta=beta, rm=rm, rv=rv, certain=certain, rows=rows, C=C_)


def make_grad(shape, seed, bf16, zeros=False):
    """N(0, 1); zeros: a mask tensor with exact +0.0 and -0.0 entries (`mask > 0` semantics)"""
    rng = np.random.RandomState(seed)
    g = rng.standard_normal(shape).astype(np.float32)
    if zeros:
        r = rng.random_sample(shape)
        g[r < 0.1] = 0.0
        g[r > 0.9] = -0.0
    return C.round_bf16(g) if bf16 else g


def replica_stats(x, replicas=32):
    """fp64 [replicas][sum | sum of squares][C], the rows dealt over ALL replicas (as the conv epilogues leave them)"""
    x64 = x.astype(np.float64)
    st = np.zeros((replicas, 2, x.shape[1]))
    for r in range(replicas):
        st[r, 0] = x64[r::replicas].sum(axis=0)
        st[r, 1] = (x64[r::replicas] ** 2).sum(axis=0)
    return st


# ---- reference -----------------------------------------------------------------------------------------------------------------
class BNRef:
    """oracle.chainer_ops.bn_fwd_train in float64 on (rows, C, 1, 1), and the coefficients recomputed from its statistics"""

    def __init__(self, d):
        self.d = d
        x = d['x'].astype(np.float64)
        self.x = x
        self.gamma, self.beta = d['gamma'].astype(np.float64), d['beta'].astype(np.float64)
        self.rm, self.rv = d['rm'].astype(np.float64), d['rv'].astype(np.float64)
        y, (xhat, rstd) = C.bn_fwd_train(x[:, :, None, None], self.gamma, self.beta, self.rm, self.rv)
        self.pre, self.xhat, self.rstd = y[:, :, 0, 0], xhat[:, :, 0, 0], rstd
        self.ctx = (xhat, rstd)
        self.mean = x.mean(axis=0)
        self.scale = self.gamma * rstd
        self.shift = self.beta - self.mean * self.scale
        self.bound, self.mag = apply_bound(x, self.mean, self.scale, self.shift)

    def backward(self, g):
        gx, gg, gb = C.bn_bwd(self.ctx, self.gamma, g[:, :, None, None])
        return gx[:, :, 0, 0], gg, gb


def apply_bound(x, mean, scale, shift):
    """|fl(fl(x sc) + sh) - (x scale + shift)| with the fp32 coefficients of bn_finalize: sc is off by 2.5 u and the product adds
    u; sh = fl(beta - fl(fl(mean) sc)) is off by u |shift| + 4.5 u |mean scale| (check_finalize); the last addition adds
    u |y| <= u (|x scale| + |shift|):  u (4.5 |x scale| + 2 |shift| + 4.5 |mean scale|).
    (The shorter form 4 u (|x scale| + |shift|) has no |mean scale| term: where beta ~ mean scale the shift cancels, its
    rounding error does not, and the fp32 restatement leaves that form by a factor of 100 -- DESIGN 3, item 11.)
    Also returns |x scale| + |shift|, which bounds |y| for the rounding of a further addition (residual, second BN)."""
    mag = np.abs(x * scale) + np.abs(shift)
    return (1 + 1e-3) * U * (4.5 * np.abs(x * scale) + 2 * np.abs(shift) + 4.5 * np.abs(mean * scale)), mag


def _bf16_round(ref, bound, bf16):
    """a bf16 output is the kernel's fp32 value v rounded once to nearest even: at most 2^-8 |v| (8 significant bits) and
    |v| <= |ref| + bound.  2^-8 |ref| is the rounding of a result that is exact before it; 2^-8 times the fp32 bound covers the elements with |ref| <
    bound (a ReLU or mask sign that is allowed to fall either way, a cancelling channel)."""
    return U16 * (np.abs(ref) + bound) if bf16 else 0.0


def _ratio(err, bound):
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    if err.size == 0:
        return 0.0
    return float(np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300)).max())


def _within(name, got, ref, bound, ratios):
    r = _ratio(np.abs(np.asarray(got, np.float64) - ref), bound)
    ratios[name] = max(ratios.get(name, 0.0), r)
    assert r <= 1.0, '%s: error / derived bound = %.3g' % (name, r)


def _share(name, amb, certain, ratios):
    """the excluded share is a condition: at most 1e-4 of the elements of a case (rows = 1 and the constant channel are
    compared through the elementwise bound only)"""
    if not certain.any():
        return
    s = float(amb[:, certain].mean()) if amb.ndim == 2 else float(amb[..., certain].mean())
    ratios['share:' + name] = max(ratios.get('share:' + name, 0.0), s)
    assert s <= MAX_AMBIGUOUS_SHARE, '%s: %.3g of the elements have an undecidable sign' % (name, s)


# ---- bn_finalize ---------------------------------------------------------------------------------------------------------------
def check_finalize(impl, d, ratios):
    """mean: one cast (u).  rstd: one cast + eps handed over as a float (u / 2): 1.5 u.  scale = fl(gamma rstd): 2.5 u.
    shift = fl(beta - fl(fl(mean) scale)): u |shift| + (1 + 2.5 + 1) u |mean scale|.  Running statistics
    fl(fl(0.9f r) + fl(fl(1 - 0.9f) v)): 0.9f is 0.9 (1 + 0.45 u) and 1 - 0.9f is 0.1 (1 + 4 u), v carries one cast, each product
    and the sum one rounding: 1.5 u |0.9 r| + 6 u |0.1 v| + u |result|.  All times 1 + 1e-3 for the second-order terms."""
    ref = BNRef(d)
    st, rm, rv = impl.finalize(replica_stats(d['x']), d['rows'], d['gamma'], d['beta'], d['rm'], d['rv'])
    s = (1 + 1e-3) * U
    _within('finalize.mean', st['mean'], ref.mean, s * np.abs(ref.mean), ratios)
    _within('finalize.rstd', st['rstd'], ref.rstd, 1.5 * s * ref.rstd, ratios)
    _within('finalize.scale', st['scale'], ref.scale, 2.5 * s * np.abs(ref.scale), ratios)
    _within('finalize.shift', st['shift'], ref.shift, s * (np.abs(ref.shift) + 4.5 * np.abs(ref.mean * ref.scale)), ratios)
    m = d['rows']
    var_term = (m / max(m - 1.0, 1.0)) * (ref.x.var(axis=0) + C.BN_EPS)
    for name, got, new, old, v in (('finalize.running_mean', rm, ref.rm, d['rm'], ref.mean),
                                   ('finalize.running_var', rv, ref.rv, d['rv'], var_term)):
        bound = s * (1.5 * np.abs(0.9 * old.astype(np.float64)) + 6 * np.abs(0.1 * v) + np.abs(new))
        _within(name, got, new, bound, ratios)
    return st


# ---- bn_apply ------------------------------------------------------------------------------------------------------------------
def _bits_of(y):
    """one byte per four channels, bit e = (y[4 i + e] > 0)"""
    return ((y.reshape(-1, 4) > 0) * np.array([1, 2, 4, 8])).sum(axis=1).astype(np.uint8)


def check_apply(impl, d, d2, res, ratios):
    """modes 0 / 1 / 2 x relu x want_bits; the second BN has its own x2, statistics and gamma / beta.  Returns what the
    backward checks need: the two states and the handle of relu(bn(x) + res) with its sign bits."""
    bf16 = impl.bf16
    ref, ref2 = BNRef(d), BNRef(d2)
    st = impl.finalize(replica_stats(d['x']), d['rows'], d['gamma'], d['beta'], d['rm'], d['rv'])[0]
    st2 = impl.finalize(replica_stats(d2['x']), d2['rows'], d2['gamma'], d2['beta'], d2['rm'], d2['rv'])[0]
    res64 = res.astype(np.float64)
    # one more fp32 addition for the residual / the second BN: u times the magnitudes it adds
    forms = ((0, ref.pre, ref.bound, {}, d['certain']),
             (1, ref.pre + res64, ref.bound + U * (ref.mag + np.abs(res64)), dict(residual=res), d['certain']),
             (2, ref.pre + ref2.pre, ref.bound + ref2.bound + U * (ref.mag + ref2.mag), dict(x2=d2['x'], st2=st2),
              d['certain'] & d2['certain']))
    keep = None
    for mode, pre, bound, kw, certain in forms:
        amb = np.abs(pre) <= bound
        _share('apply%d' % mode, amb, certain, ratios)
        for relu in (False, True):
            y_ref = np.maximum(pre, 0) if relu else pre         # ReLU is 1-Lipschitz: the bound of `pre` holds for it
            b = bound + _bf16_round(y_ref, bound, bf16)
            out = impl.apply(d['x'], st, relu=relu, **kw)
            _within('apply%d' % mode, out['y'], y_ref, b, ratios)
            assert out['bits'] is None
            if not relu:
                continue
            outb = impl.apply(d['x'], st, relu=True, want_bits=True, **kw)
            assert np.array_equal(outb['y'], out['y']), 'mode %d: want_bits changes y' % mode
            assert outb['bits'].dtype == np.uint8 and outb['bits'].size == d['x'].size // 4
            assert np.array_equal(outb['bits'], _bits_of(outb['y'])), 'mode %d: sign bits != (own y > 0)' % mode
            sure = ~amb & certain[None, :]
            assert np.array_equal((outb['y'] > 0)[sure], (pre > 0)[sure]), 'mode %d: sign differs from the reference' % mode
            if mode == 1:
                keep = dict(handle=outb, pre=pre, amb=amb | ~certain[None, :])
    own = dict(handle=impl.apply(d['x'], st, relu=True), pre=ref.pre, amb=(np.abs(ref.pre) <= ref.bound) | ~d['certain'][None, :])
    return dict(ref=ref, ref2=ref2, st=st, st2=st2, bits=keep, own=own)


# ---- bn_backward ---------------------------------------------------------------------------------------------------------------
def backward_bounds(ref, gamma, g_ref, g_abs, amb, m, g_round=0.0):
    """(gx, ggamma, gbeta) of the reference with their bounds for gx = k1 g + k2 x + k3.
    g_abs >= |g| elementwise over the elements that MAY pass the mask (reference mask or undecidable sign, `amb`).
    Sums, per channel: the kernel adds fl(g fl(fl(x - fl(mean)) fl(rstd))) in fp32 chains of at most ACC_CHAIN terms, then fp64:
      E_db = ACC u sum |g| + sum_amb |g|                                     (an undecidable sign may drop or add its term)
      E_dg = (ACC + 5) u sum |g xhat| + u |mean| rstd sum |g| + sum_amb |g xhat|
    (xhat: subtraction u, rstd 1.5 u, product u, times g u = 4.5 u; the cast of the mean moves every xhat by u |mean| rstd).
    gx: K_BWD u (|k1 g| + |k2 x| + |k1| (|mean rstd dg| + |db|) / m) for the evaluation with fp32 coefficients, k3's two
    terms taken apart because they cancel where |mean| >> std (k1 = gamma rstd: 2.5 u with its cast, k2 = -k1 rstd dg / m: 4 u,
    k3's terms 5 u and 2.5 u with the cast; one product and two additions on top: 5.5, 7, 6 and 3.5 u -- 7 u for all); plus what the sums' errors do to k2 x + k3 =
    -(k1 / m) (xhat dg + db): (|k1| / m) (|xhat| E_dg + E_db); plus |k1 g| where the sign of the element itself is undecidable.
    g_round: a named relative rounding of g itself (the three-pass pool form stores the dense gradient as bf16)."""
    gx, dg, db = ref.backward(g_ref)
    xhat_abs = np.abs(ref.xhat)
    s_g, s_gx = g_abs.sum(axis=0), (g_abs * xhat_abs).sum(axis=0)
    a_g, a_gx = (g_abs * amb).sum(axis=0), (g_abs * xhat_abs * amb).sum(axis=0)
    e_db = (ACC_CHAIN * U + g_round) * s_g + a_g
    e_dg = ((ACC_CHAIN + 5) * U + g_round) * s_gx + U * np.abs(ref.mean) * ref.rstd * s_g + a_gx
    k1 = gamma.astype(np.float64) * ref.rstd
    k2 = -k1 * ref.rstd * dg / m
    k3_abs = np.abs(k1) * (np.abs(ref.mean * ref.rstd * dg) + np.abs(db)) / m
    b_gx = K_BWD * U * (np.abs(k1 * g_ref) + np.abs(k2 * ref.x) + k3_abs) + np.abs(k1) / m * (xhat_abs * e_dg + e_db)
    b_gx = b_gx + np.abs(k1) * g_abs * (amb + g_round)
    return gx, dg, db, b_gx, e_dg, e_db


def _check_param_grads(name, got_gg, got_gb, before_gg, before_gb, dg, db, e_dg, e_db, ratios):
    """ggamma / gbeta are ACCUMULATED: before + gradient, the fp64 sum cast once (u |sum|) and added once in fp32 (u |result|)"""
    for nm, got, before, v, e in ((name + '.ggamma', got_gg, before_gg, dg, e_dg), (name + '.gbeta', got_gb, before_gb, db, e_db)):
        want = before.astype(np.float64) + v
        _within(nm, got, want, e + (1 + 1e-3) * U * (np.abs(v) + np.abs(want)), ratios)


def prefill(C_, rows, seed):
    """non-zero accumulators of the gradients' own size (~ sqrt(rows)), so that `=` for `+=` cannot hide"""
    rng = np.random.RandomState(seed)
    return [((1 + np.abs(rng.standard_normal(C_))) * np.sqrt(rows) * np.where(rng.random_sample(C_) < 0.5, -1, 1)).astype(np.float32)
            for _ in range(4)]


MASK_KINDS = ('none', 'tensor', 'own', 'bits')


def check_backward(impl, d, d2, fw, gy, mask, seed, ratios, kinds=MASK_KINDS, duals=(False, True)):
    """mask kinds none / tensor / own ReLU recomputed from x / sign bits x single / dual (own: single only, as in the product)"""
    bf16 = impl.bf16
    ref, ref2, m = fw['ref'], fw['ref2'], d['rows']
    gy64 = gy.astype(np.float64)
    for kind in kinds:
        if kind == 'none':
            passes, amb, handle = np.ones(gy.shape, bool), np.zeros(gy.shape, bool), None
        elif kind == 'tensor':
            passes, amb, handle = mask > 0, np.zeros(gy.shape, bool), impl.tensor(mask)     # -0.0 > 0 is False
        else:
            src = fw['own' if kind == 'own' else 'bits']
            passes, amb, handle = src['pre'] > 0, src['amb'], src['handle']
            _share('backward.' + kind, src['amb'][:, d['certain']], np.ones(int(d['certain'].sum()), bool), ratios)
        g_ref = gy64 * (passes & ~amb)
        g_abs = np.abs(gy64) * (passes | amb)
        for dual in duals:
            if dual and kind == 'own':
                continue
            name = 'backward.%s.%s' % (kind, 'dual' if dual else 'single')
            gx_ref, dg, db, b_gx, e_dg, e_db = backward_bounds(ref, d['gamma'], g_ref, g_abs, amb, m)
            pre_gg, pre_gb, pre_gg2, pre_gb2 = prefill(d['C'], m, seed)
            kw = {}
            if dual:
                kw = dict(x2=d2['x'], st2=fw['st2'], gamma2=d2['gamma'], ggamma2=pre_gg2, gbeta2=pre_gb2)
            out = impl.backward(gy, kind, handle, d['x'], fw['st'], d['gamma'], pre_gg, pre_gb, **kw)
            _within(name + '.gx', out['gx'], gx_ref, b_gx + _bf16_round(gx_ref, b_gx, bf16), ratios)
            _check_param_grads(name, out['ggamma'], out['gbeta'], pre_gg, pre_gb, dg, db, e_dg, e_db, ratios)
            if dual:
                gx2_ref, dg2, db2, b_gx2, e_dg2, e_db2 = backward_bounds(ref2, d2['gamma'], g_ref, g_abs, amb, m)
                _within(name + '.gx2', out['gx2'], gx2_ref, b_gx2 + _bf16_round(gx2_ref, b_gx2, bf16), ratios)
                _check_param_grads(name + '2', out['ggamma2'], out['gbeta2'], pre_gg2, pre_gb2, dg2, db2, e_dg2, e_db2, ratios)


def run_bn_case(impl, case, ratios):
    """everything of one (shape, C) cell: finalize, apply, backward"""
    (b, h, w), C_ = case
    rows = b * h * w
    bf16 = impl.bf16
    seed = 1000 * C_ + rows
    d, d2 = make_bn(rows, C_, seed, bf16), make_bn(rows, C_, seed + 1, bf16, rot=3)
    check_finalize(impl, d, ratios)
    res = make_grad((rows, C_), seed + 2, bf16)
    fw = check_apply(impl, d, d2, res, ratios)
    gy, mask = make_grad((rows, C_), seed + 3, bf16), make_grad((rows, C_), seed + 4, bf16, zeros=True)
    check_backward(impl, d, d2, fw, gy, mask, seed + 5, ratios)


FINALIZE_COUNTS = (1, 2, 3, 189, 5115)


def run_finalize_case(impl, count, C_, ratios):
    """count = 1 (adjust = 1 / max(0, 1)) and 2, sums spread over all 32 replicas, non-trivial running statistics, the
    constant channel"""
    check_finalize(impl, make_bn(count, C_, 77 * C_ + count, impl.bf16), ratios)


# ---- the stem's pool -----------------------------------------------------------------------------------------------------------
def _nchw(a):
    return np.ascontiguousarray(a.transpose(0, 3, 1, 2))


def _nhwc(a):
    return np.ascontiguousarray(a.transpose(0, 2, 3, 1))


def _windows(a, fill):
    """(B, H, W, C) -> (B, OH, OW, 9, C): the 3 x 3 / stride 2 windows with cover_all's overhang filled"""
    col = C.im2col(_nchw(a), 3, 3, 2, 2, 0, 0, pval=fill, cover_all=True)          # n, c, kh, kw, oh, ow
    n, c, kh, kw, oh, ow = col.shape
    return col.reshape(n, c, 9, oh, ow).transpose(0, 3, 4, 2, 1)


def check_pool(impl, case, ratios):
    """bn_relu_maxpool (+ want_sel), maxpool_relu_bwd, pool_bn_backward (gathering sums, xsel sums, three-pass where the fused
    pair does not tile C), gbias pre-filled.  The pool's ReLU sits behind the affine, so negative-gamma channels are in."""
    (B, H, W), C_ = case
    bf16 = impl.bf16
    rows = B * H * W
    seed = 500 * C_ + rows
    d = make_bn(rows, C_, seed, bf16)
    ref = BNRef(d)
    st = impl.finalize(replica_stats(d['x']), rows, d['gamma'], d['beta'], d['rm'], d['rv'])[0]
    shp = (B, H, W, C_)
    x4, pre4, b4 = d['x'].reshape(shp), ref.pre.reshape(shp), ref.bound.reshape(shp)
    act = np.maximum(pre4, 0)
    y_ref, idx_ref = C.max_pool_fwd(_nchw(act))
    y_ref, idx_ref = _nhwc(y_ref), _nhwc(idx_ref)
    OH, OW = y_ref.shape[1:3]
    # forward: max is 1-Lipschitz in the sup norm over its window
    out = impl.pool_fwd(x4, st, want_sel=False)
    wb = _windows(b4, 0.0).max(axis=3)
    _within('pool.y', out['y'], y_ref, wb + _bf16_round(y_ref, wb, bf16), ratios)
    idx = out['idx'].astype(np.int64)
    assert out['idx'].dtype == np.uint8 and idx.max() <= 8
    # argmax: undecidable where another entry's interval [relu(pre - b), relu(pre + b)] reaches the winner's lower end -- except
    # entries holding the winner's very x (the same value on both sides; first one wins on both) and windows that are zero for sure
    lo, hi = _windows(np.maximum(pre4 - b4, 0), -np.inf), _windows(np.maximum(pre4 + b4, 0), -np.inf)
    xw = _windows(x4.astype(np.float64), np.nan)
    take = lambda a, i: np.take_along_axis(a, i[:, :, :, None, :], axis=3)[:, :, :, 0, :]
    lo_a, x_a = take(lo, idx_ref), take(xw, idx_ref)
    rival = (hi >= lo_a[:, :, :, None, :]) & (xw != x_a[:, :, :, None, :]) & (np.arange(9)[None, None, None, :, None] != idx_ref[:, :, :, None, :])
    amb_idx = rival.any(axis=3) & (hi.max(axis=3) > 0)
    _share('pool.argmax', amb_idx, d['certain'], ratios)
    sure = ~amb_idx & d['certain']
    assert np.array_equal(idx[sure], idx_ref[sure]), 'argmax differs from the reference where it is decidable'
    # whatever was picked is a valid window position holding a value within the bound of the maximum
    valid = np.isfinite(_windows(pre4, -np.inf))
    assert take(valid, idx).all(), 'argmax points into the overhang'
    picked = take(_windows(act, -np.inf), idx)
    assert (y_ref - picked <= 2 * wb).all(), 'argmax does not hold the maximum'
    sel = impl.pool_fwd(x4, st, want_sel=True)
    assert np.array_equal(sel['y'], out['y']) and np.array_equal(sel['idx'], out['idx'])
    fused = POOL_FUSED[C_]
    want_xsel = fused and PATHS[C_][1 if bf16 else 0]
    assert (sel['xsel'] is not None) == want_xsel
    if want_xsel:
        assert np.array_equal(sel['xsel'], take(xw, idx).astype(np.float32)), 'xsel is not x at the argmax'
    # backward on the kernel's own argmax (as tests/test_gpu_kernels.py::test_stem_tail_fused_backward does)
    gy = make_grad((B, OH, OW, C_), seed + 1, bf16)
    gy64 = gy.astype(np.float64)
    dense = _nhwc(C.max_pool_bwd((B, C_, H, W), _nchw(idx), _nchw(gy64)))
    dense_abs = _nhwc(C.max_pool_bwd((B, C_, H, W), _nchw(idx), _nchw(np.abs(gy64))))
    amb = ((np.abs(pre4) <= b4) | ~d['certain']) & (dense_abs > 0)
    _share('pool.relu', amb[..., d['certain']], np.ones(int(d['certain'].sum()), bool), ratios)
    g_ref = dense * ((pre4 > 0) & ~amb)
    # maxpool_relu_bwd: at most four windows reach a pixel: three fp32 additions; an undecidable sign may pass or drop |g|
    gd = impl.pool_bwd(gy, out['idx'], x4, st)
    b_d = 3 * U * dense_abs + amb * dense_abs
    _within('pool.dense', gd, g_ref, b_d + _bf16_round(g_ref, b_d, bf16), ratios)
    g_abs = dense_abs * ((pre4 > 0) | amb)
    g_abs2 = g_abs.reshape(rows, C_) * (1 + 3 * U)
    forms = [('gather', None), ('xsel', sel['xsel'])] if want_xsel else [('gather' if fused else 'three-pass', None)]
    for name, xsel in forms:
        # the three-pass form on bf16 tensors rounds the dense gradient once (ops.pool_bn_backward's docstring)
        g_round = U16 if (bf16 and not fused) else 0.0
        gx_ref, dg, db, b_gx, e_dg, e_db = backward_bounds(ref, d['gamma'], g_ref.reshape(rows, C_), g_abs2, amb.reshape(rows, C_),
                                                           rows, g_round=g_round)
        pre_gg, pre_gb, pre_bias, _ = prefill(C_, rows, seed + 2)
        o = impl.pool_bn_bwd(gy, out['idx'], x4, st, d['gamma'], pre_gg, pre_gb, pre_bias, xsel)
        name = 'pool_bn.' + name
        b_gx = b_gx + _bf16_round(gx_ref, b_gx, bf16)
        _within(name + '.gx', o['gx'].reshape(rows, C_), gx_ref, b_gx, ratios)
        _check_param_grads(name, o['ggamma'], o['gbeta'], pre_gg, pre_gb, dg, db, e_dg, e_db, ratios)
        # gbias += sum of gx as stored: every element within b_gx; the additions form chains of fewer than `rows` terms, and the
        # blocks' float atomics of the un-replicated forms (colsum_kernel, pool_bn_bwd_apply_kernel) land on gbias ITSELF, so
        # what it held takes part in every one of them: rows u (sum |gx| + |before|)
        s_ref, s_abs = gx_ref.sum(axis=0), np.abs(gx_ref).sum(axis=0)
        want = pre_bias.astype(np.float64) + s_ref
        _within(name + '.gbias', o['gbias'], want, b_gx.sum(axis=0) + max(rows, 2) * U * (s_abs + np.abs(pre_bias)), ratios)


def check_pool_apply_plain(impl, case, ratios):
    """loans_pool_bn_bwd_apply_* with gxsum: the bias-gradient sums WITHOUT replicas.  ops.pool_bn_backward sends every channel
    count the fused pair tiles through the replica path, so the plain one is reached through the C ABI, with coefficients of
    the test's own: gx = k1 g + k2 x + k3 (two products, two additions: 3 u on the magnitudes; g as in check_pool)."""
    (B, H, W), C_ = case
    bf16 = impl.bf16
    rows = B * H * W
    seed = 900 * C_ + rows
    d = make_bn(rows, C_, seed, bf16)
    ref = BNRef(d)
    st = impl.finalize(replica_stats(d['x']), rows, d['gamma'], d['beta'], d['rm'], d['rv'])[0]
    shp = (B, H, W, C_)
    x4, pre4, b4 = d['x'].reshape(shp), ref.pre.reshape(shp), ref.bound.reshape(shp)
    out = impl.pool_fwd(x4, st, want_sel=False)
    idx = out['idx'].astype(np.int64)
    gy = make_grad(out['y'].shape, seed + 1, bf16)
    rng = np.random.RandomState(seed + 2)
    k1, k2, k3 = (rng.standard_normal(C_).astype(np.float32) for _ in range(3))
    dense = _nhwc(C.max_pool_bwd((B, C_, H, W), _nchw(idx), _nchw(gy.astype(np.float64))))
    dense_abs = _nhwc(C.max_pool_bwd((B, C_, H, W), _nchw(idx), _nchw(np.abs(gy.astype(np.float64)))))
    amb = ((np.abs(pre4) <= b4) | ~d['certain']) & (dense_abs > 0)
    g_ref = dense * ((pre4 > 0) & ~amb)
    x64 = x4.astype(np.float64)
    gx_ref = k1 * g_ref + k2 * x64 + k3
    b_gx = 3 * U * (np.abs(k1 * g_ref) + np.abs(k2 * x64) + np.abs(k3)) + np.abs(k1) * dense_abs * (3 * U + amb)
    b_gx = b_gx + _bf16_round(gx_ref, b_gx, bf16)
    pre_bias = prefill(C_, rows, seed + 3)[0]
    o = impl.pool_apply_plain(gy, out['idx'], x4, st, k1, k2, k3, pre_bias)
    _within('pool_apply_plain.gx', o['gx'], gx_ref, b_gx, ratios)
    s_ref, s_abs = gx_ref.sum(axis=(0, 1, 2)), np.abs(gx_ref).sum(axis=(0, 1, 2))
    want = pre_bias.astype(np.float64) + s_ref
    _within('pool_apply_plain.gbias', o['gbias'], want, b_gx.sum(axis=(0, 1, 2)) + max(rows, 2) * U * (s_abs + np.abs(pre_bias)), ratios)


def check_colsum(impl, rows, C_, ratios):
    """out[c] += sum over rows.  reduce_geometry: RL = 256 / min(C / 4, 256) rows in step, blocks of max(8 RL, ceil(rows / 1024))
    rows, at most 1024 of them: a thread's fp32 chain, the fold of RL partial sums, the blocks' float atomics on `out` and what
    `out` held are one chain of at most rows_per_thread + RL + blocks terms."""
    x = make_grad((rows, C_), 31 * C_ + rows, impl.bf16)
    before = prefill(C_, rows, 5)[0]
    got = impl.colsum(x, before)
    rl = 256 // min(C_ // 4, 256)
    rpb = max(8 * rl, -(-(-(-rows // 1024)) // rl) * rl)
    chain = rpb // rl + rl + -(-rows // rpb)
    s, s_abs = x.astype(np.float64).sum(axis=0), np.abs(x.astype(np.float64)).sum(axis=0)
    _within('colsum', got, before + s, chain * U * (s_abs + np.abs(before)), ratios)


def report(tag, fn, *args):
    """run one check and print the error / bound ratios it reached, also when it fails (for the table in DESIGN 3)"""
    ratios = {}
    try:
        fn(*args, ratios)
    finally:
        print('BN_RATIOS %s %s' % (tag, json.dumps(ratios, sort_keys=True)))
    return ratios


def assert_paths(C_, bf16):
    """the dispatch cell this channel count is in the grid for"""
    from loans_amd import ops
    assert ops.bn_units_ok(C_, bf16) is PATHS[C_][1 if bf16 else 0], (C_, bf16)
    if C_ in POOL_FUSED:
        assert (ops.reduce_channels_ok(C_) and C_ <= 1024) is POOL_FUSED[C_], C_


def assert_grid_covers_every_path():
    """{unit, fall-back} x {fp32, bf16} each meet the one-row, the sub-block, the odd and the big shape; the pool's unit /
    fall-back forward and fused / three-pass backward meet the minimum, an even and an odd size"""
    for bf16 in (False, True):
        for unit in (False, True):
            shapes = {s for s, c in bn_grid() if PATHS[c][1 if bf16 else 0] is unit}
            assert {S_ONE, S_FEW, S_ODD, S_BIG} <= shapes, (bf16, unit, shapes)
            for fused in (False, True):
                got = {s for s, c in pool_grid() if PATHS[c][1 if bf16 else 0] is unit and POOL_FUSED[c] is fused}
                if got:         # (in fp32 the unit condition C / 4 | 256 is also the fused pair's: two cells, four in bf16)
                    assert {(2, 3, 3), (2, 8, 7), (3, 13, 11)} <= got, (bf16, unit, fused, got)
        cells = {(PATHS[c][1 if bf16 else 0], POOL_FUSED[c]) for _, c in pool_grid()}
        assert cells == ({(True, True), (False, False), (False, True), (True, False)} if bf16 else {(True, True), (False, False)})
    assert S_BIG[0] * S_BIG[1] * S_BIG[2] * 96 * 4 < 96 << 20          # below the non-temporal switch


# ---- the fp32 restatement ------------------------------------------------------------------------------------------------------
F = np.float32


class NumpyImpl:
    """The kernels' arithmetic restated in NumPy fp32, operation by operation (no FMA; sums pairwise in fp32, then fp64)."""

    def __init__(self, bf16):
        self.bf16 = bf16

    def _out(self, v):
        return C.round_bf16(v) if self.bf16 else v

    def tensor(self, a):
        return a

    def finalize(self, stats, count, gamma, beta, rm, rv):
        s1, s2 = stats[:, 0].sum(axis=0), stats[:, 1].sum(axis=0)
        mu = s1 / count
        var = np.maximum(s2 / count - mu * mu, 0.0)
        vpe = var + np.float64(F(C.BN_EPS))
        rs, muf = (1.0 / np.sqrt(vpe)).astype(F), mu.astype(F)
        sc = gamma * rs
        sh = beta - muf * sc
        adjust = count / max(count - 1.0, 1.0)
        decay = F(C.BN_DECAY)
        rm_new = decay * rm + (F(1) - decay) * muf
        rv_new = decay * rv + (F(1) - decay) * (adjust * (vpe if C.RUNNING_VAR_INCLUDES_EPS else var)).astype(F)
        assert sc.dtype == F and sh.dtype == F and rm_new.dtype == F and rv_new.dtype == F
        return dict(mean=muf, rstd=rs, scale=sc, shift=sh), rm_new, rv_new

    def apply(self, x, st, relu=True, residual=None, x2=None, st2=None, want_bits=False):
        v = x * st['scale'] + st['shift']
        if residual is not None:
            v = v + residual
        if x2 is not None:
            v = v + (x2 * st2['scale'] + st2['shift'])
        if relu:
            v = np.maximum(v, F(0))
        assert v.dtype == F
        return dict(y=self._out(v), bits=_bits_of(v) if (want_bits and relu) else None)

    @staticmethod
    def _sums(g, x, st):
        xh = (x - st['mean']) * st['rstd']
        return g.sum(axis=0, dtype=F).astype(np.float64), (g * xh).sum(axis=0, dtype=F).astype(np.float64)

    @staticmethod
    def _coeffs(db, dg, m, gamma, st, gg0, gb0):
        rs, mu = st['rstd'].astype(np.float64), st['mean'].astype(np.float64)
        a = gamma.astype(np.float64) * rs
        return (gg0 + dg.astype(F), gb0 + db.astype(F), a.astype(F), (-a * rs * dg / m).astype(F), (a * (mu * rs * dg - db) / m).astype(F))

    def _masked(self, gy, kind, handle, x, st):
        if kind == 'none':
            return gy
        if kind == 'tensor':
            return np.where(handle > 0, gy, F(0))
        if kind == 'own':
            return np.where(x * st['scale'] + st['shift'] > 0, gy, F(0))
        bits = handle['bits']
        m = ((bits[:, None] >> np.arange(4)) & 1).astype(bool).reshape(gy.shape)
        return np.where(m, gy, F(0))

    def backward(self, gy, kind, handle, x, st, gamma, gg0, gb0, x2=None, st2=None, gamma2=None, ggamma2=None, gbeta2=None):
        g = self._masked(gy, kind, handle, x, st)
        m = x.shape[0]
        db, dg = self._sums(g, x, st)
        gg, gb, k1, k2, k3 = self._coeffs(db, dg, m, gamma, st, gg0, gb0)
        out = dict(gx=self._out(k1 * g + k2 * x + k3), ggamma=gg, gbeta=gb)
        if x2 is not None:
            db2, dg2 = self._sums(g, x2, st2)
            gg2, gb2, k1, k2, k3 = self._coeffs(db2, dg2, m, gamma2, st2, ggamma2, gbeta2)
            out.update(gx2=self._out(k1 * g + k2 * x2 + k3), ggamma2=gg2, gbeta2=gb2)
        return out

    def pool_fwd(self, x4, st, want_sel):
        B, H, W, C_ = x4.shape
        v = np.maximum(x4 * st['scale'] + st['shift'], F(0))
        win = _windows(v, -np.inf)
        idx = win.argmax(axis=3)
        y = win.max(axis=3).astype(F)
        xsel = None
        if want_sel and POOL_FUSED[C_] and PATHS[C_][1 if self.bf16 else 0]:
            xsel = np.take_along_axis(_windows(x4, np.nan), idx[:, :, :, None, :], axis=3)[:, :, :, 0, :].astype(F)
        return dict(y=self._out(y), idx=idx.astype(np.uint8), xsel=xsel)

    def _dense(self, gy, idx, x4, st):
        B, H, W, C_ = x4.shape
        dense = _nhwc(C.max_pool_bwd((B, C_, H, W), _nchw(idx.astype(np.int64)), _nchw(gy)))
        assert dense.dtype == F
        return np.where(x4 * st['scale'] + st['shift'] > 0, dense, F(0))

    def pool_bwd(self, gy, idx, x4, st):
        return self._out(self._dense(gy, idx, x4, st))

    def pool_apply_plain(self, gy, idx, x4, st, k1, k2, k3, gbias0):
        gx = self._out(k1 * self._dense(gy, idx, x4, st) + k2 * x4 + k3)
        return dict(gx=gx, gbias=gbias0 + gx.sum(axis=(0, 1, 2), dtype=F))

    def colsum(self, x, before):
        return before + x.sum(axis=0, dtype=F)

    def pool_bn_bwd(self, gy, idx, x4, st, gamma, gg0, gb0, gbias0, xsel):
        C_ = x4.shape[-1]
        g = self._dense(gy, idx, x4, st)
        if self.bf16 and not POOL_FUSED[C_]:
            g = C.round_bf16(g)
        o = self.backward(g.reshape(-1, C_), 'none', None, x4.reshape(-1, C_), st, gamma, gg0, gb0)
        o['gx'] = o['gx'].reshape(x4.shape)
        o['gbias'] = gbias0 + o['gx'].sum(axis=(0, 1, 2), dtype=F)
        return o


# ---- the kernels ---------------------------------------------------------------------------------------------------------------
class HipImpl:
    """loans_amd.ops on the GPU behind the same interface (imports torch / the library only when constructed)"""

    def __init__(self, bf16):
        import torch
        from loans_amd import ops
        self.bf16, self.torch, self.ops = bf16, torch, ops
        self.tdt = torch.bfloat16 if bf16 else torch.float32

    def tensor(self, a):
        t = self.torch.from_numpy(np.ascontiguousarray(a)).cuda()
        return t.to(self.tdt).contiguous()

    def _f(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()

    @staticmethod
    def _np(t):
        return t.detach().float().cpu().numpy()

    def finalize(self, stats, count, gamma, beta, rm, rv):
        rmd, rvd = self._f(rm), self._f(rv)
        st = self.ops.bn_finalize(self.torch.from_numpy(stats).cuda(), count, self._f(gamma), self._f(beta), rmd, rvd)
        out = dict(mean=self._np(st.mean), rstd=self._np(st.rstd), scale=self._np(st.scale), shift=self._np(st.shift), handle=st)
        return out, self._np(rmd), self._np(rvd)

    def apply(self, x, st, relu=True, residual=None, x2=None, st2=None, want_bits=False):
        y = self.ops.bn_apply(self.tensor(x), st['handle'], relu=relu,
                              residual=None if residual is None else self.tensor(residual),
                              x2=None if x2 is None else self.tensor(x2), st2=None if st2 is None else st2['handle'],
                              want_bits=want_bits)
        bits = getattr(y, 'relu_bits', None)
        return dict(y=self._np(y), bits=None if bits is None else bits.cpu().numpy(), t=y)

    def backward(self, gy, kind, handle, x, st, gamma, gg0, gb0, x2=None, st2=None, gamma2=None, ggamma2=None, gbeta2=None):
        mask = None
        if kind == 'tensor':
            mask = handle
        elif kind in ('own', 'bits'):
            mask = handle['t']
            assert (getattr(mask, 'relu_bits', None) is not None) == (kind == 'bits')
        gg, gb = self._f(gg0), self._f(gb0)
        kw = {}
        if x2 is not None:
            gg2, gb2 = self._f(ggamma2), self._f(gbeta2)
            kw = dict(x2=self.tensor(x2), st2=st2['handle'], gamma2=self._f(gamma2), ggamma2=gg2, gbeta2=gb2)
        r = self.ops.bn_backward(self.tensor(gy), mask, self.tensor(x), st['handle'], self._f(gamma), gg, gb,
                                 mask_is_own_relu=(kind == 'own'), **kw)
        if x2 is None:
            return dict(gx=self._np(r), ggamma=self._np(gg), gbeta=self._np(gb))
        return dict(gx=self._np(r[0]), gx2=self._np(r[1]), ggamma=self._np(gg), gbeta=self._np(gb), ggamma2=self._np(gg2),
                    gbeta2=self._np(gb2))

    def pool_fwd(self, x4, st, want_sel):
        r = self.ops.bn_relu_maxpool(self.tensor(x4), st['handle'], want_sel=want_sel)
        xsel = r[2] if want_sel else None
        return dict(y=self._np(r[0]), idx=r[1].cpu().numpy(), xsel=None if xsel is None else self._np(xsel), t_idx=r[1], t_xsel=xsel)

    def pool_bwd(self, gy, idx, x4, st):
        return self._np(self.ops.maxpool_relu_bwd(self.tensor(gy), self.torch.from_numpy(idx).cuda(), self.tensor(x4), st['handle']))

    def pool_bn_bwd(self, gy, idx, x4, st, gamma, gg0, gb0, gbias0, xsel):
        gg, gb, gbias = self._f(gg0), self._f(gb0), self._f(gbias0)
        gx = self.ops.pool_bn_backward(self.tensor(gy), self.torch.from_numpy(idx).cuda(), self.tensor(x4), st['handle'],
                                       self._f(gamma), gg, gb, gbias=gbias, xsel=None if xsel is None else self.tensor(xsel))
        return dict(gx=self._np(gx), ggamma=self._np(gg), gbeta=self._np(gb), gbias=self._np(gbias))

    def pool_apply_plain(self, gy, idx, x4, st, k1, k2, k3, gbias0):
        ops, h = self.ops, st['handle']
        B, H, W, C_ = x4.shape
        gyd, xd, idxd = self.tensor(gy), self.tensor(x4), self.torch.from_numpy(idx).cuda()
        kd = [self._f(k) for k in (k1, k2, k3)]
        gx, gbias = self.torch.empty_like(xd), self._f(gbias0)
        lib = ops._lib.load()
        fn = lib.loans_pool_bn_bwd_apply_bf16 if self.bf16 else lib.loans_pool_bn_bwd_apply_f32
        ops.check(fn(ops._ptr(gyd), ops._ptr(idxd), ops._ptr(xd), ops._ptr(h.scale), ops._ptr(h.shift), ops._ptr(kd[0]),
                     ops._ptr(kd[1]), ops._ptr(kd[2]), ops._ptr(gx), ops._ptr(gbias), B, H, W, C_, gy.shape[1], gy.shape[2],
                     ops._stream()), 'loans_pool_bn_bwd_apply')
        return dict(gx=self._np(gx), gbias=self._np(gbias))

    def colsum(self, x, before):
        out = self._f(before)
        self.ops.colsum_acc(self.tensor(x), out)
        return self._np(out)
