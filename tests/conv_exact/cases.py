"""Exact convolution cases: integer-valued operands so small that every product and every partial sum of
the contraction, in ANY order, is an integer below 2^24 and therefore exact in fp32.  The fp32 accumulator of every conv
kernel -- whatever its tile, K order, split-K atomics, slab fold or MFMA shape -- then holds the exact integer, and the
expected result is known to the bit:

  fp32 output            the exact integer
  bf16 output            round_bf16(exact epilogue value): ONE round-to-nearest-even
  LOANS_F_STATS          sums of the exact (unrounded) values  (include/loans_hip.h: taken from the fp32 accumulators)
  LOANS_F_BNSUMS, bf16   sums of the ROUNDED g                 (include/loans_hip.h, LOANS_F_BNSUMS)
  weight gradient        the exact integer, plus the integer start value of dw

The epilogue order is that of include/loans_hip.h and csrc/igemm_bf16.hip's epilogue loop: acc + bias, then the mask, then
+ addend (masked for LOANS_F_ADDEND_MASK), then one rounding.  The reference is oracle.chainer_ops in float64, which is exact on
these inputs (integers far below 2^53); every reference is asserted integer-valued.

Geometries are IMPORTED from the existing test modules (the smallest shapes at which each kernel's gating and tails are
reached; all of them have run on the device).  Pytest does not collect this module (as tests/bn_cases.py)."""
import zlib

import numpy as np

from oracle import chainer_ops as O

TWO24 = float(2 ** 24)

# amplitude of every operand: seeded integers, uniform in [-a, a]
PROFILES = {
    # all bf16-exact (|v| <= 256 even at the largest recorded scale); outputs run to several thousand: a bf16 store must round
    'WIDE': dict(x=32, w=8, bias=16, add=64),
    # no output needs rounding and even the sums of squares stay exact
    'SMALL': dict(x=2, w=1, bias=2, add=2),
}
MAX_SCALE = 4           # WIDE amplitudes x 4: the addend reaches 256, the last magnitude at which every integer is a bf16 value
# what `WIDE` has to show (test_cases_cpu.py asserts them on every WIDE case whose bf16 output is compared)
MIN_ROUNDED, MIN_TIES, MIN_CHANNELS = 0.30, 0.03, 0.5
# The declared exceptions to `sum_m |out[m, n]| < 2^24`, (tag of the case, geometry): LOANS_F_STATS sums every output pixel of a
# channel, and these have so many (25 088 and 65 536 for the conv1 frames of 224 x 224 and 512 x 512 pixels with |out| ~ 900;
# 16 384 for the largest BN-on-load case with |out| ~ 1800) that no power of two keeps both that sum exact and 30 % of the
# outputs rounding.  On these -- and on no other case -- the WIDE sum keeps the bound of the existing test of the call;
# assert_stats refuses any case whose condition and whose entry here disagree, test_cases_cpu.py asserts the same on the CPU.
SUM_NOT_EXACT = {
    ('WIDE', (2, 3, 224, 224, 64, 7, 2, 3)),
    ('WIDE', (1, 3, 512, 512, 64, 7, 2, 3)),
    ('AFFINE', (4, 128, 64, 64, 512, 1, 1, 0)),
}
ROUND_IN_W = 4          # ROUND_IN draws w from [-4, 4]: with |x| up to 1023 every channel sum of every geometry stays below 2^24


# ---------------------------------------------------------------------------------------------------------------- geometries
def geometries():
    """name of the family -> list of (B, Cin, H, W, Cout, k, stride, pad), taken from the modules that own them"""
    from tests import test_gpu_bf16_storage as S16
    from tests import test_gpu_kernels as F32
    from tests.conv_posmajor import test_gpu_kernels as PM
    from tests.conv_tap_loop import test_gpu_kernels as TAP
    from tests.wgrad_halo_f32 import test_gpu_kernels as WH
    stem = lambda c: (c[0], 3, c[1], c[2], 64, 7, 2, 3)                 # noqa: E731
    fam = {}
    seen = []
    for g in list(F32.CONV_CASES) + list(TAP.GEOMS.values()):
        if g not in seen:
            seen.append(g)
    fam['conv32'] = seen
    fam['splitk32'] = list(F32.SPLIT_K_CASES)
    fam['finetail32'] = [TAP.FINE_TAIL_GEOM]
    fam['posmajor32'] = [c[:8] for c in PM.CASES.values()]
    fam['pair32'] = list(F32.PAIR_CASES)                                # B, Cin, H, W, Ca, Cb, k, s, p
    fam['dense32'] = [(c[0], 3, c[1], c[2]) + c[3:] for c in F32.DENSE_ROWS_CASES]
    fam['stem32'] = [stem(c) for c in F32.STEM_DIRECT_CASES]
    fam['stem_wgrad32'] = [stem(c) for c in F32.STEM_WGRAD_CASES]
    fam['wghalo32'] = [c + (3, 1, 1) for c in WH.GEOMS.values()]
    fam['crop32'] = list(F32.CROP_DGRAD_SHAPES)                         # B, H, W
    fam['compute16'] = list(F32.BF16_COMPUTE_CASES)
    fam['bnsums'] = [(c[0], c[1], c[2], c[3], c[4], c[5], 1, c[5] // 2) for c in S16.BNSUMS_CASES]
    fam['conv16'] = list(S16.CASES)
    fam['halo16'] = [c[:6] + (1, c[6]) for c in S16.HALO_CASES]
    fam['pw16'] = [c + (1, 1, 0) for c in S16.POINTWISE_CASES]
    fam['affine16'] = [c + (1, 1, 0) for c in S16.AFFINE_CASES]
    fam['splitk16'] = list(S16.SPLIT_K_CASES)
    fam['pair16'] = list(S16.PAIR_CASES)
    fam['stem16'] = [stem(c) for c in S16.STEM_DIRECT_CASES]
    fam['stem_wgrad16'] = [stem(c) for c in S16.STEM_WGRAD_CASES]
    fam['wghalo16'] = [c + (3, 1, 1) for c in S16.WGHALO_CASES]
    fam['slab16'] = list(S16.SLAB_CASES)                                # geometry + tile
    return fam


def posmajor_cases():
    from tests.conv_posmajor import test_gpu_kernels as PM
    return PM.CASES


def gid(g):
    return 'x'.join(str(v) for v in g)


# ---------------------------------------------------------------------------------------------------------------- bf16 forms
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def round_bf16(a):
    """round to nearest even, in float64 (oracle.chainer_ops.round_bf16 on the fp32 image of an exactly representable value)"""
    a = np.asarray(a, np.float64)
    f = a.astype(np.float32)
    assert np.array_equal(f.astype(np.float64), a), 'the exact value must be an fp32 value'
    return O.round_bf16(f).astype(np.float64)


def trunc_bf16(a):
    """towards zero: the alternative a kernel that drops the low 16 bits would compute"""
    return (_bits(a) & np.uint32(0xFFFF0000)).view(np.float32).astype(np.float64)


def half_away_bf16(a):
    """round half away from zero: the alternative of adding 0x8000 before the truncation"""
    return ((_bits(a) + np.uint32(0x8000)) & np.uint32(0xFFFF0000)).view(np.float32).astype(np.float64)


def next_bf16(a):
    """the bf16 neighbour of trunc_bf16(a) away from zero"""
    return ((_bits(a) & np.uint32(0xFFFF0000)) + np.uint32(0x10000)).view(np.float32).astype(np.float64)


def is_tie(a):
    a = np.asarray(a, np.float64)
    lo, hi = trunc_bf16(a), next_bf16(a)
    return (a != lo) & (2 * a == lo + hi)


def rounding_profile(exact):
    """(share of values a bf16 store changes, share of ties RNE resolves towards zero, share it resolves away from zero)"""
    r, lo = round_bf16(exact), trunc_bf16(exact)
    tie = is_tie(exact)
    n = float(exact.size)
    return float((r != exact).sum() / n), float((tie & (r == lo)).sum() / n), float((tie & (r != lo)).sum() / n)


# ---------------------------------------------------------------------------------------------------------------- generators
def _seed(*what):
    return zlib.crc32(repr(what).encode()) & 0x7FFFFFFF


def ints(rng, shape, a):
    return rng.randint(-a, a + 1, size=shape).astype(np.float32)


def with_zeros(a, rng):
    """about 10 % exact +0.0 and 10 % exact -0.0, as bn_cases.make_grad(zeros=True): both count as `not > 0`"""
    u = rng.random_sample(a.shape)
    a = a.copy()
    a[u < 0.10] = 0.0
    a[(u >= 0.10) & (u < 0.20)] = -0.0
    return a


def mask_tensor(rng, shape):
    """a reference tensor for mask_ref / addend_mask_ref: integers with both zeros, positives and negatives"""
    return with_zeros(ints(rng, shape, 8), rng)


def outsize(size, k, s, p):
    return (size + 2 * p - k) // s + 1


def is_integer(a):
    return bool(np.array_equal(a, np.rint(a)))


class Case:
    """One geometry with one operand profile: operands (NCHW float32, integer-valued), lazily made float64 references."""

    def __init__(self, geom, profile, scale=1, round_in=False, x=None, tag=None):
        self.geom, self.profile, self.scale, self.round_in = tuple(geom), profile, scale, round_in
        self.tag = tag or ('ROUND_IN' if round_in else profile)         # what SUM_NOT_EXACT lists the case under
        B, Cin, H, W, Cout, k, s, p = self.geom
        amp = {n: max(1, int(v * scale)) for n, v in PROFILES[profile].items()}
        if scale < 1:               # SMALL at the longest K: only x shrinks (w is {-1, 0, 1} already)
            amp = dict(PROFILES[profile], x=max(1, int(PROFILES[profile]['x'] * scale)))
        if round_in:
            amp['w'] = ROUND_IN_W
        rng = np.random.RandomState(_seed(self.geom, profile, round_in))
        self.Ho, self.Wo = outsize(H, k, s, p), outsize(W, k, s, p)
        oshape = (B, Cout, self.Ho, self.Wo)
        self.x = with_zeros(ints(rng, (B, Cin, H, W), amp['x']), rng)           # (the zeros: the operand of LOANS_F_RELU_IN)
        self.w = ints(rng, (Cout, Cin, k, k), amp['w'])
        self.bias = ints(rng, Cout, amp['bias'])
        self.gy = ints(rng, oshape, amp['x'])
        self.add_y = ints(rng, oshape, amp['add'])
        self.add_x = ints(rng, (B, Cin, H, W), amp['add'])
        self.ref_x = mask_tensor(rng, (B, Cin, H, W))
        self.dw0 = ints(rng, (Cout, Cin, k, k), 64)
        if round_in:
            # the bf16-COMPUTE arm rounds fp32 operands on load: magnitudes in [256, 1024), where bf16 holds every 2nd / 4th integer
            sign = lambda sh: rng.randint(0, 2, size=sh) * 2.0 - 1.0            # noqa: E731
            self.x_raw = (sign(self.x.shape) * rng.randint(256, 1024, size=self.x.shape)).astype(np.float32)
            self.gy_raw = (sign(oshape) * rng.randint(256, 1024, size=oshape)).astype(np.float32)
            self.x = O.round_bf16(self.x_raw)
        self.unit = 1.0             # every reference is a multiple of it
        if x is not None:           # the second convolution of a pair launch reads the first one's input; an operand made on load
            self.x = x
            if not is_integer(x):
                assert is_integer(2 * x)
                self.unit = 0.5     # (LOANS_F_AFFINE_IN with scale 0.5: half-integers, as exact as integers)
        self._memo = {}

    # -- float64 references, each made once ---------------------------------------------------------------------------------
    def _get(self, key, fn):
        if key not in self._memo:
            self._memo[key] = fn()
        return self._memo[key]

    def _fwd(self, x, w):
        s, p = self.geom[6], self.geom[7]
        y, col = O.conv2d_fwd(np.asarray(x, np.float64), np.asarray(w, np.float64), None, s, p)
        assert is_integer(y / self.unit)
        return y, col

    def col(self):
        return self._get('col', lambda: self._fwd(self.x, self.w))[1]

    def conv(self):
        return self._get('col', lambda: self._fwd(self.x, self.w))[0]

    def conv_relu(self):
        return self._get('conv_relu', lambda: self._fwd(np.maximum(self.x, 0), self.w)[0])

    def _bwd(self, col, gy, need_gx):
        s, p = self.geom[6], self.geom[7]
        gx, gw, _ = O.conv2d_bwd(self.x.shape, col, self.w.astype(np.float64), np.asarray(gy, np.float64), s, p, False, need_gx=need_gx)
        assert is_integer(gw / self.unit) and (gx is None or is_integer(gx))
        return gx, gw

    def gx(self, gy=None):
        if gy is not None:
            return self._bwd(self.col(), gy, True)[0]
        return self._get('bwd', lambda: self._bwd(self.col(), self.gy, True))[0]

    def gw(self):
        return self._get('bwd', lambda: self._bwd(self.col(), self.gy, True))[1]

    def gw_relu(self):
        return self._get('gw_relu', lambda: self._bwd(self._fwd(np.maximum(self.x, 0), self.w)[1], self.gy, False)[1])

    def exact(self, kind):
        """the epilogue's value before any rounding: acc + bias, mask, + addend (masked for ADDEND_MASK)"""
        ex = (None, slice(None), None, None)
        pos = self.ref_x > 0
        if kind == 'plain':
            return self.conv()
        if kind == 'bias':
            return self.conv() + self.bias.astype(np.float64)[ex]
        if kind == 'add':
            return self.conv() + self.add_y
        if kind == 'bias_add':
            return self.conv() + self.bias.astype(np.float64)[ex] + self.add_y
        if kind == 'relu_add':
            return self.conv_relu() + self.add_y
        if kind == 'relu':
            return self.conv_relu()
        if kind == 'relu_bias':
            return self.conv_relu() + self.bias.astype(np.float64)[ex]
        if kind == 'gx':
            return self.gx()
        if kind == 'gx_mask':
            return self.gx() * pos
        if kind == 'gx_add':
            return self.gx() + self.add_x
        if kind == 'gx_mask_add':
            return self.gx() * pos + self.add_x
        if kind == 'gx_addmask':
            return self.gx() + self.add_x * pos
        raise KeyError(kind)

    def want(self, kind, bf16):
        e = self.exact(kind) + 0.0          # (-0.0 of a masked product: compared by value anyway)
        return round_bf16(e) if bf16 else e

    def stat_sums(self, kind='bias'):
        """LOANS_F_STATS: per-channel sum and sum of squares of the EXACT output"""
        e = self.exact(kind)
        return e.sum(axis=(0, 2, 3)), (e * e).sum(axis=(0, 2, 3))

    # -- the conditions: functions of the case and the reference alone ------------------------------------------------------
    def bound_fwd(self):
        """conv(|x|, |w|) + |bias| + |addend|: bounds every partial sum of every order and split of the forward contraction"""
        def make():
            y, _ = self._fwd(np.abs(self.x), np.abs(self.w))
            return float((y + np.abs(self.bias).astype(np.float64)[None, :, None, None] + np.abs(self.add_y)).max())
        return self._get('bound_fwd', make)

    def bound_dgrad(self):
        def make():
            s, p = self.geom[6], self.geom[7]
            gx, _, _ = O.conv2d_bwd(self.x.shape, self.col(), np.abs(self.w).astype(np.float64), np.abs(self.gy).astype(np.float64), s, p, False)
            return float((gx + np.abs(self.add_x)).max())
        return self._get('bound_dgrad', make)

    def bound_wgrad(self):
        def make():
            s, p = self.geom[6], self.geom[7]
            _, col = O.conv2d_fwd(np.abs(self.x).astype(np.float64), np.zeros(self.w.shape), None, s, p)
            _, gw, _ = O.conv2d_bwd(self.x.shape, col, np.zeros(self.w.shape), np.abs(self.gy).astype(np.float64), s, p, False, need_gx=False)
            return float((gw + np.abs(self.dw0)).max())
        return self._get('bound_wgrad', make)

    def stats_exact(self, kind='bias'):
        """sum_m |out[m, n]| < 2^24 for every channel: the fp32 partial sums of LOANS_F_STATS are exact in any grouping"""
        return bool(np.abs(self.exact(kind)).sum(axis=(0, 2, 3)).max() < TWO24)

    def sumsq_exact(self, kind='bias'):
        e = self.exact(kind)
        return bool((e * e).sum(axis=(0, 2, 3)).max() < TWO24)

    def small_needs_no_rounding(self):
        return all(np.array_equal(round_bf16(self.exact(k)), self.exact(k)) for k in ('bias', 'relu_add', 'add', 'bias_add'))

    def every_pixel_has_a_tap(self):
        """k >= stride: no stride-parity class of the data gradient is empty (a strided 1 x 1 leaves three of four pixels zero,
        and zeros do not round)"""
        return self.geom[5] >= self.geom[6]

    def visible(self, kind):
        """the rounding is visible on the bf16 image of `kind`: enough values change, ties of both directions, and the
        channel sums of the rounded tensor differ from the exact sums"""
        e = self.exact(kind)
        rounded, down, up = rounding_profile(e)
        channels = float((round_bf16(e).sum(axis=(0, 2, 3)) != e.sum(axis=(0, 2, 3))).mean())
        return rounded >= MIN_ROUNDED and down >= MIN_TIES and up >= MIN_TIES and channels >= MIN_CHANNELS


_cases = {}
_scales = {}


def wide_scale(geom):
    """The power of two the WIDE amplitudes of a geometry are multiplied with: 1 unless the rounding of its bf16 forward output
    is not visible enough (a very short K); then found by doubling, under the exactness condition.  A geometry on which no
    scale shows it (a 1 x 1 convolution with padding: most outputs are the bias alone) keeps 1; only fp32 tests use such."""
    geom = tuple(geom)
    if geom not in _scales:
        _scales[geom] = scale = 1
        while scale <= MAX_SCALE:
            c = Case(geom, 'WIDE', scale)
            if max(c.bound_fwd(), c.bound_dgrad()) >= TWO24:
                break
            if c.visible('bias'):
                _scales[geom] = scale
                break
            scale *= 2
    return _scales[geom]


def case(geom, profile='WIDE', round_in=False, keep=4):
    """the case of a geometry, made once; the last `keep` stay in memory"""
    geom = tuple(geom)
    key = (geom, profile, round_in)
    if key not in _cases:
        while len(_cases) >= keep:
            _cases.pop(next(iter(_cases)))
        scale = wide_scale(geom) if (profile == 'WIDE' and not round_in) else 1
        c = Case(geom, profile, scale, round_in)
        if profile == 'SMALL' and not c.small_needs_no_rounding():
            # K of 2304 and more with hundreds of thousands of outputs: a few pass 256 and would round.  x in [-1, 1] there.
            c = Case(geom, profile, 0.5, round_in)
        _cases[key] = c
    return _cases[key]


def wgrad_profile(geom):
    """WIDE where the weight gradient's exactness bound holds with it (sum over every pixel of |x| |gy|), else SMALL: the
    stems with 10^5 pixels and more"""
    return 'WIDE' if case(geom, 'WIDE').bound_wgrad() < TWO24 else 'SMALL'


# ---------------------------------------------------------------------------------------------------------------- BN tables
AFFINE_SCALES = (0.5, 1.0, 2.0, -1.0)


def affine_table(C_, seed):
    """(scale, shift) of LOANS_F_AFFINE_IN: x * scale + shift is exact whether or not the compiler contracts it"""
    rng = np.random.RandomState(_seed('affine', C_, seed))
    return np.array(AFFINE_SCALES, np.float32)[rng.randint(0, 4, size=C_)], ints(rng, C_, 16)


def affine_operand(x, scale, shift):
    """round_bf16(relu(x * scale + shift)): the operand the convolution contracts (NCHW)"""
    ex = (None, slice(None), None, None)
    a = np.maximum(x.astype(np.float64) * scale.astype(np.float64)[ex] + shift.astype(np.float64)[ex], 0)
    return round_bf16(a)


def bnsums_table(geom):
    """LOANS_F_BNSUMS: the BN's input y (the shape of the data gradient, NCHW) and its table [mean | rstd | scale | shift]"""
    B, C_, H, W = geom[:4]
    rng = np.random.RandomState(_seed('bnsums', tuple(geom)))
    y = with_zeros(ints(rng, (B, C_, H, W), 2), rng)
    mean, shift = ints(rng, C_, 1), ints(rng, C_, 2)
    scale = np.array(AFFINE_SCALES, np.float32)[rng.randint(0, 4, size=C_)]
    return y, mean, np.ones(C_, np.float32), scale, shift


def bnsums_ref(g, y, mean, scale, shift):
    """(sum_m g m, sum_m g m (y - mean), the largest sum of magnitudes), m = (y scale + shift > 0); g is the tensor as STORED"""
    ex = (None, slice(None), None, None)
    m = (y.astype(np.float64) * scale.astype(np.float64)[ex] + shift.astype(np.float64)[ex]) > 0
    gm = g * m
    t2 = gm * (y.astype(np.float64) - mean.astype(np.float64)[ex])
    bound = max(np.abs(gm).sum(axis=(0, 2, 3)).max(), np.abs(t2).sum(axis=(0, 2, 3)).max())
    return gm.sum(axis=(0, 2, 3)), t2.sum(axis=(0, 2, 3)), float(bound)


# ---------------------------------------------------------------------------------------------------------------- fp32 restatement
def contract_f32(c, how, rng):
    """The forward contraction of a case in fp32 NumPy with K in another order -- must equal the reference EXACTLY, or the case
    (not a kernel) is wrong.  how: 'perm' a random permutation of K; ('slices', n) K cut into n slices added in random order;
    'chunks' 32-wide chunks added one after the other."""
    col = c.col()
    B, Cin, kh, kw, Ho, Wo = col.shape
    A = np.ascontiguousarray(col.transpose(0, 4, 5, 1, 2, 3).reshape(B * Ho * Wo, Cin * kh * kw), dtype=np.float32)
    Wm = np.ascontiguousarray(c.w.reshape(c.w.shape[0], -1).T, dtype=np.float32)
    K = A.shape[1]
    if how == 'perm':
        order = rng.permutation(K)
        out = A[:, order] @ Wm[order]
    else:
        step = 32 if how == 'chunks' else -(-K // how[1])
        starts = list(range(0, K, step))
        if how != 'chunks':
            starts = [starts[i] for i in rng.permutation(len(starts))]
        out = np.zeros((A.shape[0], Wm.shape[1]), np.float32)
        for s0 in starts:
            out = out + A[:, s0:s0 + step] @ Wm[s0:s0 + step]
        assert out.dtype == np.float32
    return out.reshape(B, Ho, Wo, -1).transpose(0, 3, 1, 2)


# ---------------------------------------------------------------------------------------------------------------- device side
def nhwc(a, cpad=None):
    a = np.transpose(a, (0, 2, 3, 1))
    if cpad and a.shape[-1] < cpad:
        a = np.concatenate([a, np.zeros(a.shape[:-1] + (cpad - a.shape[-1],), a.dtype)], axis=-1)
    return np.ascontiguousarray(a, dtype=np.float32)


def up(a, bf16=False):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    if bf16:
        t16 = t.to(torch.bfloat16)
        assert torch.equal(t16.float(), t), 'every operand is a bf16 value'
        return t16.contiguous()
    return t


def mismatch(got, want, exact=None, channels=None):
    """None if the device tensor `got` (NHWC, or OHWI for a weight gradient) equals `want` (NCHW / OIHW float64) by VALUE
    (+0.0 == -0.0: LOANS_TILE_POSMAJOR documents that the sign of an exact zero may differ, a masked element is 0.f); else the
    report: the count, the first eight (b, y, x, c) with got / wanted, whether the pixel lies on the border, whether the
    wanted value was a tie of the rounding (`exact`: the unrounded reference)."""
    g = got.detach().float().cpu().numpy().astype(np.float64)
    w = np.transpose(want, (0, 2, 3, 1))
    if channels is not None:
        g = g[..., :channels]
    assert g.shape == w.shape, (g.shape, w.shape)
    bad = ~(g == w)
    if not bad.any():
        return None
    e = None if exact is None else np.transpose(exact, (0, 2, 3, 1))
    lines = ['%d of %d elements differ' % (int(bad.sum()), bad.size)]
    for b, y, x, c in np.argwhere(bad)[:8]:
        border = y in (0, w.shape[1] - 1) or x in (0, w.shape[2] - 1)
        tie = '' if e is None else (' exact %r%s' % (e[b, y, x, c], ' TIE' if bool(is_tie(e[b, y, x, c])) else ''))
        lines.append('(b %d, y %d, x %d, c %d): got %r wanted %r%s%s' % (b, y, x, c, g[b, y, x, c], w[b, y, x, c], ' border' if border else '', tie))
    return '\n'.join(lines)


def assert_same(got, want, what, exact=None, channels=None):
    msg = mismatch(got, want, exact, channels)
    assert msg is None, '%s: %s' % (what, msg)


def assert_out(c, got, kind, what, channels=None):
    """a device output against the case's reference of `kind`: fp32 tensors the exact integer, bf16 tensors its one rounding"""
    import torch
    bf16 = got.dtype == torch.bfloat16
    assert_same(got, c.want(kind, bf16), '%s %s' % (what, kind), exact=c.exact(kind) if bf16 else None, channels=channels)


def sum_is_exact(c):
    return (c.tag, c.geom) not in SUM_NOT_EXACT


def assert_stats(c, stats, what, kind='bias', sumsq_rtol=1e-5):
    """LOANS_F_STATS: the sum equals the EXACT sum (not the sum of the stored bf16 values) on every case but the declared
    exceptions of SUM_NOT_EXACT, which keep the bound of the existing test of the call -- a case whose sum condition disagrees
    with that list is an error, never a quiet change of the comparison.  The sum of squares equals exactly on SMALL and keeps
    the existing bound on WIDE (the issue: not compared exactly there)."""
    st = stats.sum(dim=0).cpu().numpy()
    s1, s2 = c.stat_sums(kind)
    exact = sum_is_exact(c)
    assert c.stats_exact(kind) == exact, '%s: the sum condition of %r / %r and SUM_NOT_EXACT disagree' % (what, c.tag, c.geom)
    if exact:
        bad = np.flatnonzero(st[0] != s1)
        assert bad.size == 0, '%s: sum of %d channels differs, first %d: got %r exact %r' % (what, bad.size, bad[0], st[0][bad[0]], s1[bad[0]])
    else:
        np.testing.assert_allclose(st[0], s1, rtol=sumsq_rtol, atol=1e-3)
    if c.profile == 'SMALL':
        assert c.sumsq_exact(kind)
        bad = np.flatnonzero(st[1] != s2)
        assert bad.size == 0, '%s: sum of squares of %d channels differs, first %d: got %r exact %r' % (what, bad.size, bad[0], st[1][bad[0]], s2[bad[0]])
    else:
        np.testing.assert_allclose(st[1], s2, rtol=sumsq_rtol)


_dev = {}


def device(c, bf16, cpad=None, keep=2):
    """the device tensors of a case (NHWC / OHWI; bf16 storage: activations and gradients bf16, weights and bias the fp32
    masters), uploaded once; the last `keep` stay"""
    key = (c.geom, c.profile, c.round_in, bf16, cpad)
    if key not in _dev:
        while len(_dev) >= keep:
            _dev.pop(next(iter(_dev)))
        d = dict(x=up(nhwc(c.x, cpad), bf16), w=up(nhwc(c.w, cpad)), bias=up(c.bias), gy=up(nhwc(c.gy), bf16),
                 add_y=up(nhwc(c.add_y), bf16), add_x=up(nhwc(c.add_x, cpad), bf16), ref_x=up(nhwc(c.ref_x, cpad), bf16),
                 dw0=up(nhwc(c.dw0, cpad)))
        _dev[key] = d
    return _dev[key]


# ---------------------------------------------------------------------------------------------------------------- the grid
def pair_cases(g9, profile):
    """the two convolutions of a pair launch (B, Cin, H, W, Ca, Cb, k, s, p; bf16 storage: the 8-tuple, Ca = Cb): one input"""
    g9 = tuple(g9)
    ga = g9[:5] + g9[-3:]
    gb = g9[:4] + (g9[5] if len(g9) == 9 else g9[4],) + g9[-3:]
    a = case(ga, profile)
    key = ('pair', g9, profile)
    if key not in _cases:
        b = Case(gb, profile, a.scale, x=a.x)
        rng = np.random.RandomState(_seed('pair second', g9, profile))
        b.w = ints(rng, b.w.shape, max(1, int(PROFILES[profile]['w'] * max(a.scale, 1))))         # (equal Cout: the seed of the geometry would repeat w)
        _cases[key] = b
    return a, _cases[key]


# family -> ((profile, what the GPU tests compute of it: fwd / dgrad / wgrad; bf16: a bf16 output is compared), ...)
USES = {
    'conv32': (('WIDE', 'fwd dgrad wgrad'), ('SMALL', 'fwd')),
    'splitk32': (('WIDE', 'fwd dgrad'), ('SMALL', 'fwd')),
    'finetail32': (('WIDE', 'fwd'), ('SMALL', 'fwd')),
    'posmajor32': (('WIDE', 'fwd dgrad'), ('SMALL', 'fwd')),
    'pair32': (('WIDE', 'fwd'), ('SMALL', 'fwd')),
    'dense32': (('WIDE', 'fwd wgrad'), ('SMALL', 'fwd')),
    'stem32': (('WIDE', 'fwd'), ('SMALL', 'fwd')),
    'stem_wgrad32': (('AUTO', 'wgrad'),),
    'wghalo32': (('WIDE', 'wgrad'),),
    'crop32': (('WIDE', 'dgrad'),),
    'bnsums': (('WIDE', 'dgrad bf16'),),
    'conv16': (('WIDE', 'fwd dgrad wgrad bf16'), ('SMALL', 'fwd')),
    'halo16': (('WIDE', 'fwd dgrad bf16'), ('SMALL', 'fwd')),
    'pw16': (('WIDE', 'fwd bf16'), ('SMALL', 'fwd')),
    'affine16': (('WIDE', 'fwd wgrad'),),
    'splitk16': (('WIDE', 'fwd dgrad bf16'), ('SMALL', 'fwd')),
    'pair16': (('WIDE', 'fwd bf16'), ('SMALL', 'fwd')),
    'stem16': (('WIDE', 'fwd bf16'), ('SMALL', 'fwd')),
    'stem_wgrad16': (('AUTO', 'wgrad'),),
    'wghalo16': (('WIDE', 'wgrad'),),
    'slab16': (('WIDE', 'wgrad'),),
}


STATS_KIND = {'pw16': 'plain', 'pair32': 'plain', 'pair16': 'plain', 'affine16': 'plain'}     # every other family: 'bias'


def affine_case(geom):
    """the case of LOANS_F_AFFINE_IN at a geometry: (the base case whose x the kernel reads, the case whose x is the operand the
    convolution contracts, scale, shift).  With integer x up to 32, scale in {0.5, 1, 2, -1} and integer shift up to 16 the affine
    value is itself a bf16 value (at most 80, in halves): the rounding of the operand on load is written into the reference but
    NOT exercised by these cases -- what they hold the kernel to is the affine arithmetic, the ReLU and the contraction."""
    geom = tuple(geom)
    key = ('affine', geom)
    if key not in _cases:
        base = case(geom)
        scale, shift = affine_table(geom[1], geom)
        a = affine_operand(base.x, scale, shift)
        _cases[key] = (base, Case(geom, 'WIDE', base.scale, x=a.astype(np.float32), tag='AFFINE'), scale, shift)
    return _cases[key]


def family_cases(fam, g, profile):
    """the Case objects a family's GPU tests make of one entry of its geometry list"""
    g = tuple(g)
    if fam == 'crop32':
        B, H, W = g
        return [case((B, 3, H, W, 128, 3, 1, 1), profile), case((B, 3, H, W, 128, 4, 2, 1), profile)]
    if fam in ('pair32', 'pair16'):
        return list(pair_cases(g, profile))
    if fam == 'slab16':
        g = g[:8]
    if profile == 'AUTO':
        profile = wgrad_profile(g)
    if fam == 'affine16':
        return [affine_case(g)[1]]
    return [case(g, profile)]


def grid():
    """every (family, geometry, profile, uses) the GPU tests generate"""
    out = []
    for fam, geoms in geometries().items():
        for profile, uses in USES.get(fam, ()):
            done = []
            for g in geoms:
                key = tuple(g)[:8] if fam == 'slab16' else tuple(g)
                if key not in done:
                    done.append(key)
                    out.append((fam, tuple(g), profile, uses))
    return out


# ---------------------------------------------------------------------------------------------------------------- launches
# The epilogue sets of one convolution through loans_amd.ops, shared by the fp32 and the bf16-storage files: the storage type
# of the device tensors selects the arm, the comparison is the same -- torch.equal by value against the case's reference.
def geometry(ops, c, cpad=None):
    B, Cin, H, W, Cout, k, s, p = c.geom
    return ops.ConvGeometry(B, H, W, cpad or Cin, Cout, k, s, p)


def run_fprop(ops, c, d, geo, tile, what, sumsq_rtol=1e-5, relu_in=True):
    """bias + statistics; relu(in) + addend; addend; bias + addend (the epilogue order: one rounding after the addend)"""
    st = ops.stats_buffer(geo.Cout, 'cuda')
    assert_out(c, ops.conv_fprop(d['x'], d['w'], geo, bias=d['bias'], stats=st, tile=tile), 'bias', what)
    assert_stats(c, st, what, sumsq_rtol=sumsq_rtol)
    assert_out(c, ops.conv_fprop(d['x'], d['w'], geo, relu_in=relu_in, addend=d['add_y'], tile=tile), 'relu_add' if relu_in else 'add', what)
    assert_out(c, ops.conv_fprop(d['x'], d['w'], geo, addend=d['add_y'], tile=tile), 'add', what)
    assert_out(c, ops.conv_fprop(d['x'], d['w'], geo, bias=d['bias'], addend=d['add_y'], tile=tile), 'bias_add', what)


def run_fprop_small(ops, c, d, geo, tile, what):
    """SMALL: no output rounds, the sum and the sum of squares of LOANS_F_STATS are exact"""
    assert c.profile == 'SMALL'
    st = ops.stats_buffer(geo.Cout, 'cuda')
    assert_out(c, ops.conv_fprop(d['x'], d['w'], geo, bias=d['bias'], stats=st, tile=tile), 'bias', what)
    assert_stats(c, st, what)


def run_dgrad(ops, c, d, geo, tile, what, in_place=True):
    """plain, mask_ref, addend, mask_ref + addend, addend_mask_ref, in-place accumulate; a strided 1 x 1 (tap-less classes)
    takes the plain addend only, as in the existing tests"""
    n = c.geom[1]
    assert_out(c, ops.conv_dgrad(d['gy'], d['w'], geo, tile=tile), 'gx', what, n)
    assert_out(c, ops.conv_dgrad(d['gy'], d['w'], geo, addend=d['add_x'], tile=tile), 'gx_add', what, n)
    if in_place:
        acc = d['add_x'].clone()
        ops.conv_dgrad(d['gy'], d['w'], geo, out=acc, addend=acc, tile=tile)
        assert_out(c, acc, 'gx_add', what + ' in place', n)
    if geo.dgrad_has_empty_class:
        return
    assert_out(c, ops.conv_dgrad(d['gy'], d['w'], geo, mask_ref=d['ref_x'], tile=tile), 'gx_mask', what, n)
    assert_out(c, ops.conv_dgrad(d['gy'], d['w'], geo, mask_ref=d['ref_x'], addend=d['add_x'], tile=tile), 'gx_mask_add', what, n)
    assert_out(c, ops.conv_dgrad(d['gy'], d['w'], geo, addend=d['add_x'], addend_mask_ref=d['ref_x'], tile=tile), 'gx_addmask', what, n)


def run_wgrad(ops, c, d, geo, tile, splits, what, relu_in=False, direct=True, in_affine=None, want=None):
    """dw starts as a non-zero integer tensor: the result is that plus the exact gradient"""
    dw = d['dw0'].clone()
    if direct:
        ops._conv_wgrad(d['x'], d['gy'], dw, geo, relu_in, splits, tile, in_affine=in_affine)
    else:
        ops.conv_wgrad(d['x'], d['gy'], dw, geo, relu_in=relu_in, splits=splits, tile=tile)
        ops.join_side_stream()
    if want is None:
        want = c.gw_relu() if relu_in else c.gw()
    assert_same(dw, want + c.dw0, '%s wgrad relu_in=%d splits=%d' % (what, relu_in, splits), channels=c.geom[1])


def bn_state(ops, C_, mean, rstd, scale, shift):
    """a BNState whose table holds the chosen values (not bn_finalize's)"""
    st = ops.BNState(C_, 'cuda')
    for t, v in ((st.mean, mean), (st.rstd, rstd), (st.scale, scale), (st.shift, shift)):
        t.copy_(up(v))
    return st


def run_bn_sums(ops, c, d, geo, tile, what):
    """LOANS_F_BNSUMS: g is stored unmasked; the sums take the tensor as STORED -- on bf16 tensors the ROUNDED g"""
    import torch
    bf16 = d['gy'].dtype == torch.bfloat16
    y, mean, rstd, scale, shift = bnsums_table(c.geom)
    st = bn_state(ops, c.geom[1], mean, rstd, scale, shift)
    yd = up(nhwc(y), bf16)
    assert ops.bn_sums_ok(geo, yd)
    g, sums = ops.conv_dgrad(d['gy'], d['w'], geo, tile=tile, bn_sums=(yd, st))
    assert_out(c, g, 'gx', what + ' bn_sums')
    s1, s2, bound = bnsums_ref(c.want('gx', bf16), y, mean, scale, shift)
    assert bound < TWO24
    got = sums.sum(dim=0).cpu().numpy()
    for i, (name, ref) in enumerate((('sum g m', s1), ('sum g m (y - mean)', s2))):
        bad = np.flatnonzero(got[i] != ref)
        assert bad.size == 0, '%s: %s of %d channels differs, first %d: got %r exact %r' % (what, name, bad.size, bad[0], got[i][bad[0]], ref[bad[0]])


def dense_device(ops, c, geo, bf16_frames=False):
    """the padded packed-RGB frame buffer and the window-padded weights / start gradient of a dense-row stem geometry"""
    B, Cin, H, W, Cout, k, s, p = c.geom
    xp = np.zeros((B, geo.Hp, geo.Wp, 3), np.float32)
    xp[:, p:p + H, p:p + W] = c.x.transpose(0, 2, 3, 1)
    wp = np.zeros((Cout, k, geo.kwp, 3), np.float32)
    wp[:, :, :k] = c.w.transpose(0, 2, 3, 1)
    dw0 = np.zeros_like(wp)
    dw0[:, :, :k] = c.dw0.transpose(0, 2, 3, 1)
    return dict(x=up(xp, bf16_frames), w=up(wp), bias=up(c.bias), dw0=up(dw0))


def assert_dense_dw(c, dw, want, what, pad_want=0.0):
    """a dense-layout weight gradient [Cout][k][kwp][3]: the real columns against `want` (OIHW), the window-padding columns"""
    k = c.geom[5]
    assert_same(dw[:, :, :k], want, what)
    assert bool((dw[:, :, k:] == pad_want).all()), what + ': window-padding columns'
