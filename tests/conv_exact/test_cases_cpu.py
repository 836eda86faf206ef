"""CPU: the exact convolution cases of tests/conv_exact/cases.py are what they claim to be.  Every condition of that module
on every case the GPU tests generate; an fp32 NumPy restatement of the contraction in other K orders that must reproduce
the reference EXACTLY (if it ever fails, the inputs are wrong, not a kernel); and a negative control against each
alternative the GPU assertions are meant to catch -- a reference built under that alternative differs from the true one,
so those assertions can fail."""
import numpy as np
import pytest

from tests.conv_exact import cases as X

GRID = X.grid()
BF16_FWD = ('conv16', 'halo16', 'pw16', 'splitk16', 'pair16', 'stem16')

def _id(p):
    fam, g, profile, uses = p
    return '%s-%s-%s' % (fam, X.gid(g), profile)


@pytest.mark.parametrize("entry", GRID, ids=_id)
def test_conditions(entry):
    fam, g, profile, uses = entry
    for c in X.family_cases(fam, g, profile):
        for t in (c.x / c.unit, c.w, c.bias, c.gy, c.add_y, c.add_x, c.ref_x, c.dw0):
            assert X.is_integer(t) and np.abs(t).max() <= 256, 'integers (the BN-on-load operand: halves), every one a bf16 value'
        assert np.array_equal(X.round_bf16(c.x), c.x)
        assert c.scale in (1, 2, 4) if c.profile == 'WIDE' else c.scale in (0.5, 1)
        if c.scale == 0.5:
            assert not X.Case(c.geom, 'SMALL', 1).small_needs_no_rounding()
        assert c.scale == X.wide_scale(c.geom) or c.profile != 'WIDE' or fam in ('pair32', 'pair16')
        # every mask tensor -- and x, the operand of LOANS_F_RELU_IN -- holds +0.0, -0.0, positives and negatives
        for t in (c.ref_x,) if fam == 'affine16' else (c.ref_x, c.x):
            zero = t == 0
            assert (zero & ~np.signbit(t)).any() and (zero & np.signbit(t)).any() and (t > 0).any() and (t < 0).any()
        if 'fwd' in uses:
            assert c.bound_fwd() < X.TWO24                                    # exactness, any order, any split
            for kind in ('plain', 'bias', 'relu_add', 'bias_add'):
                assert X.is_integer(c.exact(kind) / c.unit)
            # the sum condition, for the output the family's GPU calls take LOANS_F_STATS of: it holds on every case that
            # cases.SUM_NOT_EXACT does not list, and on none that it lists
            kind = X.STATS_KIND.get(fam, 'bias')
            assert c.stats_exact(kind) == X.sum_is_exact(c), np.abs(c.exact(kind)).sum(axis=(0, 2, 3)).max()
            if c.profile == 'SMALL':
                assert c.stats_exact(kind) and c.sumsq_exact(kind)
                assert c.small_needs_no_rounding()
            else:
                if fam in BF16_FWD:
                    assert c.visible('bias'), X.rounding_profile(c.exact('bias'))
                    if fam != 'stem16':
                        assert c.visible('relu_add') and c.visible('bias_add')
        if 'dgrad' in uses:
            assert c.bound_dgrad() < X.TWO24
            if 'bf16' in uses and c.every_pixel_has_a_tap():
                assert c.visible('gx'), X.rounding_profile(c.exact('gx'))      # (a masked gradient is mostly the addend alone: not held to it)
        if 'wgrad' in uses:
            assert c.bound_wgrad() < X.TWO24
            assert X.is_integer(c.gw() / c.unit)
        if fam == 'bnsums':
            y, mean, rstd, scale, shift = X.bnsums_table(c.geom)
            s1, s2, bound = X.bnsums_ref(X.round_bf16(c.gx()), y, mean, scale, shift)
            assert bound < X.TWO24 and X.bnsums_ref(c.gx(), y, mean, scale, shift)[2] < X.TWO24
            m = (y * scale[None, :, None, None] + shift[None, :, None, None]) > 0
            assert m.any() and not m.all()
        if fam == 'affine16':
            base, ca, scale, shift = X.affine_case(c.geom)
            assert ca is c and c.tag == 'AFFINE'
            assert (c.x == 0).mean() > 0.1 and set(np.unique(scale)) == set(X.AFFINE_SCALES) and X.is_integer(shift)
            pre = base.x.astype(np.float64) * scale[None, :, None, None] + shift[None, :, None, None]
            # (the affine value is a bf16 value on these tables: the operand's rounding on load is not exercised, cases.affine_case)
            assert np.array_equal(X.round_bf16(np.maximum(pre, 0)), np.maximum(pre, 0)) and np.array_equal(np.maximum(pre, 0), c.x)


@pytest.mark.parametrize("geom", X.geometries()['compute16'], ids=X.gid)
def test_round_in_conditions(geom):
    """ROUND_IN (bf16 compute on fp32 tensors): the operand rounding itself is exercised, the rounded operands stay exact"""
    c = X.case(geom, 'WIDE', round_in=True)
    assert (np.abs(c.x_raw) >= 256).all() and (np.abs(c.x_raw) < 1024).all() and X.is_integer(c.x_raw)
    assert (c.x != c.x_raw).mean() > 0.3 and X.is_tie(c.x_raw).mean() > 0.1
    assert c.bound_fwd() < X.TWO24 and c.bound_wgrad() < X.TWO24
    assert c.tag == 'ROUND_IN' and X.sum_is_exact(c) and c.stats_exact('plain')         # the statistics of every ROUND_IN call are exact
    assert np.abs(c.w).max() <= X.ROUND_IN_W
    gy = X.O.round_bf16(c.gy_raw)
    s, p = geom[6], geom[7]
    bound = X.O.conv2d_bwd(c.x.shape, c.col(), np.abs(c.w).astype(np.float64), np.abs(gy).astype(np.float64), s, p, False)[0]
    assert bound.max() < X.TWO24 and X.is_integer(c.gx(gy=gy))


@pytest.mark.parametrize("entry", [e for e in GRID if 'fwd' in e[3]], ids=_id)
def test_any_order_of_k_gives_the_reference_in_fp32(entry):
    fam, g, profile, uses = entry
    rng = np.random.RandomState(X._seed('orders', g, profile))
    for c in X.family_cases(fam, g, profile):
        want = c.conv()
        for how in ('perm', ('slices', 2), ('slices', 7), ('slices', 16), 'chunks'):
            got = X.contract_f32(c, how, rng)
            assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), want), how


def _border_product(c):
    """(output index, product) of one non-zero x * w term of a border output pixel of image 0 (a 1 x 1 convolution with
    padding has no tap there: then of the first pixel that has one)"""
    B, Cin, H, W, Cout, k, s, p = c.geom
    order = sorted(((oy, ox) for oy in range(c.Ho) for ox in range(c.Wo)),
                   key=lambda q: not (q[0] in (0, c.Ho - 1) or q[1] in (0, c.Wo - 1)))
    for oy, ox in order:
        if True:
            for ky in range(k):
                for kx in range(k):
                    iy, ix = oy * s + ky - p, ox * s + kx - p
                    if 0 <= iy < H and 0 <= ix < W:
                        prod = c.x[0, :, iy, ix].astype(np.float64)[None, :] * c.w[:, :, ky, kx]
                        if prod.any():
                            o, ci = np.argwhere(prod)[0]
                            return (0, o, oy, ox), float(prod[o, ci])
    raise AssertionError('no non-zero product at a border pixel')


@pytest.mark.parametrize("entry", [e for e in GRID if e[2] == 'WIDE' and 'fwd' in e[3] and e[0] != 'affine16'], ids=_id)
def test_negative_controls(entry):
    """a reference built under each alternative differs from the true one in at least one element"""
    fam, g, profile, uses = entry
    c = X.family_cases(fam, g, profile)[0]
    e = c.exact('bias_add')
    true = X.round_bf16(e)
    # asserted for every family that compares a bf16 forward output; the fp32-only families run them where the rounding shows
    # (one position-major geometry, a 1 x 1 with padding whose outputs are mostly the bias alone, never shows it)
    if fam in BF16_FWD or c.visible('bias'):
        assert not np.array_equal(X.trunc_bf16(e), true), 'truncation'
        assert not np.array_equal(X.half_away_bf16(e), true), 'round half away'
        twice = X.round_bf16(X.round_bf16(c.exact('bias')) + c.add_y)
        assert not np.array_equal(twice, true), 'rounding after the bias and again after the addend'
        eb = c.exact('bias')
        assert not np.array_equal(X.round_bf16(eb).sum(axis=(0, 2, 3)), eb.sum(axis=(0, 2, 3))), 'statistics from rounded outputs'
    idx, prod = _border_product(c)
    eb = c.exact('bias')
    for alt in (-prod, prod):                   # one product removed at a border pixel / one product doubled
        wrong = eb.copy()
        wrong[idx] += alt
        assert not np.array_equal(wrong, eb)
        assert not np.array_equal(wrong.sum(axis=(0, 2, 3)), eb.sum(axis=(0, 2, 3)))


@pytest.mark.parametrize("geom", X.geometries()['bnsums'], ids=X.gid)
def test_negative_control_bnsums_from_unrounded_g(geom):
    c = X.case(geom, 'WIDE')
    y, mean, rstd, scale, shift = X.bnsums_table(geom)
    r1, r2, _ = X.bnsums_ref(X.round_bf16(c.gx()), y, mean, scale, shift)
    u1, u2, _ = X.bnsums_ref(c.gx(), y, mean, scale, shift)
    assert (r1 != u1).mean() >= 0.5 and (r2 != u2).mean() >= 0.5


def test_bf16_forms():
    v = np.array([257.0, 259.0, -257.0, -259.0, 256.0, 258.0, 513.0, 514.0, 518.0, 3.0], np.float64)
    assert X.round_bf16(v).tolist() == [256.0, 260.0, -256.0, -260.0, 256.0, 258.0, 512.0, 512.0, 520.0, 3.0]
    assert X.trunc_bf16(v).tolist() == [256.0, 258.0, -256.0, -258.0, 256.0, 258.0, 512.0, 512.0, 516.0, 3.0]
    assert X.half_away_bf16(v).tolist() == [258.0, 260.0, -258.0, -260.0, 256.0, 258.0, 512.0, 516.0, 520.0, 3.0]
    assert X.is_tie(v).tolist() == [True, True, True, True, False, False, False, True, True, False]
