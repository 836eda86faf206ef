"""No GPU: the linear rule's rates over the models' residual units, the reference of tests/imagenet_droppath/reference.py against
the oracle's units (r = 1) and against finite differences, ``DropPath``'s draw stream, and the trainer's options."""
import numpy as np
import pytest

from loans_amd.functions import drop_path as DP
from loans_amd.runtime import checkpoint
from oracle import model as M
from tests.imagenet_droppath import reference as D


# ---- the rates -------------------------------------------------------------------------------------------------------------------
def test_linear_rule():
    assert DP.linear_rates(0.3, 1) == [0.3]
    assert DP.linear_rates(0.0, 5) == [0.0] * 5
    for L in (2, 8, 12, 16):
        rates = DP.linear_rates(0.2, L)
        assert len(rates) == L and rates[0] == 0.0 and rates[-1] == 0.2
        assert rates == [0.2 * l / (L - 1) for l in range(L)]
    for bad in (-0.1, 1.0, 1.5, float('nan')):
        with pytest.raises(ValueError):
            DP.linear_rates(bad, 8)


def _units(model):
    return [u for stage in model.drop_path_stages() for u in DP.stage_units(stage)]


def test_rates_and_slots_of_the_models():
    import loans_amd
    from loans_amd.sheep.resnet import BasicA, BasicB, ResNet
    np.random.seed(0)
    net = ResNet(18)
    dp = net.set_drop_path(0.1, seed=0)
    units = _units(net)
    assert len(units) == 8 and dp.rates == [0.1 * l / 7 for l in range(8)] and dp.active == list(range(1, 8))
    assert [type(u) for u in units] == [BasicA, BasicB] * 4
    assert [u.__dict__['drop_slot'] for u in units] == list(range(8)) and all(u.__dict__['drop_path'] is dp for u in units)
    assert units[0] is net.res2[0] and units[3] is net.res3[1] and units[7] is net.res5[1]
    assert net.set_drop_path(0) is None and net.drop_path is None and all(u.__dict__['drop_path'] is None for u in units)
    assert len(ResNet(20).set_drop_path(0.1).rates) == 12
    # the 20-layer localizer: the backbone's eight units, then res6 and res7; the localizer owns the table, not its backbone
    loc = loans_amd.SheepLocalizer((75, 75))
    loc.feature_extractor.set_drop_path(0.3)
    dp = loc.set_drop_path(0.2, seed=1)
    units = _units(loc)
    assert len(units) == 12 and dp.rates == [0.2 * l / 11 for l in range(12)]
    assert units[8] is loc.res6[0] and units[11] is loc.res7[1] and units[11].__dict__['drop_slot'] == 11
    assert loc.drop_path is dp and loc.feature_extractor.drop_path is None
    # ... and the other way round: the backbone takes its units back, the localizer's table goes as a whole (res6 / res7 too)
    inner = loc.feature_extractor.set_drop_path(0.1)
    assert loc.drop_path is None and loc.feature_extractor.drop_path is inner and len(inner.rates) == 8
    assert all(u.__dict__['drop_path'] is inner for u in units[:8]) and all(u.__dict__['drop_path'] is None for u in units[8:])
    assert [u.__dict__['drop_slot'] for u in units[:8]] == list(range(8))
    assert len(loans_amd.SheepLocalizer((75, 75), train_imagenet=True).set_drop_path(0.2).rates) == 8


def test_rates_of_resnet50():
    import loans_amd
    np.random.seed(0)
    loc = loans_amd.Resnet50SheepLocalizer((75, 75), train_imagenet=True)
    dp = loc.set_drop_path(0.05, seed=0)
    units = _units(loc)
    fe = loc.feature_extractor
    assert len(units) == 16 and dp.rates == [0.05 * l / 15 for l in range(16)]
    assert units[0] is fe.res2.a and units[2] is fe.res2.b2 and units[3] is fe.res3.a and units[15] is fe.res5.b2
    assert [u.__dict__['drop_slot'] for u in units] == list(range(16))
    # the extractor has the surface too; setting it there takes the units from the localizer, which stops drawing
    inner = fe.set_drop_path(0.05)
    assert len(inner.rates) == 16 and loc.drop_path is None and fe.drop_path is inner
    assert all(u.__dict__['drop_path'] is inner for u in units)


# ---- the reference ---------------------------------------------------------------------------------------------------------------
def _tiny_params(rng, ch=4):
    p = {}
    M._basic_block(p, rng, 'u', ch, ch)
    for k in list(p):
        if k.endswith('/gamma'):
            p[k] = 1 + 0.2 * rng.standard_normal(ch)
        elif k.endswith('/beta'):
            p[k] = 0.2 * rng.standard_normal(ch)
    return M.cast_params(p, np.float64)


RES_STAGES = [('u/0/conv1', 'u/0/bn1', 1, 1), ('u/0/conv2', 'u/0/bn2', 1, 1)]


def _make(kind, p, r):
    if kind == 'basic_a':
        return D.DropBasicA(p, 'u/0', 1, True, r), M._BasicA(p, 'u/0', 1, True)
    if kind == 'basic_b':
        return D.DropBasicB(p, 'u/1', True, r), M._BasicB(p, 'u/1', True)
    if kind == 'res_identity':
        return D.DropResUnit(p, RES_STAGES, None, True, r), M._ResUnit(p, RES_STAGES, None, True)
    sc = ('u/0/conv3', 'u/0/bn3', 1, 1)
    return D.DropResUnit(p, RES_STAGES, sc, True, r), M._ResUnit(p, RES_STAGES, sc, True)


KINDS = ('basic_a', 'basic_b', 'res_identity', 'res_shortcut')


@pytest.mark.parametrize('kind', KINDS)
def test_reference_with_all_ones_is_the_oracles_unit_exactly(kind):
    rng = np.random.RandomState(1)
    x, gy = rng.standard_normal((3, 4, 5, 5)), rng.standard_normal((3, 4, 5, 5))
    outs = []
    for i in range(2):
        unit = _make(kind, _tiny_params(np.random.RandomState(2)), np.ones(3, np.float32))[i]
        grads = {}
        out = unit.fwd(x)
        outs.append((out, unit.bwd(gy, grads), grads))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    assert set(outs[0][2]) == set(outs[1][2]) and all(np.array_equal(outs[0][2][k], outs[1][2][k]) for k in outs[0][2])
    # ... and in test mode r is ignored
    p = _tiny_params(np.random.RandomState(2))
    assert np.array_equal(D.DropBasicB(p, 'u/1', False, np.zeros(3, np.float32)).fwd(x), M._BasicB(p, 'u/1', False).fwd(x))


@pytest.mark.parametrize('kind', KINDS)
def test_reference_gradients_against_finite_differences(kind):
    """float64, B = 3, 4 channels, 5 x 5, the middle sample dropped at p = 0.5: L = sum(out * gy); central differences with
    h = 1e-6 are exact to ~1e-9 relative away from a ReLU kink, the comparison allows 1e-6 of the gradient's largest entry"""
    rng = np.random.RandomState(3)
    x, gy = rng.standard_normal((3, 4, 5, 5)), rng.standard_normal((3, 4, 5, 5))
    r = np.array([1, 0, 1], np.float32) * D.keep_factor(0.5)
    base = _tiny_params(np.random.RandomState(4))

    def loss(p, xv):
        p = {k: v.copy() for k, v in p.items()}
        return float((_make(kind, p, r)[0].fwd(xv) * gy).sum())

    unit = _make(kind, {k: v.copy() for k, v in base.items()}, r)[0]
    grads = {}
    out = unit.fwd(x)
    gx = unit.bwd(gy, grads)
    if kind in ('basic_b', 'res_identity'):
        assert np.array_equal(out[1], np.maximum(x[1], 0))         # the dropped sample is its shortcut
    h = 1e-6

    def numeric(get, n):
        g = np.zeros(n)
        for i in range(n):
            lo, hi = get(i, -h), get(i, h)
            g[i] = (hi - lo) / (2 * h)
        return g

    def at_x(i, d):
        xv = x.copy()
        xv.reshape(-1)[i] += d
        return loss(base, xv)
    num = numeric(at_x, x.size).reshape(x.shape)
    assert np.abs(num - gx).max() <= 1e-6 * np.abs(gx).max(), 'gx'
    assert np.abs(gx[1]).max() > 0          # the dropped sample still takes a gradient: through the shortcut and the statistics
    checked = 0
    for key in sorted(grads):
        if not key.endswith(('/gamma', '/beta')):
            continue

        def at_p(i, d, key=key):
            p = {k: v.copy() for k, v in base.items()}
            p[key][i] += d
            return loss(p, x)
        num = numeric(at_p, base[key].size)
        assert np.abs(num - grads[key]).max() <= 1e-6 * max(np.abs(grads[key]).max(), 1.0), key
        checked += 1
    assert checked == (6 if kind in ('basic_a', 'res_shortcut') else 4)


def test_junction_reference_is_the_units_junction():
    """the NHWC junction functions the kernel tests use give what the unit does at its last BN, for the statistics of x"""
    rng = np.random.RandomState(5)
    B, P, C_ = 3, 10, 8
    x, res, gy = (rng.standard_normal((B, P, C_)) for _ in range(3))
    gamma, beta = 1 + 0.1 * rng.standard_normal(C_), 0.1 * rng.standard_normal(C_)
    r = np.array([2.0, 0.0, 2.0])
    mean, var = x.mean(axis=(0, 1)), x.var(axis=(0, 1))
    rstd = (var + 2e-5) ** -0.5
    st = dict(mean=mean, rstd=rstd, scale=gamma * rstd, shift=beta - mean * gamma * rstd)
    out = D.junction_fwd(x, st, r, res)
    a = gamma * (x - mean) * rstd + beta
    want = np.maximum(r[:, None, None] * a + res, 0)
    assert np.allclose(out, want, rtol=1e-12, atol=1e-12) and np.array_equal(out[1], np.maximum(res[1], 0))
    bits = D.bits_of(out)
    assert np.array_equal(D.mask_of(bits, out.shape), out > 0)
    got = D.junction_bwd(gy, out > 0, r, x, st, gamma, np.zeros(C_), np.zeros(C_))
    # the oracle's BN backward fed r g
    from oracle import chainer_ops as C
    g = (gy * (out > 0) * r[:, None, None]).reshape(B * P, C_, 1, 1)
    xhat = ((x - mean) * rstd).reshape(B * P, C_, 1, 1)
    gx, gg, gb = C.bn_bwd((xhat, rstd), gamma, g)
    assert np.allclose(got['gx'].reshape(B * P, C_), gx[:, :, 0, 0], rtol=1e-10, atol=1e-12)
    assert np.allclose(got['ggamma'], gg) and np.allclose(got['gbeta'], gb)


# ---- the draws -------------------------------------------------------------------------------------------------------------------
def test_draws_are_reproducible_and_ranks_differ():
    a, b = DP.DropPath(0.5, 8, seed=3), DP.DropPath(0.5, 8, seed=3)
    first = [a.sample(16) for _ in range(3)]
    assert all(np.array_equal(x, b.sample(16)) for x in first)
    assert first[0].shape == (7, 16) and first[0].dtype == np.float32
    rank1 = DP.DropPath(0.5, 8, seed=3 + 7919)
    assert not np.array_equal(rank1.sample(16), first[0])
    # every value is 0 or fl(1 / (1 - p_l))
    for i, l in enumerate(a.active):
        want = np.float32(1.0 / (1.0 - a.rates[l]))
        assert want == D.keep_factor(a.rates[l])
        for t in first:
            assert set(np.unique(t[i])) <= {np.float32(0), want}
    assert DP.DropPath(0.0, 8, seed=1).active == [] and DP.DropPath(0.0, 8).draw(4, None) is None


def test_stream_state_round_trips_mid_run():
    a = DP.DropPath(0.3, 16, seed=5)
    for _ in range(3):
        a.sample(8)
    arrays = {}
    packed = checkpoint.pack(a.state_dict(), 'rank', arrays)
    state = checkpoint.unpack(packed, arrays)
    want = [a.sample(8) for _ in range(3)]
    b = DP.DropPath(0.3, 16, seed=99)
    b.load_state_dict(state)
    assert all(np.array_equal(w, b.sample(8)) for w in want)
    with pytest.raises(ValueError, match='drop path'):
        DP.DropPath(0.2, 16).load_state_dict(state)


def test_kept_share_over_a_seeded_run():
    """200 draws of 32 samples, seed 0: the kept share of every unit within 4 binomial standard deviations of 1 - p_l"""
    dp = DP.DropPath(0.5, 16, seed=0)
    n, kept = 0, np.zeros(len(dp.active))
    for _ in range(200):
        t = dp.sample(32)
        kept += (t > 0).sum(axis=1)
        n += 32
    for i, l in enumerate(dp.active):
        q = 1.0 - dp.rates[l]
        assert abs(kept[i] / n - q) <= 4 * np.sqrt(q * (1 - q) / n), (l, kept[i] / n, q)


# ---- the trainer's options -------------------------------------------------------------------------------------------------------
NEW = ('drop_path', 'drop_path_seed')


def test_the_options_parse_and_leave_the_default_namespace_alone():
    import train_imagenet as T
    bare = T.parse_args([])
    assert not set(NEW) & set(vars(bare)) and (bare.drop_path, bare.drop_path_seed) == (0.0, None)
    args = T.parse_args(['--drop-path', '0.05', '--drop-path-seed', '3'])
    assert (args.drop_path, args.drop_path_seed) == (0.05, 3)
    assert set(vars(args)) == set(vars(bare)) | set(NEW)
    assert set(T.Arguments._DROP) == set(NEW) and set(NEW) <= set(T.RESUME_FIXED)
    for ok in ('0', '0.999'):
        T.parse_args(['--drop-path', ok])
    # with every optimiser, storage type and loss
    T.parse_args(['--drop-path', '0.1', '--optimizer', 'lamb', '--dtype', 'bf16', '--loss', 'bce', '--gpus', '2'])


@pytest.mark.parametrize('value', ['-0.1', '1', '1.5', 'nan'])
def test_a_rate_outside_the_unit_interval_is_refused(value, capsys):
    import train_imagenet as T
    with pytest.raises(SystemExit):
        T.parse_args(['--drop-path=' + value])
    assert '--drop-path' in capsys.readouterr().err
    args = T.Arguments()
    args.drop_path = float(value)
    with pytest.raises(ValueError, match='--drop-path'):
        T.check_drop_arguments(args)


def test_the_options_are_in_the_help_text(capsys):
    import train_imagenet as T
    with pytest.raises(SystemExit):
        T.parse_args(['--help'])
    text = capsys.readouterr().out
    assert '--drop-path P' in text and '--drop-path-seed' in text and 'stochastic depth' in text
    assert '--drop-path' in T.__doc__ and '--drop-path-seed' in T.__doc__


def test_resume_tables_and_the_argument_record():
    import train_imagenet as T
    assert T.RESUME_DEFAULTS_DROP == {'drop_path': 0.0, 'drop_path_seed': None}
    assert T.RESUME_DEFAULTS_WITH_DROP == dict(T.RESUME_DEFAULTS_WITH_RA, **T.RESUME_DEFAULTS_DROP)
    assert not set(NEW) & set(T.RESUME_DEFAULTS_WITH_RA)                       # the older tables are what they were
    fixed = [k for k in T.RESUME_FIXED if k != 'gpus']
    # a checkpoint from before the options resumes at their defaults only
    args = T.parse_args([])
    saved = {k: v for k, v in checkpoint.plain_arguments(args).items() if k not in NEW}
    assert checkpoint.check_arguments(saved, args, fixed, checkpoint.SILENT, T.RESUME_DEFAULTS_WITH_DROP) == []
    for extra, name in ((['--drop-path', '0.1'], 'drop_path'), (['--drop-path-seed', '1'], 'drop_path_seed')):
        with pytest.raises(ValueError, match=name):
            checkpoint.check_arguments(saved, T.parse_args(extra), fixed, checkpoint.SILENT, T.RESUME_DEFAULTS_WITH_DROP)
    # the record round-trips them, and a resume that changes either is refused
    given = T.parse_args(['--drop-path', '0.3', '--drop-path-seed', '3'])
    record = checkpoint._plain(checkpoint.plain_arguments(given))
    assert (record['drop_path'], record['drop_path_seed']) == (0.3, 3)
    assert checkpoint.check_arguments(record, given, fixed, checkpoint.SILENT, T.RESUME_DEFAULTS_WITH_DROP) == []
    for other in (['--drop-path', '0.2', '--drop-path-seed', '3'], ['--drop-path', '0.3', '--drop-path-seed', '4'], []):
        with pytest.raises(ValueError, match='drop_path'):
            checkpoint.check_arguments(record, T.parse_args(other), fixed, checkpoint.SILENT, T.RESUME_DEFAULTS_WITH_DROP)
