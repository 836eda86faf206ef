"""No GPU: the regime table and the tables of the LARS case grid, ``lars_segments``, the NumPy restatement of the kernels inside the
derived bounds on the whole grid (tests/imagenet_lars/cases.py) before any GPU run, and the trainer's new options."""
import numpy as np
import pytest

from tests.imagenet_lars import cases as A


# ---- the grid ---------------------------------------------------------------------------------------------------------------------
def test_regime_table_is_what_the_constants_give():
    from loans_amd import _lib, ops
    assert (A.UNIT, A.MAX_SEGMENTS) == (_lib.LARS_UNIT, _lib.LARS_MAX_SEGMENTS) == (ops.LARS_UNIT, ops.LARS_MAX_SEGMENTS) == (4096, 1024)
    for n, want in A.REGIMES.items():
        assert A.regime(n) == want, n
    assert set(A.REGIMES) == {1, 3, 4, 5, 64, A.UNIT - 1, A.UNIT, A.UNIT + 1, 2 * A.UNIT + 3}
    for name, (n, ends, flags) in A.TABLES.items():
        assert ends[-1] == n and len(ends) == len(flags) <= A.MAX_SEGMENTS and all(e % 4 == 0 for e in ends[:-1]) and sorted(set(ends)) == ends, name
        first, units = A.first_units(ends)
        got_first, got_units = ops.lars_first_units(ends)
        assert got_first.tolist() == first and got_units == units, name
    assert len(A.RESNET_SHAPES) == 161 and sum(len(s) <= 1 for s in A.RESNET_SHAPES) == 107
    sizes = A.arena_layout(A.RESNET_SHAPES)[0]
    assert any(n % 8 == 4 for n in sizes) and any(n % 4 for n in sizes)
    assert A.first_units(A.TABLES['many'][1])[1] > A.GRID_CAP
    n, ends, flags = A.TABLES['kinds']
    assert n % 4 == 3 and {(k, f) for k, f in zip(A.kinds_of(20, 'kinds'), flags)} == {(k, f) for k in A.KINDS for f in range(4)}
    assert set(A.kinds_of(len(A.TABLES['resnet'][1]), 'resnet')) == set(A.KINDS)
    assert {gs for _, gs, _ in A.GRID} == set(A.GRAD_SCALES) and {wd for _, _, wd in A.GRID} == set(A.DECAYS)
    assert {name for name, _, _ in A.GRID} == set(A.TABLES)
    p, g, v = A.make('kinds')
    assert np.isnan(p[n:]).all() and np.isnan(g[n:]).all() and (v[n:] == A.V_GUARD).all() and len(p) == n + A.GUARD
    with np.errstate(all='ignore'):
        lo = 0
        for hi, kind in zip(ends, A.kinds_of(20, 'kinds')):      # the fp32 sum of squares is what the kinds say it is
            s = np.sum(np.square(p[lo:hi]), dtype=np.float32)
            assert {'tiny': s == 0, 'huge': np.isinf(s), 'zero_w': s == 0}.get(kind, np.isfinite(s) and s > 0), kind
            assert np.sum(np.square(p[lo:hi].astype(np.float64))) > 0 or kind == 'zero_w'
            lo = hi


# ---- lars_segments ----------------------------------------------------------------------------------------------------------------
def test_lars_segments_of_a_made_up_layout():
    from loans_amd.runtime.optimizers import lars_segments
    shapes = [(6, 3, 2, 2), (6,), (6,), (5, 6), (3, 2), (5,)]
    sizes, offsets, at = A.arena_layout(shapes)
    assert (sizes, offsets, at) == ([72, 6, 6, 30, 6, 5], [0, 72, 80, 88, 120, 128], 136)
    one_d = [len(s) <= 1 for s in shapes]
    ends, flags = lars_segments(sizes, offsets, one_d, one_d, at)
    assert ends.dtype == np.int64 and flags.dtype == np.uint8
    # gamma and beta are one segment; the two adapting neighbours (5, 6) and (3, 2) are not, equal flags or not
    assert ends.tolist() == [72, 88, 120, 128, 136] and flags.tolist() == [0, 3, 0, 0, 3]
    ends, flags = lars_segments(sizes, offsets, [False] * 6, one_d, at)
    assert ends.tolist() == [72, 88, 120, 128, 136] and flags.tolist() == [0, 2, 0, 0, 2]
    # exempt neighbours merge only where the whole flag byte is equal
    ends, flags = lars_segments(sizes, offsets, [False, True, False, False, False, False], one_d, at)
    assert ends.tolist() == [72, 80, 88, 120, 128, 136] and flags.tolist() == [0, 3, 2, 0, 0, 2]
    # nothing adapts: one segment; everything adapts: one per parameter, each running to the next offset (the padding adds zeros)
    assert [a.tolist() for a in lars_segments(sizes, offsets, [True] * 6, [True] * 6, at)] == [[136], [3]]
    assert [a.tolist() for a in lars_segments(sizes, offsets, [False] * 6, [False] * 6, at)] == [offsets[1:] + [at], [0] * 6]
    ends, flags = lars_segments([8, 3], [0, 8], [False, True], [False, True], 11)
    assert ends.tolist() == [8, 11] and flags.tolist() == [0, 3]
    for bad in (([8, 3], [0, 6], [0, 1], [0, 1], 11), ([8, 3], [0, 8], [0, 1], [0, 1], 10), ([8], [8], [0], [0], 16), ([], [], [], [], 0),
                ([8, 3], [0, 8], [0], [0, 1], 11), ([8, 3], [0, 8], [0, 1], [0], 11)):
        with pytest.raises(ValueError):
            lars_segments(*bad)
    # the grid's ResNet-50-like table is what the builder gives
    sizes, offsets, at = A.arena_layout(A.RESNET_SHAPES)
    one_d = [len(s) <= 1 for s in A.RESNET_SHAPES]
    ends, flags = lars_segments(sizes, offsets, one_d, one_d, at)
    assert (at, ends.tolist(), flags.tolist()) == A.TABLES['resnet']


def test_lars_segments_of_resnet50_fit_the_kernel():
    """161 parameters: 54 weights that adapt, a segment each; gamma and beta of one BN merge; fc's bias"""
    import loans_amd
    from loans_amd.runtime.optimizers import lars_segments
    np.random.seed(0)
    model = loans_amd.Classifier(loans_amd.Resnet50SheepLocalizer((75, 75), train_imagenet=True))
    params = list(model.params())
    sizes, offsets, at = A.arena_layout([(p.size,) for p in params])       # (the physical size: conv1 holds a fourth, zero channel)
    one_d = [len(p.logical_shape) <= 1 for p in params]
    ends, flags = lars_segments(sizes, offsets, one_d, one_d, at)
    assert len(ends) <= A.MAX_SEGMENTS and ends[-1] == at
    assert sum(f == 0 for f in flags) == sum(not d for d in one_d)          # every adapting parameter is a segment of its own
    stops = offsets[1:] + [at]
    assert {stop for stop, d in zip(stops, one_d) if not d} <= set(ends.tolist())
    assert all(not (a == b == 3) for a, b in zip(flags, flags[1:]))


# ---- the restatement inside the bounds, on the whole grid -----------------------------------------------------------------------------
_SHARED = {}


def _values(name):
    if name not in _SHARED:
        _SHARED[name] = A.make(name)
    return _SHARED[name]


@pytest.mark.parametrize('name,gs,wd', A.GRID, ids=['%s-gs%g-wd%g' % c for c in A.GRID])
def test_restatement_sits_inside_the_bounds(name, gs, wd):
    n, ends, flags = A.TABLES[name]
    p, g, v = _values(name)
    r32 = A.ratios_numpy(p, g, ends, flags, wd, gs)
    worst = A.check_ratios(r32, p, g, ends, flags, wd, gs)
    assert worst <= 1.0, worst
    h = A.UPDATE_HYPER
    p1, v1 = A.update_numpy(p, g, v, r32, ends, flags, h['lr'], h['momentum'], wd, gs)
    step = A.check_step(p1, v1, p, g, v, ends, flags, h['lr'], h['momentum'], wd, gs)
    assert step <= 1.0, step
    assert not np.array_equal(p1, p[:n])


def test_reference_ratios_are_the_rule():
    """by hand: p = (3, 4) -> W = 5, g = (6, 8) -> |g| = 10"""
    p, g = np.array([3, 4, 0, 0], np.float32), np.array([6, 8, 0, 0], np.float32)
    for flag, wd, gs, want in ((0, 0.0, 1.0, 0.001 * 5 / (10 + 1e-8)), (0, 0.5, 0.5, 0.001 * 5 / (5 + 2.5 + 1e-8)),
                               (1, 0.5, -0.5, 0.001 * 5 / (5 + 1e-8)), (2, 0.5, 1.0, 1.0), (3, 0.5, 1.0, 1.0)):
        assert A.ratios_ref(p, g, [4], [flag], wd, gs)[0][0] == pytest.approx(want, rel=1e-15)
        assert A.ratios_numpy(p, g, [4], [flag], wd, gs)[0] == np.float32(want)
    z = np.zeros(4, np.float32)
    assert A.ratios_ref(z, g, [4], [0], 0.1, 1.0)[0][0] == 1.0 == A.ratios_ref(p, z, [4], [0], 0.1, 1.0)[0][0]
    p1, v1, r = A.lars_ref(p, g, z, [4], [0], 2.0, 0.9, 0.0, 1.0)
    assert np.allclose(p1, p - 2.0 * r[0] * g, rtol=1e-15) and np.allclose(v1, -2.0 * r[0] * g, rtol=1e-15)


# ---- the trainer's options ----------------------------------------------------------------------------------------------------------
def test_parser_takes_and_refuses(capsys):
    import train_imagenet as T
    args = T.parse_args(['--optimizer', 'lars', '--lars-eta', '0.002', '--lars-eps', '1e-6', '--momentum', '0.8', '--weight-decay', '5e-5',
                         '--no-decay-1d'])
    assert (args.optimizer, args.lars_eta, args.lars_eps, args.momentum, args.weight_decay, args.no_decay_1d) == ('lars', 0.002, 1e-6, 0.8, 5e-5, True)
    plain = T.parse_args(['--optimizer', 'lars'])
    assert (plain.lars_eta, plain.lars_eps, plain.no_decay_1d) == (0.001, 1e-8, False) and 'lars_eta' not in vars(plain)
    assert T.resolved_topk(plain) == 5 and T.resolved_topk(T.parse_args(['--optimizer', 'sgd'])) == 5 and T.resolved_topk(T.parse_args([])) is None
    assert T.resolved_topk(T.parse_args(['--optimizer', 'lars', '--topk', '0'])) is None
    for argv, words in ((['--optimizer', 'lars', '--lars-eta', '0'], '--lars-eta must be positive'),
                        (['--optimizer', 'lars', '--lars-eta', '-1'], '--lars-eta must be positive'),
                        (['--optimizer', 'lars', '--lars-eps=-1e-9'], '--lars-eps must not be negative'),
                        (['--optimizer', 'sgd', '--lars-eta', '0.01'], 'belong to --optimizer lars'),
                        (['--lars-eps', '0.01'], 'belong to --optimizer lars'),
                        (['--no-decay-1d'], '--no-decay-1d is built for --optimizer sgd'),
                        (['--no-decay-1d', '--optimizer', 'adam'], '--no-decay-1d is built for --optimizer sgd')):
        with pytest.raises(SystemExit):
            T.parse_args(argv)
        assert words in capsys.readouterr().err, argv
    with pytest.raises(ValueError, match='--no-decay-1d is built for --optimizer sgd'):
        T.check_average_arguments(T.argparse.Namespace(ema_decay=0.0, lr_schedule='step', lr_drop_epochs=[], lr_min=0.0, no_decay_1d=True,
                                                       optimizer='adam'))


def test_resume_table_holds_the_new_defaults():
    import train_imagenet as T
    from loans_amd.runtime import checkpoint
    assert T.RESUME_DEFAULTS_LARS == {'lars_eta': 0.001, 'lars_eps': 1e-8}
    assert T.RESUME_DEFAULTS_WITH_LARS == dict(T.ALL_RESUME_DEFAULTS, **T.RESUME_DEFAULTS_LARS)
    assert 'optimizer' in T.RESUME_FIXED and not set(T.Arguments._LARS) & set(T.RESUME_FIXED)
    fixed = [k for k in T.RESUME_FIXED if k != 'gpus']
    # a checkpoint from before the options existed resumes; an sgd checkpoint does not become a lars run
    args = T.parse_args(['--optimizer', 'sgd'])
    saved = {k: v for k, v in checkpoint.plain_arguments(args).items() if k not in T.Arguments._LARS}
    assert checkpoint.check_arguments(saved, args, fixed, checkpoint.SILENT, T.RESUME_DEFAULTS_WITH_LARS) == []
    with pytest.raises(ValueError, match='optimizer'):
        checkpoint.check_arguments(saved, T.parse_args(['--optimizer', 'lars']), fixed, checkpoint.SILENT, T.RESUME_DEFAULTS_WITH_LARS)
    # eta and eps may change on resume, like --momentum: reported, not refused
    saved = checkpoint.plain_arguments(T.parse_args(['--optimizer', 'lars']))
    later = T.parse_args(['--optimizer', 'lars', '--lars-eta', '0.002', '--lars-eps', '0', '--momentum', '0.8'])
    lines = checkpoint.check_arguments(saved, later, fixed, checkpoint.SILENT, T.RESUME_DEFAULTS_WITH_LARS)
    assert sorted(l.split()[1] for l in lines) == ['lars_eps', 'lars_eta', 'momentum']


def test_optimiser_class_without_a_gpu():
    import loans_amd
    opt = loans_amd.LARS(lr=0.5, weight_decay_rate=5e-5, decay_exempt_1d=True)
    assert vars(opt.hyperparam) == dict(lr=0.5, momentum=0.9, weight_decay_rate=5e-5, eta=0.001, eps=1e-8, decay_exempt_1d=True)
    assert opt._state_names() == ('v',) and opt.lr == 0.5
    opt.lr = 0.25
    assert opt.hyperparam.lr == 0.25
    with pytest.raises(RuntimeError, match='no step'):
        opt.trust_ratios()
