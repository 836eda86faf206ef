"""No GPU: the pure functions of the weight average, the cosine rate and the decay-free 1-d parameters, the parser's refusals,
the segment table builder, and the fp32 NumPy restatement of the average's UPDATE inside the derived bound on the whole case grid
(tests/weight_average/cases.py) before any GPU run."""
import math

import numpy as np
import pytest

from tests.weight_average import cases as A


# ---- pure functions -----------------------------------------------------------------------------------------------------------------
def test_ema_decay_warms_up_monotonically_to_its_cap():
    from loans_amd import ema_decay_at
    assert ema_decay_at(0.9999, 1) == 2.0 / 11.0
    values = [ema_decay_at(0.9999, t) for t in range(1, 200001, 7)]
    assert all(b >= a for a, b in zip(values, values[1:]))
    assert values[-1] == 0.9999 and max(values) == 0.9999
    assert ema_decay_at(0.5, 1) == 2.0 / 11.0 and ema_decay_at(0.5, 8) == 0.5 == ema_decay_at(0.5, 9)      # (1 + 8) / (10 + 8) = 0.5
    assert ema_decay_at(0.1, 1) == 0.1                                                                       # the cap from the start


def test_cosine_rate():
    import train_imagenet as T
    base, lo = 0.4, 0.004
    assert T.cosine_lr(base, 5.0, 90, 5.0, lo) == base                              # the end of the warm-up
    assert T.cosine_lr(base, 2.0, 90, 5.0, lo) == base                              # inside it: progress clips to 0
    assert T.cosine_lr(base, 90.0, 90, 5.0, lo) == pytest.approx(lo, rel=1e-12)     # the end
    assert T.cosine_lr(base, 47.5, 90, 5.0, lo) == pytest.approx((base + lo) / 2, rel=1e-12)        # the midpoint
    assert T.cosine_lr(base, 26.25, 90, 5.0, lo) == pytest.approx(lo + (base - lo) * (1 + math.cos(math.pi / 4)) / 2, rel=1e-12)
    assert T.cosine_lr(base, 90.0, 90, 5.0, lo) == T.cosine_lr(base, 123.0, 90, 5.0, lo)            # constant beyond num_epoch
    assert T.cosine_lr(base, 10.0, 90, 0.0, 0.0) == pytest.approx(base * (1 + math.cos(math.pi / 9)) / 2, rel=1e-12)
    rates = [T.cosine_lr(base, e / 4, 90, 5.0, lo) for e in range(0, 4 * 90 + 1)]
    assert all(b <= a for a, b in zip(rates, rates[1:]))
    # the warm-up multiplies in, as it does for the stepped rate
    lr = T.cosine_lr(base, 2.5, 90, 5.0, lo) * T.warmup_factor(2.5, 5.0, 0.1)
    assert lr == pytest.approx(base * 0.55, rel=1e-12)


def test_parser_refusals(capsys):
    import train_imagenet as T
    for argv, words in ((['--lr-schedule', 'cosine', '--lr-drop-epochs', '30'], '--lr-drop-epochs belongs to --lr-schedule step'),
                        (['--no-decay-1d'], '--no-decay-1d is built for --optimizer sgd'),
                        (['--no-decay-1d', '--optimizer', 'adam'], '--no-decay-1d is built for --optimizer sgd'),
                        (['--ema-decay', '1.0'], '--ema-decay is a decay'),
                        (['--ema-decay', '-0.1'], '--ema-decay is a decay'),
                        (['--lr-schedule', 'cosine', '--lr-min', '-1'], '--lr-min must not be negative')):
        with pytest.raises(SystemExit):
            T.parse_args(argv)
        assert words in capsys.readouterr().err, argv
    args = T.parse_args(['--optimizer', 'sgd', '--no-decay-1d', '--ema-decay', '0.9999', '--lr-schedule', 'cosine', '--lr-min', '1e-5'])
    assert (args.no_decay_1d, args.ema_decay, args.lr_schedule, args.lr_min) == (True, 0.9999, 'cosine', 1e-5)
    plain = T.parse_args([])
    assert (plain.no_decay_1d, plain.ema_decay, plain.lr_schedule, plain.lr_min) == (False, 0.0, 'step', 0.0)
    assert 'ema_decay' not in vars(plain)           # SUPPRESS defaults: the namespace class holds them
    assert 'ema_decay' in T.RESUME_FIXED and not set(T.Arguments._AVERAGE[1:]) & set(T.RESUME_FIXED)
    assert T.RESUME_DEFAULTS_AVERAGE == {'ema_decay': 0.0, 'lr_schedule': 'step', 'lr_min': 0.0, 'no_decay_1d': False}
    assert T.ALL_RESUME_DEFAULTS == dict(T.RESUME_DEFAULTS, **T.RESUME_DEFAULTS_AVERAGE)


def test_a_checkpoint_from_before_the_options_resumes_at_their_defaults_only():
    import train_imagenet as T
    from loans_amd.runtime import checkpoint
    args = T.parse_args(['--optimizer', 'sgd'])
    saved = {k: v for k, v in checkpoint.plain_arguments(args).items() if k not in T.Arguments._AVERAGE}
    fixed = [k for k in T.RESUME_FIXED if k != 'gpus']
    assert checkpoint.check_arguments(saved, args, fixed, checkpoint.SILENT, T.ALL_RESUME_DEFAULTS) == []
    with pytest.raises(ValueError, match='ema_decay'):
        checkpoint.check_arguments(saved, T.parse_args(['--optimizer', 'sgd', '--ema-decay', '0.999']), fixed, checkpoint.SILENT, T.ALL_RESUME_DEFAULTS)
    # the schedule and the exemption may change on resume: reported, not refused
    later = T.parse_args(['--optimizer', 'sgd', '--lr-schedule', 'cosine', '--lr-min', '0.01', '--no-decay-1d'])
    lines = checkpoint.check_arguments(saved, later, fixed, checkpoint.SILENT, T.ALL_RESUME_DEFAULTS)
    assert sorted(l.split()[1] for l in lines) == ['lr_min', 'lr_schedule', 'no_decay_1d']


# ---- the segment table -------------------------------------------------------------------------------------------------------------
def test_segment_table_of_a_made_up_layout():
    from loans_amd.runtime.optimizers import decay_segments
    # a 4-d weight, gamma, beta, a 2-d weight and a bias; every size but the first needs padding to 8
    shapes = [(6, 3, 2, 2), (6,), (6,), (5, 6), (5,)]
    sizes = [int(np.prod(s)) for s in shapes]
    offsets, at = [], 0
    for n in sizes:
        offsets.append(at)
        at += (n + 7) // 8 * 8
    assert (sizes, offsets, at) == ([72, 6, 6, 30, 5], [0, 72, 80, 88, 120], 128)
    ends, flags = decay_segments(sizes, offsets, [len(s) <= 1 for s in shapes], at)
    assert ends.dtype == np.int64 and flags.dtype == np.uint8
    assert ends.tolist() == [72, 88, 120, 128] and flags.tolist() == [0, 1, 0, 1]         # gamma and beta are one segment
    assert ends[-1] == at and all(e % 4 == 0 for e in ends[:-1])
    # nothing exempt, everything exempt: one segment
    assert [a.tolist() for a in decay_segments(sizes, offsets, [False] * 5, at)] == [[128], [0]]
    assert [a.tolist() for a in decay_segments(sizes, offsets, [True] * 5, at)] == [[128], [1]]
    # a buffer that ends with its last parameter, ragged
    ends, flags = decay_segments([8, 3], [0, 8], [False, True], 11)
    assert ends.tolist() == [8, 11] and flags.tolist() == [0, 1]
    for bad in (([8, 3], [0, 6], [0, 1], 11), ([8, 3], [0, 8], [0, 1], 10), ([8], [8], [0], 16), ([], [], [], 0), ([8, 3], [0, 8], [0], 11)):
        with pytest.raises(ValueError):
            decay_segments(*bad)


def test_segment_table_of_resnet50_fits_the_kernel():
    """161 parameters; gamma and beta of one BN merge, a conv weight in front of each: well under the 1024 segments of LDS"""
    import loans_amd
    from loans_amd.runtime.optimizers import decay_segments
    np.random.seed(0)
    model = loans_amd.Classifier(loans_amd.Resnet50SheepLocalizer((75, 75), train_imagenet=True))
    params = list(model.params())
    assert len([p for p in params if p.host is not None]) == len(params)
    sizes, offsets, at = [p.size for p in params], [], 0
    for n in sizes:
        offsets.append(at)
        at += (n + 7) // 8 * 8
    exempt = [len(p.logical_shape) <= 1 for p in params]
    ends, flags = decay_segments(sizes, offsets, exempt, at)
    assert len(ends) <= A.SGD_MAX_SEGMENTS and len(ends) < len(params) and ends[-1] == at
    assert all(a != b for a, b in zip(flags, flags[1:]))
    assert sum(n for n, e in zip(sizes, exempt) if e) < 0.01 * sum(sizes)          # the exempt share of the floats is tiny
    names = [k for k, _ in model.namedparams()]
    assert all(e == k.endswith(('/gamma', '/beta', '/b')) for e, k in zip(exempt, names))


# ---- the grid and the restatement --------------------------------------------------------------------------------------------------
def test_regime_table_is_what_the_constants_give():
    from loans_amd import _lib
    assert (A.UNIT, A.GRID_CAP, A.SGD_TRIP, A.SGD_BLOCK) == (_lib.AVG_UNIT, 2048, 2097152, 1024) and _lib.AVG_UNIT == 4096
    for n, want in A.REGIMES.items():
        assert A.average_regime(n) == want, n
    assert set(A.SINGLE_N) == {1, 3, 4, 5, 64, 2048, A.UNIT - 1, A.UNIT, A.UNIT + 1, 2 * A.UNIT + 3}
    assert A.average_regime(A.LONG_N)[3] == 2 and len(A.TABLE_N) == 121 and A.TABLE_N[0] > max(A.TABLE_N[1:])
    assert any(n % 4 for n in A.TABLE_N[1:]) and any(n > 2048 for n in A.TABLE_N[1:])
    for name, (n, ends, flags) in A.SGD_CASES.items():
        assert ends[-1] == n and len(ends) == len(flags) and all(e % 4 == 0 for e in ends[:-1]) and sorted(set(ends)) == ends, name
    n, ends, flags = A.SGD_CASES['edges']
    assert n & 3 == 3 and (n - ends[-2]) % 4 == 3 and flags[-1] == 1 and A.SGD_CASES['one'][0] & 3 == 3
    assert {8, 1016, 1024, 1032, A.SGD_TRIP - 8, A.SGD_TRIP, A.SGD_TRIP + 8} <= set(ends)
    assert len(A.SGD_CASES['eights'][1]) == 300


@pytest.mark.parametrize('ns', [(n,) for n in A.SINGLE_N] + [A.TABLE_N, (A.LONG_N,)], ids=lambda ns: 'n%d' % ns[0] if len(ns) == 1 else 'table')
def test_restatement_of_update_sits_inside_the_bound(ns):
    for k, omd in enumerate(A.OMDS):
        dst, src = A.make_update(ns, 10 + k)
        got = dst.copy()
        for n, o in zip(ns, A.layout(ns)[0]):
            got[o:o + n] = A.update_numpy(dst[o:o + n], src[o:o + n], omd)
        worst = A.check_update(got, dst, src, omd, ns)
        assert worst <= 1.0, (omd, worst)
    for omd in A.OMDS_EQUAL:
        dst, src = A.make_update(ns, 20, equal=True)
        got = A.update_numpy(dst, src, omd)
        offsets = A.layout(ns)[0]
        for n, o in zip(ns, offsets):
            assert np.array_equal(got[o:o + n].view(np.int32), dst[o:o + n].view(np.int32)), omd


def test_swap_values_hold_the_specials():
    dst, src = A.make_swap((64,), 3)
    o = A.layout((64,))[0][0]
    for buf in (dst, src):
        v = buf[o:o + 64]
        assert np.isnan(v).any() and (v.view(np.uint32) == 0x80000000).any()
        assert ((v.view(np.uint32) & 0x7f800000) == 0).sum() >= 3           # zeros and denormals
