"""No GPU: the LAMB case grid, the NumPy restatement of the three passes inside the derived bounds on the whole grid
(tests/imagenet_lamb/cases.py) before any GPU run, five wrong implementations outside them, the identity |p' - p| = lr |p|, the
host side of ``loans_amd.LAMB``, the C ABI's declarations and the trainer's new options."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from tests.imagenet_lamb import cases as A

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


# ---- the grid ---------------------------------------------------------------------------------------------------------------------
def test_grid_covers_what_it_says():
    assert {c[0] for c in A.GRID} == set(A.TABLES) and len(set(A.GRID)) == len(A.GRID)
    kinds = [c[1:] for c in A.GRID if c[0] == 'kinds']
    assert set(kinds) == {(t, gs, wd, warm) for t in (1, 2, 1000) for gs in (1.0, 0.5, 0.125) for wd in (0.0, 5e-5) for warm in (False, True)}
    c1, c2 = A.corrections(1)
    assert c1 == pytest.approx(10.0) and c2 == pytest.approx(1000.0)
    c1, c2 = A.corrections(1000)
    assert 1.0 <= c1 < 1.0 + 1e-12 and 1.5 < c2 < 1.6
    assert float(np.float32(A.LR)) == A.LR
    n, ends, flags = A.TABLES['kinds']
    p, g, m, v = A.make('kinds')
    assert len(p) == n + A.GUARD and np.isnan(p[n:]).all() and np.isnan(g[n:]).all() and (m[n:] == A.S_GUARD).all() and (v[n:] == A.S_GUARD).all()
    assert (v[:n] >= 0).all() and np.abs(g[:n].astype(np.float64)).max() < 1e15
    cold = A.make('kinds', warm=False)
    assert not cold[2][:n].any() and not cold[3][:n].any() and np.array_equal(cold[0][:n], p[:n])
    with np.errstate(all='ignore'):
        lo = 0
        for hi, kind in zip(ends, A.kinds_of(len(ends), 'kinds')):      # the fp32 sum of squares is what the kinds say it is
            s = np.sum(np.square(p[lo:hi]), dtype=np.float32)
            assert {'tiny': s == 0, 'huge': np.isinf(s), 'zero_w': s == 0}.get(kind, np.isfinite(s) and s > 0), kind
            if kind == 'zero_g':
                assert not g[lo:hi].any() and not m[lo:hi].any() and not v[lo:hi].any()
            if kind == 'huge':
                assert 0.1 < np.sqrt(np.mean(np.square(g[lo:hi].astype(np.float64)))) < 10
            lo = hi


# ---- the restatement inside the bounds, on the whole grid -----------------------------------------------------------------------------
_SHARED = {}


def _values(name, warm):
    if (name, warm) not in _SHARED:
        _SHARED[name, warm] = A.make(name, warm)
    return _SHARED[name, warm]


@pytest.mark.parametrize('name,t,gs,wd,warm', A.GRID, ids=A.IDS)
def test_restatement_sits_inside_the_bounds(name, t, gs, wd, warm):
    n, ends, flags = A.TABLES[name]
    p, g, m, v = _values(name, warm)
    got = A.lamb_numpy(p, g, m, v, ends, flags, t, A.LR, wd, gs)
    worst = A.check(got, p, g, m, v, ends, flags, t, A.LR, wd, gs)
    print('%s: error / bound %s' % (name, ' '.join('%s %.3f' % kv for kv in sorted(worst.items()))))
    assert set(worst) == {'p', 'm', 'v', 'u', 'r', 'W', 'U'} and max(worst.values()) <= 1.0, worst
    ident, count = A.identity_check(got['p'], p, g, m, v, ends, flags, t, A.LR, wd, gs)
    assert ident <= 1.0, ident
    if name == 'kinds':
        # zero weights and (zero gradients, zero moments, no decay) do not adapt; everything else under flags 0 and 1 does
        kinds = A.kinds_of(len(ends), name)
        assert count == sum(not f & 2 and k != 'zero_w' and not (k == 'zero_g' and (wd == 0 or f & 1)) for f, k in zip(flags, kinds))


def _outside(got, *case):
    try:
        return max(A.check(got, *case).values()) > 1.0
    except AssertionError:
        return True             # a ratio the rule makes 1 is not 1, or a value is not finite


@pytest.mark.parametrize('wrong', A.VARIANTS)
def test_a_wrong_implementation_falls_outside(wrong):
    n, ends, flags = A.TABLES['kinds']
    caught = []
    for t, wd, warm in ((1, 5e-5, False), (2, 5e-5, True), (1000, 0.0, True)):
        p, g, m, v = _values('kinds', warm)
        case = (p, g, m, v, ends, flags, t, A.LR, wd, 1.0)
        assert not _outside(A.lamb_numpy(*case), *case)
        caught.append(_outside(A.lamb_numpy(*case, wrong=wrong), *case))
    assert any(caught), wrong
    if wrong == 'no_bias_correction':
        assert caught[0]            # at t = 1, where c1 = 10 and c2 = 1000


def test_reference_is_the_rule_by_hand():
    """p = (3, 4), g = (0.5, -0.25), zero moments, t = 1, eps = 0: m^ = g, v^ = g^2, a = sign(g)"""
    p, g, z = np.array([3, 4], np.float32), np.array([0.5, -0.25], np.float32), np.zeros(2, np.float32)
    out = A.lamb_ref(p, g, z, z, [2], [0], 1, 0.5, 0.0, 1.0, eps=0.0)
    assert np.allclose(out['m'], 0.1 * g, rtol=1e-15) and np.allclose(out['v'], 0.001 * g.astype(np.float64) ** 2, rtol=1e-12)
    assert np.allclose(out['u'], [1, -1], rtol=1e-12) and out['W'][0] == 5.0 and out['U'][0] == pytest.approx(np.sqrt(2), rel=1e-12)
    assert np.allclose(out['p'], [3 - 0.5 * 5 / np.sqrt(2), 4 + 0.5 * 5 / np.sqrt(2)], rtol=1e-12)
    # decay sits inside u and inside the ratio; bit 0 takes it out, bit 1 pins the ratio
    out = A.lamb_ref(p, g, z, z, [2], [0], 1, 0.5, 0.5, 1.0, eps=0.0)
    assert np.allclose(out['u'], [2.5, 1], rtol=1e-12) and out['r'][0] == pytest.approx(5 / np.sqrt(7.25), rel=1e-12)
    assert np.allclose(A.lamb_ref(p, g, z, z, [2], [1], 1, 0.5, 0.5, 1.0, eps=0.0)['u'], [1, -1], rtol=1e-12)
    out = A.lamb_ref(p, g, z, z, [2], [2], 1, 0.5, 0.5, 1.0, eps=0.0)
    assert out['r'][0] == 1.0 and np.allclose(out['p'], p - 0.5 * np.array([2.5, 1]), rtol=1e-12)
    # a zero norm: the ratio is 1; zero gradient, zero moments and decay: U = wd W, the step is lr p whatever wd is
    assert A.lamb_ref(z, g, z, z, [2], [0], 1, 0.5, 0.5, 1.0)['r'][0] == 1.0 == A.lamb_ref(p, z, z, z, [2], [0], 1, 0.5, 0.0, 1.0)['r'][0]
    out = A.lamb_ref(p, z, z, z, [2], [0], 7, 0.5, 0.01, 1.0)
    assert out['U'][0] == pytest.approx(0.05, rel=1e-12) and np.allclose(out['p'], 0.5 * p, rtol=1e-12)
    # the gradient scale multiplies the gradient before anything else
    a, b = A.lamb_ref(p, g, z, z, [2], [0], 3, 0.5, 0.1, 0.5), A.lamb_ref(p, 0.5 * g, z, z, [2], [0], 3, 0.5, 0.1, 1.0)
    assert all(np.array_equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize('t,wd,warm', [(1, 5e-5, False), (2, 0.0, True), (1000, 5e-5, True)])
def test_adapting_segments_move_by_lr_of_their_norm(t, wd, warm):
    for name in ('kinds', 'resnet'):
        n, ends, flags = A.TABLES[name]
        p, g, m, v = _values(name, warm)
        for lr in (A.LR, 0.3):
            ref = A.lamb_ref(p, g, m, v, ends, flags, t, lr, wd, 0.5)
            on = A.adapting(ref, flags)
            assert on.sum() >= 4
            lo = 0
            for hi, adapts, W in zip(ends, on, ref['W']):
                if adapts:
                    assert A._norm(ref['p'][lo:hi] - p[lo:hi].astype(np.float64)) == pytest.approx(lr * W, rel=1e-12)
                lo = hi


# ---- loans_amd.LAMB without a GPU -------------------------------------------------------------------------------------------------------
def test_optimiser_class_without_a_gpu():
    import loans_amd
    from loans_amd.runtime.optimizers import LARS, GradientMethod
    opt = loans_amd.LAMB()
    assert vars(opt.hyperparam) == dict(lr=0.001, beta1=0.9, beta2=0.999, eps=1e-6, weight_decay_rate=0.0, decay_exempt_1d=False)
    opt = loans_amd.LAMB(lr=0.5, beta1=0.8, weight_decay_rate=5e-5, decay_exempt_1d=True)
    assert isinstance(opt, GradientMethod) and not isinstance(opt, LARS)
    assert opt._state_names() == ('m', 'v') and opt.lr == 0.5 and opt.t == 0
    made = []
    assert len(opt._new_state(lambda: made.append(0) or len(made))) == 2 and len(made) == 2
    opt.lr = 0.25
    assert opt.hyperparam.lr == 0.25 and opt.lr == 0.25         # the plain hyperparameter: no bias correction inside the rate
    with pytest.raises(RuntimeError, match='no step'):
        opt.trust_ratios()
    with pytest.raises(ValueError, match='class: the checkpoint holds LARS, this optimiser is LAMB'):
        opt.load_state_dict({'class': 'LARS', 't': 3, 'hyperparam': {}, 'stepped_cold': None, 'state': {}})
    for line in ('g^  = g * gs', "m'  = m + (1 - beta1) (g^ - m)", "a   = (m' c1) / (sqrt(v' c2) + eps)", 'r   = (f & 2) or W == 0 or U == 0 ?  1  :  W / U',
                 "p'  = p - (lr r) u"):
        assert line in loans_amd.LAMB.__doc__, line


def test_segment_table_with_and_without_the_exemption():
    import torch
    import loans_amd
    from loans_amd import ops
    shapes = [(6, 3, 2, 2), (6,), (6,), (5, 6), (3, 2), (5,)]
    sizes, offsets, numel = A.arena_layout(shapes)
    arena = SimpleNamespace(data=torch.zeros(numel), params=[SimpleNamespace(size=n, logical_shape=s) for n, s in zip(sizes, shapes)],
                            offsets=offsets, numel=numel, device=torch.device('cpu'))
    opt = loans_amd.LAMB(decay_exempt_1d=True)
    table = opt._segment_table(arena, numel)
    assert isinstance(table, ops.LarsTable) and table.ends_host.tolist() == [72, 88, 120, 128, 136] and table.flags_host.tolist() == [0, 3, 0, 0, 3]
    assert opt._segment_table(arena, numel) is table                    # built once per arena ...
    cut = opt._segment_table(arena, 80)
    assert cut.ends_host.tolist() == [72, 80] and opt._segment_table(arena, 80) is cut and cut.workspace is table.workspace        # ... cut once per prefix
    opt.hyperparam.decay_exempt_1d = False                              # (may change on resume)
    assert opt._segment_table(arena, numel).flags_host.tolist() == [0, 2, 0, 0, 2]
    assert loans_amd.LAMB()._segment_table(arena, numel).flags_host.tolist() == [0, 2, 0, 0, 2]


def test_entries_are_declared_and_registered():
    from loans_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'loans_hip.h')).read()
    source = open(os.path.join(ROOT, 'loans_amd', 'csrc', 'lamb.hip')).read()
    P, I64, I32, F64 = _lib.C.c_void_p, _lib.C.c_int64, _lib.C.c_int32, _lib.C.c_double
    kinds = {'*': P, 'int64_t': I64, 'int32_t': I32, 'double': F64}
    for name in ('loans_lamb_moments_f32', 'loans_lamb_ratios_f32', 'loans_lamb_update_f32'):
        assert name in _lib.SIGNATURES and name not in _lib.RESTYPES
        for text in (header, source):
            found = re.search(r'int %s\(([^)]*)\)' % name, text)
            assert found, name
            args = [a.strip() for a in found.group(1).replace('\n', ' ').split(',')]
            assert [kinds['*' if '*' in a else a.split()[0]] for a in args] == _lib.SIGNATURES[name], name
    assert 'lamb.hip' in open(os.path.join(ROOT, 'loans_amd', 'csrc', 'Makefile')).read()
    for line in ("m'  = fmaf(omb1, g^ - m, m)", "v'  = fmaf(omb2, fmaf(g^, g^, -v), v)", "u   = fmaf(wd_s, p, a)", "p'  = fmaf(-rate_s, u, p)"):
        assert line in source, line


# ---- the trainer's options ----------------------------------------------------------------------------------------------------------
def test_parser_takes_and_refuses(capsys):
    import train_imagenet as T
    args = T.parse_args(['--optimizer', 'lamb', '--lamb-beta1', '0.8', '--lamb-beta2', '0.99', '--lamb-eps', '1e-8', '--weight-decay', '0.02',
                         '--no-decay-1d', '--lr', '5e-3'])
    assert (args.optimizer, args.lamb_beta1, args.lamb_beta2, args.lamb_eps, args.weight_decay, args.no_decay_1d, args.learning_rate) == \
        ('lamb', 0.8, 0.99, 1e-8, 0.02, True, 5e-3)
    plain = T.parse_args(['--optimizer', 'lamb'])
    assert (plain.lamb_beta1, plain.lamb_beta2, plain.lamb_eps, plain.no_decay_1d) == (0.9, 0.999, 1e-6, False)
    assert not set(T.Arguments._LAMB) & set(vars(plain)) and T.Arguments._LAMB == ('lamb_beta1', 'lamb_beta2', 'lamb_eps')
    # the bare namespace is what it was: nothing of LAMB in it
    assert not [k for k in vars(T.parse_args([])) if 'lamb' in k]
    assert set(vars(T.parse_args(['--optimizer', 'lamb']))) == set(vars(T.parse_args([])))
    assert T.resolved_topk(plain) == 5 and T.resolved_topk(T.parse_args([])) is None
    assert T.resolved_topk(T.parse_args(['--optimizer', 'lamb', '--topk', '0'])) is None
    assert T.parse_args(['--optimizer', 'lamb', '--lamb-beta1', '0', '--lamb-eps', '0']).lamb_beta1 == 0.0
    for argv, words in ((['--optimizer', 'lamb', '--lamb-beta1', '1'], '--lamb-beta1 must lie in [0, 1)'),
                        (['--optimizer', 'lamb', '--lamb-beta1=-0.1'], '--lamb-beta1 must lie in [0, 1)'),
                        (['--optimizer', 'lamb', '--lamb-beta2', '1.5'], '--lamb-beta2 must lie in [0, 1)'),
                        (['--optimizer', 'lamb', '--lamb-beta2', 'nan'], '--lamb-beta2 must lie in [0, 1)'),
                        (['--optimizer', 'lamb', '--lamb-eps=-1e-9'], '--lamb-eps must not be negative'),
                        (['--optimizer', 'sgd', '--lamb-beta1', '0.9'], 'belong to --optimizer lamb'),
                        (['--optimizer', 'lars', '--lamb-eps', '1e-6'], 'belong to --optimizer lamb'),
                        (['--lamb-beta2', '0.99'], 'belong to --optimizer lamb'),
                        (['--optimizer', 'lamb', '--lars-eta', '0.01'], 'belong to --optimizer lars'),
                        (['--no-decay-1d'], '--no-decay-1d is built for --optimizer sgd: Adam\'s kernel applies one weight decay to every parameter'),
                        (['--no-decay-1d', '--optimizer', 'adam'], '--no-decay-1d is built for --optimizer sgd: Adam\'s kernel applies one weight decay to every parameter')):
        with pytest.raises(SystemExit):
            T.parse_args(argv)
        assert words in capsys.readouterr().err, argv
    with pytest.raises(ValueError, match='belong to --optimizer lamb'):
        T.check_lamb_arguments(T.argparse.Namespace(optimizer='adam', lamb_beta1=0.9, lamb_beta2=0.999, lamb_eps=1e-6))
    T.check_lamb_arguments(T.argparse.Namespace(optimizer='lamb', lamb_beta1=0.9, lamb_beta2=0.999, lamb_eps=1e-6))


def test_resume_table_holds_the_new_defaults():
    import train_imagenet as T
    from loans_amd.runtime import checkpoint
    assert T.RESUME_DEFAULTS_LAMB == {'lamb_beta1': 0.9, 'lamb_beta2': 0.999, 'lamb_eps': 1e-6}
    assert T.RESUME_DEFAULTS_WITH_LAMB == dict(T.RESUME_DEFAULTS_WITH_PHOTO, **T.RESUME_DEFAULTS_LAMB)
    # the older tables stay what they are
    assert not [k for table in (T.RESUME_DEFAULTS, T.ALL_RESUME_DEFAULTS, T.RESUME_DEFAULTS_WITH_LARS, T.RESUME_DEFAULTS_WITH_PHOTO)
                for k in table if 'lamb' in k]
    assert T.RESUME_DEFAULTS_WITH_PHOTO == dict(T.RESUME_DEFAULTS_WITH_LARS, **T.RESUME_DEFAULTS_PHOTO)
    assert 'optimizer' in T.RESUME_FIXED and not set(T.Arguments._LAMB) & set(T.RESUME_FIXED)
    fixed = [k for k in T.RESUME_FIXED if k != 'gpus']
    # a checkpoint from before the options existed resumes; an adam checkpoint does not become a lamb run
    args = T.parse_args([])
    saved = {k: v for k, v in checkpoint.plain_arguments(args).items() if k not in T.Arguments._LAMB}
    assert checkpoint.check_arguments(saved, args, fixed, checkpoint.SILENT, T.RESUME_DEFAULTS_WITH_LAMB) == []
    with pytest.raises(ValueError, match='optimizer'):
        checkpoint.check_arguments(saved, T.parse_args(['--optimizer', 'lamb']), fixed, checkpoint.SILENT, T.RESUME_DEFAULTS_WITH_LAMB)
    # the betas and eps may change on resume, like --momentum: reported, not refused
    saved = checkpoint.plain_arguments(T.parse_args(['--optimizer', 'lamb']))
    later = T.parse_args(['--optimizer', 'lamb', '--lamb-beta1', '0.8', '--lamb-beta2', '0.99', '--lamb-eps', '0'])
    lines = checkpoint.check_arguments(saved, later, fixed, checkpoint.SILENT, T.RESUME_DEFAULTS_WITH_LAMB)
    assert sorted(l.split()[1] for l in lines) == ['lamb_beta1', 'lamb_beta2', 'lamb_eps']
