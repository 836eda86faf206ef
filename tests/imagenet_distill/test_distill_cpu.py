"""No GPU, no launch: the fp32 restatement of the distillation loss held to the derived bound over the case grid, the float64
reference against torch's ``cross_entropy`` + ``kl_div``, its properties, the entry's argument checks, and the options of
``Classifier`` and of the trainer with their resume rules."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests.imagenet import reference as R
from tests.imagenet_distill import reference as D
from tests.imagenet_mix import reference as X

K = 2
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def check_case(hard, soft, alpha, T, tag, extremes, worst=None):
    ref = D.combine(hard, soft, alpha, T)
    got = D.combine_fp32(hard, soft, alpha, T)
    err = np.abs(got['row_loss'].astype(np.float64) - ref['row_loss'])
    kerr = np.abs(got['row_kl'].astype(np.float64) - ref['row_kl'])
    gerr = np.abs(got['gz'].astype(np.float64) - ref['gz'])
    assert np.all(err <= ref['lb']), tag + ('row_loss', float((err - ref['lb']).max()))
    assert np.all(kerr <= ref['kb']), tag + ('row_kl', float((kerr - ref['kb']).max()))
    assert np.all(gerr <= ref['gb']), tag + ('gz', float((gerr - ref['gb']).max()))
    assert abs(got['out'][0] - ref['loss']) <= ref['bb'], tag + (got['out'][0], ref['loss'], ref['bb'])
    assert abs(got['out'][3] - ref['kl']) <= ref['bkl'], tag + (got['out'][3], ref['kl'], ref['bkl'])
    hit, hitk, thit = D.hits(hard, soft)
    assert got['out'][1] == float(np.float32(hit.mean())) and got['out'][2] == float(np.float32(hitk.mean())), tag
    assert got['out'][4] == float(np.float32(thit.mean())), tag
    assert np.all(ref['row_kl'] >= -ref['kb']), tag                 # KL >= 0, to the reference's own rounding
    valid = hard.valid
    if extremes:
        assert np.all(np.isfinite(got['row_loss'])) and np.all(np.isfinite(got['row_kl'])) and np.all(np.isfinite(got['gz'])), tag
        assert np.all(np.isfinite(ref['row_loss'])) and np.all(np.isfinite(ref['gz'])), tag
    if not valid.any():
        assert got['out'][0] == 0.0 and got['out'][3] == 0.0 and not got['gz'].any() and not got['row_loss'].any(), tag
        assert not hit.any() and not hitk.any() and not thit.any(), tag
    elif worst is not None:
        worst['loss'] = max(worst['loss'], float((err[valid] / ref['lb'][valid]).max()))
        worst['kl'] = max(worst['kl'], float((kerr[valid] / ref['kb'][valid]).max()))
        worst['gz'] = max(worst['gz'], float((gerr[valid] / ref['gb'][valid]).max()))
        worst['batch'] = max(worst['batch'], abs(got['out'][0] - ref['loss']) / ref['bb'], abs(got['out'][3] - ref['kl']) / ref['bkl'])
    return ref


# ---- reference, restatement and bound -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', D.DISTILL_N)
def test_restatement_is_inside_the_bound_over_the_grid(N):
    worst = {'loss': 0.0, 'kl': 0.0, 'gz': 0.0, 'batch': 0.0}
    cases = 0
    for B in D.DISTILL_B:
        pupils = list(D.students(N, B))
        masters = list(D.teachers(N, B))
        assert len(pupils) == len(masters) == D.profiles(N)
        for sname, c, t, expect in pupils:
            assert R.argmax_margin_ok(c.z32), sname
            hards = []
            for kind in X.PAIRS:
                ta, tb = X.label_pair(kind, t, N)
                for lam in X.LAMS:
                    wa, wb = X.weights(lam)
                    for eps in D.DISTILL_EPS:
                        hard = D.Hard(c, ta, tb, wa, wb, eps, K)
                        hards.append(((kind, lam, eps), hard))
                        if expect is not None and np.array_equal(ta if wa >= wb else tb, t):
                            # the tie expectations, against the dominant label: the first of two equal maxima is the hit
                            np.testing.assert_array_equal(hard.hit, expect & hard.valid, err_msg=sname)
            for tname, ct in masters:
                assert R.argmax_margin_ok(ct.z32), tname
                for T in D.TEMPERATURES:
                    soft = D.Soft(c, ct, T)
                    for key, hard in hards:
                        for alpha in D.ALPHAS:
                            tag = (B, sname, tname, T, alpha) + key
                            check_case(hard, soft, alpha, T, tag, D.EXTREMES in (sname, tname), worst)
                            cases += 1
    assert cases == len(D.DISTILL_B) * D.profiles(N) ** 2 * len(X.PAIRS) * len(X.LAMS) * len(D.DISTILL_EPS) * len(D.ALPHAS) * len(D.TEMPERATURES)
    assert max(worst.values()) < 1.0
    print('N=%d worst error / bound: row loss %.3f, row kl %.3f, gz %.3f, batch %.3f' % (N, worst['loss'], worst['kl'], worst['gz'], worst['batch']))


def test_restatement_at_the_lds_limit():
    c, ct, ta, tb = D.lds_limit_case()
    assert (c.B, c.N) == (2, 8192)
    wa, wb = X.weights(np.float32(0.3))
    worst = {'loss': 0.0, 'kl': 0.0, 'gz': 0.0, 'batch': 0.0}
    hard = D.Hard(c, ta, tb, wa, wb, 0.1, K)
    for T in D.TEMPERATURES:
        soft = D.Soft(c, ct, T)
        for alpha in D.ALPHAS:
            check_case(hard, soft, alpha, T, ('lds', T, alpha), False, worst)
    assert max(worst.values()) < 1.0
    print('N=8192 worst error / bound: row loss %.3f, row kl %.3f, gz %.3f, batch %.3f' % (worst['loss'], worst['kl'], worst['gz'], worst['batch']))


def test_the_array_entry_points_are_the_combination_and_alpha_zero_is_the_mix_reference():
    N, B = 257, 5
    rng = np.random.Generator(np.random.PCG64(3))
    z, zt = R.make_logits('normal', B, N, rng), R.make_logits('dominant', B, N, rng)
    t = R.make_labels('first_last', B, N, None)
    for kind in X.PAIRS:
        ta, tb = X.label_pair(kind, t, N)
        for lam in X.LAMS:
            wa, wb = X.weights(lam)
            ref = D.distill_ref(z, zt, ta, tb, wa, wb, 0.1, K, 0.5, 4.0)
            got = D.distill_fp32(z, zt, ta, tb, wa, wb, 0.1, K, 0.5, 4.0)
            assert np.all(np.abs(got['gz'] - ref['gz']) <= ref['gb']) and abs(got['out'][0] - ref['loss']) <= ref['bb']
            assert got['out'][3] == pytest.approx(ref['distill_loss'], abs=ref['bkl'])
            assert got['out'][4] == float(np.float32(ref['teacher_accuracy']))
            # alpha == 0: X's reference exactly in float64, X's restatement exactly in fp32, zeros for the teacher
            zero = D.distill_ref(z, zt, ta, tb, wa, wb, 0.1, K, 0.0, 4.0)
            mix = X.mixed_ref(z, ta, tb, wa, wb, 0.1, K)
            assert zero['loss'] == pytest.approx(mix[0], rel=1e-15, abs=1e-300)
            np.testing.assert_allclose(zero['gz'], mix[3], rtol=1e-14, atol=1e-300)
            np.testing.assert_allclose(zero['row_loss'], mix[4], rtol=1e-15, atol=1e-300)
            np.testing.assert_array_equal(zero['hit'], mix[5])
            np.testing.assert_array_equal(zero['hitk'], mix[6])
            assert not zero['row_kl'].any() and not zero['thit'].any() and zero['distill_loss'] == 0.0
            zero32, mix32 = D.distill_fp32(z, None, ta, tb, wa, wb, 0.1, K, 0.0, 4.0), X.mixed_fp32(z, ta, tb, wa, wb, 0.1, K)
            assert zero32['out'] == [mix32[0], mix32[1], mix32[2], 0.0, 0.0]
            np.testing.assert_array_equal(zero32['gz'], mix32[3])
            np.testing.assert_array_equal(zero32['row_loss'], mix32[4])


@pytest.mark.parametrize('T', D.TEMPERATURES)
@pytest.mark.parametrize('alpha', (0.25, 0.5, 1.0))
@pytest.mark.parametrize('eps', D.DISTILL_EPS)
def test_float64_reference_is_torch_cross_entropy_plus_kl_div(eps, alpha, T):
    """a dense target built here, independently; batches without ignored rows; alpha and T exact in fp32, so that the constants
    the reference takes from the launcher are the numbers torch is given; 1e-12 relative (the gradient: relative to its scale
    max(1, T) / B, differences of probabilities of order one being formed on both sides)"""
    F = torch.nn.functional
    for N, B in ((1, 5), (2, 5), (257, 5), (1000, 3)):
        for profile, tprofile in (('normal', 'dominant'), ('dominant', 'normal'), ('normal', D.EXTREMES), ('pm80', 'normal')):
            rng = np.random.Generator(np.random.PCG64([N, B, 5]))
            z = R.make_logits(profile, B, N, rng)
            zt = D.Q.extreme_logits(B, N) if tprofile == D.EXTREMES else R.make_logits(tprofile, B, N, rng)
            t = R.make_labels('first_last', B, N, None)
            for kind in ('different', 'equal'):
                ta, tb = X.label_pair(kind, t, N)
                for lam in X.LAMS:
                    wa, wb = X.weights(lam)
                    dense = np.zeros((B, N))
                    for b in range(B):
                        dense[b, ta[b]] += wa
                        dense[b, tb[b]] += wb
                    dense = (1.0 - eps) * dense + eps / N
                    zv = torch.tensor(z, dtype=torch.float64, requires_grad=True)
                    # (the scaled rows as the kernel defines them: fp32 products; exact at these temperatures)
                    zs = zv * (1.0 / T)
                    zts = torch.tensor((zt * np.float32(1.0 / T)).astype(np.float32), dtype=torch.float64)
                    assert np.array_equal((z * np.float32(1.0 / T)).astype(np.float32).astype(np.float64), zs.detach().numpy())
                    want = (1 - alpha) * F.cross_entropy(zv, torch.from_numpy(dense)) \
                        + alpha * T * T * F.kl_div(F.log_softmax(zs, dim=1), F.softmax(zts, dim=1), reduction='batchmean')
                    want.backward()
                    got = D.distill_ref(z, zt, ta, tb, wa, wb, eps, K, alpha, T)
                    assert got['loss'] == pytest.approx(want.item(), rel=1e-12), (N, profile, tprofile, kind, lam)
                    np.testing.assert_allclose(got['gz'], zv.grad.numpy(), rtol=1e-12, atol=1e-12 * max(1.0, T) / B)


def test_float64_reference_properties():
    N, B = 65, 6
    rng = np.random.Generator(np.random.PCG64(9))
    # (teacher rows on a grid of 2^-10: a shift by a power of two is then exact in fp32, and so is every scaled row)
    z, zt = R.make_logits('normal', B, N, rng), (np.round(3 * R.make_logits('normal', B, N, rng) * 1024) / 1024).astype(np.float32)
    t = R.make_labels('first_last', B, N, None)
    ta, tb = X.label_pair('different', t, N)
    wa, wb = X.weights(0.3)
    for T in D.TEMPERATURES:
        # the teacher's own logits: no divergence, and the soft part of gz is zero -- at alpha = 1 the whole of it
        same = D.distill_ref(z, z, ta, tb, wa, wb, 0.1, K, 1.0, T)
        assert not same['row_kl'].any() and same['distill_loss'] == 0.0 and same['loss'] == 0.0 and not same['gz'].any()
        half = D.distill_ref(z, z, ta, tb, wa, wb, 0.1, K, 0.5, T)
        np.testing.assert_allclose(half['gz'], 0.5 * X.mixed_ref(z, ta, tb, wa, wb, 0.1, K)[3], rtol=1e-14, atol=1e-300)
        # a constant added to a teacher row changes nothing (an exact shift of the scaled row: a multiple of T large enough to
        # be exact in fp32 on every element)
        shift = np.float32(64.0 * T)
        ref = D.distill_ref(z, zt, ta, tb, wa, wb, 0.1, K, 0.5, T)
        moved = (zt.astype(np.float64) + shift).astype(np.float32)
        assert np.array_equal(moved.astype(np.float64), zt.astype(np.float64) + shift)
        got = D.distill_ref(z, moved, ta, tb, wa, wb, 0.1, K, 0.5, T)
        np.testing.assert_array_equal(got['row_kl'], ref['row_kl'])
        np.testing.assert_array_equal(got['gz'], ref['gz'])
        np.testing.assert_array_equal(got['thit'], ref['thit'])
        assert np.all(ref['row_kl'] > 0)
    # the one-label weights: the label of weight zero is not read
    for w, lab in (((1.0, 0.0), ta), ((0.0, 1.0), tb)):
        a = D.distill_ref(z, zt, ta, tb, w[0], w[1], 0.1, K, 0.5, 4.0)
        b = D.distill_ref(z, zt, lab, lab, w[0], w[1], 0.1, K, 0.5, 4.0)
        ign = np.full(B, -1)
        c = D.distill_ref(z, zt, lab if w[0] else ign, ign if w[0] else lab, w[0], w[1], 0.1, K, 0.5, 4.0)
        for key in ('gz', 'row_loss', 'row_kl', 'hit', 'hitk', 'thit'):
            np.testing.assert_array_equal(a[key], b[key])
            np.testing.assert_array_equal(a[key], c[key])
    # by hand: two classes, T = 1, one row
    zz, zzt = np.array([[0.0, 0.0]], np.float32), np.array([[np.log(3.0), 0.0]], np.float32)
    got = D.distill_ref(zz, zzt, [0], [0], 1.0, 0.0, 0.0, 1, 1.0, 1.0)
    p = np.exp(zzt.astype(np.float64)[0]) / np.exp(zzt.astype(np.float64)[0]).sum()
    assert got['loss'] == pytest.approx(float((p * (np.log(p) - np.log(0.5))).sum()), rel=1e-14)
    np.testing.assert_allclose(got['gz'][0], 0.5 - p, rtol=1e-14)
    assert got['teacher_accuracy'] == 1.0


# ---- the entry without a GPU --------------------------------------------------------------------------------------------------
def test_distill_entry_checks_its_arguments_before_any_hip_call():
    from loans_amd import _lib
    f = _lib.load().loans_softmax_distill_fwd_f32
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    inf, nan = float('inf'), float('nan')

    def call(ptrs=None, lam=0.5, oml=0.5, B=4, N=8, eps=0.1, k=1, alpha=0.5, T=1.0):
        z, zt, ta, tb, gz, rl, rh, rhk, rkl, rth, out = ptrs or [p] * 11
        return f(z, zt, ta, tb, lam, oml, gz, rl, rh, rhk, rkl, rth, out, B, N, eps, k, alpha, T, 0)

    for lam, oml in ((0.5, 0.5), (1.0, 0.0), (0.0, 1.0)):
        for alpha in (0.0, 0.5, 1.0):
            kw = dict(lam=lam, oml=oml, alpha=alpha)
            for missing in range(11):
                if missing == 1 and alpha == 0.0:
                    continue                # a null zt is allowed where it is not read; that call would launch
                ptrs = [p] * 11
                ptrs[missing] = 0
                assert call(ptrs, **kw) == -1, (lam, oml, alpha, missing)
            assert call(k=0, **kw) == -1
            assert call(B=0, **kw) == -1 and call(N=0, **kw) == -1 and call(B=-3, **kw) == -1 and call(N=-1, **kw) == -1
            assert call(eps=1.0, **kw) == -1 and call(eps=-0.1, **kw) == -1 and call(eps=nan, **kw) == -1
            assert call(N=8193, **kw) == -2 and call(B=65537, **kw) == -2
            for T in (0.0, -1.0, 2.0 ** -7, 65.0, inf, -inf, nan):
                assert call(T=T, **kw) == -1, T
    for alpha in (-0.1, 1.5, inf, -inf, nan):
        assert call(alpha=alpha) == -1, alpha
    for lam, oml in ((nan, 0.5), (0.5, inf), (-inf, 0.0)):
        assert call(lam=lam, oml=oml) == -1
    assert bytes(buf) == bytes(64)


def test_distill_entry_is_declared_and_registered():
    from loans_amd import _lib
    assert 'loans_softmax_distill_fwd_f32' in _lib.SIGNATURES
    with open(os.path.join(ROOT, 'include', 'loans_hip.h')) as f:
        header = f.read()

    def declared(name):
        m = re.search(r'int %s\(([^;]*)\);' % name, header)
        assert m is not None, name
        return [a.strip() for a in re.sub(r'/\*.*?\*/', '', m.group(1), flags=re.S).split(',')]

    got, mix = declared('loans_softmax_distill_fwd_f32'), declared('loans_softmax_xent_mix_fwd_f32')
    # the mix entry's arguments with the teacher's logits behind the student's, the two row arrays behind the hits, then the
    # weight and the temperature, then the stream
    assert got == mix[:1] + ['const float* zt'] + mix[1:9] + ['float* row_kl', 'float* row_thit'] + mix[9:-1] + ['double alpha', 'double T'] + mix[-1:]
    sig = _lib.SIGNATURES['loans_softmax_distill_fwd_f32']
    assert len(sig) == len(got)
    assert sig[-3:] == [ctypes.c_double, ctypes.c_double, ctypes.c_void_p]


# ---- Classifier ---------------------------------------------------------------------------------------------------------------
def test_classifier_refuses_what_it_cannot_build():
    import loans_amd
    from loans_amd import functions
    from loans_amd.sheep.resnet import ResNet

    def build(**kw):
        return loans_amd.Classifier(loans_amd.Chain(), **kw)

    nan, inf = float('nan'), float('inf')
    for bad in (dict(distill_alpha=0.5), dict(distill_alpha=1.0), dict(teacher=loans_amd.Chain(), loss='bce'),
                dict(teacher=loans_amd.Chain(), distill_alpha=-0.1), dict(teacher=loans_amd.Chain(), distill_alpha=1.5),
                dict(teacher=loans_amd.Chain(), distill_alpha=nan), dict(teacher=loans_amd.Chain(), distill_alpha=0.5, distill_temperature=0.0),
                dict(teacher=loans_amd.Chain(), distill_alpha=0.5, distill_temperature=2.0 ** -7),
                dict(teacher=loans_amd.Chain(), distill_alpha=0.5, distill_temperature=65.0),
                dict(teacher=loans_amd.Chain(), distill_alpha=0.5, distill_temperature=nan),
                dict(teacher=loans_amd.Chain(), distill_alpha=0.5, distill_temperature=inf),
                dict(distill_temperature=0.0), dict(distill_alpha=-1.0)):
        with pytest.raises(ValueError):
            build(**bad)
    with pytest.raises(ValueError, match='classes'):
        loans_amd.Classifier(ResNet(18, class_labels=10), teacher=ResNet(18, class_labels=12), distill_alpha=0.5)
    teacher = ResNet(18, class_labels=10)
    model = loans_amd.Classifier(ResNet(18, class_labels=10), teacher=teacher, distill_alpha=0.25, distill_temperature=4.0, label_smoothing=0.1, topk=5)
    assert (model.teacher, model.distill_alpha, model.distill_temperature) == (teacher, 0.25, 4.0)
    # the teacher is no child link: its parameters are not the model's
    assert all(link is not teacher for link in model.links())
    own = {id(p) for p in model.params()}
    assert own and not own & {id(p) for p in teacher.params()}
    assert not any(k.startswith('teacher') or '/teacher' in k for k, _ in model.namedparams())
    plain = build()
    assert (plain.teacher, plain.distill_alpha, plain.distill_temperature) == (None, 0.0, 1.0)
    assert build(teacher=loans_amd.Chain()).distill_alpha == 0.0               # a teacher that is never run
    assert callable(functions.softmax_cross_entropy_distilled)
    for bad in (dict(alpha=1.5), dict(alpha=-0.5), dict(temperature=0.0), dict(temperature=128.0)):
        with pytest.raises(ValueError):
            functions.softmax_cross_entropy_distilled(None, None, None, **bad)


# ---- the trainer's options ----------------------------------------------------------------------------------------------------
NEW = ('teacher', 'teacher_arch', 'teacher_dtype', 'distill_alpha', 'distill_temperature')


def test_the_distill_options_parse_and_leave_the_default_namespace_alone():
    import train_imagenet as T
    bare = T.parse_args([])
    assert not set(NEW) & set(vars(bare))                                     # class-level defaults, not parsed values
    assert tuple(getattr(bare, n) for n in NEW) == (None, 'resnet50', None, None, 1.0)
    assert set(T.Arguments._DISTILL) == set(NEW) and not set(NEW) & set(T.RESUME_FIXED)
    assert not set(NEW) & set(T.RESUME_DEFAULTS_WITH_ACCUM)
    only = T.parse_args(['--teacher', 'a.npz'])
    assert set(vars(only)) == set(vars(bare)) | {'teacher'}
    assert T.distill_options(only) == (0.5, 1.0, 'f32')
    assert T.distill_options(T.parse_args(['--teacher', 'a.npz', '--dtype', 'bf16'])) == (0.5, 1.0, 'bf16')
    args = T.parse_args(['--teacher', 'a_ema_10.npz', '--teacher-arch', 'resnet18', '--teacher-dtype', 'fp32', '--distill-alpha', '0.25',
                         '--distill-temperature', '4', '--dtype', 'bf16', '--use-resnet-18'])
    assert tuple(getattr(args, n) for n in NEW) == ('a_ema_10.npz', 'resnet18', 'fp32', 0.25, 4.0)
    assert set(vars(args)) == set(vars(bare)) | set(NEW)
    assert T.distill_options(args) == (0.25, 4.0, 'f32')
    assert T.distill_options(T.parse_args(['--teacher', 'a.npz', '--teacher-dtype', 'bf16'])) == (0.5, 1.0, 'bf16')
    for a in (bare, only, args, T.parse_args(['--teacher', 'a.npz', '--distill-alpha', '1', '--distill-temperature', '64', '--label-smoothing', '0.1',
                                             '--optimizer', 'lamb', '--accum-steps', '2', '--ema-decay', '0.99', '--drop-path', '0.1'])):
        T.check_distill_arguments(a)


@pytest.mark.parametrize('argv', [
    ['--teacher-arch', 'resnet18'],                                 # the options belong to --teacher
    ['--teacher-dtype', 'bf16'],
    ['--distill-alpha', '0.5'],
    ['--distill-temperature', '1.0'],
    ['--teacher', 'a.npz', '--distill-alpha', '0'],
    ['--teacher', 'a.npz', '--distill-alpha', '-0.1'],
    ['--teacher', 'a.npz', '--distill-alpha', '1.5'],
    ['--teacher', 'a.npz', '--distill-alpha', 'nan'],
    ['--teacher', 'a.npz', '--distill-temperature', '0'],
    ['--teacher', 'a.npz', '--distill-temperature', '0.0078125'],
    ['--teacher', 'a.npz', '--distill-temperature', '65'],
    ['--teacher', 'a.npz', '--distill-temperature', 'nan'],
    ['--teacher', 'a.npz', '--distill-temperature', 'inf'],
    ['--teacher', 'a.npz', '--loss', 'bce'],
])
def test_the_distill_options_are_refused_by_the_parser_and_by_the_check(argv, capsys):
    import train_imagenet as T
    with pytest.raises(SystemExit):
        T.parse_args(argv)
    capsys.readouterr()
    # the same values on a namespace that never went through the parser (``run`` calls the check too)
    args = T.Arguments()
    it = iter(argv)
    for flag in it:
        name = flag[2:].replace('-', '_')
        value = next(it)
        setattr(args, name, float(value) if name in ('distill_alpha', 'distill_temperature') else value)
    with pytest.raises(ValueError):
        T.check_distill_arguments(args)


def test_unknown_architecture_and_dtype_are_refused():
    import train_imagenet as T
    for name, value in (('teacher_arch', 'resnet101'), ('teacher_dtype', 'fp16')):
        args = T.Arguments()
        args.teacher = 'a.npz'
        setattr(args, name, value)
        with pytest.raises(ValueError):
            T.check_distill_arguments(args)
        with pytest.raises(SystemExit):
            T.parse_args(['--teacher', 'a.npz', '--' + name.replace('_', '-'), value])
