"""No GPU, no launch: the fp32 restatement of the sigmoid binary cross-entropy held to the derived bound over the case grid, the
float64 reference against torch's ``binary_cross_entropy_with_logits``, the threshold's edge, the entry's argument checks, and the
options of ``Classifier`` and of the trainer with their resume rules."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from loans_amd.runtime import checkpoint
from tests.imagenet import reference as R
from tests.imagenet_bce import reference as Q
from tests.imagenet_mix import reference as X

K = 2
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def check_case(c, ta, tb, wa, wb, eps, thresh, sum_classes, tag, extremes, worst=None):
    ref = Q.bce_ref(c, ta, tb, wa, wb, eps, K, thresh, sum_classes)
    lb, gb, bb = Q.bce_bounds(c, ta, tb, wa, wb, eps, thresh, sum_classes)
    f_loss, f_acc, f_acck, f_gz, f_row = Q.bce_fp32(c, ta, tb, wa, wb, eps, K, thresh, sum_classes)
    loss, acc, acck, gz, row_loss, hit, hitk = ref
    err = np.abs(f_row.astype(np.float64) - row_loss)
    gerr = np.abs(f_gz.astype(np.float64) - gz)
    assert np.all(err <= lb), tag + (float((err - lb).max()),)
    assert np.all(gerr <= gb), tag + (float((gerr - gb).max()),)
    assert abs(f_loss - loss) <= bb, tag + (f_loss, loss, bb)
    assert f_acc == float(np.float32(acc)) and f_acck == float(np.float32(acck)), tag           # the hits are equal exactly
    valid = lb > 0
    if extremes:
        assert np.all(np.isfinite(f_row)) and np.all(np.isfinite(row_loss)), tag
        assert np.all(np.abs(f_gz) <= np.float32(Q.gz_limit(max(int(valid.sum()), 1), c.N, sum_classes))), tag
    if not valid.any():
        assert f_loss == 0.0 and not f_gz.any() and not f_row.any() and not hit.any() and not hitk.any(), tag
    elif worst is not None:
        worst['loss'] = max(worst['loss'], float((err[valid] / lb[valid]).max()))
        worst['gz'] = max(worst['gz'], float((gerr[valid] / gb[valid]).max()))
        worst['batch'] = max(worst['batch'], abs(f_loss - loss) / bb)
    return ref


# ---- reference, restatement and bound -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', Q.BCE_N)
def test_restatement_is_inside_the_bound_over_the_grid_and_the_threshold_leaves_out_no_case(N):
    worst = {'loss': 0.0, 'gz': 0.0, 'batch': 0.0}
    cases = near = 0
    for name, c, ta, tb, t, expect, extremes in Q.bce_cases(N):
        assert R.argmax_margin_ok(c.z32), name
        for lam in X.LAMS:
            wa, wb = X.weights(lam)
            for eps in Q.BCE_EPS:
                for thresh in Q.THRESH:
                    # no rounding of the soft target crosses a threshold anywhere in the grid: every case is checked
                    assert not Q.threshold_ambiguous(N, ta, tb, wa, wb, eps, thresh), (name, lam, eps, thresh)
                    near += Q.near_threshold(N, ta, tb, wa, wb, eps, thresh) > 0
                    for sum_classes in (False, True):
                        tag = (name, lam, eps, thresh, sum_classes)
                        ref = check_case(c, ta, tb, wa, wb, eps, thresh, sum_classes, tag, extremes, worst)
                        if expect is not None and np.array_equal(ta if wa >= wb else tb, t):
                            # the tie expectations, against the dominant label: the first of two equal maxima is the hit
                            np.testing.assert_array_equal(ref[5], expect & (Q.bce_bounds(c, ta, tb, wa, wb, eps)[0] > 0), err_msg=name)
                        cases += 1
    assert cases == len(Q.BCE_B) * Q.profiles(N) * len(X.PAIRS) * len(X.LAMS) * len(Q.BCE_EPS) * len(Q.THRESH) * 2
    # the first-order band names the one configuration reference.py describes, and nothing else
    assert (near > 0) == (N == 2)
    print('N=%d worst error / bound: row loss %.3f, gz %.3f, batch loss %.3f' % (N, worst['loss'], worst['gz'], worst['batch']))


def test_restatement_at_the_lds_limit():
    c, ta, tb = Q.lds_limit_case()
    assert (c.B, c.N) == (2, 8192)
    wa, wb = X.weights(np.float32(0.3))
    for thresh in Q.THRESH:
        for sum_classes in (False, True):
            assert not Q.threshold_ambiguous(c.N, ta, tb, wa, wb, 0.1, thresh)
            check_case(c, ta, tb, wa, wb, 0.1, thresh, sum_classes, ('lds', thresh, sum_classes), False)


def test_float64_reference_known_answers():
    # z = 0: e = 1, every element costs log 2 whatever its target, the sigmoid is 1 / 2
    N, B = 4, 3
    z = np.zeros((B, N))
    ta, tb = np.array([0, 1, 2]), np.array([3, 1, -1])
    wa, wb = X.weights(0.3)
    loss, acc, acck, gz, row_loss, hit, hitk = Q.bce_ref(z, ta, tb, wa, wb, 0.0, 2)
    np.testing.assert_allclose(row_loss, [N * np.log(2), N * np.log(2), 0.0], rtol=1e-15)
    assert loss == pytest.approx(np.log(2), rel=1e-15)                       # two rows count: / (2 N)
    assert Q.bce_ref(z, ta, tb, wa, wb, 0.0, 2, sum_classes=True)[0] == pytest.approx(N * np.log(2), rel=1e-15)
    np.testing.assert_allclose(gz[0], (0.5 - np.array([wa, 0, 0, wb])) / (2 * N), rtol=1e-15)
    np.testing.assert_allclose(gz[1], (0.5 - np.array([0, wa + wb, 0, 0])) / (2 * N), rtol=1e-15)
    assert not gz[2].any()
    # thresh = 0.2: both labels of row 0 (0.3 and 0.7) become positives; thresh = 0.5: the larger one only
    np.testing.assert_allclose(Q.bce_ref(z, ta, tb, wa, wb, 0.0, 2, 0.2)[3][0], (0.5 - np.array([1, 0, 0, 1])) / (2 * N), rtol=1e-15)
    np.testing.assert_allclose(Q.bce_ref(z, ta, tb, wa, wb, 0.0, 2, 0.5)[3][0], (0.5 - np.array([0, 0, 0, 1])) / (2 * N), rtol=1e-15)
    # one logit, by hand: l = max(z, 0) - z q + log(1 + exp(-|z|))
    got = Q.bce_ref(np.array([[2.0, -3.0]]), [0], [0], 1.0, 0.0, 0.0, 1)
    want = (2.0 - 2.0 + np.log1p(np.exp(-2.0))) + np.log1p(np.exp(-3.0))
    assert got[4][0] == pytest.approx(want, rel=1e-15) and got[0] == pytest.approx(want / 2, rel=1e-15)
    # the one-label weights: the label of weight zero is not read
    zz = np.random.RandomState(0).standard_normal((B, N))
    for w, t in (((1.0, 0.0), ta), ((0.0, 1.0), tb)):
        a = Q.bce_ref(zz, ta, tb, w[0], w[1], 0.1, 2, 0.2)
        b = Q.bce_ref(zz, t, t, w[0], w[1], 0.1, 2, 0.2)
        c = Q.bce_ref(zz, t if w[0] else np.full(B, -1), np.full(B, -1) if w[0] else t, w[0], w[1], 0.1, 2, 0.2)
        for x, y, v in zip(a, b, c):
            np.testing.assert_array_equal(np.asarray(x), np.asarray(y))
            np.testing.assert_array_equal(np.asarray(x), np.asarray(v))


@pytest.mark.parametrize('sum_classes', (False, True))
@pytest.mark.parametrize('thresh', Q.THRESH)
@pytest.mark.parametrize('eps', Q.BCE_EPS)
def test_float64_reference_is_torch_binary_cross_entropy_with_logits(eps, thresh, sum_classes):
    """a dense target built here, independently; batches without ignored rows; 1e-12 relative (the gradient: relative to its
    scale 1 / denom, the difference sigmoid - target of two numbers of order one being formed on both sides)"""
    F = torch.nn.functional
    for N, B in ((1, 5), (2, 5), (257, 5), (1000, 3)):
        for profile in ('normal', 'dominant', Q.EXTREMES):
            rng = np.random.Generator(np.random.PCG64([N, B, 5]))
            z = Q.extreme_logits(B, N) if profile == Q.EXTREMES else R.make_logits(profile, B, N, rng)
            t = R.make_labels('first_last', B, N, None)
            for kind in ('different', 'equal'):
                ta, tb = X.label_pair(kind, t, N)
                for lam in X.LAMS:
                    wa, wb = X.weights(lam)
                    dense = np.zeros((B, N))
                    for b in range(B):
                        dense[b, ta[b]] += wa
                        dense[b, tb[b]] += wb
                    dense = float(np.float32(1.0 - eps)) * dense + float(np.float32(eps / N))
                    if thresh is not None:
                        dense = (dense > float(np.float32(thresh))).astype(np.float64)
                    zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
                    want = F.binary_cross_entropy_with_logits(zt, torch.from_numpy(dense), reduction='sum' if sum_classes else 'mean')
                    if sum_classes:
                        want = want / B
                    want.backward()
                    got = Q.bce_ref(z, ta, tb, wa, wb, eps, K, thresh, sum_classes)
                    assert got[0] == pytest.approx(want.item(), rel=1e-12), (N, profile, kind, lam)
                    scale = 1.0 / (B if sum_classes else B * N)
                    np.testing.assert_allclose(got[3], zt.grad.numpy(), rtol=1e-12, atol=1e-12 * scale)


def test_threshold_edge_is_exact_and_strict():
    N, B = 5, 2
    z = np.random.RandomState(1).standard_normal((B, N)).astype(np.float32)
    ta, tb = np.array([0, 4], np.int32), np.array([3, 1], np.int32)
    wa, wb = X.weights(0.5)
    assert (wa, wb) == (0.5, 0.5)
    ia, ib = ta.astype(np.int64), tb.astype(np.int64)
    # the soft target is 0.5 in both precisions, with or without a contraction ...
    for q in (Q.target64(N, ia, ib, wa, wb, 0.0, None), Q.target32(N, ia, ib, wa, wb, 0.0, None), Q.target32(N, ia, ib, wa, wb, 0.0, None, True)):
        assert q[0].tolist() == [0.5, 0, 0, 0.5, 0] and q[1].tolist() == [0, 0.5, 0, 0, 0.5]
    # ... and the strict comparison makes both 0
    assert not Q.target64(N, ia, ib, wa, wb, 0.0, 0.5).any() and not Q.target32(N, ia, ib, wa, wb, 0.0, 0.5).any()
    assert not Q.threshold_ambiguous(N, ta, tb, wa, wb, 0.0, 0.5) and Q.near_threshold(N, ta, tb, wa, wb, 0.0, 0.5) == 0
    ref = Q.bce_ref(z, ta, tb, wa, wb, 0.0, K, 0.5)
    np.testing.assert_allclose(ref[3], Q.Logits(z).s / (B * N), rtol=1e-15)
    check_case(Q.Logits(z), ta, tb, wa, wb, 0.0, 0.5, False, ('edge',), False)
    # just below the threshold both become positives
    assert Q.target64(N, ia, ib, wa, wb, 0.0, 0.49).sum() == 4
    # a target that a rounding carries across a threshold is named: a threshold equal to the rounded target, which lies below
    # the target itself, is exceeded in float64 and not in fp32
    named = 0
    for n in range(2, 40):
        one = np.array([0], np.int64)
        q64, q32 = Q.target64(n, one, one, 1.0, 0.0, 0.1, None)[0, 0], float(Q.target32(n, one, one, 1.0, 0.0, 0.1, None)[0, 0])
        if q32 < q64:
            assert Q.threshold_ambiguous(n, one, one, 1.0, 0.0, 0.1, q32) and Q.near_threshold(n, one, one, 1.0, 0.0, 0.1, q32) > 0
            named += 1
    assert named > 0


# ---- the entry without a GPU --------------------------------------------------------------------------------------------------
def test_bce_entry_checks_its_arguments_before_any_hip_call():
    from loans_amd import _lib
    f = _lib.load().loans_sigmoid_bce_fwd_f32
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    inf, nan = float('inf'), float('nan')

    def call(ptrs=None, lam=0.5, oml=0.5, B=4, N=8, eps=0.1, k=1, thresh=-1.0, sum_classes=0):
        z, ta, tb, gz, rl, rh, rhk, out = ptrs or [p] * 8
        return f(z, ta, tb, lam, oml, gz, rl, rh, rhk, out, B, N, eps, k, thresh, sum_classes, 0)

    for lam, oml in ((0.5, 0.5), (1.0, 0.0), (0.0, 1.0)):
        for thresh in (-1.0, 0.2):
            kw = dict(lam=lam, oml=oml, thresh=thresh)
            for missing in range(8):
                if missing == 2:
                    continue                # a null tb is one label (below)
                ptrs = [p] * 8
                ptrs[missing] = 0
                assert call(ptrs, **kw) == -1, (lam, oml, missing)
            assert call(k=0, **kw) == -1
            assert call(B=0, **kw) == -1 and call(N=0, **kw) == -1 and call(B=-3, **kw) == -1 and call(N=-1, **kw) == -1
            assert call(eps=1.0, **kw) == -1 and call(eps=-0.1, **kw) == -1 and call(eps=nan, **kw) == -1
            assert call(N=8193, **kw) == -2 and call(B=65537, **kw) == -2
            for sum_classes in (0, 1):
                assert call(sum_classes=sum_classes, k=0, **kw) == -1
    for lam, oml in ((nan, 0.5), (0.5, inf), (-inf, 0.0)):
        assert call(lam=lam, oml=oml) == -1
    for thresh in (1.0, 1.5, inf, nan):
        assert call(thresh=thresh) == -1, thresh
    # one label (tb null): the same checks, and the limits
    one = [p, p, 0, p, p, p, p, p]
    assert call(one, k=0) == -1 and call(one, eps=1.0) == -1 and call(one, thresh=1.0) == -1 and call(one, B=0) == -1
    assert call([p, 0, 0, p, p, p, p, p]) == -1
    assert call(one, N=8193) == -2 and call(one, B=65537) == -2
    assert bytes(buf) == bytes(64)


def test_bce_entry_is_declared_and_registered():
    from loans_amd import _lib
    assert 'loans_sigmoid_bce_fwd_f32' in _lib.SIGNATURES
    with open(os.path.join(ROOT, 'include', 'loans_hip.h')) as f:
        header = f.read()
    m = re.search(r'int loans_sigmoid_bce_fwd_f32\(([^;]*)\);', header)
    assert m is not None
    declared = [a.strip() for a in re.sub(r'/\*.*?\*/', '', m.group(1), flags=re.S).split(',')]
    mix = [a.strip() for a in re.sub(r'/\*.*?\*/', '', re.search(r'int loans_softmax_xent_mix_fwd_f32\(([^;]*)\);', header).group(1),
                                     flags=re.S).split(',')]
    # the mix entry's arguments, then the threshold and the reduction, then the stream
    assert declared == mix[:-1] + ['float thresh', 'int32_t sum_classes'] + mix[-1:]
    assert len(_lib.SIGNATURES['loans_sigmoid_bce_fwd_f32']) == len(declared)
    assert _lib.SIGNATURES['loans_sigmoid_bce_fwd_f32'][:14] == _lib.SIGNATURES['loans_softmax_xent_mix_fwd_f32'][:14]
    assert _lib.SIGNATURES['loans_sigmoid_bce_fwd_f32'][14:] == [ctypes.c_float, ctypes.c_int32, ctypes.c_void_p]


# ---- Classifier ---------------------------------------------------------------------------------------------------------------
def test_classifier_refuses_what_it_cannot_build():
    import loans_amd
    from loans_amd import functions

    def build(**kw):
        return loans_amd.Classifier(loans_amd.Chain(), **kw)

    for bad in (dict(loss='hinge'), dict(loss=None), dict(loss='bce', bce_target_threshold=1.0), dict(loss='bce', bce_target_threshold=-0.1),
                dict(loss='bce', bce_target_threshold=float('nan')), dict(bce_target_threshold=0.2), dict(bce_sum=True),
                dict(loss='softmax', bce_target_threshold=0.0), dict(loss='softmax', bce_sum=True)):
        with pytest.raises(ValueError):
            build(**bad)
    model = build(loss='bce', bce_target_threshold=0.2, bce_sum=True, label_smoothing=0.1, topk=5)
    assert (model.loss_name, model.bce_target_threshold, model.bce_sum) == ('bce', 0.2, True)
    assert build(loss='bce', bce_target_threshold=0.0).bce_target_threshold == 0.0
    plain = build()
    assert (plain.loss_name, plain.bce_target_threshold, plain.bce_sum) == ('softmax', None, False)
    assert callable(functions.sigmoid_binary_cross_entropy)
    with pytest.raises(ValueError):
        functions.sigmoid_binary_cross_entropy(None, None, target_threshold=1.0)


# ---- the trainer's options ----------------------------------------------------------------------------------------------------
NEW = ('loss', 'bce_target_thresh', 'bce_sum')


def test_the_loss_options_parse_and_leave_the_default_namespace_alone():
    import train_imagenet as T
    bare = T.parse_args([])
    assert not set(NEW) & set(vars(bare))                                     # class-level defaults, not parsed values
    assert tuple(getattr(bare, n) for n in NEW) == ('softmax', None, False)
    assert T.loss_options(bare) == {}
    args = T.parse_args(['--loss', 'bce', '--bce-target-thresh', '0.2', '--bce-sum'])
    assert tuple(getattr(args, n) for n in NEW) == ('bce', 0.2, True)
    assert set(vars(args)) == set(vars(bare)) | set(NEW)
    assert T.loss_options(args) == dict(loss='bce', bce_target_threshold=0.2, bce_sum=True)
    only = T.parse_args(['--loss', 'bce'])
    assert set(vars(only)) == set(vars(bare)) | {'loss'} and T.loss_options(only) == dict(loss='bce', bce_target_threshold=None, bce_sum=False)
    assert set(T.Arguments._LOSS) == set(NEW) and not set(NEW) & set(T.RESUME_FIXED)
    for a in (bare, args, only, T.parse_args(['--loss', 'softmax'])):
        T.check_loss_arguments(a)


@pytest.mark.parametrize('argv', [
    ['--bce-target-thresh', '0.2'],                                 # the BCE options belong to --loss bce
    ['--bce-sum'],
    ['--loss', 'softmax', '--bce-target-thresh', '0.2'],
    ['--loss', 'softmax', '--bce-sum'],
    ['--loss', 'bce', '--bce-target-thresh', '1.0'],
    ['--loss', 'bce', '--bce-target-thresh', '-0.1'],
    ['--loss', 'bce', '--bce-target-thresh', 'nan'],
])
def test_the_loss_options_are_refused_by_the_parser_and_by_the_check(argv, capsys):
    import train_imagenet as T
    with pytest.raises(SystemExit):
        T.parse_args(argv)
    capsys.readouterr()
    # the same values on a namespace that never went through the parser (``run`` calls the check too)
    args = T.Arguments()
    it = iter(argv)
    for flag in it:
        name = flag[2:].replace('-', '_')
        setattr(args, name, True if name == 'bce_sum' else (next(it) if name == 'loss' else float(next(it))))
    with pytest.raises(ValueError, match='bce'):
        T.check_loss_arguments(args)
    with pytest.raises(ValueError):
        args = T.Arguments()
        args.loss = 'hinge'
        T.check_loss_arguments(args)


def test_a_checkpoint_from_before_the_options_resumes_at_their_defaults_and_a_changed_loss_is_a_line():
    import train_imagenet as T
    assert T.RESUME_DEFAULTS_LOSS == {'loss': 'softmax', 'bce_target_thresh': None, 'bce_sum': False}
    assert T.RESUME_DEFAULTS_WITH_LOSS == dict(T.RESUME_DEFAULTS_WITH_CLIP, **T.RESUME_DEFAULTS_LOSS)
    assert set(T.RESUME_DEFAULTS_WITH_CLIP) < set(T.RESUME_DEFAULTS_WITH_LOSS)
    args = T.parse_args([])
    saved = {k: v for k, v in checkpoint.plain_arguments(args).items() if k not in NEW}
    fixed = [k for k in T.RESUME_FIXED if k != 'gpus']
    assert checkpoint.check_arguments(saved, args, fixed, checkpoint.SILENT, T.RESUME_DEFAULTS_WITH_LOSS) == []
    bce = T.parse_args(['--loss', 'bce', '--bce-target-thresh', '0.2'])
    lines = checkpoint.check_arguments(saved, bce, fixed, checkpoint.SILENT, T.RESUME_DEFAULTS_WITH_LOSS)
    assert lines == ["resume: bce_target_thresh was None, is now 0.2", "resume: loss was 'softmax', is now 'bce'"]
    # a checkpoint that holds the keys is compared as it is; back to softmax is a line too
    now = checkpoint.plain_arguments(bce)
    assert checkpoint.check_arguments(now, bce, fixed, checkpoint.SILENT, T.RESUME_DEFAULTS_WITH_LOSS) == []
    back = checkpoint.check_arguments(now, args, fixed, checkpoint.SILENT, T.RESUME_DEFAULTS_WITH_LOSS)
    assert "resume: loss was 'bce', is now 'softmax'" in back and len(back) == 2
