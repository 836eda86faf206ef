"""-m gpu: the test-mode forward (``config.train`` false: BatchNormalization on running statistics) through the model surface,
against the float64 oracle composed in tests/eval_mode/cases.py: ``Classifier(SheepLocalizer(train_imagenet=True, **options))``
plain, with ``se_ratio=16``, with ``blur_pool=True`` and with both, the bf16 storage arm of the first and the last, and one strided
chainercv bottleneck with and without the blur.  Logits and loss within tests/imagenet/test_gpu_model._tol (bf16: cases.tol_bf16),
accuracy and top-5 accuracy equal; nothing is written; samples do not couple; backward is refused; the running averages a training
step leaves are the oracle's and are what the next test-mode forward reads; training mode without backprop is training mode.

The running statistics are far from the batch statistics: tests/eval_mode/test_cases_cpu.py asserts that the training-mode logits
of every variant lie at least 100 fp32 bounds from the test-mode ones (measured: 1323 to 1805) and, in the bf16 arms, at least 30
bf16 bounds (measured: 32 and 42; cases.BF16_SEPARATION), so a path that used batch statistics fails the logit comparisons here."""
import numpy as np
import pytest
import torch

import loans_amd
from loans_amd import ops
from loans_amd.runtime.core import Variable
from oracle import model as M
from tests.eval_mode import cases as K
from tests.gpu_util import dev
from tests.imagenet import reference as R
from tests.imagenet import test_gpu_model as G

pytestmark = pytest.mark.gpu
ARMS = [(v, False) for v in K.VARIANTS] + [(v, True) for v in K.BF16_ARMS]
arm_id = lambda a: a[0] + ('-bf16' if a[1] else '')        # noqa: E731


def _model(variant, bf16=False):
    loc = K.build_localizer(variant)
    model = loans_amd.Classifier(loc, topk=K.TOPK)
    if bf16:
        model.set_precision('bf16', 'bf16')
    model.to_gpu(0)
    return model, loc


def _snapshot(link):
    return {k: np.array(v, copy=True) for k, v in link.state_dict_chainer().items()}


def _assert_same_bits(before, after):
    assert set(before) == set(after)
    for k in before:
        a, b = np.asarray(before[k]), np.asarray(after[k])
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), k


def _test_forward(model, frames, t):
    """(logits, loss, accuracy, top-k accuracy) of a test-mode forward without backprop"""
    with loans_amd.using_config('train', False), loans_amd.using_config('enable_backprop', False):
        model(dev(frames), dev(t))
    return model.y.data.cpu().numpy(), float(model.loss.data), float(model.accuracy.data), float(model.accuracy_topk.data)


def _report(name, got, r64, bound):
    got, r64, bound = (np.atleast_1d(np.asarray(a, np.float64)) for a in (got, r64, bound))
    err = np.abs(got - r64)
    i = np.unravel_index(np.argmax(err / bound), err.shape)
    print('%s: worst error / bound %.3g (there: %.7g for %.7g, bound %.3g; max error %.3g, largest |ref| %.4g)'
          % (name, float(err[i] / bound[i]), got[i], r64[i], bound[i], float(err.max()), float(np.abs(r64).max())))
    assert np.all(err <= bound), name


@pytest.mark.parametrize('arm', ARMS, ids=arm_id)
def test_forward_in_test_mode_and_nothing_moves(arm):
    variant, bf16 = arm
    frames, t = K.frames3()[:2], K.labels(variant)[:2]
    model, loc = _model(variant, bf16)
    before = _snapshot(loc)
    model.arena.grad.fill_(1.25)
    z, loss, acc, acck = _test_forward(model, frames, t)
    r64, bound = K.model_tol(variant, bf16, slice(0, 2))
    other = K.reference(variant, 'bf16' if bf16 else 'f32').logits[:2]
    if bf16:
        print('%s: the emulated fp32 oracle is %.4g from the float64 oracle' % (variant, float(np.abs(other - r64).max())))
    _report('logits', z, r64, bound)
    loss64, acc64, acck64 = K.metrics(r64, t)
    loss_o = K.metrics(other, t)[0]
    _report('loss', loss, loss64, (K.tol_bf16 if bf16 else G._tol)(loss_o, loss64))
    assert (acc, acck) == (acc64, acck64) == (0.5, 1.0)         # decided within the bound of either arm (cases.label_margin)
    loss_own, acc_own, acck_own = K.metrics(z, t)               # and the loss kernel on the logits it was given
    assert abs(loss - loss_own) <= R.row_bounds(z, t)[2] and (acc, acck) == (acc_own, acck_own)
    # nothing moves: parameters, running statistics, counters, the gradient arena
    ops.join_side_stream()
    torch.cuda.synchronize()
    _assert_same_bits(before, _snapshot(loc))
    assert bool((model.arena.grad == 1.25).all())


@pytest.mark.parametrize('blur_pool', [False, True], ids=['plain', 'blur'])
def test_a_single_strided_bottleneck_in_test_mode(blur_pool):
    """1 x 1 -> 3 x 3 -> 1 x 1 with a 1 x 1 shortcut: the test-mode arm of the bottleneck units without a whole ResNet-50"""
    blk, x = K.build_bottleneck(blur_pool)
    blk.finalize(torch.device('cuda', 0))
    before = _snapshot(blk)
    blk.arena.grad.fill_(1.25)
    with loans_amd.using_config('train', False), loans_amd.using_config('enable_backprop', False):
        out = blk(Variable(dev(np.ascontiguousarray(x.transpose(0, 2, 3, 1))), requires_grad=False))
    ref = {}
    for dtype in (np.float32, np.float64):
        unit = K.RefUnit(M.cast_params(dict(before), dtype), K.BOTTLENECK_STAGES, K.BOTTLENECK_SHORTCUT, False, blur_pool)
        ref[dtype] = unit.fwd(x.astype(dtype))
        assert dtype != np.float64 or min(np.abs(a).min() for a in unit.pre) >= 1e-6
    assert tuple(out.shape) == (4, 5, 5, 128)
    _report('out', out.data.cpu().numpy().transpose(0, 3, 1, 2), ref[np.float64], G._tol(ref[np.float32], ref[np.float64]))
    torch.cuda.synchronize()
    _assert_same_bits(before, _snapshot(blk))
    assert bool((blk.arena.grad == 1.25).all())
    with loans_amd.using_config('train', False):
        out = blk(Variable(dev(np.ascontiguousarray(x.transpose(0, 2, 3, 1))), requires_grad=True))
        out.grad = torch.ones_like(out.data)
        with pytest.raises(RuntimeError, match='test-mode BatchNormalization'):
            out.backward()


@pytest.mark.parametrize('variant', list(K.VARIANTS))
def test_no_coupling_across_samples(variant):
    """sample b alone, in the batch of two and in the batch of three: launch plans may differ with B, the bound does not"""
    frames, t = K.frames3(), K.labels(variant)
    model, _ = _model(variant)
    r64, bound = K.model_tol(variant, False)
    z3 = _test_forward(model, frames, t)[0]
    z2 = _test_forward(model, frames[:2], t[:2])[0]
    _report('B = 3', z3, r64, bound)
    _report('B = 2', z2, r64[:2], bound[:2])
    for b in range(3):
        z1 = _test_forward(model, frames[b:b + 1], t[b:b + 1])[0]
        _report('sample %d alone' % b, z1[0], r64[b], bound[b])
        _report('sample %d alone against the batch of three' % b, z1[0], z3[b].astype(np.float64), bound[b])
        if b < 2:
            _report('sample %d alone against the batch of two' % b, z1[0], z2[b].astype(np.float64), bound[b])


@pytest.mark.parametrize('variant', list(K.VARIANTS))
def test_backward_is_refused(variant):
    model, _ = _model(variant)
    with loans_amd.using_config('train', False):
        loss = model(dev(K.frames3()[:2]), dev(K.labels(variant)[:2]))
        model.cleargrads()
        with pytest.raises(RuntimeError, match='test-mode BatchNormalization is not on the training path'):
            loss.backward()
    ops.join_side_stream()
    torch.cuda.synchronize()


@pytest.mark.parametrize('variant', ['se', 'blur', 'se_blur'])
def test_the_state_that_test_mode_reads(variant):
    """One training step on the device; the oracle's training forward writes the running averages it should have left (a blurred
    stage takes its statistics over the full-resolution map: count B H W at stride 1, which only the unbiased-variance correction
    of avg_var shows).  Then the test-mode forward reads them: its logits against the oracle in test mode on the oracle's running
    averages and the parameters the device's optimiser left -- Adam's first step is sign-like, so the oracle's own updated
    parameters are comparable only where the gradients agree in sign (tests/imagenet/test_gpu_model.py)."""
    frames, t = K.frames3()[:2], K.labels(variant)[:2]
    model, loc = _model(variant)
    opt = loans_amd.Adam(alpha=1e-3, amsgrad=True)
    opt.setup(model)
    opt.update(model, dev(frames), dev(t))
    ops.join_side_stream()
    torch.cuda.synchronize()
    state = loc.state_dict_chainer()
    o64, o32 = K.reference(variant, 'f64', train=True).p, K.reference(variant, 'f32', train=True).p
    start = K.start_params(variant)
    keys = [k[:-len('/avg_mean')] for k in state if k.endswith('/avg_mean')]
    assert len(keys) == 21 and set(K.STATE_KEYS) <= set(keys)
    worst = {}
    for bn in keys:
        for name, atol in (('/avg_mean', 1e-5), ('/avg_var', 1e-6)):
            got, want = state[bn + name], o64[bn + name]
            assert not np.array_equal(got, start[bn + name]), bn + name
            err = np.abs(got - want) / (atol + 1e-4 * np.abs(want))
            worst[name] = max(worst.get(name, 0.0), float(err.max()))
            if bn in K.STATE_KEYS:
                print('%s%s: worst error / (atol + rtol |ref|) %.3g' % (bn, name, float(err.max())))
            np.testing.assert_allclose(got, want, rtol=1e-4, atol=atol, err_msg=bn + name)
    print('all 21 BNs: %s' % worst)
    refs = []
    for dtype, running in ((np.float32, o32), (np.float64, o64)):
        p = {k: (running[k] if k.endswith(('/avg_mean', '/avg_var')) else v) for k, v in state.items()}
        refs.append(K.run(p, variant, frames, False, dtype).logits)
    assert np.abs(refs[1] - K.reference(variant, 'f64').logits[:2]).max() > 100 * G._tol(refs[0], refs[1]).max()      # the state moved
    _report('test-mode logits after the step', _test_forward(model, frames, t)[0], refs[1], G._tol(refs[0], refs[1]))


@pytest.mark.parametrize('variant', ['plain', 'se_blur'])
def test_training_mode_without_gradient(variant, deterministic_forward):
    """``train=True, enable_backprop=False``: the training-mode forward (batch statistics), and the same running averages, bit for
    bit, as the forward that keeps its graph"""
    frames, t = K.frames3()[:2], K.labels(variant)[:2]
    r64, r32 = K.reference(variant, 'f64', train=True), K.reference(variant, 'f32', train=True)
    states = []
    for backprop in (False, True):
        model, loc = _model(variant)
        with loans_amd.using_config('enable_backprop', backprop):
            model(dev(frames), dev(t))
        ops.join_side_stream()
        torch.cuda.synchronize()
        _report('logits, backprop %s' % backprop, model.y.data.cpu().numpy(), r64.logits, G._tol(r32.logits, r64.logits))
        states.append(_snapshot(loc))
    moved = [k for k in states[0] if k.endswith(('/avg_mean', '/avg_var'))]
    assert len(moved) == 42 and not any(np.array_equal(states[0][k], K.start_params(variant)[k]) for k in moved)
    _assert_same_bits(states[0], states[1])
    np.testing.assert_allclose(states[0][K.FE + 'bn1/avg_var'], r64.p[K.FE + 'bn1/avg_var'], rtol=1e-4, atol=1e-6)
