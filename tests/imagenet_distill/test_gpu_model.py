"""-m gpu: ``Classifier(ResNet(18, class_labels=10), teacher=ResNet(18, class_labels=10), ...)`` at the shapes, with the helpers and
at the tolerances of tests/imagenet/test_gpu_model.py: one training step against ``R.ResNet18Classifier`` with its loss and gz
replaced by the float64 distillation reference (the teacher's logits from the same oracle in test mode), the teacher left bit for
bit and outside arena, optimiser and serialisation, the step arena on and off, and test mode / ``evaluate`` unchanged."""
import numpy as np
import pytest
import torch

import loans_amd
from loans_amd import ops
from loans_amd.datasets import synthetic
from loans_amd.runtime import training
from oracle import model as M
from tests.gpu_util import dev, rel_err
from tests.imagenet import reference as R
from tests.imagenet import test_gpu_model as G
from tests.imagenet_distill import reference as D

pytestmark = pytest.mark.gpu
B, H, W = G.B, G.H, G.W
ALPHA, TEMP, SMOOTH, TOPK, LAM = 0.5, 4.0, 0.1, 2, 0.3


def _teacher(seed=20):
    """a ResNet-18 with running statistics away from (0, 1), as a trained one has"""
    _, net = G._classifier(seed)
    rng = np.random.RandomState(seed + 1)
    for _, link, name in net.namedpersistents():
        v = getattr(link, name)
        if name == 'avg_mean':
            v[...] = 0.1 * rng.standard_normal(v.shape)
        elif name == 'avg_var':
            v[...] = 1.0 + 0.2 * rng.random_sample(v.shape)
    return net


def _snapshot(net):
    return {k: np.array(v, copy=True) for k, v in net.state_dict_chainer().items()}


def _assert_same_bits(before, after):
    assert set(before) == set(after)
    for k in before:
        a, b = np.asarray(before[k]), np.asarray(after[k])
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), k


def _oracles(net, teacher, frames, t, **kw):
    """(fp32, fp64) ``DistilledClassifier`` of the student on the oracle teacher's test-mode logits in the same precision"""
    out = []
    for dtype in (np.float32, np.float64):
        p, pt = G._params(net, dtype), G._params(teacher, dtype)
        ot = R.ResNet18Classifier(pt, train=False)
        ot.forward(frames.astype(dtype), t)
        out.append((D.DistilledClassifier(p, ot.logits, ALPHA, TEMP, label_smoothing=SMOOTH, topk=TOPK, **kw), p, ot.logits))
    return out


@pytest.mark.parametrize('mixed', (False, True))
def test_one_distilled_step_and_the_teacher_is_left_alone(mixed):
    _, net = G._classifier(0)
    teacher = _teacher()
    model = loans_amd.Classifier(net, label_smoothing=SMOOTH, topk=TOPK, teacher=teacher, distill_alpha=ALPHA, distill_temperature=TEMP)
    frames = synthetic.make_frames(1, B, H, W)
    ta, tb = np.array([3, 7], np.int32), np.array([7, 1], np.int32)
    (o32, p32, zt32), (o64, p64, zt64) = _oracles(net, teacher, frames, ta, **(dict(tb=tb, lam=LAM) if mixed else {}))
    before = _snapshot(teacher)
    opt = loans_amd.Adam(alpha=1e-3, amsgrad=True)
    opt.setup(model)
    seen = {}
    opt.add_hook(lambda o: seen.update({k[len('/predictor/'):]: p.grad_logical().copy() for k, p in o.target.namedparams()}))
    model.to_gpu(0)
    labels = loans_amd.MixedLabels(dev(ta), dev(tb), LAM) if mixed else dev(ta)
    loans_amd.reporter.observation.clear()
    opt.update(model, G._prepared(net, frames), labels)
    got_loss = float(model.loss.data)
    assert set(loans_amd.reporter.observation) == {'loss', 'accuracy', 'accuracy_top%d' % TOPK, 'distill_loss', 'teacher_accuracy'}

    r32 = o32.step(frames, ta, M.AdamAMSGrad(p32))
    r64 = o64.step(frames.astype(np.float64), ta, M.AdamAMSGrad(p64))
    print('loss %.7f  fp32 oracle %.7f  fp64 oracle %.7f  distill %.7f (oracle %.7f)' % (got_loss, r32[0], r64[0], float(model.distill_loss.data), o64.distill_loss))
    assert np.all(np.abs(model.y.data.cpu().numpy() - r64[2]) <= G._tol(r32[2], r64[2]))
    assert abs(got_loss - r64[0]) <= G._tol(r32[0], r64[0])
    assert abs(float(model.distill_loss.data) - o64.distill_loss) <= G._tol(o32.distill_loss, o64.distill_loss)
    assert float(model.accuracy.data) == r64[1] and float(model.accuracy_topk.data) == o64.accuracy_topk
    assert float(model.teacher_accuracy.data) == o64.teacher_accuracy
    worst = 0.0
    for key, ref in r64[3].items():
        if key == 'conv1/b':            # analytically zero gradient (BN follows): rounding noise on both sides
            continue
        e = rel_err(seen[key], ref)
        worst = max(worst, e)
        assert e <= max(5 * rel_err(r32[3][key], ref), 5e-4), (key, e, rel_err(r32[3][key], ref))
    print('worst relative gradient error %.3g' % worst)
    assert set(seen) == {k for k in p64 if M.is_trainable(k)}

    # the teacher: the same bits in every parameter, BN statistic and counter; no gradient; an arena of its own
    ops.join_side_stream()
    torch.cuda.synchronize()
    _assert_same_bits(before, _snapshot(teacher))
    assert teacher.arena is not None and teacher.arena is not model.arena and not bool(teacher.arena.grad.any())
    ours = {id(p) for p in model.arena.params}
    assert ours == {id(p) for p in net.params()} and not ours & {id(p) for p in teacher.params()}
    assert model.arena.numel == sum((p.size + 7) // 8 * 8 for p in net.params())
    assert {id(p) for p in opt.target.params()} == ours
    state = model.state_dict_chainer()
    assert set(state) == {'predictor/' + k for k in net.state_dict_chainer()}
    # the teacher's logits the loss saw are the oracle's
    assert np.all(np.abs(model.teacher_logits(G._prepared(net, frames)).cpu().numpy() - zt64) <= G._tol(zt32, zt64))


@pytest.mark.parametrize('step_arena', (True, False), ids=('arena', 'no-arena'))
def test_three_distilled_steps_with_and_without_the_step_arena(step_arena, monkeypatch, deterministic_forward):
    monkeypatch.setattr(ops, 'STEP_ARENA', step_arena)
    _, net = G._classifier(2)
    teacher = _teacher(30)
    model = loans_amd.Classifier(net, label_smoothing=SMOOTH, topk=TOPK, teacher=teacher, distill_alpha=ALPHA, distill_temperature=TEMP)
    frames = synthetic.make_frames(3, B, H, W)
    t = np.array([1, 9], np.int32)
    (o32, p32, _), (o64, p64, _) = _oracles(net, teacher, frames, t)
    a32, a64 = M.AdamAMSGrad(p32), M.AdamAMSGrad(p64)
    before = _snapshot(teacher)
    opt = loans_amd.Adam(alpha=1e-3, amsgrad=True)
    opt.setup(model)
    model.to_gpu(0)
    upd = training.StandardUpdater(training.DeviceBatchIterator([(dev(frames), dev(t))]), opt,
                                   converter=lambda batch, device: (G._prepared(net, batch[0].cpu().numpy()), batch[1]), device=0)
    for it in range(3):
        r32 = o32.step(frames, t, a32)
        r64 = o64.step(frames.astype(np.float64), t, a64)
        upd.update()
        got, kl = float(loans_amd.reporter.observation['loss']), float(loans_amd.reporter.observation['distill_loss'])
        tol = float(G._tol(r32[0], r64[0]))
        print('step %d: loss %.7f  fp32 oracle %.7f  fp64 oracle %.7f  tol %.3g  distill %.7f' % (it, got, r32[0], r64[0], tol, kl))
        assert abs(got - r64[0]) <= tol, (it, got, r64[0], r32[0], tol)
        assert abs(kl - o64.distill_loss) <= float(G._tol(o32.distill_loss, o64.distill_loss))
    torch.cuda.synchronize()
    _assert_same_bits(before, _snapshot(teacher))
    assert not bool(teacher.arena.grad.any())


def test_test_mode_and_evaluate_are_those_of_a_classifier_without_a_teacher(deterministic_forward):
    frames = synthetic.make_frames(6, B, H, W)
    t = np.array([3, 7], np.int32)
    results = []
    for with_teacher in (False, True):
        _, net = G._classifier(0)
        kw = dict(teacher=_teacher(), distill_alpha=ALPHA, distill_temperature=TEMP) if with_teacher else {}
        model = loans_amd.Classifier(net, label_smoothing=SMOOTH, topk=TOPK, **kw)
        model.to_gpu(0)
        x = G._prepared(net, frames)
        ran = []
        if with_teacher:
            old = model.teacher_logits
            model.__dict__['teacher_logits'] = lambda *xs: ran.append(1) or old(*xs)
        got = []
        with loans_amd.using_config('train', False), loans_amd.using_config('enable_backprop', False):
            loans_amd.reporter.observation.clear()
            model(x, dev(t))
            assert set(loans_amd.reporter.observation) == {'loss', 'accuracy', 'accuracy_top%d' % TOPK}
            got += [model.loss.data.clone(), model.accuracy.data.clone(), model.accuracy_topk.data.clone(), model.y.data.clone()]
        metrics = loans_amd.ClassificationMetrics(topk=TOPK)
        model.evaluate(x, dev(t), metrics)
        got += [metrics.acc.clone()]
        assert not ran and (not with_teacher or model.teacher.arena is None)           # the teacher was never run, nor moved to the device
        results.append(got)
    for a, b in zip(*results):
        assert torch.equal(a, b)
