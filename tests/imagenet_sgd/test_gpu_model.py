"""-m gpu: the ImageNet recipe end to end against the test-side oracle: ``Classifier(ResNet(18, class_labels=10),
label_smoothing, topk)`` under ``MomentumSGD`` for one and three steps, the momentum buffer on zero gradients and beyond the
active prefix, ``Classifier``'s defaults, and the bf16 arm (shapes and helpers of tests/imagenet/test_gpu_model.py)."""
import numpy as np
import pytest
import torch

import loans_amd
from loans_amd import links as L
from loans_amd import ops
from loans_amd.datasets import synthetic
from loans_amd.sheep.resnet import ResNet
from oracle import model as M
from tests.gpu_util import dev, rel_err
from tests.imagenet import test_gpu_model as G
from tests.imagenet_sgd import reference as S

pytestmark = pytest.mark.gpu
B, H, W = G.B, G.H, G.W
LR, MOMENTUM, DECAY, SMOOTH, TOPK = 0.05, 0.9, 5e-4, 0.1, 3


def _classifier(seed, classes=10, **kw):
    np.random.seed(seed)
    net = ResNet(18, class_labels=classes)
    net.materialize_head()
    G._randomize(net, np.random.RandomState(seed + 100))
    return loans_amd.Classifier(net, **kw), net


def _grad_hook(seen, prefix='/predictor/'):
    return lambda o: seen.update({k[len(prefix):]: p.grad_logical().copy() for k, p in o.target.namedparams() if k.startswith(prefix)})


def _check_sgd_step(start, seen, new, lr, momentum, decay):
    """the parameters after the first step (v = 0 before it) against the float64 rule on the gradients the HIP step produced"""
    worst = 0.0
    for key, p0 in start.items():
        if not M.is_trainable(key):
            continue
        g = seen[key]
        want, _ = S.momentum_sgd_ref(p0, g, np.zeros_like(g), lr, momentum, decay)
        bound, _ = S.momentum_sgd_bound(p0, g, np.zeros_like(g), lr, momentum, decay)
        err = np.abs(new[key].astype(np.float64) - want)
        assert np.all(err <= bound), (key, float((err / bound).max()))
        worst = max(worst, float((err / bound).max()))
    return worst


def test_one_sgd_step_of_the_smoothed_classifier():
    model, net = _classifier(0, label_smoothing=SMOOTH, topk=TOPK)
    frames = synthetic.make_frames(1, B, H, W)
    t = np.array([3, 7], np.int32)
    p32, p64 = G._params(net, np.float32), G._params(net, np.float64)
    start = {k: v.copy() for k, v in p32.items()}
    opt = loans_amd.MomentumSGD(lr=LR, momentum=MOMENTUM, weight_decay_rate=DECAY)
    opt.setup(model)
    seen = {}
    opt.add_hook(_grad_hook(seen))

    model.to_gpu(0)
    loans_amd.reporter.observation.clear()
    opt.update(model, G._prepared(net, frames), dev(t))
    got_loss, got_acc, got_topk = float(model.loss.data), float(model.accuracy.data), float(model.accuracy_topk.data)
    got_logits = model.y.data.cpu().numpy()
    assert set(loans_amd.reporter.observation) == {'loss', 'accuracy', 'accuracy_top%d' % TOPK}
    assert float(loans_amd.reporter.observation['accuracy_top%d' % TOPK]) == got_topk and opt.t == 1

    r32 = S.SmoothedClassifier(p32, SMOOTH, TOPK)
    r64 = S.SmoothedClassifier(p64, SMOOTH, TOPK)
    s32 = r32.step(frames, t, S.MomentumSGD(p32, LR, MOMENTUM, DECAY))
    s64 = r64.step(frames.astype(np.float64), t, S.MomentumSGD(p64, LR, MOMENTUM, DECAY))
    print('loss %.7f  fp32 oracle %.7f  fp64 oracle %.7f' % (got_loss, s32[0], s64[0]))
    assert np.all(np.abs(got_logits - s64[2]) <= G._tol(s32[2], s64[2]))
    assert abs(got_loss - s64[0]) <= G._tol(s32[0], s64[0])
    # the hits on the logits the kernel was given (exact), and the oracle's where its logits leave no doubt
    _, acc, acck = S.softmax_xent_ls_ref(got_logits, t, SMOOTH, TOPK)[:3]
    assert got_acc == acc and got_topk == acck and got_topk >= got_acc
    assert got_acc == s64[1]
    worst = 0.0
    for key, ref in s64[3].items():
        if key == 'conv1/b':            # analytically zero gradient (BN follows): rounding noise on both sides
            continue
        e = rel_err(seen[key], ref)
        worst = max(worst, e)
        assert e <= max(5 * rel_err(s32[3][key], ref), 5e-4), (key, e, rel_err(s32[3][key], ref))
    print('worst relative gradient error %.3g' % worst)
    assert set(seen) == {k for k in p64 if M.is_trainable(k)}
    print('worst SGD error / bound %.3f' % _check_sgd_step(start, seen, net.state_dict_chainer(), LR, MOMENTUM, DECAY))


def test_three_sgd_steps_loss_trajectory(deterministic_forward):
    model, net = _classifier(2, label_smoothing=SMOOTH, topk=TOPK)
    frames = synthetic.make_frames(3, B, H, W)
    t = np.array([1, 9], np.int32)
    p32, p64 = G._params(net, np.float32), G._params(net, np.float64)
    lr = 0.01
    o32, o64 = S.MomentumSGD(p32, lr, MOMENTUM, DECAY), S.MomentumSGD(p64, lr, MOMENTUM, DECAY)
    opt = loans_amd.MomentumSGD(lr=lr, momentum=MOMENTUM, weight_decay_rate=DECAY)
    opt.setup(model)
    model.to_gpu(0)
    from loans_amd.runtime import training
    upd = training.StandardUpdater(training.DeviceBatchIterator([(dev(frames), dev(t))]), opt,
                                   converter=lambda batch, device: (G._prepared(net, batch[0].cpu().numpy()), batch[1]), device=0)
    for it in range(3):
        r32 = S.SmoothedClassifier(p32, SMOOTH, TOPK).step(frames, t, o32)
        r64 = S.SmoothedClassifier(p64, SMOOTH, TOPK).step(frames.astype(np.float64), t, o64)
        upd.update()
        got = float(loans_amd.reporter.observation['loss'])
        tol = float(G._tol(r32[0], r64[0]))
        print('step %d: loss %.7f  fp32 oracle %.7f  fp64 oracle %.7f  tol %.3g' % (it, got, r32[0], r64[0], tol))
        assert abs(got - r64[0]) <= tol, (it, got, r64[0], r32[0], tol)
    assert upd.iteration == 3 and opt.t == 3


def test_momentum_keeps_moving_on_zero_gradients_and_skips_what_never_had_one():
    model, net = _classifier(4)
    with model.init_scope():
        model.spare = L.Linear(8, 4)            # a link no graph of this test reaches, at the arena's cold end
    model.cold_links = ('spare',)
    frames = synthetic.make_frames(5, B, H, W)
    t = np.array([0, 5], np.int32)
    opt = loans_amd.MomentumSGD(lr=LR, momentum=MOMENTUM)                   # no decay: a zero gradient leaves only the momentum
    opt.setup(model)
    model.to_gpu(0)
    arena = model.arena
    arena.set_active('spare')
    n = arena.active_numel
    assert 0 < n < arena.numel and arena.numel - n >= 8 * 4 + 4
    p0 = arena.data.clone()

    opt.update(model, G._prepared(net, frames), dev(t))
    p1, v1 = arena.data.clone(), opt._state[0].clone()
    assert v1[:n].abs().max() > 0 and not v1[n:].any()
    assert torch.equal(p1[n:], p0[n:])
    assert torch.equal(p1[:n], p0[:n] + v1[:n])                              # v was zero: p moved by this step's v

    model.cleargrads()
    opt.update()                                                             # all-zero gradients
    assert opt.t == 2
    want_v = v1[:n] * torch.tensor(MOMENTUM, dtype=torch.float32)
    assert torch.equal(opt._state[0][:n], want_v)
    assert torch.equal(arena.data[:n], p1[:n] + want_v)                      # exactly momentum * v
    assert (arena.data[:n] != p1[:n]).any()
    assert torch.equal(arena.data[n:], p0[n:]) and not opt._state[0][n:].any()       # never had a gradient: bit-identical
    np.testing.assert_array_equal(model.spare.W.get_logical(), p0[n:n + 32].cpu().numpy().reshape(4, 8))


def test_classifier_defaults_are_the_plain_path():
    model, net = _classifier(6)
    assert model.label_smoothing == 0.0 and model.topk is None
    frames = synthetic.make_frames(7, B, H, W)
    t = dev(np.array([2, 8], np.int32))
    model.to_gpu(0)
    loans_amd.reporter.observation.clear()
    loss = model(G._prepared(net, frames), t)
    assert set(loans_amd.reporter.observation) == {'loss', 'accuracy'}
    out, _, _, _ = ops.softmax_xent_fwd(model.y.data.contiguous(), t)
    assert torch.equal(loss.data, out[0]) and torch.equal(model.accuracy.data, out[1])
    assert model.accuracy_topk is None

    # smoothing is a training-time regulariser: in evaluation mode the loss is the plain one, bit for bit, top-k still reported
    smooth, net2 = _classifier(6, label_smoothing=SMOOTH, topk=TOPK)
    smooth.to_gpu(0)
    x = G._prepared(net2, frames)
    with loans_amd.using_config('train', False), loans_amd.using_config('enable_backprop', False):
        loans_amd.reporter.observation.clear()
        eval_loss = smooth(x, t)
        assert set(loans_amd.reporter.observation) == {'loss', 'accuracy', 'accuracy_top%d' % TOPK}
        plain, _, _, _ = ops.softmax_xent_fwd(smooth.y.data.contiguous(), t)
        assert torch.equal(eval_loss.data, plain[0]) and torch.equal(smooth.accuracy.data, plain[1])
    train_loss = smooth(x, t)
    want = S.softmax_xent_ls_ref(smooth.y.data.cpu().numpy(), t.cpu().numpy(), SMOOTH, TOPK)[0]
    bound = S.ls_bounds(smooth.y.data.cpu().numpy(), t.cpu().numpy(), SMOOTH)[2]
    assert abs(float(train_loss.data) - want) <= bound


def test_bf16_arm_one_sgd_step(monkeypatch):
    from loans_amd.sheep import resnet
    taps = G._tapped_gap(resnet, monkeypatch)
    model, net = _classifier(10)
    model.set_precision('bf16', 'bf16')
    frames = synthetic.make_frames(11, B, H, W)
    t = np.array([2, 4], np.int32)
    opt = loans_amd.MomentumSGD(lr=LR, momentum=MOMENTUM, weight_decay_rate=DECAY)
    opt.setup(model)
    seen = {}
    opt.add_hook(_grad_hook(seen))
    model.to_gpu(0)
    start = net.state_dict_chainer()
    W0, b0 = net.fc.W.get_logical(), net.fc.b.get_logical()
    opt.update(model, G._prepared(net, frames), dev(t))
    pooled = taps[0].seen
    assert pooled.dtype == torch.float32 and taps[0].gseen.dtype == torch.float32
    G._head_check(pooled.cpu().numpy(), model.y.data.cpu().numpy(), W0, b0, t, float(model.loss.data), float(model.accuracy.data),
                  seen['fc/W'], seen['fc/b'], taps[0].gseen.cpu().numpy())
    assert np.abs(seen['res5/1/conv2/W']).max() > 0 and np.isfinite(seen['conv1/W']).all()
    # the fp32 master parameters follow the rule on the gradients the bf16 step produced
    assert net.conv1.W.data.dtype == torch.float32
    print('worst SGD error / bound %.3f' % _check_sgd_step(start, seen, net.state_dict_chainer(), LR, MOMENTUM, DECAY))
