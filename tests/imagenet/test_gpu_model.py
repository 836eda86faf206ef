"""-m gpu: the ImageNet pre-training arm end to end against the test-side oracle (tests/imagenet/reference.py): one and three
training steps of ``Classifier(ResNet(18, class_labels=10))``, the forward of both ``train_imagenet=True`` localizers, and the
bf16 arm with the head teacher-forced."""
import numpy as np
import pytest
import torch

import loans_amd
from loans_amd import ops
from loans_amd.datasets import synthetic
from loans_amd.sheep.resnet import ResNet
from oracle import chainer_ops as C
from oracle import model as M
from tests.gpu_util import dev, rel_err
from tests.imagenet import reference as R

pytestmark = pytest.mark.gpu
B, H, W = 2, 64, 64


def _randomize(link, rng):
    """BN affine parameters away from (1, 0), a non-zero conv1 bias and head bias"""
    for key, p in link.namedparams():
        if key.endswith('/gamma'):
            p.set_logical((1 + 0.1 * rng.standard_normal(p.logical_shape)).astype(np.float32))
        elif key.endswith(('/beta', 'conv1/b', 'fc/b', 'fc6/b')):
            p.set_logical((0.1 * rng.standard_normal(p.logical_shape)).astype(np.float32))


def _classifier(seed, classes=10):
    np.random.seed(seed)
    net = ResNet(18, class_labels=classes)
    net.materialize_head()
    _randomize(net, np.random.RandomState(seed + 100))
    return loans_amd.Classifier(net), net


def _prepared(net, frames):
    """what ``SheepLocalizer.prepare_images`` hands the backbone"""
    x = dev(frames)
    return loans_amd.Variable(ops.prep_images(x, net.conv1.geometry(*([x.shape[0]] + list(x.shape[2:])))), requires_grad=False)


def _tol(r32, r64):
    """the project's form: max(5 |fp32 oracle - fp64 oracle|, 5e-4 |ref|, 1e-5)"""
    r32, r64 = np.asarray(r32, np.float64), np.asarray(r64, np.float64)
    return np.maximum(np.maximum(5 * np.abs(r32 - r64), 5e-4 * np.abs(r64)), 1e-5)


def _params(link, dtype):
    return M.cast_params(link.state_dict_chainer(), dtype)


def test_one_training_step_of_the_resnet18_classifier():
    model, net = _classifier(0)
    frames = synthetic.make_frames(1, B, H, W)
    t = np.array([3, 7], np.int32)
    p32, p64 = _params(net, np.float32), _params(net, np.float64)
    start = {k: v.copy() for k, v in p64.items()}
    opt = loans_amd.Adam(alpha=1e-3, amsgrad=True)
    opt.setup(model)
    seen = {}
    opt.add_hook(lambda o: seen.update({k[len('/predictor/'):]: p.grad_logical().copy() for k, p in o.target.namedparams()}))

    model.to_gpu(0)
    opt.update(model, _prepared(net, frames), dev(t))
    got_loss, got_acc = float(model.loss.data), float(model.accuracy.data)
    got_logits = model.y.data.cpu().numpy()

    r32 = R.ResNet18Classifier(p32).step(frames, t, M.AdamAMSGrad(p32))
    r64 = R.ResNet18Classifier(p64).step(frames.astype(np.float64), t, M.AdamAMSGrad(p64))
    print('loss %.7f  fp32 oracle %.7f  fp64 oracle %.7f' % (got_loss, r32[0], r64[0]))
    assert np.all(np.abs(got_logits - r64[2]) <= _tol(r32[2], r64[2]))
    assert abs(got_loss - r64[0]) <= _tol(r32[0], r64[0])
    assert got_acc == r64[1]
    worst = 0.0
    for key, ref in r64[3].items():
        if key == 'conv1/b':            # analytically zero gradient (BN follows): rounding noise on both sides
            continue
        e = rel_err(seen[key], ref)
        worst = max(worst, e)
        assert e <= max(5 * rel_err(r32[3][key], ref), 5e-4), (key, e, rel_err(r32[3][key], ref))
    print('worst relative gradient error %.3g' % worst)
    assert set(seen) == {k for k in p64 if M.is_trainable(k)}
    # Adam-updated parameters: the oracle's Adam applied to the gradients the HIP step produced lands where the fused kernel
    # landed (a sign-like first step is only comparable for equal gradients), and nowhere further than ~2 lr from the oracle
    new = net.state_dict_chainer()
    for key in p64:
        if not M.is_trainable(key):
            continue
        want = start[key].copy()
        z = np.zeros_like(want)
        C.adam_amsgrad_update(want, seen[key].astype(np.float64), z.copy(), z.copy(), z.copy(), 1)
        np.testing.assert_allclose(new[key], want, rtol=0, atol=2e-6, err_msg=key)
        if key != 'conv1/b':
            assert np.abs(new[key] - p64[key]).max() < 2.1e-3, key


def test_three_steps_loss_trajectory(deterministic_forward):
    model, net = _classifier(2)
    frames = synthetic.make_frames(3, B, H, W)
    t = np.array([1, 9], np.int32)
    p32, p64 = _params(net, np.float32), _params(net, np.float64)
    o32, o64 = M.AdamAMSGrad(p32), M.AdamAMSGrad(p64)
    opt = loans_amd.Adam(alpha=1e-3, amsgrad=True)
    opt.setup(model)
    model.to_gpu(0)
    from loans_amd.runtime import training
    upd = training.StandardUpdater(training.DeviceBatchIterator([(dev(frames), dev(t))]), opt,
                                   converter=lambda batch, device: (_prepared(net, batch[0].cpu().numpy()), batch[1]), device=0)
    for it in range(3):
        r32 = R.ResNet18Classifier(p32).step(frames, t, o32)
        r64 = R.ResNet18Classifier(p64).step(frames.astype(np.float64), t, o64)
        upd.update()
        got = float(loans_amd.reporter.observation['loss'])
        tol = float(_tol(r32[0], r64[0]))
        print('step %d: loss %.7f  fp32 oracle %.7f  fp64 oracle %.7f  tol %.3g' % (it, got, r32[0], r64[0], tol))
        assert abs(got - r64[0]) <= tol, (it, got, r64[0], r32[0], tol)
    assert upd.iteration == 3


def test_sheep_localizer_train_imagenet_forward():
    np.random.seed(4)
    loc = loans_amd.SheepLocalizer((75, 75), train_imagenet=True)
    loc.feature_extractor.materialize_head()
    _randomize(loc, np.random.RandomState(5))
    frames = synthetic.make_frames(6, B, H, W)
    p32, p64 = _params(loc, np.float32), _params(loc, np.float64)
    logits = loc(dev(frames))
    assert tuple(logits.shape) == (B, 1000)
    t = np.array([0, 999], np.int32)
    o32 = R.ResNet18Classifier(p32, 'feature_extractor/')
    o64 = R.ResNet18Classifier(p64, 'feature_extractor/')
    o32.forward(frames, t)
    o64.forward(frames.astype(np.float64), t)
    assert np.all(np.abs(logits.data.cpu().numpy() - o64.logits) <= _tol(o32.logits, o64.logits))


def _head_check(pooled, logits, W, b, t, loss, acc, gW, gb, gpooled, tol_scale=1.0):
    """the head and the loss alone, teacher-forced with the pooled features the HIP path produced"""
    x = pooled.astype(np.float64)
    ref_logits = C.linear_fwd(x, W.astype(np.float64), b.astype(np.float64))
    assert rel_err(logits, ref_logits) < 2e-6 * tol_scale
    ref_loss, ref_acc, gz, _, _ = R.softmax_xent_ref(logits, t)       # the loss on the logits the kernel was given
    _, _, bb = R.row_bounds(logits, t)
    assert abs(loss - ref_loss) <= bb, (loss, ref_loss, bb)
    assert acc == ref_acc
    rgx, rgW, rgb = C.linear_bwd(x, W.astype(np.float64), gz, True)
    assert rel_err(gW, rgW) < 5e-6 * tol_scale and rel_err(gb, rgb) < 5e-6 * tol_scale
    if gpooled is not None:
        assert rel_err(gpooled, rgx) < 5e-6 * tol_scale


class _Tap(loans_amd.Function):
    """identity that keeps the array it saw and the gradient that came back through it"""

    def forward(self, inputs):
        self.seen = inputs[0]
        return inputs[0]

    def backward(self, inputs, gys):
        self.gseen = gys[0]
        return gys[0]


def _tapped_gap(module, monkeypatch):
    """route the backbone's global_average_pooling_2d through a tap: (taps list)"""
    taps = []
    orig = module.global_average_pooling_2d

    def gap(h):
        tap = _Tap()
        taps.append(tap)
        return tap(orig(h))
    monkeypatch.setattr(module, 'global_average_pooling_2d', gap)
    return taps


def test_resnet50_localizer_train_imagenet_forward_backward(monkeypatch):
    from loans_amd.iou import iou_regressor
    taps = _tapped_gap(iou_regressor, monkeypatch)
    np.random.seed(7)
    loc = loans_amd.Resnet50SheepLocalizer((75, 75), train_imagenet=True)
    _randomize(loc, np.random.RandomState(8))
    model = loans_amd.Classifier(loc)
    frames = synthetic.make_frames(9, B, H, W)
    t = np.array([5, 998], np.int32)
    loss = model(dev(frames), dev(t))
    model.cleargrads()
    loss.backward()
    ops.join_side_stream()
    assert tuple(model.y.shape) == (B, 1000) and torch.isfinite(model.y.data).all() and torch.isfinite(loss.data)
    for key, p in model.namedparams():
        g = p.grad_logical()
        assert g.shape == p.logical_shape and np.isfinite(g).all(), key
    assert np.abs(loc.feature_extractor.res2.a.conv1.W.grad_logical()).max() > 0
    fc6 = loc.feature_extractor.fc6
    assert taps[0].seen.dtype == torch.float32 and tuple(taps[0].seen.shape) == (B, 2048)
    _head_check(taps[0].seen.cpu().numpy(), model.y.data.cpu().numpy(), fc6.W.get_logical(), fc6.b.get_logical(), t,
                float(loss.data), float(model.accuracy.data), fc6.W.grad_logical(), fc6.b.grad_logical(),
                taps[0].gseen.cpu().numpy())


def test_bf16_arm_one_step_head_and_loss(monkeypatch):
    from loans_amd.sheep import resnet
    taps = _tapped_gap(resnet, monkeypatch)
    model, net = _classifier(10)
    model.set_precision('bf16', 'bf16')
    frames = synthetic.make_frames(11, B, H, W)
    t = np.array([2, 4], np.int32)
    opt = loans_amd.Adam(alpha=1e-3, amsgrad=True)
    opt.setup(model)
    seen = {}
    opt.add_hook(lambda o: seen.update({k: p.grad_logical().copy() for k, p in o.target.namedparams()}))
    model.to_gpu(0)
    W0, b0 = net.fc.W.get_logical(), net.fc.b.get_logical()
    from loans_amd.runtime import training
    upd = training.StandardUpdater(training.DeviceBatchIterator([(dev(frames), dev(t))]), opt,
                                   converter=lambda batch, device: (_prepared(net, batch[0].cpu().numpy()), batch[1]), device=0)
    upd.update()
    pooled = taps[0].seen
    assert pooled.dtype == torch.float32                   # the pooled features leave the bf16 region as fp32
    assert taps[0].gseen.dtype == torch.float32
    _head_check(pooled.cpu().numpy(), model.y.data.cpu().numpy(), W0, b0, t, float(model.loss.data), float(model.accuracy.data),
                seen['/predictor/fc/W'], seen['/predictor/fc/b'], taps[0].gseen.cpu().numpy())
    # ... and the backbone behind it moved
    assert np.abs(seen['/predictor/res5/1/conv2/W']).max() > 0 and np.isfinite(seen['/predictor/conv1/W']).all()
