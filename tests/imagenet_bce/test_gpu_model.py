"""-m gpu: one training step of ``Classifier(SheepLocalizer(train_imagenet=True), loss='bce', ...)`` on plain labels and on
``MixedLabels`` against the float64 reference of the loss on the model's own logits (shapes, helpers and tolerances of
tests/imagenet/test_gpu_model.py and tests/imagenet_mix/test_gpu_model.py), its test mode, and ``loss='softmax'``."""
import numpy as np
import pytest
import torch

import loans_amd
from loans_amd import ops
from loans_amd.datasets import synthetic
from oracle import chainer_ops as C
from tests.gpu_util import dev, rel_err
from tests.imagenet import test_gpu_model as G
from tests.imagenet_bce import reference as Q
from tests.imagenet_mix import reference as X

pytestmark = pytest.mark.gpu
B, H, W = G.B, G.H, G.W
LAM, SMOOTH, TOPK, THRESH = 0.3, 0.1, 2, 0.2
FE = 'feature_extractor/'


def _localizer():
    np.random.seed(4)
    loc = loans_amd.SheepLocalizer((75, 75), train_imagenet=True)
    loc.feature_extractor.materialize_head()
    G._randomize(loc, np.random.RandomState(5))
    return loc


def _head_grads(pooled, W, gz):
    """the head's gradients of the reference's gz pushed through R's float64 head: fc/W, fc/b"""
    _, gW, gb = C.linear_bwd(pooled, W, gz.astype(pooled.dtype), True)
    return {FE + 'fc/W': gW, FE + 'fc/b': gb}


@pytest.mark.parametrize('mixed', (False, True))
def test_one_bce_step_then_test_mode_is_the_plain_softmax_loss(mixed):
    loc = _localizer()
    model = loans_amd.Classifier(loc, loss='bce', label_smoothing=SMOOTH, topk=TOPK, bce_target_threshold=THRESH)
    frames = synthetic.make_frames(6, B, H, W)
    ta, tb = np.array([3, 999], np.int32), np.array([999, 3], np.int32)
    p32, p64 = G._params(loc, np.float32), G._params(loc, np.float64)
    opt = loans_amd.MomentumSGD(lr=0.01, momentum=0.9)
    opt.setup(model)
    seen = {}
    opt.add_hook(lambda o: seen.update({k[len('/predictor/'):]: p.grad_logical().copy() for k, p in o.target.namedparams()}))

    model.to_gpu(0)
    labels = loans_amd.MixedLabels(dev(ta), dev(tb), LAM) if mixed else dev(ta)
    loans_amd.reporter.observation.clear()
    opt.update(model, dev(frames), labels)
    got_loss, got_acc, got_topk = float(model.loss.data), float(model.accuracy.data), float(model.accuracy_topk.data)
    got_logits = model.y.data.cpu().numpy()
    assert model.y.data.dtype == torch.float32
    assert set(loans_amd.reporter.observation) == {'loss', 'accuracy', 'accuracy_top%d' % TOPK}

    oracle = dict(tb=tb if mixed else None, lam=LAM if mixed else 1.0, label_smoothing=SMOOTH, topk=TOPK, thresh=THRESH, prefix=FE)
    o32, o64 = Q.BceClassifier(p32, **oracle), Q.BceClassifier(p64, **oracle)
    l32 = o32.forward(frames, ta)
    l64 = o64.forward(frames.astype(np.float64), ta)
    print('loss %.7f  fp32 oracle %.7f  fp64 oracle %.7f' % (got_loss, l32, l64))
    assert np.all(np.abs(got_logits - o64.logits) <= G._tol(o32.logits, o64.logits))
    assert abs(got_loss - l64) <= G._tol(l32, l64)
    # the loss and the hits on the logits the kernel was given: inside the kernel's own bound, and exact
    wa, wb = X.weights(LAM) if mixed else (1.0, 0.0)
    second = tb if mixed else ta
    assert not Q.threshold_ambiguous(got_logits.shape[1], ta, second, wa, wb, SMOOTH, THRESH)
    ref = Q.bce_ref(got_logits, ta, second, wa, wb, SMOOTH, TOPK, THRESH)
    assert abs(got_loss - ref[0]) <= Q.bce_bounds(got_logits, ta, second, wa, wb, SMOOTH, THRESH)[2]
    assert got_acc == ref[1] and got_topk == ref[2] and got_acc == o64.accuracy
    # the head's gradients: the reference gz through the float64 head, at the softmax step's tolerance
    g32 = _head_grads(o32.pooled, p32[FE + 'fc/W'], o32.gz)
    g64 = _head_grads(o64.pooled, p64[FE + 'fc/W'], o64.gz)
    for key, want in g64.items():
        e = rel_err(seen[key], want)
        print('%s relative gradient error %.3g' % (key, e))
        assert e <= max(5 * rel_err(g32[key], want), 5e-4), (key, e, rel_err(g32[key], want))
    # against the softmax loss the gradient would be another one
    soft = X.MixedClassifier(p64, second, LAM if mixed else 1.0, SMOOTH, TOPK, prefix=FE)
    soft.forward(frames.astype(np.float64), ta)
    assert rel_err(_head_grads(soft.pooled, p64[FE + 'fc/W'], soft.gz)[FE + 'fc/W'], g64[FE + 'fc/W']) > 0.1

    # test mode: the plain softmax cross-entropy of ops.softmax_xent_fwd on the model's logits, bit for bit
    from loans_amd.functions import ops_small
    calls = []
    old = ops_small.SigmoidBCE.forward
    ops_small.SigmoidBCE.forward = lambda self, inputs: calls.append(1) or old(self, inputs)
    try:
        with loans_amd.using_config('train', False), loans_amd.using_config('enable_backprop', False):
            loans_amd.reporter.observation.clear()
            model(dev(frames), dev(ta))
            assert set(loans_amd.reporter.observation) == {'loss', 'accuracy', 'accuracy_top%d' % TOPK}
            out = ops.softmax_xent_fwd(model.y.data.contiguous(), dev(ta))[0]
            assert torch.equal(model.loss.data, out[0]) and torch.equal(model.accuracy.data, out[1])
            assert not calls
    finally:
        ops_small.SigmoidBCE.forward = old


def test_loss_softmax_is_the_classifier_without_the_argument(deterministic_forward):
    frames = synthetic.make_frames(6, B, H, W)
    ta, tb = np.array([3, 999], np.int32), np.array([999, 3], np.int32)
    results = []
    for kw in ({}, {'loss': 'softmax'}):
        model = loans_amd.Classifier(_localizer(), label_smoothing=SMOOTH, topk=TOPK, **kw)
        opt = loans_amd.MomentumSGD(lr=0.01, momentum=0.9)
        opt.setup(model)
        seen = {}
        opt.add_hook(lambda o: seen.update({k: p.grad_logical().copy() for k, p in o.target.namedparams()}))
        model.to_gpu(0)
        got = []
        with loans_amd.using_config('train', True):
            for labels in (dev(ta), loans_amd.MixedLabels(dev(ta), dev(tb), LAM)):
                model(dev(frames), labels)
                got += [model.loss.data.clone(), model.accuracy.data.clone(), model.accuracy_topk.data.clone(), model.y.data.clone()]
        # the head's gradients of one step (the backbone's fp32 weight gradients close with atomics: not a matter of bits)
        opt.update(model, dev(frames), dev(ta))
        got += [torch.from_numpy(seen['/predictor/' + FE + 'fc/b'])]
        results.append(got)
    for a, b in zip(*results):
        assert torch.equal(a, b)
