"""-m gpu: one training step of ``Classifier(SheepLocalizer(train_imagenet=True))`` on ``MixedLabels`` against the test-side
oracle with the float64 mixed loss (shapes, helpers and tolerances of tests/imagenet/test_gpu_model.py), and the same model on
plain labels afterwards."""
import numpy as np
import pytest

import loans_amd
from loans_amd.datasets import synthetic
from oracle import chainer_ops as C
from tests.gpu_util import dev, rel_err
from tests.imagenet import test_gpu_model as G
from tests.imagenet_mix import reference as X
from tests.imagenet_sgd import reference as S

pytestmark = pytest.mark.gpu
B, H, W = G.B, G.H, G.W
LAM, SMOOTH, TOPK = 0.3, 0.1, 5
FE = 'feature_extractor/'


def _head_grads(oracle, params):
    """the head's gradients of the oracle's forward: fc/W, fc/b"""
    gz = oracle.gz.astype(oracle.logits.dtype)
    _, gW, gb = C.linear_bwd(oracle.pooled, params[FE + 'fc/W'], gz, True)
    return {FE + 'fc/W': gW, FE + 'fc/b': gb}


def test_one_step_on_mixed_labels_then_plain_labels_take_the_old_branch():
    np.random.seed(4)
    loc = loans_amd.SheepLocalizer((75, 75), train_imagenet=True)
    loc.feature_extractor.materialize_head()
    G._randomize(loc, np.random.RandomState(5))
    model = loans_amd.Classifier(loc, label_smoothing=SMOOTH, topk=TOPK)
    frames = synthetic.make_frames(6, B, H, W)
    ta, tb = np.array([3, 999], np.int32), np.array([999, 3], np.int32)
    p32, p64 = G._params(loc, np.float32), G._params(loc, np.float64)
    opt = loans_amd.MomentumSGD(lr=0.01, momentum=0.9)
    opt.setup(model)
    seen = {}
    opt.add_hook(lambda o: seen.update({k[len('/predictor/'):]: p.grad_logical().copy() for k, p in o.target.namedparams()}))

    model.to_gpu(0)
    labels = loans_amd.MixedLabels(dev(ta), dev(tb), LAM)
    loans_amd.reporter.observation.clear()
    opt.update(model, dev(frames), labels)
    got_loss, got_acc, got_topk = float(model.loss.data), float(model.accuracy.data), float(model.accuracy_topk.data)
    got_logits = model.y.data.cpu().numpy()
    assert set(loans_amd.reporter.observation) == {'loss', 'accuracy', 'accuracy_top%d' % TOPK}

    o32 = X.MixedClassifier(p32, tb, LAM, SMOOTH, TOPK, prefix=FE)
    o64 = X.MixedClassifier(p64, tb, LAM, SMOOTH, TOPK, prefix=FE)
    l32 = o32.forward(frames, ta)
    l64 = o64.forward(frames.astype(np.float64), ta)
    print('loss %.7f  fp32 oracle %.7f  fp64 oracle %.7f' % (got_loss, l32, l64))
    assert np.all(np.abs(got_logits - o64.logits) <= G._tol(o32.logits, o64.logits))
    assert abs(got_loss - l64) <= G._tol(l32, l64)
    # the loss and the hits on the logits the kernel was given: inside the kernel's own bound, and exact
    wa, wb = X.weights(LAM)
    ref = X.mixed_ref(got_logits, ta, tb, wa, wb, SMOOTH, TOPK)
    assert abs(got_loss - ref[0]) <= X.mixed_bounds(got_logits, ta, tb, wa, wb, SMOOTH)[2]
    assert got_acc == ref[1] and got_topk == ref[2] and got_acc == o64.accuracy
    g32, g64 = _head_grads(o32, p32), _head_grads(o64, p64)
    for key, want in g64.items():
        e = rel_err(seen[key], want)
        print('%s relative gradient error %.3g' % (key, e))
        assert e <= max(5 * rel_err(g32[key], want), 5e-4), (key, e, rel_err(g32[key], want))
    # against the one-label loss the gradient would be another one: the test sees the second label
    plain = S.SmoothedClassifier(p64, SMOOTH, TOPK, prefix=FE)
    plain.forward(frames.astype(np.float64), ta)
    assert rel_err(_head_grads(plain, p64)[FE + 'fc/W'], g64[FE + 'fc/W']) > 0.1

    # plain labels afterwards: the old branch, the old function
    from loans_amd.functions import ops_small
    calls = []
    old = ops_small.SoftmaxCrossEntropyMixed.forward
    ops_small.SoftmaxCrossEntropyMixed.forward = lambda self, inputs: calls.append(1) or old(self, inputs)
    try:
        with loans_amd.using_config('train', False), loans_amd.using_config('enable_backprop', False):
            model(dev(frames), dev(ta))
            logits = model.y.data.cpu().numpy()
            want = S.softmax_xent_ls_ref(logits, ta, 0.0, TOPK)
            assert abs(float(model.loss.data) - want[0]) <= S.ls_bounds(logits, ta, 0.0)[2]
            assert float(model.accuracy.data) == want[1] and float(model.accuracy_topk.data) == want[2]
            assert not calls
            # weights (1, 0): the new branch, the one-label loss (its bits are held at kernel level)
            model(dev(frames), loans_amd.MixedLabels(dev(ta), dev(tb), 1.0))
            logits = model.y.data.cpu().numpy()
            want = S.softmax_xent_ls_ref(logits, ta, 0.0, TOPK)
            assert calls == [1] and abs(float(model.loss.data) - want[0]) <= S.ls_bounds(logits, ta, 0.0)[2]
            assert float(model.accuracy.data) == want[1] and float(model.accuracy_topk.data) == want[2]
    finally:
        ops_small.SoftmaxCrossEntropyMixed.forward = old
