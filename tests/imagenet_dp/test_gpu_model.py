"""-m gpu: ``ClassificationMetrics`` and ``Classifier.evaluate`` on the ResNet-18 classifier of tests/imagenet/test_gpu_model.py
and on hand-made logits: the sums are what the loss kernels report per batch, weighted by rows."""
import numpy as np
import pytest
import torch

import loans_amd
from loans_amd.datasets import synthetic
from tests.gpu_util import dev
from tests.imagenet import test_gpu_model as G
from tests.imagenet_sgd import reference as S
from tests.imagenet_sgd.test_gpu_model import _classifier

pytestmark = pytest.mark.gpu
B, H, W = G.B, G.H, G.W
TOPK = 3


def test_evaluate_matches_the_test_mode_call_and_leaves_nothing_behind():
    model, net = _classifier(0, label_smoothing=0.1, topk=TOPK)
    frames = synthetic.make_frames(1, B, H, W)
    t = np.array([3, 7], np.int32)
    model.to_gpu(0)
    x = G._prepared(net, frames)
    with loans_amd.using_config('train', False), loans_amd.using_config('enable_backprop', False):
        model(x, dev(t))
    want_acc, want_topk = float(model.accuracy.data), float(model.accuracy_topk.data)
    logits = model.y.data.cpu().numpy()

    model.cleargrads()
    model.arena.grad.zero_()
    model.loss = model.accuracy = model.accuracy_topk = None
    loans_amd.reporter.observation.clear()
    metrics = loans_amd.ClassificationMetrics(topk=TOPK)
    metrics.reset()
    assert metrics.acc.dtype == torch.float64 and metrics.acc.numel() == 5 and metrics.acc.is_cuda and not metrics.acc.any()
    assert model.evaluate(x, dev(t), metrics) is None
    got = metrics.result()
    assert loans_amd.reporter.observation == {}                                        # nothing is reported
    assert model.loss is None and model.accuracy is None                                # no loss function ran
    assert model.y.grad is None and not model.arena.grad.any()                         # no gradient is left
    np.testing.assert_array_equal(model.y.data.cpu().numpy(), logits)                   # the same test-mode forward
    assert set(got) == {'loss', 'accuracy', 'accuracy_top%d' % TOPK, 'rows', 'valid'}
    assert got['accuracy'] == want_acc and got['accuracy_top%d' % TOPK] == want_topk
    assert (got['rows'], got['valid']) == (B, B) and isinstance(got['rows'], int) and isinstance(got['valid'], int)
    ref = S.softmax_xent_ls_ref(logits, t, 0.0, TOPK)
    assert abs(got['loss'] - ref[0]) <= S.ls_bounds(logits, t, 0.0)[2], (got['loss'], ref[0])
    assert got['accuracy'] == ref[1] and got['accuracy_top%d' % TOPK] == ref[2]

    # labels as the loss takes them: a NumPy array, a Variable; the sums go on
    model.evaluate(x, t, metrics)
    model.evaluate(x, loans_amd.Variable(dev(t), requires_grad=False), metrics)
    again = metrics.result()
    assert again['rows'] == 3 * B and again['accuracy'] == want_acc and abs(again['loss'] - got['loss']) <= 1e-12
    metrics.reset()
    assert not metrics.acc.any() and metrics.result()['rows'] == 0 and metrics.result()['loss'] == 0.0


def test_batches_of_different_sizes_weigh_their_rows():
    N = 10
    z3 = np.zeros((3, N), np.float32)                        # uniform rows: loss log(10) each, labels not the first index
    t3 = np.array([1, 2, 3], np.int32)
    z1 = np.zeros((1, N), np.float32)
    z1[0, 4] = 20.0                                           # confident and right: loss ~ 0
    t1 = np.array([4], np.int32)
    metrics = loans_amd.ClassificationMetrics(topk=2)
    metrics.add(dev(z3), dev(t3))
    metrics.add(loans_amd.Variable(dev(z1)), t1)
    got = metrics.result()
    rows = np.concatenate([S.softmax_xent_ls_ref(z3, t3, 0.0, 2)[4], S.softmax_xent_ls_ref(z1, t1, 0.0, 2)[4]])
    bound = (S.ls_bounds(z3, t3, 0.0)[0].sum() + S.ls_bounds(z1, t1, 0.0)[0].sum()) / 4
    assert abs(got['loss'] - rows.mean()) <= bound
    mean_of_means = 0.5 * (rows[:3].mean() + rows[3])
    assert abs(got['loss'] - mean_of_means) > 0.25 * np.log(N) - 1e-3 > 1000 * bound     # 3/4 log 10 against 1/2 log 10
    # hits: the uniform rows' argmax is index 0, never the label; with k = 2 only the row labelled 1 is in the top two
    assert (got['accuracy'], got['accuracy_top2']) == (0.25, 0.5) and (got['rows'], got['valid']) == (4, 4)
    # an ignored row counts as a row for the accuracies and not for the loss
    metrics.add(dev(z1), dev(np.array([-1], np.int32)))
    more = metrics.result()
    assert (more['rows'], more['valid']) == (5, 4) and more['accuracy'] == 0.2 and abs(more['loss'] - got['loss']) <= 1e-15
    with pytest.raises(ValueError):
        loans_amd.ClassificationMetrics(topk=0)
