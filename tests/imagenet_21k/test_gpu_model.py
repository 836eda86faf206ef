"""-m gpu: one ``Classifier`` step of the ResNet-18 localizer with a head of 8200 classes -- a second chunk of 8 logits -- and a
validation pass through ``ClassificationMetrics``, against float64 on the step's own tensors.  The loss bound is the kernel
test's; the head's weight gradient (two products and a sum per entry, of a gz inside GZ_TOL) is held to the 5e-6 of the maximum
that tests/imagenet/test_gpu_model.py holds the same GEMM to."""
import numpy as np
import pytest

import loans_amd
from loans_amd import ops
from loans_amd.datasets import synthetic
from tests.gpu_util import dev, rel_err
from tests.imagenet import test_gpu_model as G
from tests.imagenet_21k import test_gpu_kernels as K

pytestmark = pytest.mark.gpu
N = 8200


def test_one_classifier_step_and_a_validation_pass_at_8200_classes(monkeypatch):
    from loans_amd.sheep import resnet
    taps = G._tapped_gap(resnet, monkeypatch)
    np.random.seed(4)
    loc = loans_amd.SheepLocalizer((75, 75), train_imagenet=True, class_labels=N)
    loc.feature_extractor.materialize_head()
    G._randomize(loc, np.random.RandomState(5))
    model = loans_amd.Classifier(loc)
    frames = synthetic.make_frames(6, G.B, G.H, G.W)
    t = np.array([N - 1, 3], np.int32)
    loss = model(dev(frames), dev(t))
    model.cleargrads()
    loss.backward()
    ops.join_side_stream()
    logits = model.y.data.cpu().numpy()
    _, _, _, want, gz = K.reference(logits, t, t, 1.0, 0.0, 0.0, 1)
    gW = loc.feature_extractor.fc.W.grad_logical()
    want_gW = gz.T @ taps[0].seen.cpu().numpy().astype(np.float64)
    print('loss %.7f  float64 %.7f  fc/W relative gradient error %.3g' % (float(loss.data), want[0], rel_err(gW, want_gW)))
    assert logits.shape == (G.B, N) and np.isfinite(float(loss.data)) and abs(float(loss.data) - want[0]) <= K.LOSS_TOL
    assert float(model.accuracy.data) == want[1]
    assert np.abs(gW).max() > 0 and rel_err(gW, want_gW) <= 5e-6

    metrics = loans_amd.ClassificationMetrics(topk=5)
    model.evaluate(dev(frames), dev(t), metrics)
    row_loss, hit, hitk, _, _ = K.reference(model.y.data.cpu().numpy(), t, t, 1.0, 0.0, 0.0, 5)
    got = metrics.result()
    assert abs(got['loss'] - row_loss.mean()) <= K.LOSS_TOL
    assert (got['accuracy'], got['accuracy_top5'], got['rows'], got['valid']) == (hit.mean(), hitk.mean(), 2, 2)
