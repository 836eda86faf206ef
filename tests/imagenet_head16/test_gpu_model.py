"""-m gpu: one ResNet-18 classification step at 64 x 64, batch 6, 24 classes, with ``head_dtype='bf16'``: the head's logits, gW, gb
and the gradient entering the pooling against float64 of the rounded operands, taken from the model's own pooled features and
loss gradient, within the bound of the kernel tests."""
import numpy as np
import pytest
import torch

import loans_amd
from loans_amd import ops
from loans_amd.datasets import synthetic
from tests.gpu_util import dev
from tests.imagenet import test_gpu_model as G

pytestmark = pytest.mark.gpu
B, N = 6, 24


def test_one_resnet18_step_with_the_bf16_head(monkeypatch):
    from loans_amd.sheep import resnet
    taps = G._tapped_gap(resnet, monkeypatch)
    linear = resnet.linear
    monkeypatch.setattr(resnet, 'linear', lambda *a, **kw: taps.append(G._Tap()) or taps[-1](linear(*a, **kw)))
    np.random.seed(11)
    loc = loans_amd.SheepLocalizer((75, 75), train_imagenet=True, class_labels=N, head_dtype='bf16')
    loc.feature_extractor.materialize_head()
    G._randomize(loc, np.random.RandomState(12))
    fc = loc.feature_extractor.fc
    assert fc.compute == 'bf16'
    plain = loans_amd.SheepLocalizer((75, 75), train_imagenet=True, class_labels=N)
    assert plain.feature_extractor.fc.compute == 'f32'                      # the default model runs the fp32 entry
    with pytest.raises(ValueError):
        loans_amd.SheepLocalizer((75, 75), head_dtype='bf16')               # no classification head to apply it to
    model = loans_amd.Classifier(loc)
    loss = model(dev(synthetic.make_frames(13, B, 64, 64)), dev(np.array([0, 5, 23, 7, 7, 12], np.int32)))
    model.cleargrads()
    loss.backward()
    ops.join_side_stream()

    r = lambda a: a.cpu().to(torch.bfloat16).double()
    x, gy = taps[0].seen, taps[1].gseen
    W, b = torch.from_numpy(fc.W.get_logical()), torch.from_numpy(fc.b.get_logical()).double()
    K = x.shape[1]
    checks = [('logits', model.y.data, r(x) @ r(W).T + b, r(x).abs() @ r(W).abs().T, K),
              ('gW', torch.from_numpy(fc.W.grad_logical()), r(gy).T @ r(x), r(gy).abs().T @ r(x).abs(), B),
              ('gb', torch.from_numpy(fc.b.grad_logical()), gy.cpu().double().sum(0), gy.cpu().double().abs().sum(0), B),
              ('gpooled', taps[0].gseen, r(gy) @ r(W), r(gy).abs() @ r(W).abs(), N)]
    for name, out, ref, mass, R in checks:
        out = out.cpu().double()
        err = (out - ref).abs()
        bound = R * 2.0 ** -23 * mass + 2.0 ** -24 * out.abs()
        print('%s: max error %.3g, smallest margin %.3g' % (name, err.max(), (bound - err).min()))
        assert out.shape == ref.shape and float(ref.abs().max()) > 0 and bool((err <= bound).all()), name
