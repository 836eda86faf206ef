"""-m gpu: squeeze-and-excitation through the model surface: one training step of ``Classifier(SheepLocalizer(train_imagenet=True,
se_ratio=16))`` against the oracle's ResNet-18 with the gate composed from its own float64 operations
(tests/imagenet_se/reference.py), the model without the option, and a snapshot round trip with the new keys."""
import numpy as np
import pytest
import torch

import loans_amd
from loans_amd.datasets import synthetic
from oracle import model as M
from tests.gpu_util import dev, rel_err
from tests.imagenet import test_gpu_model as G
from tests.imagenet_se import reference as S

pytestmark = pytest.mark.gpu
B, H, W = 2, 64, 64
FE = 'feature_extractor/'
UNIT = FE + 'res3/0/'           # a unit with a conv shortcut; res5/1 is one with an identity


def _step(se_ratio, frames, t):
    """one optimiser step as a trainer makes it: (model, localizer, its parameters before the step, gradients by key)"""
    np.random.seed(5)
    loc = loans_amd.SheepLocalizer((75, 75), train_imagenet=True, se_ratio=se_ratio)
    loc.feature_extractor.materialize_head()
    rng = np.random.RandomState(105)
    G._randomize(loc, rng)
    for key, p in loc.namedparams():          # biases off zero, so that every gate differs from the others
        if key.endswith(('se/down/b', 'se/up/b')):
            p.set_logical((0.5 * rng.standard_normal(p.logical_shape)).astype(np.float32))
    start = loc.state_dict_chainer()
    model = loans_amd.Classifier(loc)
    model.to_gpu(0)
    opt = loans_amd.Adam(alpha=1e-3, amsgrad=True)
    opt.setup(model)
    seen = {}
    opt.add_hook(lambda o: seen.update({k[len('/predictor/'):]: p.grad_logical().copy() for k, p in o.target.namedparams()}))
    opt.update(model, dev(frames), dev(t))
    torch.cuda.synchronize()
    return model, loc, start, seen


def test_one_training_step_against_the_composed_float64_model(tmp_path):
    frames, t = synthetic.make_frames(1, B, H, W), np.array([3, 7], np.int32)
    model, loc, start, seen = _step(16, frames, t)
    p32, p64 = M.cast_params(dict(start), np.float32), M.cast_params(dict(start), np.float64)
    r32 = S.SEResNet18Classifier(p32, FE).step(frames, t, M.AdamAMSGrad(p32))
    r64 = S.SEResNet18Classifier(p64, FE).step(frames.astype(np.float64), t, M.AdamAMSGrad(p64))
    got = float(model.loss.data)
    print('loss %.7f  fp32 reference %.7f  fp64 reference %.7f' % (got, r32[0], r64[0]))
    assert abs(got - r64[0]) <= G._tol(r32[0], r64[0])
    for key in [UNIT + k for k in S.SE_KEYS] + [FE + 'res5/1/' + k for k in S.SE_KEYS] + [FE + 'conv1/W']:
        e, e32 = rel_err(seen[key], r64[3][key]), rel_err(r32[3][key], r64[3][key])
        print('%s: relative error %.3g (fp32 reference %.3g)' % (key, e, e32))
        assert e <= max(5 * e32, 5e-4), key
    assert set(seen) == {k for k in p64 if M.is_trainable(k)}
    # a snapshot round trip with the new keys
    path = str(tmp_path / 'se.npz')
    loans_amd.save_npz(path, loc)
    with np.load(path) as f:
        assert all(UNIT + k in f.files for k in S.SE_KEYS)
    other = loans_amd.SheepLocalizer((75, 75), train_imagenet=True, se_ratio=16)
    other.feature_extractor.materialize_head()
    loans_amd.load_npz(path, other, strict=True)
    now = loc.state_dict_chainer()
    assert all(np.array_equal(v, now[k]) for k, v in other.state_dict_chainer().items())


def test_without_the_option_the_model_is_the_parents(deterministic_forward):
    """``se_ratio=None`` and 0: the parameter list of the model that never heard of the option, and the bits of its step"""
    frames, t = synthetic.make_frames(1, B, H, W), np.array([3, 7], np.int32)
    plain = loans_amd.SheepLocalizer((75, 75), train_imagenet=True)
    plain.feature_extractor.materialize_head()
    names = [k for k, _ in plain.namedparams()]
    runs = [_step(r, frames, t) for r in (None, 0, None)]
    for model, loc, _, seen in runs:
        assert [k for k, _ in loc.namedparams()] == names and not any('/se/' in k for k in seen)
        assert torch.equal(model.loss.data, runs[0][0].loss.data) and torch.equal(model.y.data, runs[0][0].y.data)
        for key, g in runs[0][3].items():
            if key != FE + 'conv1/W':           # the stem's weight gradient closes with float atomics (tests/imagenet_droppath)
                assert np.array_equal(seen[key], g), key
