"""-m gpu: ``blur_pool=True`` through the model surface: one training step of the ResNet-18 classifier and a single strided
bottleneck against the oracle's units with the blur composed in float64, within tests/imagenet_se/test_gpu_model.py's bound."""
import numpy as np
import pytest
import torch

import loans_amd
from loans_amd.datasets import synthetic
from oracle import chainer_ops as C
from oracle import model as M
from tests.gpu_util import dev, rel_err
from tests.imagenet import reference as R
from tests.imagenet import test_gpu_model as G
from tests.imagenet_blurpool.test_gpu_kernels import _blur

pytestmark = pytest.mark.gpu
FE = 'feature_extractor/'


def blur_fwd(a):          # NCHW NumPy, through the kernel test's torch reference
    return _blur(torch.from_numpy(np.ascontiguousarray(a))).numpy()


def blur_bwd(g, shape):
    x = torch.zeros(shape, dtype=torch.from_numpy(g).dtype, requires_grad=True)
    _blur(x).backward(torch.from_numpy(np.ascontiguousarray(g)))
    return x.grad.numpy()


class BlurResUnit(M._ResUnit):
    """M._ResUnit, every stride-2 convolution at stride 1: a strided stage hands blur(relu(bn(conv))) on, a strided shortcut reads blur(x)"""

    def __init__(self, p, stages, shortcut, train):
        one = lambda t: t[:2] + (1,) + t[3:]        # noqa: E731
        super().__init__(p, [one(t) for t in stages], None if shortcut is None else one(shortcut), train)
        self.blurred, self.blur_sc = [t[2] == 2 for t in stages], shortcut is not None and shortcut[2] == 2

    def fwd(self, x):
        self.acts, self.x_shape, h = [], x.shape, x
        for i, st in enumerate(self.stages[:-1]):
            self.acts.append(C.relu(st.fwd(h)))
            h = blur_fwd(self.acts[i]) if self.blurred[i] else self.acts[i]
        sc = x if self.shortcut is None else self.shortcut.fwd(blur_fwd(x) if self.blur_sc else x)
        self.out = C.relu(self.stages[-1].fwd(h) + sc)
        return self.out

    def bwd(self, gy, grads):
        g = gz = gy * (self.out > 0)
        gx = gz if self.shortcut is None else self.shortcut.bwd(gz, grads)
        gx = blur_bwd(gx, self.x_shape) if self.blur_sc else gx
        for i in range(len(self.stages) - 1, 0, -1):
            g = self.stages[i].bwd(g, grads)
            g = (blur_bwd(g, self.acts[i - 1].shape) if self.blurred[i - 1] else g) * (self.acts[i - 1] > 0)
        return gx + self.stages[0].bwd(g, grads)


def _blur_basic_a(p, a, stride, train):
    return BlurResUnit(p, [(a + '/conv1', a + '/bn1', stride, 1), (a + '/conv2', a + '/bn2', 1, 1)], (a + '/conv3', a + '/bn3', stride, 1), train)


class BlurResNet18Classifier(R.ResNet18Classifier):
    def forward(self, images, t):           # the oracle's composition with its first unit of a stage replaced
        old, M._BasicA = M._BasicA, _blur_basic_a
        try:
            return super().forward(images, t)
        finally:
            M._BasicA = old


def _step(frames, t, drop_path=0.0, **options):
    np.random.seed(5)
    loc = loans_amd.SheepLocalizer((75, 75), train_imagenet=True, **options)
    loc.feature_extractor.materialize_head()
    G._randomize(loc, np.random.RandomState(105))
    start = loc.state_dict_chainer()
    model = loans_amd.Classifier(loc)
    if drop_path:
        loc.set_drop_path(drop_path, seed=0)
    model.to_gpu(0)
    opt = loans_amd.Adam(alpha=1e-3, amsgrad=True)
    opt.setup(model)
    seen = {}
    opt.add_hook(lambda o: seen.update({k[len('/predictor/'):]: p.grad_logical().copy() for k, p in o.target.namedparams()}))
    opt.update(model, dev(frames), dev(t))
    torch.cuda.synchronize()
    return model, loc, start, seen


@pytest.mark.parametrize('H, W', [(64, 64), (70, 62)])
def test_one_training_step_against_the_composed_float64_model(H, W):
    frames, t = synthetic.make_frames(1, 2, H, W), np.array([3, 7], np.int32)
    model, loc, start, seen = _step(frames, t, blur_pool=True)
    p32, p64 = M.cast_params(dict(start), np.float32), M.cast_params(dict(start), np.float64)
    r32 = BlurResNet18Classifier(p32, FE).step(frames, t, M.AdamAMSGrad(p32))
    r64 = BlurResNet18Classifier(p64, FE).step(frames.astype(np.float64), t, M.AdamAMSGrad(p64))
    got = float(model.loss.data)
    print('loss %.7f  fp32 reference %.7f  fp64 reference %.7f' % (got, r32[0], r64[0]))
    assert abs(got - r64[0]) <= G._tol(r32[0], r64[0])
    for key in [FE + 'res3/0/' + k for k in ('conv1/W', 'bn1/gamma', 'bn1/beta', 'conv3/W')] + [FE + 'res2/1/conv1/W', FE + 'conv1/W']:
        e, e32 = rel_err(seen[key], r64[3][key]), rel_err(r32[3][key], r64[3][key])
        print('%s: relative error %.3g (fp32 reference %.3g)' % (key, e, e32))
        assert e <= max(5 * e32, 5e-4), key
    # no parameter more, no other output shape
    plain = _step(frames, t)
    assert set(seen) == set(plain[3]) == {k for k in p64 if M.is_trainable(k)}
    assert model.y.data.shape == plain[0].y.data.shape and not torch.equal(model.y.data, plain[0].y.data)


@pytest.mark.parametrize('options', [dict(se_ratio=16), dict(drop_path=0.5)], ids=['se', 'drop_path'])
def test_composes_with_the_other_unit_options(options):
    frames, t = synthetic.make_frames(1, 2, 64, 64), np.array([3, 7], np.int32)
    model, _, _, seen = _step(frames, t, blur_pool=True, **options)
    other = _step(frames, t, **options)
    assert np.isfinite(float(model.loss.data)) and float(model.loss.data) != float(other[0].loss.data)
    assert set(seen) == set(other[3]) and all(np.isfinite(g).all() for g in seen.values())
    # (a unit whose two samples are both dropped has no gradient in its main branch: the blurred shortcut and the stem always do)
    assert all(np.abs(seen[FE + k]).max() > 0 for k in ('res3/0/conv3/W', 'res5/0/conv3/W', 'conv1/W'))


def test_a_single_strided_bottleneck():
    from loans_amd.chainercv_resnet import Bottleneck
    from loans_amd.runtime.core import Variable
    rng = np.random.RandomState(3)
    np.random.seed(4)
    B, H, W, cin, mid, cout = 4, 9, 10, 64, 64, 128
    blk = Bottleneck(cin, mid, cout, 2, loans_amd.links.HeNormal(), residual_conv=True, blur_pool=True)
    G._randomize(blk, rng)
    blk.finalize(torch.device('cuda', 0))
    stages = [('conv1/conv', 'conv1/bn', 1, 0), ('conv2/conv', 'conv2/bn', 2, 1), ('conv3/conv', 'conv3/bn', 1, 0)]
    x = rng.standard_normal((B, cin, H, W)).astype(np.float32)
    gy = rng.standard_normal((B, cout, 5, 5)).astype(np.float32)
    xv = Variable(dev(np.ascontiguousarray(x.transpose(0, 2, 3, 1))), requires_grad=True)
    out = blk(xv)
    out.grad = dev(np.ascontiguousarray(gy.transpose(0, 2, 3, 1)))
    blk.cleargrads()
    out.backward()
    ref = {}
    for dtype in (np.float32, np.float64):
        unit = BlurResUnit(M.cast_params(blk.state_dict_chainer(), dtype), stages, ('residual_conv/conv', 'residual_conv/bn', 2, 0), True)
        ref[dtype] = {'out': unit.fwd(x.astype(dtype))}
        ref[dtype]['gx'] = unit.bwd(gy.astype(dtype), ref[dtype])
    got = dict({k[1:]: p.grad_logical() for k, p in blk.namedparams()}, out=out.data.cpu().numpy().transpose(0, 3, 1, 2),
               gx=xv.grad.cpu().numpy().transpose(0, 3, 1, 2))
    for key, value in got.items():
        e, e32 = rel_err(value, ref[np.float64][key]), rel_err(ref[np.float32][key], ref[np.float64][key])
        print('%s: relative error %.3g (fp32 reference %.3g)' % (key, e, e32))
        assert e <= max(5 * e32, 5e-4), key
