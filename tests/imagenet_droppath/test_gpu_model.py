"""-m gpu: stochastic depth through the model surface against tests/imagenet_droppath/reference.py: one training step of
``Classifier(ResNet(18, class_labels=10))`` with a forced keep table, the model with the rate at 0 and in test mode, a bottleneck
unit in fp32 and on the bf16 arm, and the refusal of a captured step."""
import numpy as np
import pytest
import torch

import loans_amd
from loans_amd.datasets import synthetic
from loans_amd.functions import drop_path as DP
from oracle import model as M
from tests.gpu_util import dev, rel_err
from tests.imagenet import test_gpu_model as G
from tests.imagenet_droppath import reference as D

pytestmark = pytest.mark.gpu
B, H, W = 4, 64, 64
# units 1 .. 7 of ResNet-18 (unit 0 has p = 0): every one drops at least one sample and keeps at least one
KEEP = np.array([[1, 0, 1, 1], [0, 1, 1, 0], [1, 1, 0, 1], [0, 0, 1, 1], [1, 0, 0, 1], [0, 1, 0, 0], [1, 1, 1, 0]], np.float32)


def _forced(monkeypatch, keep):
    """``DropPath.draw`` replaced by one that uploads ``keep`` [units with p > 0][B] times the units' factors; returns the table"""
    made = {}

    def draw(self, batch, device):
        assert keep.shape == (len(self.active), batch)
        made['r'] = (keep * self.scale[:, None]).astype(np.float32)
        self.table = dev(made['r'])
        return self.table
    monkeypatch.setattr(DP.DropPath, 'draw', draw)
    return made


def test_one_training_step_with_a_forced_table(monkeypatch):
    made = _forced(monkeypatch, KEEP)
    model, net = G._classifier(0)
    dp = net.set_drop_path(0.5, seed=1)
    assert dp.active == list(range(1, 8)) and dp.rates[0] == 0.0 and dp.rates[-1] == 0.5
    frames = synthetic.make_frames(1, B, H, W)
    t = np.array([3, 7, 0, 9], np.int32)
    p32, p64 = G._params(net, np.float32), G._params(net, np.float64)
    opt = loans_amd.Adam(alpha=1e-3, amsgrad=True)
    opt.setup(model)
    seen = {}
    opt.add_hook(lambda o: seen.update({k[len('/predictor/'):]: p.grad_logical().copy() for k, p in o.target.namedparams()}))
    model.to_gpu(0)
    opt.update(model, G._prepared(net, frames), dev(t))
    got_loss, got_logits = float(model.loss.data), model.y.data.cpu().numpy()
    table = {l: made['r'][i] for i, l in enumerate(dp.active)}
    assert all(np.array_equal(v, KEEP[i] * D.keep_factor(dp.rates[l])) for i, (l, v) in enumerate(table.items()))
    r32 = D.DropResNet18Classifier(p32, table).step(frames, t, M.AdamAMSGrad(p32))
    r64 = D.DropResNet18Classifier(p64, table).step(frames.astype(np.float64), t, M.AdamAMSGrad(p64))
    print('loss %.7f  fp32 reference %.7f  fp64 reference %.7f' % (got_loss, r32[0], r64[0]))
    assert np.all(np.abs(got_logits - r64[2]) <= G._tol(r32[2], r64[2]))
    assert abs(got_loss - r64[0]) <= G._tol(r32[0], r64[0])
    assert float(model.accuracy.data) == r64[1]
    worst = 0.0
    for key, ref in r64[3].items():
        if key == 'conv1/b':            # analytically zero gradient (BN follows): rounding noise on both sides
            continue
        e = rel_err(seen[key], ref)
        worst = max(worst, e)
        assert e <= max(5 * rel_err(r32[3][key], ref), 5e-4), (key, e, rel_err(r32[3][key], ref))
    print('worst relative gradient error %.3g' % worst)
    assert set(seen) == {k for k in p64 if M.is_trainable(k)}


# Two steps of ONE unchanged model give the same bits in every gradient but conv1's weight gradient on fp32 frames: that kernel
# (csrc/stem.hip, stem7_wgrad_kernel) closes with one float atomic add per element and block onto the gradient itself, the only
# unordered sum of the step on the order-preserving kernels.  On the bf16 arm the localizer prepares bf16 frames and the stem's
# weight gradient goes through slabs folded in a fixed order, so there every gradient is reproducible.  Measured on an MI355X,
# three steps per arm of the model without stochastic depth, B = 4, 64 x 64: bf16 0 parameters differ; fp32 conv1/W alone, 5913 ..
# 5985 of its 9408 elements, by at most 1.79e-07 at a largest entry of 0.69 .. 0.90: d0 = 2.6e-7.
STEM_WGRAD_D0 = 2.6e-7


def _step(dtype, setup):
    """loss, logits and every parameter's gradient of one step of the ResNet-18 classifier (the localizer's ImageNet form,
    B = 4, 64 x 64) through the optimiser, as a trainer steps"""
    np.random.seed(5)
    loc = loans_amd.SheepLocalizer((75, 75), train_imagenet=True)
    loc.feature_extractor.materialize_head()
    G._randomize(loc, np.random.RandomState(105))
    setup(loc)
    model = loans_amd.Classifier(loc)
    if dtype == 'bf16':
        model.set_precision('bf16', 'bf16')
    model.to_gpu(0)
    opt = loans_amd.Adam(alpha=1e-3, amsgrad=True)
    opt.setup(model)
    seen = {}
    opt.add_hook(lambda o: seen.update({k: p.grad_logical().copy() for k, p in o.target.namedparams()}))
    opt.update(model, dev(synthetic.make_frames(3, B, H, W)), dev(np.array([1, 2, 3, 4], np.int32)))
    torch.cuda.synchronize()
    return model.loss.data.clone(), model.y.data.clone(), seen


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_rate_zero_is_the_model_without_stochastic_depth_bit_for_bit(dtype, deterministic_forward):
    """loss, logits and gradients of the model at rate 0, and of one whose rate was set and taken back, are the bits of the model
    that never called set_drop_path -- and of that model stepped again.  The one exception is named above: conv1's weight
    gradient on the fp32 arm, held to tests/resume/util.py's max(4 d0, 1e-6) with the fixed, measured d0."""
    from tests.resume import util
    never = _step(dtype, lambda loc: None)
    others = (('the same model again', _step(dtype, lambda loc: None)),
              ('rate 0', _step(dtype, lambda loc: loc.set_drop_path(0.0))),
              ('rate 0.5, then 0', _step(dtype, lambda loc: (loc.set_drop_path(0.5, seed=2), loc.set_drop_path(0)))))
    on = _step(dtype, lambda loc: loc.set_drop_path(0.5, seed=2))
    unordered = {'/predictor/feature_extractor/conv1/W'} if dtype == 'f32' else set()
    for name, other in others:
        assert torch.equal(never[0], other[0]) and torch.equal(never[1], other[1]), name
        assert set(other[2]) == set(never[2])
        for key, g in never[2].items():
            if key in unordered:
                d = util.rel(other[2][key], g)
                print('%s: %s %.3g from the model without (allowed %.3g)' % (name, key, d, util.tolerance(STEM_WGRAD_D0)))
                assert d <= util.tolerance(STEM_WGRAD_D0), (name, key)
            else:
                assert np.array_equal(other[2][key], g), (name, key)
    assert not torch.equal(never[1], on[1])


def test_rate_zero_trains_to_the_same_bits(tmp_path, deterministic_forward):
    """the trainer on its bf16 arm, where two runs of one command give the same bits (tests/imagenet_mix/test_gpu_trainer.py),
    with momentum SGD, whose step is linear in the gradient: ``--drop-path 0`` logs and snapshots what the run without it does"""
    import os
    import train_imagenet as T
    from tests.imagenet_mix.test_gpu_trainer import BITS, RUN
    from tests.resume import util
    argv = list(RUN) + ['--optimizer', 'sgd', '--lr', '0.1'] + BITS
    argv[argv.index('--iterations') + 1] = '2'
    logs = {}
    for name, extra in (('without', []), ('zero', ['--drop-path', '0', '--drop-path-seed', '5']), ('on', ['--drop-path', '0.5', '--drop-path-seed', '5'])):
        T.run(T.parse_args(argv + extra + ['-l', str(tmp_path / name)]), log=lambda *a: None)
        logs[name] = util.read_log(str(tmp_path / name))
    for key in ('loss', 'accuracy', 'validation/loss', 'validation/accuracy'):
        assert [e[key] for e in logs['zero']] == [e[key] for e in logs['without']], key
    assert [e['loss'] for e in logs['on']] != [e['loss'] for e in logs['without']]
    with np.load(os.path.join(str(tmp_path / 'zero'), 'SheepLocalizer_2.npz')) as a, \
            np.load(os.path.join(str(tmp_path / 'without'), 'SheepLocalizer_2.npz')) as b:
        assert set(a.files) == set(b.files)
        for k in a.files:
            assert np.array_equal(a[k], b[k]), k


def test_test_mode_draws_nothing_and_scales_nothing(deterministic_forward):
    outs = []
    for rate in (0.0, 0.5):
        model, net = G._classifier(6)
        dp = net.set_drop_path(rate, seed=3)
        model.to_gpu(0)
        with loans_amd.using_config('train', False), loans_amd.using_config('enable_backprop', False):
            model(G._prepared(net, synthetic.make_frames(4, B, H, W)), dev(np.array([1, 2, 3, 4], np.int32)))
        outs.append((model.loss.data.clone(), model.y.data.clone()))
        assert dp is None or dp.table is None           # nothing was drawn
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def _bottleneck(kind):
    from loans_amd.iou.iou_regressor import BottleneckA, BottleneckB
    w = loans_amd.links.HeNormal()
    if kind == 'a':
        blk = BottleneckA(64, 32, 128, 2, w)
        return blk, 64, [('conv1', 'bn1', 2, 0), ('conv2', 'bn2', 1, 1), ('conv3', 'bn3', 1, 0)], ('conv4', 'bn4', 2, 0)
    blk = BottleneckB(128, 32, w)
    return blk, 128, [('conv1', 'bn1', 1, 0), ('conv2', 'bn2', 1, 1), ('conv3', 'bn3', 1, 0)], None


def _unit_case(kind, bf16):
    """(block, input Variable, x, gy, r, stages, shortcut, parameter state) of one bottleneck unit at B = 3, 8 x 8 with the middle
    sample dropped at p = 0.5"""
    from loans_amd.runtime.core import Variable
    rng = np.random.RandomState(3)
    np.random.seed(4)
    blk, cin, stages, sc = _bottleneck(kind)
    for key, p in blk.namedparams():
        if key.endswith('/gamma'):
            p.set_logical((1 + 0.2 * rng.standard_normal(p.logical_shape)).astype(np.float32))
        elif key.endswith('/beta'):
            p.set_logical((0.2 * rng.standard_normal(p.logical_shape)).astype(np.float32))
    blk.finalize(torch.device('cuda', 0))
    q = (lambda a: torch.from_numpy(a).to(torch.bfloat16).float().numpy()) if bf16 else (lambda a: a)
    x = q(rng.standard_normal((3, cin, 8, 8)).astype(np.float32))
    xd = dev(np.ascontiguousarray(x.transpose(0, 2, 3, 1)))
    xv = Variable(xd.to(torch.bfloat16) if bf16 else xd, requires_grad=True)
    dp = DP.DropPath(0.5, 1)
    assert dp.rates == [0.5] and dp.active == [0]
    r = np.array([1, 0, 1], np.float32) * D.keep_factor(0.5)
    dp.table = dev(r[None])
    blk.__dict__['drop_path'], blk.__dict__['drop_slot'] = dp, 0
    return blk, xv, x, rng, q, r, stages, sc, blk.state_dict_chainer()


@pytest.mark.parametrize("kind", ["a", "b"])
def test_bottleneck_unit_against_the_reference(kind):
    """fp32, 1 x 1 shortcut and identity: output and gradients within max(5 x the fp32 reference's own distance, the bound of
    tests/test_gpu_model.py::test_bottleneck_unit_forward_backward) of the float64 reference, max norm"""
    blk, xv, x, rng, q, r, stages, sc, state = _unit_case(kind, False)
    out = blk(xv)
    u64 = D.DropResUnit(M.cast_params(state, np.float64), stages, sc, True, r)
    u32 = D.DropResUnit(M.cast_params(state, np.float32), stages, sc, True, r)
    o64, o32 = u64.fwd(x.astype(np.float64)), u32.fwd(x)
    got = out.data.cpu().numpy().transpose(0, 3, 1, 2)
    e, e32 = rel_err(got, o64), rel_err(o32, o64)
    print('forward %.3g (fp32 reference %.3g)' % (e, e32))
    assert e <= max(5 * e32, 2e-5)
    if sc is None:      # the dropped sample is relu(x) to the bit
        assert np.array_equal(got[1], np.maximum(x[1], 0))
    gy = rng.standard_normal(o64.shape).astype(np.float32)
    out.grad = dev(np.ascontiguousarray(gy.transpose(0, 2, 3, 1)))
    blk.cleargrads()
    out.backward()
    g64, g32 = {}, {}
    gx64, gx32 = u64.bwd(gy.astype(np.float64), g64), u32.bwd(gy, g32)
    e, e32 = rel_err(xv.grad.cpu().numpy().transpose(0, 3, 1, 2), gx64), rel_err(gx32, gx64)
    print('gx %.3g (fp32 reference %.3g)' % (e, e32))
    assert e <= max(5 * e32, 1e-4)
    for key, p in blk.namedparams():
        e, e32 = rel_err(p.grad_logical(), g64[key[1:]]), rel_err(g32[key[1:]], g64[key[1:]])
        print('%s %.3g (fp32 reference %.3g)' % (key, e, e32))
        assert e <= max(5 * e32, 1e-4), key


@pytest.mark.parametrize("kind", ["a", "b"])
def test_bottleneck_unit_bf16_arm_against_the_rounding_reference(kind):
    """the same unit on bf16 tensors against the reference evaluated with bf16-rounded tensors where the arm stores one
    (oracle.model.emulate_bf16_storage), L2 norm, within the bounds tests/test_gpu_model.py::test_residual_unit_bf16_storage
    holds the junction without stochastic depth to: 1e-3 on the output, 1e-2 on every gradient"""
    blk, xv, x, rng, q, r, stages, sc, state = _unit_case(kind, True)
    l2 = lambda a, b: float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))   # noqa: E731
    loans_amd.set_compute_dtype('bf16')
    loans_amd.set_storage_dtype('bf16')
    try:
        out = blk(xv)
        assert out.data.dtype == torch.bfloat16
        unit = D.DropResUnit(M.cast_params(state, np.float64), stages, sc, True, r)
        with M.emulate_bf16_storage():
            e_out = unit.fwd(x.astype(np.float64))
        got = out.data.float().cpu().numpy().transpose(0, 3, 1, 2)
        print('forward l2 %.3g' % l2(got, e_out))
        assert l2(got, e_out) < 1e-3
        gy = q(rng.standard_normal(e_out.shape).astype(np.float32))
        out.grad = dev(np.ascontiguousarray(gy.transpose(0, 2, 3, 1))).to(torch.bfloat16)
        blk.cleargrads()
        out.backward()
        ge = {}
        with M.emulate_bf16_storage():
            gx_e = unit.bwd(gy.astype(np.float64), ge)
        gx = xv.grad.float().cpu().numpy().transpose(0, 3, 1, 2)
        print('gx l2 %.3g' % l2(gx, gx_e))
        assert xv.grad.dtype == torch.bfloat16 and l2(gx, gx_e) < 1e-2
        for key, p in blk.namedparams():
            print('%s l2 %.3g' % (key, l2(p.grad_logical(), ge[key[1:]])))
            assert l2(p.grad_logical(), ge[key[1:]]) < 1e-2, key
    finally:
        loans_amd.set_compute_dtype('f32')


def test_a_captured_step_refuses_a_model_with_a_rate():
    """the LoANs trainer's captured step asks ``refuse_captured_step`` before it records anything; a model whose rate is 0, or
    was set back to 0, passes"""
    np.random.seed(8)
    loc = loans_amd.SheepLocalizer((16, 16))
    DP.refuse_captured_step(loc)
    dp = loc.set_drop_path(0.2, seed=1)
    assert len(dp.rates) == 12 and dp.rates[-1] == 0.2       # res2 .. res5 of the backbone, then res6 and res7
    with pytest.raises(RuntimeError, match='stochastic depth is not built for a captured step'):
        DP.refuse_captured_step(loc)
    assert loc.set_drop_path(0) is None
    DP.refuse_captured_step(loc)


def test_the_trainers_captured_step_refuses_before_it_records(monkeypatch):
    """``SheepAssessor(use_graph=True)`` on a localizer with a rate: ``update()`` raises the sentence at its first step, before the
    warm-up and before any capture begins; with the rate taken back the same updater steps.  ``DropPath.draw`` holds the same
    line for a stream that is already capturing."""
    from loans_amd.runtime import training
    crop = (16, 16)
    np.random.seed(0)
    loc, dis = loans_amd.SheepLocalizer(crop), loans_amd.ResnetAssessor()
    frames = synthetic.make_frames(0, 2, 64, 64)
    real, labels = synthetic.make_assessor_batch(1, 2, 16, 16, src=64)
    with loans_amd.using_config('enable_backprop', False):
        dis(dev(real))                              # materialise the lazy l4
    og, od = loans_amd.Adam(alpha=1e-3, amsgrad=True), loans_amd.Adam(alpha=1e-3, amsgrad=True)
    og.setup(loc)
    od.setup(dis)
    upd = loans_amd.SheepAssessor(
        models=[loc, dis],
        iterator={'main': training.DeviceBatchIterator([dev(frames)]), 'real': training.DeviceBatchIterator([(dev(real), dev(labels))])},
        optimizer={'opt_gen': og, 'opt_dis': od}, converter=training.identity_converter, device=0, use_graph=True)
    dp = loc.set_drop_path(0.2, seed=1)
    with pytest.raises(RuntimeError, match='stochastic depth is not built for a captured step'):
        upd.update()
    assert upd._graph is None and dp.table is None and not torch.cuda.is_current_stream_capturing()     # nothing drawn, nothing recorded
    loc.set_drop_path(0)
    upd.update()                                    # (an eager warm-up step of the same updater)
    assert upd._graph is None and np.isfinite(float(loans_amd.reporter.observation['loss_localizer']))
    monkeypatch.setattr(torch.cuda, 'is_current_stream_capturing', lambda: True)
    with pytest.raises(RuntimeError, match='stochastic depth is not built for a captured step'):
        dp.draw(2, torch.device('cuda', 0))
    assert dp.table is None
