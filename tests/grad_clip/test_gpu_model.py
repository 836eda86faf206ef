"""-m gpu: ``loans_amd.GradientClipping`` on ``Classifier(ResNet(18, class_labels=10))``, 64 x 64 frames, batch 2 (shapes and helpers
of tests/imagenet_sgd/test_gpu_model.py), under ``MomentumSGD``, ``Adam`` and ``LAMB``: two steps with a threshold below the norm --
the gradient a hook behind the clipping hook sees is the gradient a hook in front of it saw (the unclipped step's) times the float64
``k``, and the parameters follow each optimiser's float64 reference fed with the clipped gradient --, a threshold above the norm,
the cold tail of the arena, and the refusal inside a stream capture."""
import math

import numpy as np
import pytest
import torch

import loans_amd
from loans_amd.datasets import synthetic
from oracle import chainer_ops as C
from oracle import model as M
from tests.gpu_util import dev
from tests.grad_clip import cases as A
from tests.imagenet import test_gpu_model as G
from tests.imagenet_lamb import cases as LA
from tests.imagenet_sgd import reference as S
from tests.imagenet_sgd import test_gpu_model as GS
from tests.misc_kernels import cases as MK

pytestmark = pytest.mark.gpu
B, H, W = G.B, G.H, G.W
PREFIX = 'predictor/'
THRESHOLD = 0.05            # below the norm of a freshly initialised classifier's gradient; asserted where it is used
SGD = dict(lr=0.05, momentum=0.9, weight_decay_rate=5e-4)
ADAM = dict(alpha=MK.ADAM_ALPHA, beta1=MK.ADAM_BETA1, beta2=0.999, eps=MK.ADAM_EPS, eta=0.5, weight_decay_rate=1e-2)
LAMB = dict(lr=LA.LR, beta1=LA.BETA1, beta2=LA.BETA2, eps=LA.EPS, weight_decay_rate=5e-4, decay_exempt_1d=True)
OPTIMISERS = {'sgd': lambda: loans_amd.MomentumSGD(**SGD), 'adam': lambda: loans_amd.Adam(**ADAM), 'lamb': lambda: loans_amd.LAMB(**LAMB)}


def _recorder(store, key):
    """a hook that keeps the flat gradient of the active prefix and the gradients per parameter, as they stand when it is called"""
    def hook(o):
        arena = o.target.arena
        store[key] = (arena.grad[:arena.active_numel].clone(),
                      {k[len('/' + PREFIX):]: p.grad_logical().copy() for k, p in o.target.namedparams() if k.startswith('/' + PREFIX)})
    return hook


def _norm64(flat):
    return float(np.sqrt(np.sum(np.square(flat.cpu().numpy().astype(np.longdouble)))))


def _parameters_follow(name, key, p0, g, state, new, t, physical, monkeypatch):
    """error / bound of one parameter after one step from the fp32 state (p0, state) with the gradient g, by the optimiser's own
    float64 reference and bound"""
    if name == 'sgd':
        v0 = state[PREFIX + key + '/v']
        want, _ = S.momentum_sgd_ref(p0, g, v0, SGD['lr'], SGD['momentum'], SGD['weight_decay_rate'])
        bound, _ = S.momentum_sgd_bound(p0, g, v0, SGD['lr'], SGD['momentum'], SGD['weight_decay_rate'])
    elif name == 'adam':
        monkeypatch.setattr(MK, 'ADAM_T', t)
        lr = C.adam_lr(ADAM['alpha'], ADAM['beta1'], ADAM['beta2'], t)
        refs, bounds = MK.adam_ref(p0, g, state[PREFIX + key + '/m'], state[PREFIX + key + '/v'], None, lr, ADAM['beta2'], ADAM['eta'],
                                   ADAM['weight_decay_rate'], 1.0)
        want, bound = refs[0], bounds[0]
    else:
        n = p0.size
        flag = 3 if p0.ndim <= 1 else 0
        T = [16 + 6 + 3 + -(-((physical + 7) // 8 * 8) // LA.UNIT)]
        b = LA.lamb_bounds(p0.ravel(), g.ravel(), state[PREFIX + key + '/m'].ravel(), state[PREFIX + key + '/v'].ravel(), [n], [flag], t,
                           LAMB['lr'], LAMB['weight_decay_rate'], 1.0, T=T)
        want, bound = b['ref']['p'].reshape(p0.shape), b['p'].reshape(p0.shape)
    err = np.abs(new.astype(np.float64) - want)
    bound = np.broadcast_to(bound, err.shape)
    with np.errstate(all='ignore'):       # (a bound of exactly 0 asks for an error of exactly 0)
        return float(np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf)).max())


@pytest.mark.parametrize('name', sorted(OPTIMISERS))
def test_two_clipped_steps(name, monkeypatch):
    model, net = GS._classifier(30)
    opt = OPTIMISERS[name]()
    opt.setup(model)
    seen = {}
    clip = loans_amd.GradientClipping(THRESHOLD)
    opt.add_hook(_recorder(seen, 'before'), name='before')
    opt.add_hook(clip)
    opt.add_hook(_recorder(seen, 'after'), name='after')
    model.to_gpu(0)
    physical = {k[len('/' + PREFIX):]: p.size for k, p in model.namedparams()}
    worst_g = worst_p = 0.0
    for step in range(2):
        start = net.state_dict_chainer()
        state = opt.state_dict()['state']
        keys = [k for k in start if M.is_trainable(k)]
        frames = synthetic.make_frames(60 + step, B, H, W)
        opt.update(model, G._prepared(net, frames), dev(np.array([(3 + step) % 10, (7 * step + 1) % 10], np.int32)))
        (flat0, grads0), (flat1, grads1) = seen['before'], seen['after']
        n = flat0.numel()
        assert n == model.arena.active_numel and set(grads1) == set(keys)
        N64 = _norm64(flat0)
        k64 = A.coefficient(N64, THRESHOLD)
        got_N, got_k = clip.last_norm(), clip.last_coefficient()
        print('%s step %d: N %.6g (float64 %.6g), k %.6g (float64 %.6g)' % (name, step, got_N, N64, got_k, k64))
        if step == 0:
            assert k64 < 1.0, 'THRESHOLD is not below the first step\'s norm %r' % N64
        assert abs(got_N - N64) <= A.norm_rel_bound(n) * N64
        g64 = flat0.cpu().numpy().astype(np.float64)
        if k64 < 1.0:
            rel_k = A.coefficient_rel_bound(n)
            assert abs(got_k - k64) <= rel_k * k64
            want = g64 * k64
            bound = (A.U32 + rel_k) * np.abs(want) * A.SLACK + A.SUBNORMAL
            ratio = float((np.abs(flat1.cpu().numpy().astype(np.float64) - want) / bound).max())        # every float of the prefix
            worst_g = max(worst_g, ratio)
            assert ratio <= 1.0, (step, ratio)
            assert abs(_norm64(flat1) - THRESHOLD) <= (A.clipped_norm_bound(n, THRESHOLD) - THRESHOLD)
        else:
            assert got_k == 1.0 and torch.equal(flat0, flat1)
        new = net.state_dict_chainer()
        for key in keys:
            ratio = _parameters_follow(name, key, start[key], grads1[key], state, new[key], step + 1, physical[key], monkeypatch)
            worst_p = max(worst_p, ratio)
            assert ratio <= 1.0, (step, key, ratio)
    assert opt.t == 2
    print('%s: clipped gradient error / bound %.3f, parameter error / bound %.3f' % (name, worst_g, worst_p))


@pytest.mark.parametrize('name', sorted(OPTIMISERS))
def test_a_threshold_above_the_norm_changes_no_bit(name):
    """the second step on the first step's gradients, without the hook and -- from the same parameters and state -- with it"""
    model, net = GS._classifier(31)
    opt = OPTIMISERS[name]()
    opt.setup(model)
    model.to_gpu(0)
    opt.update(model, G._prepared(net, synthetic.make_frames(70, B, H, W)), dev(np.array([1, 2], np.int32)))
    arena = model.arena
    data1, grad1, state1 = arena.data.clone(), arena.grad.clone(), [s.clone() for s in opt._state]
    opt.update()
    want, want_state = arena.data.clone(), [s.clone() for s in opt._state]
    assert not torch.equal(want, data1)
    arena.data.copy_(data1)
    arena.grad.copy_(grad1)
    for s, s1 in zip(opt._state, state1):
        s.copy_(s1)
    opt.t = 1
    clip = loans_amd.GradientClipping(1e30)
    opt.add_hook(clip)
    opt.update()
    assert opt.t == 2 and clip.last_coefficient() == 1.0 and clip.last_norm() > 0
    assert torch.equal(arena.grad, grad1) and torch.equal(arena.data, want)
    assert all(torch.equal(a, b) for a, b in zip(opt._state, want_state))


def test_the_cold_tail_is_neither_read_nor_written():
    from loans_amd import links as L
    model, net = GS._classifier(32)
    with model.init_scope():
        model.spare = L.Linear(8, 4)            # a link no graph of this test reaches, at the arena's cold end
    model.cold_links = ('spare',)
    opt = loans_amd.MomentumSGD(lr=0.05, momentum=0.9)
    opt.setup(model)
    model.to_gpu(0)
    arena = model.arena
    arena.set_active('spare')
    n = arena.active_numel
    assert 0 < n < arena.numel
    opt.update(model, G._prepared(net, synthetic.make_frames(80, B, H, W)), dev(np.array([0, 5], np.int32)))
    arena.grad[n:] = float('nan')           # a hook that read behind the active prefix would record a NaN and clip nothing
    data1 = arena.data.clone()
    N64 = _norm64(arena.grad[:n])
    clip = loans_amd.GradientClipping(N64 / 4)
    opt.add_hook(clip)
    before = arena.grad[:n].clone()
    opt.update()
    assert abs(clip.last_norm() - N64) <= A.norm_rel_bound(n) * N64
    assert abs(clip.last_coefficient() - 0.25) <= A.coefficient_rel_bound(n) * 0.25
    assert torch.isnan(arena.grad[n:]).all() and torch.equal(arena.data[n:], data1[n:])
    assert torch.equal(arena.grad[:n], before * torch.tensor(clip.last_coefficient(), dtype=torch.float32, device=before.device))
    assert not torch.equal(arena.data[:n], data1[:n]) and torch.isfinite(arena.data[:n]).all()


def test_a_captured_step_with_the_hook_is_refused():
    model, net = GS._classifier(33)
    opt = loans_amd.MomentumSGD(lr=0.05)
    opt.setup(model)
    model.to_gpu(0)
    opt.update(model, G._prepared(net, synthetic.make_frames(90, B, H, W)), dev(np.array([1, 2], np.int32)))
    clip = loans_amd.GradientClipping(1.0)
    opt.add_hook(clip)
    opt.prepare_capture()
    arena = model.arena
    data1, grad1 = arena.data.clone(), arena.grad.clone()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    counter = torch.zeros(4, device='cuda')
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=stream):
        counter.add_(1.0)
        with pytest.raises(RuntimeError, match='optimizer hooks run on the host: not inside a captured step'):
            opt.update()
    torch.cuda.synchronize()
    assert opt.t == 1 and torch.equal(arena.data, data1) and torch.equal(arena.grad, grad1)
    with pytest.raises(RuntimeError, match='no step'):
        clip.last_norm()
    assert math.isfinite(float(arena.data.abs().max()))
