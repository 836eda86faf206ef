"""-m gpu: ``loans_amd.LAMB`` on ``Classifier(ResNet(18, class_labels=10))``, 64 x 64 frames, batch 2: two steps against the
float64 rule applied to the gradients the HIP steps produced (a hook reads them off the device, so the convolutions' error does not
enter), ``trust_ratios()`` against the same reference, ``state_dict`` -> fresh optimiser -> ``load_state_dict`` bit for bit, and
the refusal inside a stream capture."""
import numpy as np
import pytest
import torch

import loans_amd
from loans_amd.datasets import synthetic
from oracle import model as M
from tests.gpu_util import dev
from tests.imagenet import test_gpu_model as G
from tests.imagenet_lamb import cases as A
from tests.imagenet_sgd import test_gpu_model as GS

pytestmark = pytest.mark.gpu
B, H, W = G.B, G.H, G.W
HYPER = dict(lr=A.LR, beta1=0.9, beta2=0.999, eps=1e-6, weight_decay_rate=5e-4, decay_exempt_1d=True)
PREFIX = 'predictor/'


def additions_of(size):
    """T of a parameter's segment: it runs to the next parameter's offset, ParamArena pads to 8"""
    return [16 + 6 + 3 + -(-((size + 7) // 8 * 8) // A.UNIT)]


def test_two_lamb_steps_follow_the_float64_rule():
    model, net = GS._classifier(20, label_smoothing=0.1, topk=3)
    opt = loans_amd.LAMB(**HYPER)
    opt.setup(model)
    seen = {}
    opt.add_hook(GS._grad_hook(seen))
    start = G._params(net, np.float64)
    keys = [k for k in start if M.is_trainable(k)]
    ref = {k: dict(p=start[k].ravel().copy(), m=np.zeros(start[k].size), v=np.zeros(start[k].size)) for k in keys}
    err = {k: dict(p=0.0, m=0.0, v=0.0) for k in keys}
    model.to_gpu(0)
    physical = {k[len('/' + PREFIX):]: p.size for k, p in model.namedparams()}
    worst_r = 0.0
    for step in range(2):
        frames = synthetic.make_frames(30 + step, B, H, W)
        t = np.array([(3 + step) % 10, (7 * step + 1) % 10], np.int32)
        opt.update(model, G._prepared(net, frames), dev(t))
        got_r = opt.trust_ratios()
        assert set(got_r) == {PREFIX + k for k in keys} and set(seen) == set(keys)
        adapting = 0
        for k in keys:
            flag = 3 if start[k].ndim <= 1 else 0
            n = start[k].size
            case = (ref[k]['p'], seen[k].ravel(), ref[k]['m'], ref[k]['v'], [n], [flag], step + 1, HYPER['lr'], HYPER['weight_decay_rate'], 1.0)
            b = A.lamb_bounds(*case, ep=err[k]['p'], em=err[k]['m'], ev=err[k]['v'], T=additions_of(physical[k]))
            want = b['ref']['r'][0]
            if b['rel_r'][0] == 0.0:
                assert got_r[PREFIX + k] == 1.0 == want, (step, k)
            else:
                adapting += 1
                e = abs(got_r[PREFIX + k] - want) / (b['rel_r'][0] * want)
                worst_r = max(worst_r, e)
                assert e <= 1.0, (step, k, got_r[PREFIX + k], want, e)
            ref[k] = {name: b['ref'][name] for name in 'pmv'}
            err[k] = {name: b[name] for name in 'pmv'}
        assert adapting == sum(start[k].ndim > 1 for k in keys) > 15            # every weight tensor adapts
    assert opt.t == 2
    new = net.state_dict_chainer()
    state = opt.state_dict()['state']
    worst = 0.0
    for k in keys:
        for name, have in (('p', new[k]), ('m', state[PREFIX + k + '/m']), ('v', state[PREFIX + k + '/v'])):
            e = np.abs(have.astype(np.float64).ravel() - ref[k][name]) / err[k][name]
            worst = max(worst, float(e.max()))
            assert np.all(e <= 1.0), (k, name, float(e.max()))
        assert np.abs(new[k] - start[k]).max() > 0 or k == 'conv1/b', k
    print('two LAMB steps: ratio error / bound %.3f, parameter and moment error / bound %.3f' % (worst_r, worst))
    # a weight tensor moves by lr of its norm per step, whatever the gradient's scale: that is the point of the rule
    w0, w2 = start['res3/0/conv1/W'], new['res3/0/conv1/W']
    moved = np.sqrt(np.sum((w2 - w0) ** 2) / np.sum(w0 ** 2))
    assert 0.2 * HYPER['lr'] < moved <= 2 * HYPER['lr'] * (1 + 1e-3), moved


def test_state_dict_into_a_fresh_optimiser_continues_bit_for_bit():
    model, net = GS._classifier(21)
    opt = loans_amd.LAMB(**HYPER)
    opt.setup(model)
    model.to_gpu(0)
    for step in range(2):
        opt.update(model, G._prepared(net, synthetic.make_frames(40 + step, B, H, W)), dev(np.array([step, 9 - step], np.int32)))
    arena = model.arena
    sd = opt.state_dict()
    assert (sd['class'], sd['t']) == ('LAMB', 2) and sd['hyperparam'] == HYPER
    for name in ('m', 'v'):
        assert np.abs(sd['state']['predictor/conv1/W/' + name]).max() > 0
    assert not [k for k in sd['state'] if not k.endswith(('/m', '/v'))] and sd['state']['predictor/conv1/W/v'].min() >= 0
    data2, grad3 = arena.data.clone(), arena.grad.clone()       # the third step runs on the second step's gradients, both times
    opt.update()
    want_p, want_m, want_v, want_r = arena.data.clone(), opt._state[0].clone(), opt._state[1].clone(), opt.trust_ratios()
    assert not torch.equal(want_p, data2)

    arena.data.copy_(data2)
    arena.grad.copy_(grad3)
    fresh = loans_amd.LAMB(lr=0.123, beta1=0.5, beta2=0.5, eps=0.25)
    fresh.setup(model)
    fresh.load_state_dict(sd)
    assert fresh.t == 2 and vars(fresh.hyperparam) == vars(opt.hyperparam)
    fresh.update()
    assert fresh.t == 3
    assert torch.equal(arena.data, want_p) and torch.equal(fresh._state[0], want_m) and torch.equal(fresh._state[1], want_v)
    assert fresh.trust_ratios() == want_r
    with pytest.raises(ValueError, match='class: the checkpoint holds LAMB, this optimiser is LARS'):
        loans_amd.LARS().setup(model).load_state_dict(sd)
    with pytest.raises(ValueError, match='class'):
        loans_amd.Adam().setup(model).load_state_dict(sd)


def test_a_captured_step_is_refused_with_a_sentence():
    """the refusal comes before any launch: the rate of a captured step is a device scalar, and LAMB's c1, c2 are launch arguments"""
    model, net = GS._classifier(22)
    opt = loans_amd.LAMB(**HYPER)
    opt.setup(model)
    model.to_gpu(0)
    opt.update(model, G._prepared(net, synthetic.make_frames(50, B, H, W)), dev(np.array([1, 2], np.int32)))
    arena = model.arena
    before = arena.data.clone()
    with pytest.raises(RuntimeError, match='LAMB is not built for a captured step'):
        opt._step(arena, arena.active_numel, opt._state, torch.zeros(1, device=arena.device), 1.0)
    assert torch.equal(arena.data, before) and opt.t == 1
