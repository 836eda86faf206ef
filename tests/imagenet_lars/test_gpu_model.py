"""-m gpu: ``loans_amd.LARS`` on ``Classifier(ResNet(18, class_labels=10))``, 64 x 64 frames, batch 2: three steps against the
float64 rule applied to the gradients the HIP steps produced (a hook reads them off the device, so the convolutions' error does not
enter), ``trust_ratios()`` against the same reference, and ``state_dict`` -> fresh optimiser -> ``load_state_dict`` bit for bit."""
import numpy as np
import pytest
import torch

import loans_amd
from loans_amd.datasets import synthetic
from oracle import model as M
from tests.gpu_util import dev
from tests.imagenet import test_gpu_model as G
from tests.imagenet_lars import cases as A
from tests.imagenet_sgd import reference as S
from tests.imagenet_sgd import test_gpu_model as GS

pytestmark = pytest.mark.gpu
B, H, W = G.B, G.H, G.W
LR, MOMENTUM, DECAY, ETA, EPS = 0.1, 0.9, 5e-4, 0.2, 1e-8
PREFIX = 'predictor/'


def _additions(size):
    """T of a parameter's segment: it runs to the next parameter's offset, ParamArena pads to 8"""
    return 16 + 6 + 3 + -(-((size + 7) // 8 * 8) // A.UNIT)


def test_three_lars_steps_follow_the_float64_rule():
    model, net = GS._classifier(20, label_smoothing=0.1, topk=3)
    opt = loans_amd.LARS(lr=LR, momentum=MOMENTUM, weight_decay_rate=DECAY, eta=ETA, eps=EPS, decay_exempt_1d=True)
    opt.setup(model)
    seen = {}
    opt.add_hook(GS._grad_hook(seen))
    start = G._params(net, np.float64)
    keys = [k for k in start if M.is_trainable(k)]
    ref_p = {k: start[k].copy() for k in keys}
    ref_v = {k: np.zeros_like(start[k]) for k in keys}
    ep = {k: 0.0 for k in keys}
    ev = {k: 0.0 for k in keys}
    model.to_gpu(0)
    physical = {k[len('/' + PREFIX):]: p.size for k, p in model.namedparams()}
    worst_r = 0.0
    for step in range(3):
        frames = synthetic.make_frames(30 + step, B, H, W)
        t = np.array([(3 + step) % 10, (7 * step + 1) % 10], np.int32)
        opt.update(model, G._prepared(net, frames), dev(t))
        got_r = opt.trust_ratios()
        assert set(got_r) == {PREFIX + k for k in keys} and set(seen) == set(keys)
        adapting = 0
        for k in keys:
            g = seen[k].astype(np.float64)
            flag = 3 if ref_p[k].ndim <= 1 else 0
            wd_s = 0.0 if flag & 1 else DECAY
            Wn, Gn = float(np.sqrt(np.sum(ref_p[k] ** 2))), float(np.sqrt(np.sum(g ** 2)))
            r = A.ratio_of(Wn, Gn, flag, DECAY, ETA, EPS)
            if r == 1.0:
                rel_r = 0.0
                assert got_r[PREFIX + k] == 1.0, (step, k)
            else:
                adapting += 1
                rel_r = (A.U32 + A.C * _additions(physical[k]) * A.U64) * A.SLACK + float(np.sqrt(np.sum(np.square(ep[k])))) / Wn
                err = abs(got_r[PREFIX + k] - r) / (rel_r * r)
                worst_r = max(worst_r, err)
                assert err <= 1.0, (step, k, got_r[PREFIX + k], r, err)
            bp, bv = A.lars_step_bound(ref_p[k], g, ref_v[k], LR, r, rel_r, MOMENTUM, wd_s, 1.0, ep[k], ev[k])
            ref_p[k], ref_v[k] = S.momentum_sgd_ref(ref_p[k], g, ref_v[k], LR * r, MOMENTUM, wd_s)
            ep[k], ev[k] = bp, bv
        assert adapting == sum(start[k].ndim > 1 for k in keys) > 15            # every weight tensor adapts
    assert opt.t == 3
    new = net.state_dict_chainer()
    worst = 0.0
    for k in keys:
        err = np.abs(new[k].astype(np.float64) - ref_p[k]) / ep[k]
        worst = max(worst, float(err.max()))
        assert np.all(err <= 1.0), (k, float(err.max()))
        assert np.abs(new[k] - start[k]).max() > 0 or k == 'conv1/b', k
    print('three LARS steps: ratio error / bound %.3f, parameter error / bound %.3f' % (worst_r, worst))
    # the weights moved by about lr * eta per step, whatever the gradient's scale: that is the point of the rule
    moved = np.sqrt(np.sum((new['res3/0/conv1/W'] - start['res3/0/conv1/W']) ** 2) / np.sum(start['res3/0/conv1/W'] ** 2))
    assert 0.2 * LR * ETA < moved < 3 * 2.71 * LR * ETA, moved


def test_state_dict_into_a_fresh_optimiser_continues_bit_for_bit():
    model, net = GS._classifier(21)
    opt = loans_amd.LARS(lr=LR, momentum=MOMENTUM, weight_decay_rate=DECAY, eta=ETA, eps=EPS, decay_exempt_1d=True)
    opt.setup(model)
    model.to_gpu(0)
    for step in range(2):
        opt.update(model, G._prepared(net, synthetic.make_frames(40 + step, B, H, W)), dev(np.array([step, 9 - step], np.int32)))
    arena = model.arena
    sd = opt.state_dict()
    assert (sd['class'], sd['t']) == ('LARS', 2) and sd['hyperparam'] == dict(lr=LR, momentum=MOMENTUM, weight_decay_rate=DECAY, eta=ETA,
                                                                               eps=EPS, decay_exempt_1d=True)
    assert 'predictor/conv1/W/v' in sd['state'] and np.abs(sd['state']['predictor/conv1/W/v']).max() > 0
    data2, grad3 = arena.data.clone(), arena.grad.clone()       # the third step runs on the second step's gradients, both times
    opt.update()
    want_p, want_v, want_r = arena.data.clone(), opt._state[0].clone(), opt.trust_ratios()
    assert not torch.equal(want_p, data2)

    arena.data.copy_(data2)
    arena.grad.copy_(grad3)
    fresh = loans_amd.LARS(lr=0.123, momentum=0.5, eta=0.5, eps=0.25)
    fresh.setup(model)
    fresh.load_state_dict(sd)
    assert fresh.t == 2 and vars(fresh.hyperparam) == vars(opt.hyperparam)
    fresh.update()
    assert fresh.t == 3
    assert torch.equal(arena.data, want_p) and torch.equal(fresh._state[0], want_v) and fresh.trust_ratios() == want_r
    with pytest.raises(ValueError, match='class'):
        loans_amd.MomentumSGD().setup(model).load_state_dict(sd)
