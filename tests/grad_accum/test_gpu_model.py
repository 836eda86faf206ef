"""-m gpu: ``GradientMethod.accumulate`` / the closing ``update`` on ``Classifier(ResNet(18, class_labels=10))``, 64 x 64 frames, batch 2
(shapes and helpers of tests/imagenet_sgd/test_gpu_model.py), on the bf16 arm: its kernels keep their order at these shapes, so a
twin model built from the same seed computes the same micro-gradients bit for bit (two fp32 runs differ by their closing atomics,
tests/weight_average/test_gpu_trainer.py).  The twin never calls ``update``: it runs forward, ``cleargrads``, backward and the
side-stream join by hand, and is stepped through its optimiser's own ``_step``.

Every micro-batch runs inside a step workspace (``ops.begin_step`` / ``ops.end_step``), as ``StandardUpdater`` runs it and as the
trainer runs whose bit-identical repeats the sentence above rests on: outside one, two passes of ONE model over one batch were
measured to differ in the last bit of a third of conv1's weight gradient (1.2e-7 absolute) and nowhere else; inside one, twin
and model agree in every bit."""
import contextlib

import numpy as np
import pytest
import torch

import loans_amd
from loans_amd import ops
from loans_amd.datasets import synthetic
from tests.gpu_util import dev
from tests.grad_clip import cases as CL
from tests.imagenet import test_gpu_model as G
from tests.imagenet_lamb import cases as LA
from tests.imagenet_sgd import test_gpu_model as GS
from tests.misc_kernels import cases as MK

pytestmark = pytest.mark.gpu
B, H, W = G.B, G.H, G.W
SGD = dict(lr=0.05, momentum=0.9, weight_decay_rate=5e-4)
ADAM = dict(alpha=MK.ADAM_ALPHA, beta1=MK.ADAM_BETA1, beta2=0.999, eps=MK.ADAM_EPS, eta=0.5, weight_decay_rate=1e-2)
LAMB = dict(lr=LA.LR, beta1=LA.BETA1, beta2=LA.BETA2, eps=LA.EPS, weight_decay_rate=5e-4, decay_exempt_1d=True)
OPTIMISERS = {'sgd': lambda: loans_amd.MomentumSGD(**SGD), 'adam': lambda: loans_amd.Adam(**ADAM), 'lamb': lambda: loans_amd.LAMB(**LAMB)}


def _pair(seed, name='sgd'):
    """(model, net, optimiser) twice from one seed, on the bf16 arm, on the device"""
    out = []
    for _ in range(2):
        model, net = GS._classifier(seed)
        model.set_precision('bf16', 'bf16')
        opt = OPTIMISERS[name]()
        opt.setup(model)
        model.to_gpu(0)
        out.append((model, net, opt))
    assert torch.equal(out[0][0].arena.data, out[1][0].arena.data)
    return out


def _batch(net, i):
    return G._prepared(net, synthetic.make_frames(200 + i, B, H, W)), dev(np.array([(3 + i) % 10, (7 * i + 1) % 10], np.int32))


@contextlib.contextmanager
def _step():
    """the step workspace of one micro-batch, in the models' precision: what ``StandardUpdater._micro_step`` puts around it"""
    with ops.precision('bf16', 'bf16'):
        ops.begin_step(torch.device('cuda', 0))
        try:
            yield
        finally:
            ops.end_step()


def _by_hand(model, net, i, batch=_batch):
    """the gradient of micro-batch i as the first half of ``update(lossfun, ..)`` leaves it in the arena: a clone of the active prefix"""
    with _step():
        loss = model(*batch(net, i))
        model.cleargrads()
        loss.backward()
        del loss
        arena = model.arena
        ops.join_side_stream(arena.device)
        return arena.grad[:arena.active_numel].clone()


def _accumulate(opt, model, net, i, batch=_batch):
    with _step():
        opt.accumulate(model, *batch(net, i))


def _update(opt, model, net, i, batch=_batch):
    with _step():
        opt.update(model, *batch(net, i))


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _recorder(seen):
    def hook(o):
        arena = o.target.arena
        seen['g'] = arena.grad[:arena.active_numel].clone()
        seen['calls'] = seen.get('calls', 0) + 1
    return hook


@pytest.mark.parametrize('name', sorted(OPTIMISERS))
def test_three_micro_batches_are_one_step_on_their_sequential_sum(name, deterministic_forward):
    (model, net, opt), (twin, twin_net, twin_opt) = _pair(40, name)
    seen = {}
    opt.add_hook(_recorder(seen), name='record')
    arena = model.arena
    n = arena.active_numel
    start = arena.data.clone()
    micro = [_by_hand(twin, twin_net, i) for i in range(3)]
    assert all(g.numel() == n and torch.isfinite(g).all() and float(g.abs().max()) > 0 for g in micro)
    assert not _same(micro[0], micro[1])
    assert opt._accum is None
    _accumulate(opt, model, net, 0)
    assert opt._accum is not None and opt._accum[1].numel() == arena.numel and opt._accum[1].data_ptr() % 16 == 0
    pointer = opt._accum[1].data_ptr()
    assert _same(arena.grad[:n], micro[0]) and _same(opt._accum[1][:n], micro[0])           # STORE: the first gradient, whatever was there
    _accumulate(opt, model, net, 1)
    assert _same(arena.grad[:n], micro[1]) and _same(opt._accum[1][:n], torch.add(micro[0], micro[1]))
    assert opt.t == 0 and opt._accum_count == 2 and 'calls' not in seen
    assert _same(arena.data, start)                                                         # no parameter moved
    _update(opt, model, net, 2)
    want = torch.add(torch.add(micro[0], micro[1]), micro[2])
    assert seen['calls'] == 1 and _same(seen['g'], want)                                    # (g1 + g2) + g3, torch's bits
    assert opt.grad_scale == 1.0 / 3 and opt.t == 1 and opt._accum_count == 0
    assert opt._accum[1].data_ptr() == pointer and _same(opt._accum[1][:n], torch.add(micro[0], micro[1]))         # CLOSE left it alone
    assert not _same(arena.data, start)
    # the optimiser's own step on that sum, on the twin
    twin_arena = twin_opt._ensure_state()
    assert _same(twin_arena.data, start)
    twin_arena.grad[:n].copy_(want)
    twin_opt.t = 1
    twin_opt._step(twin_arena, n, twin_opt._state, twin_opt.lr, 1.0 / 3)
    assert _same(arena.data, twin_arena.data)
    assert all(_same(a, b) for a, b in zip(opt._state, twin_opt._state))

    # a second accumulated step starts with STORE: nothing of what the accumulator held reaches it
    opt._accum[1].fill_(float('nan'))
    micro = [_by_hand(twin, twin_net, i) for i in (3, 4)]
    _accumulate(opt, model, net, 3)
    _update(opt, model, net, 4)
    assert seen['calls'] == 2 and _same(seen['g'], torch.add(micro[0], micro[1])) and torch.isfinite(seen['g']).all()
    assert opt.grad_scale == 0.5 and opt.t == 2 and torch.isfinite(arena.data).all()
    # ... and a plain update() behind it is the plain step again
    _update(opt, model, net, 5)
    assert opt.grad_scale == 1.0 and opt.t == 3 and seen['calls'] == 3


def test_clipping_sees_the_norm_of_the_averaged_accumulated_gradient(deterministic_forward):
    (model, net, opt), (twin, twin_net, _) = _pair(41)
    seen = {}
    clip = loans_amd.GradientClipping(float('inf'))
    opt.add_hook(_recorder(seen), name='record')
    opt.add_hook(clip)
    micro = [_by_hand(twin, twin_net, i) for i in range(3)]
    _accumulate(opt, model, net, 0)
    _accumulate(opt, model, net, 1)
    _update(opt, model, net, 2)
    total = torch.add(torch.add(micro[0], micro[1]), micro[2])
    assert _same(seen['g'], total)
    n = total.numel()
    N64 = float(np.sqrt(np.sum(np.square(total.cpu().numpy().astype(np.longdouble)))) / 3)
    got = clip.last_norm()
    print('N %.9g, float64 |sum| / 3 %.9g' % (got, N64))
    assert N64 > 0 and abs(got - N64) <= CL.norm_rel_bound(n) * N64
    assert clip.last_coefficient() == 1.0


def test_refusals(monkeypatch):
    (model, net, opt), _ = _pair(42)
    arena = model.arena
    # inside a stream capture: accumulate(), and the update() that would close a step
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    counter = torch.zeros(4, device='cuda')
    batch = _batch(net, 0)
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=stream):
        counter.add_(1.0)
        with pytest.raises(RuntimeError, match='not inside a captured step'):
            opt.accumulate(model, *batch)
    torch.cuda.synchronize()
    assert opt._accum_count == 0 and opt._accum is None
    opt.accumulate(model, *batch)
    assert opt._accum_count == 1
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=stream):
        counter.add_(1.0)
        with pytest.raises(RuntimeError, match='closed from the host: not inside a captured step'):
            opt.update()
    torch.cuda.synchronize()
    assert opt._accum_count == 1 and opt.t == 0
    # a checkpoint in the middle of a step
    with pytest.raises(RuntimeError, match=r'state_dict\(\) in the middle of an accumulated step \(1 micro-batches'):
        opt.state_dict()
    with pytest.raises(RuntimeError, match=r'load_state_dict\(\) in the middle of an accumulated step'):
        opt.load_state_dict({})
    # another active prefix than the step's first micro-batch covered
    n = arena.active_numel
    data = arena.data.clone()
    monkeypatch.setattr(arena, 'active_numel', n - 8)
    with pytest.raises(RuntimeError, match='the active parameter prefix changed from %d to %d floats' % (n, n - 8)):
        opt.update()
    monkeypatch.setattr(arena, 'active_numel', n)
    assert opt._accum_count == 1 and opt.t == 0 and torch.equal(arena.data, data)
    # the step can still be closed, and a checkpoint taken behind it
    _update(opt, model, net, 1)
    assert opt._accum_count == 0 and opt.t == 1 and opt.grad_scale == 0.5
    sd = opt.state_dict()
    assert sd['t'] == 1 and not [k for k in list(sd) + list(sd['state']) if 'acc' in k.lower()]
    opt.load_state_dict(sd)


def test_an_optimiser_that_never_accumulates_holds_no_accumulator():
    (model, net, opt), _ = _pair(43)
    _update(opt, model, net, 0)
    _update(opt, model, net, 1)
    assert opt._accum is None and opt._accum_count == 0 and opt.grad_scale == 1.0 and opt.t == 2
