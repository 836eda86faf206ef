"""CPU side of the ImageNet recipe: the error bounds of the momentum-SGD and label-smoothed loss kernels established on their
fp32 NumPy restatements (tests/imagenet_sgd/reference.py) over the grid the GPU tests then run the kernels on; the float64 loss
reference against torch's ``cross_entropy(label_smoothing=)``; ``MomentumSGD``'s host logic; the trainer's new options."""
import numpy as np
import pytest
import torch

import loans_amd
from tests.imagenet import reference as R
from tests.imagenet_sgd import reference as S

SGD_N = (1, 3, 4, 5, 1023, 1024, 1027)
SGD_HYPER = [(m, wd, gs) for m in (0.0, 0.9) for wd in (0.0, 5e-4) for gs in (1.0, 0.5)]


def sgd_inputs(n, seed=0):
    rng = np.random.RandomState(1000 + n % 9973 + seed)
    p = rng.standard_normal(n).astype(np.float32)
    g = (0.1 * rng.standard_normal(n)).astype(np.float32)
    v = (0.01 * rng.standard_normal(n)).astype(np.float32)            # a non-zero starting momentum
    return p, g, v


def test_sgd_restatement_is_inside_the_derived_bound():
    worst = 0.0
    for n in SGD_N + (4 * 256 * 2048 + 6,):
        p, g, v = sgd_inputs(n)
        for mom, wd, gs in SGD_HYPER:
            p64, v64 = S.momentum_sgd_ref(p, g, v, 0.05, mom, wd, gs)
            bp, bv = S.momentum_sgd_bound(p, g, v, 0.05, mom, wd, gs)
            p32, v32 = S.momentum_sgd_fp32(p, g, v, 0.05, mom, wd, gs)
            ep, ev = np.abs(p32 - p64), np.abs(v32 - v64)
            assert np.all(ep <= bp) and np.all(ev <= bv), (n, mom, wd, gs)
            worst = max(worst, float((ep / bp).max()), float((ev / bv).max()))
            # the bound is no looser than the project's fp32 contract: 1e-6 of the magnitudes that go in
            assert np.all(bp <= 1e-6 * (np.abs(p) + np.abs(g) + np.abs(v)))
    # three steps, the errors carried from step to step
    p, g, v = sgd_inputs(1027)
    p64, v64, p32, v32, ep, ev = p, v, p, v, 0.0, 0.0
    for step in range(3):
        gk = np.roll(g, step)
        ep, ev = S.momentum_sgd_bound(p64, gk, v64, 0.05, 0.9, 5e-4, 1.0, ep, ev)
        p64, v64 = S.momentum_sgd_ref(p64, gk, v64, 0.05, 0.9, 5e-4)
        p32, v32 = S.momentum_sgd_fp32(p32, gk, v32, 0.05, 0.9, 5e-4)
        assert np.all(np.abs(p32 - p64) <= ep) and np.all(np.abs(v32 - v64) <= ev), step
        worst = max(worst, float((np.abs(p32 - p64) / ep).max()))
    print('momentum SGD worst error / bound: %.3f' % worst)
    assert worst <= 1.0


def test_sgd_oracle_class_is_the_rule():
    rng = np.random.RandomState(3)
    params = {'conv1/W': rng.standard_normal((4, 3)), 'bn1/avg_mean': rng.standard_normal(4)}
    start = {k: v.copy() for k, v in params.items()}
    opt = S.MomentumSGD(params, lr=0.05, momentum=0.9, weight_decay_rate=5e-4)
    assert set(opt.state) == {'conv1/W'}
    g = rng.standard_normal((4, 3))
    opt.update({'conv1/W': g})
    p1, v1 = S.momentum_sgd_ref(start['conv1/W'], g, 0.0 * g, 0.05, 0.9, 5e-4)
    np.testing.assert_allclose(params['conv1/W'], p1, rtol=1e-15)
    opt.update({})                                  # no gradient: zeros, the momentum and the decay go on
    p2, _ = S.momentum_sgd_ref(p1, 0.0 * g, v1, 0.05, 0.9, 5e-4)
    np.testing.assert_allclose(params['conv1/W'], p2, rtol=1e-15)
    np.testing.assert_array_equal(params['bn1/avg_mean'], start['bn1/avg_mean'])
    assert opt.t == 2


@pytest.mark.parametrize("N", R.XENT_N)
def test_smoothed_loss_restatement_is_inside_the_derived_bound(N):
    worst = {'loss': 0.0, 'gz': 0.0, 'batch': 0.0}
    for name, z, t in S.ls_cases(N):
        assert R.argmax_margin_ok(z) and S.rank_margin_ok(z, t), name
        valid = (t >= 0) & (t < N)
        for eps in S.EPS:
            lb, gb, bb = S.ls_bounds(z, t, eps)
            for k in S.TOPK:
                loss, acc, acck, gz, row_loss, hit, hitk = S.softmax_xent_ls_ref(z, t, eps, k)
                l32, a32, ak32, g32, r32 = S.softmax_xent_ls_fp32(z, t, eps, k)
                assert a32 == np.float32(acc) and ak32 == np.float32(acck), (name, eps, k)
                assert np.all(hitk >= hit), (name, k)
                if k == 1:
                    np.testing.assert_array_equal(hitk, hit, err_msg=name)
                if k >= N:
                    np.testing.assert_array_equal(hitk, valid, err_msg=name)
                if k != S.TOPK[0]:
                    continue                    # loss and gradient do not depend on k
                err = np.abs(r32.astype(np.float64) - row_loss)
                gerr = np.abs(g32.astype(np.float64) - gz)
                assert np.all(err <= lb), (name, eps, float((err - lb).max()))
                assert np.all(gerr <= gb), (name, eps, float((gerr - gb).max()))
                assert abs(l32 - loss) <= bb, (name, eps, l32, loss, bb)
                # ... and no looser than the project's fp32 contract: 1e-4 relative, or 1e-5 / 1e-6 of the largest logit where
                # lse, z_t and mean(z) cancel (the plain loss has two such terms, the smoothed one three)
                assert bb <= max(1e-4 * abs(loss), 1e-5, 1e-6 * float(np.abs(z).max())), (name, eps, bb, loss)
                np.testing.assert_allclose(gz.sum(axis=1), 0.0, atol=1e-14)        # softmax and q both sum to one
                if valid.any():
                    worst['loss'] = max(worst['loss'], float((err[valid] / lb[valid]).max()))
                    worst['gz'] = max(worst['gz'], float((gerr[valid] / gb[valid]).max()))
                    worst['batch'] = max(worst['batch'], abs(l32 - loss) / bb)
                else:
                    assert l32 == 0.0 and loss == 0.0 and not g32.any() and not gz.any(), name
                if name.startswith('equal') and valid.any():       # known answer: uniform softmax, loss = log N whatever eps
                    np.testing.assert_allclose(row_loss[valid], np.log(N), rtol=1e-12, atol=1e-15)
    print('N=%d worst error / bound: row loss %.3f, gz %.3f, batch loss %.3f' % (N, worst['loss'], worst['gz'], worst['batch']))
    assert max(worst.values()) <= 1.0


def test_topk_tie_case():
    z, t = S.topk_tie_case()
    for k, want in ((1, False), (2, True), (3, True)):
        _, acc, acck, _, _, hit, hitk = S.softmax_xent_ls_ref(z, t, 0.1, k)
        assert not hit.any() and acc == 0.0                     # the first of the three tied columns is the argmax
        assert hitk.all() == want and hitk.any() == want and acck == float(want), k
        assert S.softmax_xent_ls_fp32(z, t, 0.1, k)[2] == float(want)


@pytest.mark.parametrize("N", R.XENT_N)
def test_loss_reference_agrees_with_torch_label_smoothing(N):
    """every grid case with a valid row and no ignored label other than -1, float64 on the CPU, loss and autograd gradient"""
    import torch.nn.functional as F
    checked, worst = 0, 0.0
    for name, z, t in S.ls_cases(N):
        if not ((t >= 0) & (t < N)).any() or np.any((t < -1) | (t >= N)):
            continue
        for eps in S.EPS:
            loss, _, _, gz, _, _, _ = S.softmax_xent_ls_ref(z, t, eps, 1)
            zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
            want = F.cross_entropy(zt, torch.tensor(t, dtype=torch.int64), ignore_index=-1, label_smoothing=eps)
            want.backward()
            want = float(want.detach())
            worst = max(worst, abs(loss - want), float(np.abs(gz - zt.grad.numpy()).max()))
            assert abs(loss - want) <= 1e-12, (name, eps, loss, want)
            assert np.abs(gz - zt.grad.numpy()).max() <= 1e-12, (name, eps)
            checked += 1
    print('N=%d: %d cases, worst difference %.3g' % (N, checked, worst))
    assert checked >= 3 * 8


@pytest.mark.parametrize("N", R.XENT_N)
def test_unsmoothed_top1_reference_is_the_plain_reference(N):
    for name, z, t in S.ls_cases(N):
        loss, acc, acck, gz, row_loss, hit, hitk = S.softmax_xent_ls_ref(z, t, 0.0, 1)
        l0, a0, g0, r0, am = R.softmax_xent_ref(z, t)
        assert loss == l0 and acc == a0 and acck == a0, name
        np.testing.assert_array_equal(gz, g0, err_msg=name)
        np.testing.assert_array_equal(row_loss, r0, err_msg=name)
        np.testing.assert_array_equal(hit, am == t, err_msg=name)


# ---- host logic -----------------------------------------------------------------------------------------------------------------
def test_momentum_sgd_surface_and_hooks(monkeypatch):
    opt = loans_amd.MomentumSGD()
    assert (opt.hyperparam.lr, opt.hyperparam.momentum, opt.hyperparam.weight_decay_rate) == (0.01, 0.9, 0.0)
    opt = loans_amd.MomentumSGD(lr=0.05, momentum=0.8, weight_decay_rate=5e-4)
    assert (opt.lr, opt.hyperparam.momentum, opt.hyperparam.weight_decay_rate, opt.t) == (0.05, 0.8, 5e-4, 0)
    opt.lr = 0.005
    assert opt.hyperparam.lr == 0.005 and opt.lr == 0.005
    opt.hyperparam.lr = 0.5
    assert opt.lr == 0.5
    from loans_amd.runtime import optimizers
    assert isinstance(opt, optimizers.GradientMethod) and issubclass(loans_amd.Adam, optimizers.GradientMethod)
    # everything that is not an update rule's arithmetic lives once, in the base class
    for name in ('update', 'add_hook', 'remove_hook', 'call_hooks', 'setup', '_exchange', 'stage_done', 'update_begin',
                 'exchange_wait', 'prepare_capture', 'begin_replay', '_ensure_state'):
        assert name not in vars(loans_amd.Adam) and name not in vars(loans_amd.MomentumSGD), name
        assert hasattr(optimizers.GradientMethod, name), name

    # update() on a two-parameter link whose arena lives on the CPU, the kernel call recorded instead of launched
    class Net(loans_amd.Chain):
        def __init__(self):
            super().__init__()
            with self.init_scope():
                self.w = loans_amd.Parameter(np.arange(8, dtype=np.float32), (8,))
                self.b = loans_amd.Parameter(np.ones(3, np.float32), (3,))
    net = Net()
    net.finalize(torch.device('cpu'))
    calls = []
    from loans_amd import ops
    monkeypatch.setattr(ops, 'momentum_sgd', lambda *a: calls.append(a))
    monkeypatch.setattr(ops, 'join_side_stream', lambda *a: None)
    monkeypatch.setattr(torch.cuda, 'is_current_stream_capturing', lambda: False)         # no device to ask
    assert opt.setup(net) is opt and opt.target is net
    seen = []
    opt.add_hook(lambda o: seen.append(o.t), name='probe')
    with pytest.raises(KeyError):
        opt.add_hook(lambda o: None, name='probe')
    with pytest.raises(TypeError):
        opt.add_hook(3)
    opt.update()
    opt.update()
    assert seen == [0, 1] and opt.t == 2                 # once per update, before the step is counted
    assert len(calls) == 2
    p, g, v, lr, mom, wd, gs = calls[-1]
    assert (lr, mom, wd, gs) == (0.5, 0.8, 5e-4, 1.0)
    assert p.numel() == g.numel() == v.numel() == net.arena.numel and p.data_ptr() == net.arena.data.data_ptr()
    assert len(opt._state) == 1 and not opt._state[0].any()            # one v buffer the size of the arena
    opt.remove_hook('probe')
    opt.update()
    assert seen == [0, 1] and opt.t == 3
    net.disable_update()
    opt.update()
    assert opt.t == 3 and len(calls) == 3


TODAYS_DEFAULTS = {
    'train_file': 'synthetic', 'val_file': 'synthetic', 'use_resnet_18': False, 'batch_size': 32, 'gpu': -1,
    'learning_rate': 0.001, 'weight_decay': 0.0, 'num_epoch': 100, 'iterations': None, 'image_size': (224, 224),
    'log_dir': 'imagenet_logs', 'ln': 'test', 'log_interval': 100, 'snapshot_interval': 1000, 'dtype': 'f32', 'seed': None,
    'no_shuffle': False, 'validation': True, 'dataset_size': 256, 'validation_size': 64, 'synthetic_classes': 10,
    'data_seed': 10, 'flat_log_dir': False, 'loader_threads': 4}


def test_trainer_options_and_their_defaults():
    import train_imagenet as T
    a = vars(T.parse_args([]))
    new = {'optimizer': 'adam', 'momentum': 0.9, 'lr_drop_epochs': (), 'lr_drop_factor': 0.1, 'label_smoothing': 0.0, 'topk': None}
    assert {k: v for k, v in a.items() if k not in new} == TODAYS_DEFAULTS
    assert {k: a[k] for k in new} == new
    args = T.parse_args([])
    assert T.resolved_topk(args) is None                        # Adam and no option: the reports are today's
    model_args = T.parse_args(['--use-resnet-18'])
    np.random.seed(0)
    model = T.build_model(model_args)
    assert model.label_smoothing == 0.0 and model.topk is None
    a = T.parse_args(['--optimizer', 'sgd', '--momentum', '0.8', '--lr', '0.1', '--weight-decay', '1e-4', '--lr-drop-epochs', '30', '60',
                      '90', '--lr-drop-factor', '0.2', '--label-smoothing', '0.1', '--use-resnet-18'])
    assert (a.optimizer, a.momentum, a.learning_rate, a.weight_decay) == ('sgd', 0.8, 0.1, 1e-4)
    assert (list(a.lr_drop_epochs), a.lr_drop_factor, a.label_smoothing) == ([30, 60, 90], 0.2, 0.1)
    assert T.resolved_topk(a) == 5                              # the recipe reports top-5
    model = T.build_model(a)
    assert model.label_smoothing == 0.1 and model.topk == 5
    assert T.resolved_topk(T.parse_args(['--topk', '3'])) == 3
    assert T.resolved_topk(T.parse_args(['--optimizer', 'sgd', '--topk', '0'])) is None
    with pytest.raises(SystemExit):
        T.parse_args(['--optimizer', 'rmsprop'])
    with pytest.raises(ValueError):
        loans_amd.Classifier(model.predictor, label_smoothing=1.0)
    with pytest.raises(ValueError):
        loans_amd.Classifier(model.predictor, topk=0)


def test_lr_schedule_is_a_pure_function_of_boundaries_and_factor():
    import train_imagenet as T
    f = T.scheduled_lr
    assert [f(0.1, e, (), 0.1) for e in (0, 5, 500)] == [0.1, 0.1, 0.1]              # no boundary: the base rate, bit for bit
    assert f(0.001, 0, (), 0.1) == 0.001
    got = [f(0.1, e, (30, 60, 90), 0.1) for e in (0, 29, 30, 59, 60, 89, 90, 99)]
    np.testing.assert_allclose(got, [0.1, 0.1, 0.01, 0.01, 0.001, 0.001, 0.0001, 0.0001], rtol=1e-12)
    assert f(0.05, 0, [1], 0.1) == 0.05 and f(0.05, 1, [1], 0.1) == pytest.approx(0.005, rel=1e-12)
    assert f(0.1, 70, (60, 30, 90), 0.5) == f(0.1, 70, (30, 60, 90), 0.5) == 0.1 * 0.5 ** 2      # order is immaterial
    assert f(0.1, 70, (30, 30, 60), 0.5) == 0.1 * 0.5 ** 2                                        # a repeated epoch counts once
    assert f(0.1, 30, (30,), 0.1) == f(0.1, 30, (30,), 0.1)                                       # no hidden state
