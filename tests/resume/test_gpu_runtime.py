"""-m gpu: ``GradientMethod.state_dict()`` / ``load_state_dict()``.  The update kernels are element-wise and deterministic, so
everything here is exact: after a round trip into a fresh model and optimiser built from another seed the step count, the
hyper-parameters, every state buffer and every parameter are ``torch.equal``, and so are the parameters after one more step on
the same gradient."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

_GRADS = {}


def _classifier(seed):
    import loans_amd
    np.random.seed(seed)
    model = loans_amd.Classifier(loans_amd.SheepLocalizer((75, 75), train_imagenet=True))
    model.materialize()
    return model.to_gpu(0)


def _localizer(seed):
    import loans_amd
    np.random.seed(seed)
    return loans_amd.SheepLocalizer((75, 75)).to_gpu(0)


def _optimizer(kind):
    import loans_amd
    if kind == 'sgd':
        return loans_amd.MomentumSGD(lr=0.05, momentum=0.9, weight_decay_rate=1e-4)
    return loans_amd.Adam(alpha=1e-3, weight_decay_rate=1e-4, amsgrad=kind == 'amsgrad')


def _fill_grads(model, tag, seed):
    """seeded values into the whole gradient arena, written parameter by parameter in the Chainer layout (what a backward
    writes: channel padding and alignment gaps stay zero); built once per model kind and seed"""
    arena = model.arena
    if (tag, seed) not in _GRADS:
        rng = np.random.RandomState(seed)
        flat = np.zeros(arena.numel, np.float32)
        for p, o in zip(arena.params, arena.offsets):
            g = (1e-2 * rng.standard_normal(p.logical_shape)).astype(np.float32)
            flat[o:o + p.size] = np.ascontiguousarray(p._from_logical(g)).ravel()
        _GRADS[(tag, seed)] = torch.from_numpy(flat)
    arena.grad.copy_(_GRADS[(tag, seed)])


def _assert_same(a, b, opt_a, opt_b):
    assert opt_a.t == opt_b.t and vars(opt_a.hyperparam) == vars(opt_b.hyperparam)
    assert getattr(opt_a, '_stepped_numel', 0) == getattr(opt_b, '_stepped_numel', 0)
    assert len(opt_a._state) == len(opt_b._state)
    for name, sa, sb in zip(opt_a._state_names(), opt_a._state, opt_b._state):
        assert torch.equal(sa, sb), name
        assert float(sa.abs().max()) > 0, name
    assert torch.equal(a.arena.data, b.arena.data)
    for (ka, pa), (kb, pb) in zip(a.namedparams(), b.namedparams()):
        assert ka == kb and torch.equal(pa.data, pb.data), ka


@pytest.mark.parametrize('kind', ['sgd', 'adam', 'amsgrad'])
def test_round_trip_of_the_classifier(kind):
    a, opt_a = _classifier(1), _optimizer(kind)
    opt_a.setup(a)
    for seed in (11, 12, 11):
        _fill_grads(a, 'classifier', seed)
        opt_a.update()
    if kind != 'sgd':
        opt_a.alpha = 3e-4                      # a rate the schedule has moved travels too
    sd = opt_a.state_dict()
    assert sd['t'] == 3 and sd['class'] == type(opt_a).__name__ and sd['stepped_cold'] == []
    names = {'sgd': {'v'}, 'adam': {'m', 'v'}, 'amsgrad': {'m', 'v', 'vhat'}}[kind]
    paths = {k[1:] for k, _ in a.namedparams()}
    assert set(sd['state']) == {'%s/%s' % (p, n) for p in paths for n in names}
    assert sd['state']['predictor/feature_extractor/conv1/W/' + sorted(names)[0]].shape == (64, 3, 7, 7)       # Chainer's OIHW

    b, opt_b = _classifier(2), _optimizer(kind)
    opt_b.setup(b)
    opt_b.hyperparam.weight_decay_rate = 0.5    # overwritten by the load
    assert not torch.equal(a.arena.data, b.arena.data)
    opt_b.prepare_capture()                     # the device copy of the rate a captured step reads
    b.load_state_dict_chainer(a.state_dict_chainer(), strict=True)
    opt_b.load_state_dict(sd)
    _assert_same(a, b, opt_a, opt_b)
    assert float(opt_b._lr_dev) == float(torch.tensor(opt_b.lr, dtype=torch.float32))
    for model, opt in ((a, opt_a), (b, opt_b)):
        _fill_grads(model, 'classifier', 12)
        opt.update()
    _assert_same(a, b, opt_a, opt_b)
    assert opt_b.t == 4


def test_round_trip_keeps_the_state_behind_the_active_prefix():
    """the plain localizer on 64 x 64 frames: res6 / res7 lie behind the active prefix.  They were stepped once (a tall batch
    earlier in the run), so their moments are alive and keep decaying on zero gradients: the full-length buffers and the
    stepped prefix must both survive, or the fourth step differs"""
    import loans_amd
    frames = torch.rand(2, 3, 64, 64, device='cuda')

    def forward(model):                         # what fixes the active prefix of a step
        with loans_amd.using_config('train', False), loans_amd.using_config('enable_backprop', False):
            model(frames)

    a, opt_a = _localizer(1), _optimizer('amsgrad')
    opt_a.setup(a)
    a.arena.set_active(None)
    _fill_grads(a, 'localizer', 11)
    opt_a.update()
    forward(a)
    cold = a.arena.cold_offsets['res6']
    assert a.arena.active_numel == cold < a.arena.numel
    for seed in (12, 11):
        _fill_grads(a, 'localizer', seed)
        opt_a.update()
    sd = opt_a.state_dict()
    assert sd['stepped_cold'] == ['res6', 'res7']
    assert any(k.startswith('res7/') and np.abs(v).max() > 0 for k, v in sd['state'].items())

    b, opt_b = _localizer(2), _optimizer('amsgrad')
    opt_b.setup(b)
    b.load_state_dict_chainer(a.state_dict_chainer(), strict=True)
    opt_b.load_state_dict(sd)
    _assert_same(a, b, opt_a, opt_b)
    for name, sa, sb in zip(opt_a._state_names(), opt_a._state, opt_b._state):
        assert torch.equal(sa[cold:], sb[cold:]) and float(sa[cold:].abs().max()) > 0, name
    before = a.arena.data[cold:].clone()
    for model, opt in ((a, opt_a), (b, opt_b)):
        forward(model)
        _fill_grads(model, 'localizer', 12)
        opt.update()
    _assert_same(a, b, opt_a, opt_b)
    assert not torch.equal(a.arena.data[cold:], before)          # res6 / res7 went on moving, on both sides alike

    # a run that never left the prefix: nothing behind it is stepped after the load either
    c, opt_c = _localizer(3), _optimizer('amsgrad')
    opt_c.setup(c)
    forward(c)
    _fill_grads(c, 'localizer', 11)
    opt_c.update()
    sd = opt_c.state_dict()
    assert sd['stepped_cold'] == []
    opt_b.load_state_dict(sd)
    assert opt_b._stepped_numel == cold and opt_b.t == 1 and float(opt_b._state[0][cold:].abs().max()) == 0


def test_mismatches_name_the_key():
    a, opt_a = _classifier(1), _optimizer('amsgrad')
    opt_a.setup(a)
    _fill_grads(a, 'classifier', 11)
    opt_a.update()
    sd = opt_a.state_dict()

    def loaded(change, kind='amsgrad', model=a):
        other = dict(sd, hyperparam=dict(sd['hyperparam']), state=dict(sd['state']))
        change(other)
        opt = _optimizer(kind)
        opt.setup(model)
        return opt.load_state_dict(other)

    with pytest.raises(ValueError, match='class.*Adam.*MomentumSGD'):
        loaded(lambda o: None, kind='sgd')
    with pytest.raises(ValueError, match='amsgrad'):
        loaded(lambda o: None, kind='adam')
    key = 'predictor/feature_extractor/res3/0/conv1/W/v'
    assert key in sd['state']
    with pytest.raises(ValueError, match=key + ': not in the checkpoint'):
        loaded(lambda o: o['state'].pop(key))
    with pytest.raises(ValueError, match='predictor/res9/W/m: no such parameter'):
        loaded(lambda o: o['state'].update({'predictor/res9/W/m': np.zeros(3, np.float32)}))
    with pytest.raises(ValueError, match=key + r': shape \(1, 2\)'):
        loaded(lambda o: o['state'].update({key: np.zeros((1, 2), np.float32)}))
    with pytest.raises(ValueError, match='^feature_extractor/bn1/beta/m: not in the checkpoint'):          # the plain localizer has other parameter paths
        loaded(lambda o: None, model=_localizer(1))
    loaded(lambda o: None)                                  # and the unchanged record loads
