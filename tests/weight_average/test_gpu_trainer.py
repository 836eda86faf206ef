"""-m gpu: ``WeightAverage`` on the ``Classifier`` and ``train_imagenet.py --ema-decay / --lr-schedule cosine / --no-decay-1d``.
ResNet-18 on 64 x 64 frames, batches of 2, the synthetic classes in order, one loader thread.

Comparisons that ask for EQUAL numbers of two runs are made on the bf16 arm: its kernels keep their order at these shapes and two
runs of one command are bit-identical (tests/resume/test_gpu_trainer.py: d0 = 0 over five runs), while the fp32 weight gradients
close with atomics and two fp32 runs part in the 7th digit at iteration 2.  Comparisons inside ONE run (the averaged snapshot
against the recurrence over the live snapshots, the logged metrics against the snapshot re-evaluated) run on both arms.

A run is made once per module and shared by the tests that read it (``_run``)."""
import json
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests.weight_average import cases as A

pytestmark = pytest.mark.gpu

BASE = ['--use-resnet-18', '-b', '2', '--image-size', '64', '64', '--dataset-size', '8', '--validation-size', '4',
        '--synthetic-classes', '4', '--seed', '0', '--log-interval', '1', '--no-shuffle', '--loader-threads', '1', '--flat-log-dir']
EMA = ['--ema-decay', '0.5']
FOUR = ['--iterations', '4', '--snapshot-interval', '1']
U = A.U
_RUNS = {}


def _run(tmp_path_factory, name, argv):
    """(log directory, log entries) of ``train_imagenet.run(argv)``, made once"""
    import train_imagenet as T
    if name not in _RUNS:
        log_dir = str(tmp_path_factory.mktemp(name))
        T.run(T.parse_args(BASE + argv + ['-l', log_dir]), log=lambda *a: None)
        with open(os.path.join(log_dir, 'log')) as f:
            _RUNS[name] = (log_dir, json.load(f))
    return _RUNS[name]


def _npz(path):
    with np.load(path) as h:
        return {k: h[k] for k in h.files}


def _averaged(keys):
    """the keys of a snapshot that are averaged: every float array (BN's N is the live count)"""
    return [k for k in keys if not k.endswith('/N')]


def _recurrence(p0, lives, decay):
    """float64 average after len(lives) updates and the summed per-step bound 3 u omd |live - avg| + u |avg'| + UF"""
    from loans_amd import ema_decay_at
    avg = {k: np.asarray(v, np.float64) for k, v in p0.items()}
    bound = {k: np.zeros(np.shape(v)) for k, v in p0.items()}
    for t, live in enumerate(lives, 1):
        omd = 1.0 - ema_decay_at(decay, t)
        for k in avg:
            step = np.asarray(live[k], np.float64) - avg[k]
            avg[k] = avg[k] + omd * step
            # an error of the average so far is carried on with the factor (1 - omd) <= 1: the steps' bounds add up
            bound[k] = bound[k] + 3 * U * omd * np.abs(step) + U * np.abs(avg[k]) + A.UF
    return avg, bound


# ---- the class -----------------------------------------------------------------------------------------------------------------------
def _classifier(seed=0):
    import train_imagenet as T
    model = T.build_model(T.parse_args(BASE + ['--seed', str(seed)]))
    model.to_gpu(0)
    return model


def test_weight_average_follows_the_recurrence_and_applied_exchanges_in_place():
    import loans_amd
    model = _classifier()
    rng = np.random.RandomState(1)
    p0 = model.state_dict_chainer()
    keys = _averaged(p0)
    average = loans_amd.WeightAverage(model, 0.9)
    assert average.t == 0 and len(average.avg_persistents) == sum(k.endswith(('avg_mean', 'avg_var')) for k in p0)
    lives = []
    for step in range(3):
        # parameters and BN statistics move by known amounts: in place, as the optimiser and the BN kernels move them
        model.arena.data.add_(torch.from_numpy((0.01 * (step + 1) * rng.standard_normal(model.arena.numel)).astype(np.float32)).cuda())
        for _, link, n in model.namedpersistents():
            v = getattr(link, n)
            if torch.is_tensor(v):
                v.add_(0.125 * (step + 1))
        lives.append(model.state_dict_chainer())
        average.update()
    assert average.t == 3
    want, bound = _recurrence({k: p0[k] for k in keys}, lives, 0.9)
    before = model.state_dict_chainer()
    with average.applied():
        inside = model.state_dict_chainer()
        with pytest.raises(RuntimeError):
            average.update()
    after = model.state_dict_chainer()
    worst = 0.0
    for k in keys:
        ratio = float((np.abs(inside[k].astype(np.float64) - want[k]) / bound[k]).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, (k, ratio)
        assert np.abs(inside[k] - before[k]).max() > 0, k          # the average is not the live model
    print('averaged tensors against the float64 recurrence: error / bound %.3f' % worst)
    assert set(after) == set(before)
    for k in before:
        assert np.asarray(after[k]).tobytes() == np.asarray(before[k]).tobytes() and np.shape(after[k]) == np.shape(before[k]), k
        assert np.array_equal(np.asarray(inside[k]), np.asarray(before[k])) == k.endswith('/N'), k

    # the record: per parameter in its logical layout, one key per averaged persistent; written back in place
    sd = average.state_dict()
    assert (sd['class'], sd['t'], sd['hyperparam']) == ('WeightAverage', 3, {'decay': 0.9})
    assert set(sd['state']) == {k + '/avg' for k in keys}
    for k in keys:
        assert np.array_equal(sd['state'][k + '/avg'], inside[k]), k
    other = loans_amd.WeightAverage(model, 0.5)
    pointer = other.avg.data_ptr()
    other.load_state_dict(sd)
    assert (other.t, other.hyperparam.decay, other.avg.data_ptr()) == (3, 0.9, pointer)
    def same(a, b):       # (the arena's padding floats took this test's noise too; a record holds the parameters)
        return set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a)
    assert same(other.state_dict()['state'], sd['state']) and all(torch.equal(a, b) for a, b in zip(other.avg_persistents, average.avg_persistents))
    first = sorted(sd['state'])[0]
    for broken, word in ((dict(sd, state={k: v for k, v in sd['state'].items() if k != first}), first),
                         (dict(sd, state=dict(sd['state'], **{'no/such/avg': np.zeros(1)})), 'no/such/avg'),
                         (dict(sd, state=dict(sd['state'], **{first: np.zeros((1, 2, 3))})), first),
                         (dict(sd, **{'class': 'MomentumSGD'}), 'class')):
        with pytest.raises(ValueError, match=word):
            other.load_state_dict(broken)
    assert same(other.state_dict()['state'], sd['state']) and other.t == 3

    # between steps only, and not in a captured step
    from loans_amd import ops
    ops.begin_step(torch.device('cuda', 0))
    try:
        with pytest.raises(RuntimeError, match='between steps'):
            with average.applied():
                pass
    finally:
        ops.end_step()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    counter = torch.zeros(4, device='cuda')
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=stream):
        counter.add_(1.0)
        with pytest.raises(RuntimeError, match='captured'):
            average.update()
    assert average.t == 3


# ---- the trainer ---------------------------------------------------------------------------------------------------------------------
ARMS = {'f32': [], 'bf16': ['--dtype', 'bf16']}


def _ema_run(factory, arm):
    return _run(factory, 'ema_' + arm, ARMS[arm] + EMA + FOUR + ['--checkpoint-interval', '2'])


def test_the_average_does_not_disturb_training(tmp_path_factory, deterministic_forward):
    with_dir, with_log = _ema_run(tmp_path_factory, 'bf16')
    plain_dir, plain_log = _run(tmp_path_factory, 'plain_bf16', ARMS['bf16'] + FOUR + ['--checkpoint-interval', '2'])
    assert [e['iteration'] for e in with_log] == [e['iteration'] for e in plain_log] == [1, 2, 3, 4]
    for mine, theirs in zip(with_log, plain_log):
        keys = ['loss', 'accuracy', 'lr', 'epoch'] + [k for k in theirs if k.startswith('validation/')]
        assert 'validation/loss' in keys and not any(k.startswith('validation/ema/') for k in theirs)
        for k in keys:
            assert mine[k] == theirs[k], (mine['iteration'], k, mine[k], theirs[k])
        assert {k for k in mine if k.startswith('validation/ema/')} == {'validation/ema/loss', 'validation/ema/accuracy'}
        assert np.isfinite(mine['validation/ema/loss']) and mine['validation/ema/loss'] != mine['validation/loss']
    with open(os.path.join(with_dir, 'SheepLocalizer_4.npz'), 'rb') as a, open(os.path.join(plain_dir, 'SheepLocalizer_4.npz'), 'rb') as b:
        assert a.read() == b.read()
    assert with_log[0]['ema_decay'] == 0.5 and 'ema_decay' not in plain_log[0] and 'lr_schedule' not in plain_log[0]
    names = sorted(n for n in os.listdir(with_dir) if n.startswith('SheepLocalizer'))
    assert names == sorted(['SheepLocalizer_%d.npz' % i for i in range(1, 5)] + ['SheepLocalizer_ema_%d.npz' % i for i in range(1, 5)])
    assert not any('ema' in n for n in os.listdir(plain_dir))


@pytest.mark.parametrize('arm', sorted(ARMS))
def test_the_averaged_snapshot_is_the_average(tmp_path_factory, arm):
    import train_imagenet as T
    log_dir, _ = _ema_run(tmp_path_factory, arm)
    p0 = T.build_model(T.parse_args(BASE)).predictor.state_dict_chainer()           # the same --seed: the model the run started from
    lives = [_npz(os.path.join(log_dir, 'SheepLocalizer_%d.npz' % i)) for i in (1, 2, 3)]
    got = _npz(os.path.join(log_dir, 'SheepLocalizer_ema_3.npz'))
    assert set(got) == set(lives[0]) == set(p0)                                     # the same keys: --rl takes it as it is
    keys = _averaged(got)
    want, bound = _recurrence({k: p0[k] for k in keys}, lives, 0.5)
    worst = 0.0
    for k in keys:
        ratio = float((np.abs(got[k].astype(np.float64) - want[k]) / bound[k]).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, (k, ratio)
    print('SheepLocalizer_ema_3.npz against the recurrence over the live snapshots: error / bound %.3f' % worst)
    assert any(np.abs(got[k] - lives[2][k]).max() > 0 for k in keys if k.endswith('/W'))
    for k in got:
        if k.endswith('/N'):
            assert got[k] == lives[2][k], k


@pytest.mark.parametrize('arm', sorted(ARMS))
def test_the_averaged_snapshot_and_its_logged_metrics_go_together(tmp_path_factory, arm):
    import loans_amd
    import train_imagenet as T
    log_dir, log = _ema_run(tmp_path_factory, arm)
    args = T.parse_args(BASE + ARMS[arm])
    model = T.build_model(args)
    if arm == 'bf16':
        model.set_precision('bf16', 'bf16')
    model.to_gpu(0)
    _, validation = T.build_datasets(args)
    losses = {}
    for tag in ('', 'ema_'):
        loans_amd.load_npz(os.path.join(log_dir, 'SheepLocalizer_%s4.npz' % tag), model.predictor)
        batches = []
        for lo in range(0, len(validation), 2):             # the batches of the run's validation pass
            x, t = T.converter([validation[i] for i in range(lo, lo + 2)], 0)
            with loans_amd.using_config('train', False), loans_amd.using_config('enable_backprop', False):
                model(x, t)
            batches.append(float(model.loss.data))
        losses[tag] = sum(batches) / len(batches)
    last = log[-1]
    print('re-evaluated %r, logged live %.6f ema %.6f' % (losses, last['validation/loss'], last['validation/ema/loss']))
    assert abs(losses['ema_'] - last['validation/ema/loss']) <= 1e-4 * abs(losses['ema_']), (losses, last)
    assert abs(losses[''] - last['validation/loss']) <= 1e-4 * abs(losses['']), (losses, last)
    assert last['validation/ema/loss'] != last['validation/loss'] and losses['ema_'] != losses['']                 # two models


def test_resumed_run_continues_the_average(tmp_path_factory, tmp_path, deterministic_forward, capsys):
    import train_imagenet as T
    straight_dir, straight = _ema_run(tmp_path_factory, 'bf16')
    argv = BASE + ARMS['bf16'] + EMA + ['--snapshot-interval', '1']
    log_dir = str(tmp_path / 'interrupted')
    T.run(T.parse_args(argv + ['--iterations', '2', '--checkpoint-interval', '2', '-l', log_dir]), log=lambda *a: None)
    assert 'checkpoint_2.npz' in os.listdir(log_dir)
    with np.load(os.path.join(log_dir, 'checkpoint_2.npz')) as h:
        assert 'opt/ema' in h.files and 'opt/ema/predictor/feature_extractor/conv1/W/avg' in h.files
        assert json.loads(str(h['opt/ema'][()]))['t'] == 2
    T.run(T.parse_args(argv + ['--iterations', '4', '--resume', log_dir]), log=lambda *a: None)
    with open(os.path.join(log_dir, 'log')) as f:
        resumed = json.load(f)
    assert [e['iteration'] for e in resumed] == [1, 2, 3, 4]
    for mine, theirs in zip(resumed, straight):
        for k in theirs:
            if k in ('loss', 'accuracy', 'lr', 'epoch', 'iteration') or k.startswith('validation/'):
                assert mine[k] == theirs[k], (mine['iteration'], k, mine[k], theirs[k])
    for name in ('SheepLocalizer_ema_4.npz', 'SheepLocalizer_4.npz'):
        with open(os.path.join(log_dir, name), 'rb') as a, open(os.path.join(straight_dir, name), 'rb') as b:
            assert a.read() == b.read(), name

    # a checkpoint without an average into a run with one, and the reverse: a sentence, at the command line
    plain_dir, _ = _run(tmp_path_factory, 'plain_bf16', ARMS['bf16'] + FOUR + ['--checkpoint-interval', '2'])
    capsys.readouterr()
    with pytest.raises(SystemExit):
        T.parse_args(BASE + ARMS['bf16'] + EMA + ['--iterations', '6', '--resume', plain_dir])
    assert 'written without --ema-decay and holds no weight average' in capsys.readouterr().err
    with pytest.raises(SystemExit):
        T.parse_args(BASE + ARMS['bf16'] + ['--iterations', '6', '--resume', straight_dir])
    assert 'written with --ema-decay 0.5 and holds a weight average' in capsys.readouterr().err
    # ... and from run() itself, for a caller that built its arguments otherwise
    args = T.parse_args(BASE + ARMS['bf16'] + ['--iterations', '6'])
    args.resume = plain_dir
    args.ema_decay = 0.5
    with pytest.raises(ValueError, match='holds no weight average'):
        T.run(args, log=lambda *a: None)


def test_no_decay_1d_exempts_scales_shifts_and_biases(tmp_path_factory, deterministic_forward):
    sgd = ARMS['bf16'] + ['--optimizer', 'sgd', '--lr', '0.05', '--iterations', '1', '--no-validation']
    exempt = _npz(os.path.join(_run(tmp_path_factory, 'sgd_exempt', sgd + ['--weight-decay', '0.1', '--no-decay-1d'])[0], 'SheepLocalizer_1.npz'))
    decayed = _npz(os.path.join(_run(tmp_path_factory, 'sgd_decay', sgd + ['--weight-decay', '0.1'])[0], 'SheepLocalizer_1.npz'))
    free = _npz(os.path.join(_run(tmp_path_factory, 'sgd_free', sgd + ['--weight-decay', '0'])[0], 'SheepLocalizer_1.npz'))
    one_d = [k for k in exempt if k.endswith(('/gamma', '/beta', '/b'))]
    weights = [k for k in exempt if k.endswith('/W')]
    assert len(one_d) > 40 and 'feature_extractor/fc/b' in one_d and len(weights) > 20
    assert all(exempt[k].ndim <= 1 for k in one_d) and all(exempt[k].ndim in (2, 4) for k in weights)
    for k in one_d:
        assert np.array_equal(exempt[k], free[k]), k
    for k in weights:
        assert np.array_equal(exempt[k], decayed[k]), k
    # and the decay is there to be exempted from: gamma starts at 1, so a decayed gamma differs
    assert any(not np.array_equal(decayed[k], free[k]) for k in one_d if k.endswith('/gamma'))
    assert any(not np.array_equal(decayed[k], free[k]) for k in weights)
    log = _RUNS['sgd_exempt'][1]
    assert log[0]['no_decay_1d'] is True and 'no_decay_1d' not in _RUNS['sgd_decay'][1][0]


def test_cosine_schedule_is_what_the_log_holds(tmp_path_factory):
    import train_imagenet as T
    argv = ['--optimizer', 'sgd', '--lr', '0.05', '--lr-schedule', 'cosine', '--lr-min', '0.001', '--num-epoch', '2', '--warmup-epochs', '0.5',
            '--no-validation', '--snapshot-interval', '1000']
    _, log = _run(tmp_path_factory, 'cosine', argv)
    assert [e['iteration'] for e in log] == list(range(1, 9))          # 8 examples, batches of 2: four iterations an epoch
    for e in log:
        detail = (e['iteration'] - 1) / 4.0                             # epoch_detail in front of the logged step
        want = T.cosine_lr(0.05, detail, 2, 0.5, 0.001) * T.warmup_factor(detail, 0.5, 0.1)
        assert e['lr'] == pytest.approx(want, rel=1e-12), e
    rates = [e['lr'] for e in log]
    assert rates[0] == pytest.approx(0.005, rel=1e-12) and rates[2] == pytest.approx(0.05, rel=1e-12) and rates[2:] == sorted(rates[2:], reverse=True)
    assert log[0]['lr_schedule'] == 'cosine' and log[0]['lr_min'] == 0.001


# ---- two ranks on one GPU ----------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, outdir):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      LOANS_DIST_BACKEND='gloo')
    import train_imagenet as T
    from loans_amd import parallel
    argv = BASE + EMA + ['--iterations', '2', '--snapshot-interval', '1', '--validation-size', '5', '-l', os.path.join(outdir, 'log_%d' % rank)]
    entries, _ = T.run(T.parse_args(argv), log=lambda *a: None)
    with open(os.path.join(outdir, 'entries_%d.json' % rank), 'w') as f:
        json.dump(entries, f, default=str)
    parallel.shutdown()


def test_two_ranks_log_the_same_averaged_validation(tmp_path):
    out = str(tmp_path)
    mp.spawn(_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    assert not os.path.exists(os.path.join(out, 'log_1'))              # rank 0 alone writes
    names = sorted(os.listdir(os.path.join(out, 'log_0')))
    assert names == ['SheepLocalizer_1.npz', 'SheepLocalizer_2.npz', 'SheepLocalizer_ema_1.npz', 'SheepLocalizer_ema_2.npz', 'log']
    mine, theirs = (json.load(open(os.path.join(out, 'entries_%d.json' % r))) for r in (0, 1))
    assert [e['iteration'] for e in mine] == [e['iteration'] for e in theirs] == [1, 2]
    for a, b in zip(mine, theirs):
        for k in ('validation/ema/loss', 'validation/ema/accuracy', 'validation/loss', 'validation/accuracy'):
            assert a[k] == b[k] and np.isfinite(a[k]), k
        assert a['validation/rows'] == 5
    assert mine[-1]['validation/ema/loss'] != mine[-1]['validation/loss']
