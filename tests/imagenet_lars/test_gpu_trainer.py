"""-m gpu: ``train_imagenet.py --optimizer lars``.  ResNet-18 on 64 x 64 frames, batches of 2, the synthetic classes in order, one
loader thread (the ``BASE`` arguments of tests/weight_average/test_gpu_trainer.py).  Comparisons that ask for EQUAL numbers of two
runs are made on the bf16 arm, for the reason given there.  Two ranks on GPU 0 exchange through gloo, as in
tests/imagenet_dp/test_gpu_parallel.py.  A run is made once per module and shared by the tests that read it."""
import json
import os
import socket

import numpy as np
import pytest
import torch.multiprocessing as mp

from tests.imagenet_lars import cases as A
from tests.weight_average.test_gpu_trainer import ARMS, BASE, FOUR, _npz

pytestmark = pytest.mark.gpu

LARS = ['--optimizer', 'lars', '--lr', '0.1', '--lars-eta', '0.2', '--weight-decay', '5e-5', '--no-decay-1d']
_RUNS = {}


def _run(tmp_path_factory, name, argv):
    import train_imagenet as T
    if name not in _RUNS:
        log_dir = str(tmp_path_factory.mktemp(name))
        T.run(T.parse_args(BASE + argv + ['-l', log_dir]), log=lambda *a: None)
        with open(os.path.join(log_dir, 'log')) as f:
            _RUNS[name] = (log_dir, json.load(f))
    return _RUNS[name]


def _lars_run(factory, arm):
    return _run(factory, 'lars_' + arm, ARMS[arm] + LARS + FOUR + ['--checkpoint-interval', '2'])


@pytest.mark.parametrize('arm', sorted(ARMS))
def test_lars_runs_logs_and_writes_snapshots(tmp_path_factory, arm):
    import train_imagenet as T
    log_dir, log = _lars_run(tmp_path_factory, arm)
    assert [e['iteration'] for e in log] == [1, 2, 3, 4]
    first = log[0]
    assert (first['optimizer'], first['lars_eta'], first['lars_eps'], first['no_decay_1d']) == ('lars', 0.2, 1e-8, True)
    for e in log:
        assert e['lr'] == 0.1 and np.isfinite(e['loss']) and np.isfinite(e['validation/loss'])
        assert 'accuracy_top5' in e and 'validation/accuracy_top5' in e            # the top-k default of the SGD recipe
    names = sorted(n for n in os.listdir(log_dir) if n.startswith('SheepLocalizer'))
    assert names == ['SheepLocalizer_%d.npz' % i for i in range(1, 5)]
    p0 = T.build_model(T.parse_args(BASE)).predictor.state_dict_chainer()
    p1, p4 = _npz(os.path.join(log_dir, 'SheepLocalizer_1.npz')), _npz(os.path.join(log_dir, 'SheepLocalizer_4.npz'))
    assert set(p4) == set(p0)
    moved = []
    for k in p0:
        assert np.isfinite(p4[k]).all(), k
        if k.endswith('/W'):
            # one step from v = 0 moves a weight tensor by lr * r * |g'| = lr * eta * |w| |g'| / (|g| + wd |w| + eps) <= lr * eta * |w|, and
            # by nearly that unless its gradient vanishes
            step = np.sqrt(np.sum((p1[k].astype(np.float64) - p0[k]) ** 2) / np.sum(p0[k].astype(np.float64) ** 2))
            assert step <= 0.1 * 0.2 * (1 + 1e-3), (k, step)
            moved.append(step)
    assert len(moved) > 20 and np.median(moved) > 0.5 * 0.1 * 0.2, moved
    with np.load(os.path.join(log_dir, 'checkpoint_4.npz')) as h:
        record = json.loads(str(h['opt/main'][()]))
        assert record['class'] == 'LARS' and record['t'] == 4 and record['hyperparam']['eta'] == 0.2
        assert 'opt/main/predictor/feature_extractor/conv1/W/v' in h.files


def test_resumed_run_equals_the_uninterrupted_one(tmp_path_factory, tmp_path, deterministic_forward, capsys):
    import train_imagenet as T
    straight_dir, straight = _lars_run(tmp_path_factory, 'bf16')
    argv = BASE + ARMS['bf16'] + LARS + ['--snapshot-interval', '1']
    log_dir = str(tmp_path / 'interrupted')
    T.run(T.parse_args(argv + ['--iterations', '2', '--checkpoint-interval', '2', '-l', log_dir]), log=lambda *a: None)
    assert 'checkpoint_2.npz' in os.listdir(log_dir)
    T.run(T.parse_args(argv + ['--iterations', '4', '--resume', log_dir]), log=lambda *a: None)
    with open(os.path.join(log_dir, 'log')) as f:
        resumed = json.load(f)
    assert [e['iteration'] for e in resumed] == [1, 2, 3, 4]
    for mine, theirs in zip(resumed, straight):
        for k in theirs:
            if k in ('loss', 'accuracy', 'accuracy_top5', 'lr', 'epoch', 'iteration') or k.startswith('validation/'):
                assert mine[k] == theirs[k], (mine['iteration'], k, mine[k], theirs[k])
    for name in ('SheepLocalizer_3.npz', 'SheepLocalizer_4.npz'):
        with open(os.path.join(log_dir, name), 'rb') as a, open(os.path.join(straight_dir, name), 'rb') as b:
            assert a.read() == b.read(), name
    # the optimiser stays fixed on resume
    capsys.readouterr()
    with pytest.raises(SystemExit):
        T.parse_args(BASE + ARMS['bf16'] + ['--optimizer', 'sgd', '--lr', '0.1', '--iterations', '6', '--resume', log_dir])
    assert "optimizer: 'lars' in the checkpoint, 'sgd' now" in capsys.readouterr().err


def test_the_sgd_log_is_what_it_was(tmp_path_factory):
    _, log = _run(tmp_path_factory, 'sgd', ARMS['bf16'] + ['--optimizer', 'sgd', '--lr', '0.05', '--iterations', '1', '--no-validation'])
    assert log[0]['optimizer'] == 'sgd' and not [k for e in log for k in e if 'lars' in k]


# ---- two ranks on one GPU ----------------------------------------------------------------------------------------------------------
WORLD, B, H, W = 2, 2, 64, 64
HYPER = dict(lr=0.1, momentum=0.9, weight_decay_rate=5e-4, eta=0.2, eps=1e-8, decay_exempt_1d=True)
LABELS = ((np.array([3, 7], np.int32), np.array([0, 9], np.int32)), (np.array([1, 2], np.int32), np.array([8, 4], np.int32)))


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, outdir):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      LOANS_DIST_BACKEND='gloo')
    import torch
    import loans_amd
    from loans_amd import parallel
    from loans_amd.datasets import synthetic
    from tests.gpu_util import dev
    from tests.imagenet import test_gpu_model as G
    from tests.imagenet_sgd.test_gpu_model import _classifier
    comm = parallel.init_from_env()
    assert comm.active and comm.size == world
    model, net = _classifier(60 + rank)             # different weights per rank, rank 0's broadcast
    model.to_gpu(0)
    comm.bcast_data(model)
    opt = parallel.create_multi_node_optimizer(loans_amd.LARS(**HYPER).setup(model), comm)
    kept = {}

    def keep(o):        # the arena holds the SUM over the ranks; the kernels apply grad_scale
        torch.cuda.synchronize()
        kept['grads'] = {k[len('/predictor/'):]: p.grad_logical().copy() for k, p in o.target.namedparams()}
        kept['before'] = net.state_dict_chainer()
    opt.add_hook(keep, name='keep')
    for step in range(2):
        opt.update(model, G._prepared(net, synthetic.make_frames(70 + 2 * step + rank, B, H, W)), dev(LABELS[step][rank]))
    torch.cuda.synchronize()
    assert opt.grad_scale == 1.0 / world and opt.t == 2
    np.savez(os.path.join(outdir, 'after_%d.npz' % rank), **net.state_dict_chainer())
    if rank == 0:
        np.savez(os.path.join(outdir, 'grads.npz'), **kept['grads'])
        np.savez(os.path.join(outdir, 'before.npz'), **kept['before'])
        with open(os.path.join(outdir, 'ratios.json'), 'w') as f:
            json.dump(dict(ratios=opt.trust_ratios(), sizes={k[len('/predictor/'):]: p.size for k, p in model.namedparams()}), f)
    comm.barrier()
    parallel.shutdown()


def test_two_ranks_stay_in_step_and_adapt_to_the_averaged_gradient(tmp_path):
    from oracle import model as M
    out = str(tmp_path)
    mp.spawn(_worker, args=(WORLD, _free_port(), out), nprocs=WORLD, join=True)
    load = lambda n: dict(np.load(os.path.join(out, n)))       # noqa: E731
    after = [load('after_%d.npz' % r) for r in range(WORLD)]
    for k in after[0]:                                          # replicas stay in sync (BN running statistics are local)
        if 'avg_' not in k and not k.endswith('/N'):
            assert after[0][k].tobytes() == after[1][k].tobytes(), k
    grads, before = load('grads.npz'), load('before.npz')
    with open(os.path.join(out, 'ratios.json')) as f:
        record = json.load(f)
    keys = [k for k in before if M.is_trainable(k)]
    assert set(record['ratios']) == {'predictor/' + k for k in keys}
    worst, adapting = 0.0, 0
    for k in keys:
        flag = 3 if before[k].ndim <= 1 else 0
        Wn = float(np.sqrt(np.sum(before[k].astype(np.float64) ** 2)))
        Gn = float(np.sqrt(np.sum(grads[k].astype(np.float64) ** 2))) / WORLD          # the averaged gradient's norm
        want = A.ratio_of(Wn, Gn, flag, HYPER['weight_decay_rate'], HYPER['eta'], HYPER['eps'])
        got = record['ratios']['predictor/' + k]
        if want == 1.0:
            assert got == 1.0, k
            continue
        adapting += 1
        T = 16 + 6 + 3 + -(-((record['sizes'][k] + 7) // 8 * 8) // A.UNIT)
        err = abs(got - want) / ((A.U32 + A.C * T * A.U64) * A.SLACK * want)
        worst = max(worst, err)
        assert err <= 1.0, (k, got, want, err)
    assert adapting > 15 and np.abs(after[0]['res5/1/conv2/W'] - before['res5/1/conv2/W']).max() > 0
    print('rank 0 ratios of step 2 against the float64 rule on the averaged gradient: error / bound %.3f' % worst)
