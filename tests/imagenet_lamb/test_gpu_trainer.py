"""-m gpu: ``train_imagenet.py --optimizer lamb``.  ResNet-18 on 64 x 64 frames, batches of 2, the synthetic classes in order, one
loader thread (the ``BASE`` arguments of tests/weight_average/test_gpu_trainer.py).  Comparisons that ask for EQUAL numbers of two
runs are made on the bf16 arm, for the reason given there.  Two ranks on GPU 0 exchange through gloo, as in
tests/imagenet_dp/test_gpu_parallel.py.  A run is made once per module and shared by the tests that read it."""
import json
import os

import numpy as np
import pytest
import torch.multiprocessing as mp

from tests.imagenet_lamb import cases as A
from tests.imagenet_lars.test_gpu_trainer import _free_port
from tests.weight_average.test_gpu_trainer import ARMS, BASE, FOUR, _npz

pytestmark = pytest.mark.gpu

LR = 0.01
LAMB = ['--optimizer', 'lamb', '--lr', '0.01', '--weight-decay', '5e-5', '--no-decay-1d']
_RUNS = {}


def _run(tmp_path_factory, name, argv):
    import train_imagenet as T
    if name not in _RUNS:
        log_dir = str(tmp_path_factory.mktemp(name))
        T.run(T.parse_args(BASE + argv + ['-l', log_dir]), log=lambda *a: None)
        with open(os.path.join(log_dir, 'log')) as f:
            _RUNS[name] = (log_dir, json.load(f))
    return _RUNS[name]


def _lamb_run(factory, arm):
    return _run(factory, 'lamb_' + arm, ARMS[arm] + LAMB + FOUR + ['--checkpoint-interval', '2'])


@pytest.mark.parametrize('arm', sorted(ARMS))
def test_lamb_runs_logs_and_writes_snapshots(tmp_path_factory, arm):
    import train_imagenet as T
    log_dir, log = _lamb_run(tmp_path_factory, arm)
    assert [e['iteration'] for e in log] == [1, 2, 3, 4]
    first = log[0]
    assert (first['optimizer'], first['lamb_beta1'], first['lamb_beta2'], first['lamb_eps'], first['no_decay_1d']) == ('lamb', 0.9, 0.999, 1e-6, True)
    assert not [k for k in first if 'lars' in k]
    for e in log:
        assert e['lr'] == LR and np.isfinite(e['loss']) and np.isfinite(e['validation/loss'])
        assert 'accuracy_top5' in e and 'validation/accuracy_top5' in e            # the top-k default of the SGD recipe
    names = sorted(n for n in os.listdir(log_dir) if n.startswith('SheepLocalizer'))
    assert names == ['SheepLocalizer_%d.npz' % i for i in range(1, 5)]
    with np.load(os.path.join(log_dir, 'checkpoint_4.npz')) as h:
        record = json.loads(str(h['opt/main'][()]))
        assert record['class'] == 'LAMB' and record['t'] == 4 and record['hyperparam']['beta2'] == 0.999
        assert 'opt/main/predictor/feature_extractor/conv1/W/m' in h.files and 'opt/main/predictor/feature_extractor/conv1/W/v' in h.files
    snaps = [T.build_model(T.parse_args(BASE)).predictor.state_dict_chainer()] + \
        [_npz(os.path.join(log_dir, 'SheepLocalizer_%d.npz' % i)) for i in range(1, 5)]
    assert set(snaps[4]) == set(snaps[0])
    moved, still = [], []
    for k in snaps[0]:
        assert np.isfinite(snaps[4][k]).all(), k
        if not k.endswith('/W'):
            continue
        steps = []
        for before, after in zip(snaps, snaps[1:]):
            w = before[k].astype(np.float64)
            steps.append(np.sqrt(np.sum((after[k].astype(np.float64) - w) ** 2) / np.sum(w ** 2)))
        if any(steps):
            # inside the stepped prefix a weight tensor adapts: every step moves it by lr |w|, whatever its gradient
            assert np.allclose(steps, LR, rtol=1e-3, atol=0), (k, steps)
            moved.append(k)
        else:
            still.append(k)     # behind the stepped prefix: nothing is touched
    assert len(moved) > 20, (moved, still)
    for k in still:
        assert all(np.array_equal(s[k], snaps[0][k]) for s in snaps), k


def test_resumed_run_equals_the_uninterrupted_one(tmp_path_factory, tmp_path, deterministic_forward, capsys):
    import train_imagenet as T
    straight_dir, straight = _lamb_run(tmp_path_factory, 'bf16')
    argv = BASE + ARMS['bf16'] + LAMB + ['--snapshot-interval', '1']
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
    assert "optimizer: 'lamb' in the checkpoint, 'sgd' now" in capsys.readouterr().err


@pytest.mark.parametrize('optimizer', ['sgd', 'adam'])
def test_the_other_optimisers_log_what_they_logged(tmp_path_factory, optimizer):
    _, log = _run(tmp_path_factory, optimizer, ARMS['bf16'] + ['--optimizer', optimizer, '--lr', '0.001', '--iterations', '1', '--no-validation'])
    assert log[0]['optimizer'] == optimizer and not [k for e in log for k in e if 'lamb' in k]


# ---- two ranks on one GPU ----------------------------------------------------------------------------------------------------------
WORLD, B, H, W = 2, 2, 64, 64
HYPER = dict(lr=A.LR, beta1=0.9, beta2=0.999, eps=1e-6, weight_decay_rate=5e-4, decay_exempt_1d=True)
LABELS = ((np.array([3, 7], np.int32), np.array([0, 9], np.int32)), (np.array([1, 2], np.int32), np.array([8, 4], np.int32)))


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
    opt = parallel.create_multi_node_optimizer(loans_amd.LAMB(**HYPER).setup(model), comm)
    kept = {}

    def keep(o):        # the arena holds the SUM over the ranks; the kernels apply grad_scale.  The moments are the last step's
        torch.cuda.synchronize()
        kept['grads'] = {k[len('/predictor/'):]: p.grad_logical().copy() for k, p in o.target.namedparams()}
        kept['before'] = net.state_dict_chainer()
        kept['state'] = {k[len('predictor/'):]: a for k, a in o.state_dict()['state'].items()}
    opt.add_hook(keep, name='keep')
    for step in range(2):
        opt.update(model, G._prepared(net, synthetic.make_frames(70 + 2 * step + rank, B, H, W)), dev(LABELS[step][rank]))
    torch.cuda.synchronize()
    assert opt.grad_scale == 1.0 / world and opt.t == 2
    np.savez(os.path.join(outdir, 'after_%d.npz' % rank), **net.state_dict_chainer())
    if rank == 0:
        for name in ('grads', 'before', 'state'):
            np.savez(os.path.join(outdir, name + '.npz'), **kept[name])
        with open(os.path.join(outdir, 'ratios.json'), 'w') as f:
            json.dump(dict(ratios=opt.trust_ratios(), sizes={k[len('/predictor/'):]: p.size for k, p in model.namedparams()}), f)
    comm.barrier()
    parallel.shutdown()


def test_two_ranks_stay_in_step_and_adapt_to_the_averaged_gradient(tmp_path):
    from oracle import model as M
    from tests.imagenet_lamb.test_gpu_model import additions_of
    out = str(tmp_path)
    mp.spawn(_worker, args=(WORLD, _free_port(), out), nprocs=WORLD, join=True)
    load = lambda n: dict(np.load(os.path.join(out, n)))       # noqa: E731
    after = [load('after_%d.npz' % r) for r in range(WORLD)]
    for k in after[0]:                                          # replicas stay in sync (BN running statistics are local)
        if 'avg_' not in k and not k.endswith('/N'):
            assert after[0][k].tobytes() == after[1][k].tobytes(), k
    grads, before, state = load('grads.npz'), load('before.npz'), load('state.npz')
    with open(os.path.join(out, 'ratios.json')) as f:
        record = json.load(f)
    keys = [k for k in before if M.is_trainable(k)]
    assert set(record['ratios']) == {'predictor/' + k for k in keys}
    worst, adapting = 0.0, 0
    for k in keys:
        flag = 3 if before[k].ndim <= 1 else 0
        n = before[k].size
        # step 2 from the state step 1 left, on the SUM of the ranks' gradients scaled by 1 / WORLD
        b = A.lamb_bounds(before[k].ravel(), grads[k].ravel(), state[k + '/m'].ravel(), state[k + '/v'].ravel(), [n], [flag], 2, HYPER['lr'],
                          HYPER['weight_decay_rate'], 1.0 / WORLD, T=additions_of(record['sizes'][k]))
        want, got = b['ref']['r'][0], record['ratios']['predictor/' + k]
        if b['rel_r'][0] == 0.0:
            assert got == 1.0 == want, k
            continue
        adapting += 1
        err = abs(got - want) / (b['rel_r'][0] * want)
        worst = max(worst, err)
        assert err <= 1.0, (k, got, want, err)
    assert adapting > 15 and np.abs(after[0]['res5/1/conv2/W'] - before['res5/1/conv2/W']).max() > 0
    print('rank 0 ratios of step 2 against the float64 rule on the averaged gradient: error / bound %.3f' % worst)
