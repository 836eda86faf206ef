"""-m gpu: ``train_imagenet.py --clip-grad-norm``.  ResNet-18 on 64 x 64 frames, batches of 2, the synthetic classes in order, one
loader thread (the ``BASE`` arguments of tests/weight_average/test_gpu_trainer.py).  Comparisons that ask for EQUAL numbers of two
runs are made on the bf16 arm, for the reason given there.  Two ranks on GPU 0 exchange through gloo, as in
tests/imagenet_lamb/test_gpu_trainer.py.  A run is made once per module and shared by the tests that read it."""
import json
import math
import os

import numpy as np
import pytest
import torch.multiprocessing as mp

from tests.grad_clip import cases as A
from tests.imagenet_lars.test_gpu_trainer import _free_port
from tests.weight_average.test_gpu_trainer import ARMS, BASE, FOUR, _npz

pytestmark = pytest.mark.gpu

LR, C = 0.05, 0.1
SGD = ['--optimizer', 'sgd', '--lr', str(LR), '--weight-decay', '0']
CLIP = ['--clip-grad-norm', str(C)]
_RUNS = {}


def _run(tmp_path_factory, name, argv):
    import train_imagenet as T
    if name not in _RUNS:
        log_dir = str(tmp_path_factory.mktemp(name))
        T.run(T.parse_args(BASE + argv + ['-l', log_dir]), log=lambda *a: None)
        with open(os.path.join(log_dir, 'log')) as f:
            _RUNS[name] = (log_dir, json.load(f))
    return _RUNS[name]


def _clip_run(factory, arm):
    return _run(factory, 'clip_' + arm, ARMS[arm] + SGD + CLIP + FOUR + ['--checkpoint-interval', '2'])


def _plain_run(factory):
    return _run(factory, 'plain_bf16', ARMS['bf16'] + SGD + FOUR)


def _same_files(a, b):
    with open(a, 'rb') as f, open(b, 'rb') as g:
        return f.read() == g.read()


@pytest.mark.parametrize('arm', sorted(ARMS))
def test_a_clipped_run_logs_the_norm_and_steps_by_the_threshold(tmp_path_factory, arm, deterministic_forward):
    import train_imagenet as T
    from oracle import model as M
    log_dir, log = _clip_run(tmp_path_factory, arm)
    assert [e['iteration'] for e in log] == [1, 2, 3, 4]
    assert log[0]['clip_grad_norm'] == C and log[0]['optimizer'] == 'sgd'
    for e in log:
        assert math.isfinite(e['grad_norm']) and e['grad_norm'] > C, e      # the threshold lies below the norms: every step clips
        assert math.isfinite(e['loss']) and math.isfinite(e['validation/loss'])
    print('%s: grad_norm %r' % (arm, [e['grad_norm'] for e in log]))
    # the first step starts from v = 0 without decay: p1 - p0 = -lr k g, a vector of length lr c.  Rounding: p1 = fl(p0 + v) is off by
    # u |p1| per element and v by 3 u |v| (tests/imagenet_sgd/reference.py), k by its bound
    p0 = T.build_model(T.parse_args(BASE)).predictor.state_dict_chainer()
    p1 = _npz(os.path.join(log_dir, 'SheepLocalizer_1.npz'))
    keys = [k for k in p0 if M.is_trainable(k)]
    moved = math.sqrt(sum(float(np.sum((p1[k].astype(np.float64) - p0[k].astype(np.float64)) ** 2)) for k in keys))
    size = math.sqrt(sum(float(np.sum(p1[k].astype(np.float64) ** 2)) for k in keys))
    n = sum(p0[k].size for k in keys)
    tol = (A.U32 * size + (3 * A.U32 + A.U32 + A.coefficient_rel_bound(n)) * LR * C) * A.SLACK
    print('%s: first step of length %.9g, lr c = %.9g, tolerance %.3g' % (arm, moved, LR * C, tol))
    assert abs(moved - LR * C) <= tol, (moved, LR * C, tol)
    if arm == 'bf16':
        plain_dir, plain = _plain_run(tmp_path_factory)
        assert not _same_files(os.path.join(log_dir, 'SheepLocalizer_1.npz'), os.path.join(plain_dir, 'SheepLocalizer_1.npz'))
        assert not _same_files(os.path.join(log_dir, 'SheepLocalizer_4.npz'), os.path.join(plain_dir, 'SheepLocalizer_4.npz'))
        assert log[0]['loss'] == plain[0]['loss'] and log[-1]['loss'] != plain[-1]['loss']      # the same start, another trajectory


def test_measure_only_changes_no_byte_and_logs_the_norm(tmp_path_factory, deterministic_forward):
    plain_dir, plain = _plain_run(tmp_path_factory)
    inf_dir, log = _run(tmp_path_factory, 'inf_bf16', ARMS['bf16'] + SGD + ['--clip-grad-norm', 'inf'] + FOUR)
    assert log[0]['clip_grad_norm'] == math.inf and 'clip_grad_norm' not in plain[0]
    for mine, theirs in zip(log, plain):
        assert 'grad_norm' not in theirs and math.isfinite(mine['grad_norm']) and mine['grad_norm'] > 0
        assert set(mine) - set(theirs) == {'grad_norm'} | ({'clip_grad_norm'} if mine['iteration'] == 1 else set())
        for k in theirs:
            if k in ('loss', 'accuracy', 'accuracy_top5', 'lr', 'epoch', 'iteration') or k.startswith('validation/'):
                assert mine[k] == theirs[k], (mine['iteration'], k, mine[k], theirs[k])
    for i in range(1, 5):
        assert _same_files(os.path.join(inf_dir, 'SheepLocalizer_%d.npz' % i), os.path.join(plain_dir, 'SheepLocalizer_%d.npz' % i)), i
    # the clipped run's first norm is this run's: the same first gradient
    assert _clip_run(tmp_path_factory, 'bf16')[1][0]['grad_norm'] == log[0]['grad_norm']


def test_resumed_run_equals_the_uninterrupted_one_and_takes_a_new_threshold(tmp_path_factory, tmp_path, deterministic_forward):
    import train_imagenet as T
    straight_dir, straight = _clip_run(tmp_path_factory, 'bf16')
    argv = BASE + ARMS['bf16'] + SGD + ['--snapshot-interval', '1']
    log_dir = str(tmp_path / 'interrupted')
    T.run(T.parse_args(argv + CLIP + ['--iterations', '2', '--checkpoint-interval', '2', '-l', log_dir]), log=lambda *a: None)
    assert 'checkpoint_2.npz' in os.listdir(log_dir)
    with np.load(os.path.join(log_dir, 'checkpoint_2.npz')) as h:
        assert json.loads(str(h['meta'][()]))['args']['clip_grad_norm'] == C
        assert not [k for k in h.files if 'clip' in k.lower()]              # the hook has no state: nothing of it in the checkpoint
    T.run(T.parse_args(argv + CLIP + ['--iterations', '4', '--resume', log_dir]), log=lambda *a: None)
    with open(os.path.join(log_dir, 'log')) as f:
        resumed = json.load(f)
    assert [e['iteration'] for e in resumed] == [1, 2, 3, 4]
    for mine, theirs in zip(resumed, straight):
        for k in theirs:
            if k in ('loss', 'accuracy', 'accuracy_top5', 'lr', 'epoch', 'iteration', 'grad_norm') or k.startswith('validation/'):
                assert mine[k] == theirs[k], (mine['iteration'], k, mine[k], theirs[k])
    for name in ('SheepLocalizer_3.npz', 'SheepLocalizer_4.npz'):
        assert _same_files(os.path.join(log_dir, name), os.path.join(straight_dir, name)), name
    # another threshold on resume is reported and taken: no clipping from here on, the norm still logged
    lines = []
    T.run(T.parse_args(argv + ['--clip-grad-norm', 'inf', '--iterations', '5', '--resume', log_dir]), log=lambda *a: lines.append(str(a[0])))
    assert [l for l in lines if l.startswith('resume: clip_grad_norm was %r, is now inf' % C)], lines
    with open(os.path.join(log_dir, 'log')) as f:
        last = json.load(f)[-1]
    assert last['iteration'] == 5 and math.isfinite(last['grad_norm']) and last['grad_norm'] > C


def test_the_recipe_line_runs(tmp_path_factory):
    """LAMB, the cosine rate behind a warm-up and the weight average together with the option"""
    argv = ARMS['bf16'] + ['--optimizer', 'lamb', '--lr', '0.01', '--weight-decay', '0.02', '--no-decay-1d', '--lr-schedule', 'cosine',
                           '--warmup-epochs', '0.5', '--num-epoch', '2', '--ema-decay', '0.5', '--clip-grad-norm', '1.0', '--iterations', '2',
                           '--snapshot-interval', '1000']
    _, log = _run(tmp_path_factory, 'recipe', argv)
    assert [e['iteration'] for e in log] == [1, 2] and log[0]['clip_grad_norm'] == 1.0 and log[0]['ema_decay'] == 0.5
    for e in log:
        assert math.isfinite(e['grad_norm']) and e['grad_norm'] > 0 and math.isfinite(e['validation/ema/loss'])


@pytest.mark.parametrize('optimizer', ['sgd', 'adam'])
def test_runs_without_the_option_log_no_new_key(tmp_path_factory, optimizer):
    _, log = _run(tmp_path_factory, optimizer, ARMS['bf16'] + ['--optimizer', optimizer, '--lr', '0.001', '--iterations', '1', '--no-validation'])
    assert log[0]['optimizer'] == optimizer and not [k for e in log for k in e if 'clip' in k or 'grad_norm' in k]


# ---- two ranks on one GPU ----------------------------------------------------------------------------------------------------------
WORLD, B, H, W = 2, 2, 64, 64
THRESHOLD = 0.05
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
    opt = parallel.create_multi_node_optimizer(loans_amd.MomentumSGD(lr=0.05, momentum=0.9).setup(model), comm)
    clip = loans_amd.GradientClipping(THRESHOLD)
    kept = {}

    def keep(o):        # in front of the clipping hook: the arena holds the SUM over the ranks
        arena = o.target.arena
        kept['sum'] = arena.grad[:arena.active_numel].cpu().numpy().copy()
    opt.add_hook(keep, name='keep')
    opt.add_hook(clip)
    records = []
    for step in range(2):
        opt.update(model, G._prepared(net, synthetic.make_frames(70 + 2 * step + rank, B, H, W)), dev(LABELS[step][rank]))
        records.append(np.array([clip.last_norm(), clip.last_coefficient()], np.float32))       # (fp32 values: exact)
    torch.cuda.synchronize()
    assert opt.grad_scale == 1.0 / world and opt.t == 2
    np.savez(os.path.join(outdir, 'after_%d.npz' % rank), **net.state_dict_chainer())
    np.save(os.path.join(outdir, 'records_%d.npy' % rank), np.stack(records))
    if rank == 0:
        np.save(os.path.join(outdir, 'sum.npy'), kept['sum'])
    comm.barrier()
    parallel.shutdown()


def test_two_ranks_record_the_same_norm_of_the_averaged_gradient(tmp_path):
    out = str(tmp_path)
    mp.spawn(_worker, args=(WORLD, _free_port(), out), nprocs=WORLD, join=True)
    after = [dict(np.load(os.path.join(out, 'after_%d.npz' % r))) for r in range(WORLD)]
    for k in after[0]:                                          # replicas stay in sync (BN running statistics are local)
        if 'avg_' not in k and not k.endswith('/N'):
            assert after[0][k].tobytes() == after[1][k].tobytes(), k
    records = [np.load(os.path.join(out, 'records_%d.npy' % r)) for r in range(WORLD)]
    assert records[0].shape == (2, 2) and records[0].tobytes() == records[1].tobytes()         # N and k of both steps, bit for bit
    total = np.load(os.path.join(out, 'sum.npy'))
    n = total.size
    N64 = float(np.sqrt(np.sum(np.square(total.astype(np.longdouble)))) / WORLD)        # the second step's: |sum of the ranks' gradients| / 2
    N, k = (float(x) for x in records[0][1])
    print('two ranks: N %.9g (float64 %.9g), k %.9g' % (N, N64, k))
    assert abs(N - N64) <= A.norm_rel_bound(n) * N64
    assert N64 > THRESHOLD and abs(k - THRESHOLD / N64) <= A.coefficient_rel_bound(n) * THRESHOLD / N64
