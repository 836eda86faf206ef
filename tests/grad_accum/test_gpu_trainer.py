"""-m gpu: ``train_imagenet.py --accum-steps K``.  ResNet-18 on 64 x 64 frames, batches of 2, the synthetic classes in order, one loader
thread (the ``BASE`` / ``ARMS`` / ``FOUR`` arguments of tests/weight_average/test_gpu_trainer.py).  Comparisons that ask for EQUAL
numbers of two runs are made on the bf16 arm, for the reason given there.  Two ranks on GPU 0 exchange through gloo, as in
tests/grad_clip/test_gpu_trainer.py.  A run is made once per module and shared by the tests that read it."""
import json
import math
import os

import numpy as np
import pytest
import torch.multiprocessing as mp

from tests.grad_accum import cases as A
from tests.imagenet_lars.test_gpu_trainer import _free_port
from tests.weight_average.test_gpu_trainer import ARMS, BASE, FOUR, _npz

pytestmark = pytest.mark.gpu

ACCUM = ['--accum-steps', '2']
_RUNS = {}


def _run(tmp_path_factory, name, argv):
    import train_imagenet as T
    if name not in _RUNS:
        log_dir = str(tmp_path_factory.mktemp(name))
        T.run(T.parse_args(BASE + argv + ['-l', log_dir]), log=lambda *a: None)
        with open(os.path.join(log_dir, 'log')) as f:
            _RUNS[name] = (log_dir, json.load(f))
    return _RUNS[name]


def _accum_run(factory, arm):
    return _run(factory, 'accum_' + arm, ARMS[arm] + ACCUM + FOUR + ['--checkpoint-interval', '2'])


def _plain_run(factory, arm):
    return _run(factory, 'plain_' + arm, ARMS[arm] + FOUR)


def _same_files(a, b):
    with open(a, 'rb') as f, open(b, 'rb') as g:
        return f.read() == g.read()


@pytest.mark.parametrize('arm', sorted(ARMS))
def test_an_accumulated_run_counts_optimiser_steps_and_consumes_twice_the_batches(tmp_path_factory, arm, deterministic_forward):
    log_dir, log = _accum_run(tmp_path_factory, arm)
    plain_dir, plain = _plain_run(tmp_path_factory, arm)
    assert [e['iteration'] for e in log] == [1, 2, 3, 4] and log[0]['accum_steps'] == 2
    # 8 examples in batches of 2: four batches an epoch, two of them per iteration
    assert [e['epoch'] for e in log] == [epoch for epoch, _ in A.updater_schedule(8, 2, 2, 4)] == [0, 1, 1, 2]
    assert [e['epoch'] for e in plain] == [0, 0, 0, 1]
    for e in log:
        assert math.isfinite(e['loss']) and math.isfinite(e['validation/loss']) and 0.0 <= e['accuracy'] <= 1.0, e
    names = sorted(n for n in os.listdir(log_dir) if n.startswith('SheepLocalizer'))
    assert names == ['SheepLocalizer_%d.npz' % i for i in range(1, 5)]
    assert not _same_files(os.path.join(log_dir, 'SheepLocalizer_1.npz'), os.path.join(plain_dir, 'SheepLocalizer_1.npz'))
    mine, theirs = _npz(os.path.join(log_dir, 'SheepLocalizer_4.npz')), _npz(os.path.join(plain_dir, 'SheepLocalizer_4.npz'))
    assert set(mine) == set(theirs) and any(not np.array_equal(mine[k], theirs[k]) for k in mine if k.endswith('/W'))
    assert all(np.isfinite(v).all() for v in mine.values())


def test_accum_steps_one_is_the_run_without_the_option(tmp_path_factory, deterministic_forward):
    plain_dir, plain = _plain_run(tmp_path_factory, 'bf16')
    one_dir, one = _run(tmp_path_factory, 'one_bf16', ARMS['bf16'] + ['--accum-steps', '1'] + FOUR)
    for i in range(1, 5):
        assert _same_files(os.path.join(one_dir, 'SheepLocalizer_%d.npz' % i), os.path.join(plain_dir, 'SheepLocalizer_%d.npz' % i)), i
    assert not [k for e in plain for k in e if 'accum' in k]                # the plain run's log gains no key
    assert one[0]['accum_steps'] == 1 and set(one[0]) - set(plain[0]) == {'accum_steps'}
    for mine, theirs in zip(one, plain):
        for k in theirs:
            if k in ('loss', 'accuracy', 'lr', 'epoch', 'iteration') or k.startswith('validation/'):
                assert mine[k] == theirs[k], (mine['iteration'], k, mine[k], theirs[k])


def test_a_boundary_on_the_first_of_two_micro_batches_is_logged_and_validated(tmp_path_factory):
    """6 examples in batches of 2: three batches an epoch.  Iteration 2 draws batches 3 and 4 -- the boundary falls on its first
    micro-batch, the iterator says "no new epoch" behind its second --, iteration 3 ends on one.  Nothing else triggers an entry
    but the run's last iteration."""
    argv = ARMS['bf16'] + ACCUM + ['--dataset-size', '6', '--iterations', '4', '--log-interval', '1000', '--snapshot-interval', '1000']
    _, log = _run(tmp_path_factory, 'boundary', argv)
    schedule = A.updater_schedule(6, 2, 2, 4)
    assert schedule == [(0, False), (1, True), (2, True), (2, False)]
    assert [e['iteration'] for e in log] == [2, 3, 4]
    assert [e['epoch'] for e in log] == [1, 2, 2]
    assert all(math.isfinite(e['validation/loss']) and math.isfinite(e['loss']) for e in log)


def test_resumed_run_equals_the_uninterrupted_one_and_another_K_is_refused(tmp_path_factory, tmp_path, deterministic_forward, capsys):
    import train_imagenet as T
    straight_dir, straight = _accum_run(tmp_path_factory, 'bf16')
    argv = BASE + ARMS['bf16'] + ['--snapshot-interval', '1']
    log_dir = str(tmp_path / 'interrupted')
    T.run(T.parse_args(argv + ACCUM + ['--iterations', '2', '--checkpoint-interval', '2', '-l', log_dir]), log=lambda *a: None)
    assert 'checkpoint_2.npz' in os.listdir(log_dir)
    with np.load(os.path.join(log_dir, 'checkpoint_2.npz')) as h:
        assert json.loads(str(h['meta'][()]))['args']['accum_steps'] == 2
        assert not [k for k in h.files if 'accum' in k.lower()]            # a checkpoint lies between steps: nothing of the accumulator
    T.run(T.parse_args(argv + ACCUM + ['--iterations', '4', '--resume', log_dir]), log=lambda *a: None)
    with open(os.path.join(log_dir, 'log')) as f:
        resumed = json.load(f)
    assert [e['iteration'] for e in resumed] == [1, 2, 3, 4]
    for mine, theirs in zip(resumed, straight):
        for k in theirs:
            if k in ('loss', 'accuracy', 'lr', 'epoch', 'iteration') or k.startswith('validation/'):
                assert mine[k] == theirs[k], (mine['iteration'], k, mine[k], theirs[k])
    for name in ('SheepLocalizer_3.npz', 'SheepLocalizer_4.npz'):
        assert _same_files(os.path.join(log_dir, name), os.path.join(straight_dir, name)), name
    # another K, or none, on resume: refused in the one message that lists the fixed arguments
    capsys.readouterr()
    for other, now in ((['--accum-steps', '4'], 4), ([], 1)):
        with pytest.raises(SystemExit):
            T.parse_args(argv + other + ['--iterations', '6', '--resume', log_dir])
        err = capsys.readouterr().err
        assert 'these arguments must equal the checkpointed run\'s' in err and 'accum_steps: 2 in the checkpoint, %d now' % now in err


def test_the_recipe_line_runs(tmp_path_factory):
    """LAMB, the cosine rate behind a warm-up, the weight average, clipping, stochastic depth and mixup together with the option"""
    argv = ARMS['bf16'] + ACCUM + ['--optimizer', 'lamb', '--lr', '0.01', '--weight-decay', '0.02', '--no-decay-1d', '--lr-schedule', 'cosine',
                                   '--warmup-epochs', '0.5', '--num-epoch', '2', '--ema-decay', '0.5', '--clip-grad-norm', '1.0',
                                   '--drop-path', '0.1', '--drop-path-seed', '3', '--augment', 'rrc', '--augment-seed', '1',
                                   '--mixup-alpha', '0.2', '--mix-seed', '2', '--iterations', '2', '--snapshot-interval', '1000']
    _, log = _run(tmp_path_factory, 'recipe', argv)
    assert [e['iteration'] for e in log] == [1, 2] and log[0]['accum_steps'] == 2 and log[0]['clip_grad_norm'] == 1.0
    assert [e['epoch'] for e in log] == [0, 1]                  # four batches an epoch, two per iteration
    for e in log:
        assert math.isfinite(e['grad_norm']) and e['grad_norm'] > 0 and math.isfinite(e['validation/ema/loss']) and math.isfinite(e['loss'])


# ---- two ranks on one GPU ----------------------------------------------------------------------------------------------------------
WORLD, B, H, W = 2, 2, 64, 64
LABELS = (np.array([3, 7], np.int32), np.array([0, 9], np.int32), np.array([1, 2], np.int32), np.array([8, 4], np.int32))


def _worker(rank, world, port, outdir):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      LOANS_DIST_BACKEND='gloo')
    import torch
    import loans_amd
    from loans_amd import ops, parallel
    from loans_amd.datasets import synthetic
    from tests.gpu_util import dev
    from tests.grad_accum import test_gpu_model as M
    from tests.imagenet import test_gpu_model as G
    from tests.imagenet_sgd.test_gpu_model import _classifier
    ops.SPLITK = False                              # the order-preserving kernels: the twin below repeats the gradients bit for bit
    comm = parallel.init_from_env()
    assert comm.active and comm.size == world
    model, net = _classifier(60 + rank)             # different weights per rank, rank 0's broadcast
    model.set_precision('bf16', 'bf16')
    model.to_gpu(0)
    comm.bcast_data(model)
    opt = parallel.create_multi_node_optimizer(loans_amd.MomentumSGD(lr=0.05, momentum=0.9).setup(model), comm)
    twin, twin_net = _classifier(60)                # rank 0's weights: what every rank holds after the broadcast
    twin.set_precision('bf16', 'bf16')
    twin.to_gpu(0)
    assert torch.equal(twin.arena.data, model.arena.data)
    calls = {'grad': 0, 'range': 0}
    grad, span = comm.allreduce_grad, comm.allreduce_range

    def counted_grad(*a, **kw):
        calls['grad'] += 1
        return grad(*a, **kw)

    def counted_range(*a, **kw):
        calls['range'] += 1
        return span(*a, **kw)
    comm.allreduce_grad, comm.allreduce_range = counted_grad, counted_range
    kept = []

    def keep(o):        # in front of the step: the arena holds the SUM over the ranks of the ranks' accumulated sums
        arena = o.target.arena
        kept.append(arena.grad[:arena.active_numel].cpu().numpy().copy())
    opt.add_hook(keep, name='keep')

    def batch(n, i):        # micro-batch i of this rank; inside a step workspace, as the updater runs it (M._step)
        return G._prepared(n, synthetic.make_frames(70 + 2 * i + rank, B, H, W)), dev(LABELS[(i + rank) % 4])

    local = None
    per_step = []
    for step in range(2):
        if step == 0:       # this rank's own ((g1 + g2)), by hand on the twin
            parts = [M._by_hand(twin, twin_net, micro, batch) for micro in range(2)]
            local = torch.add(parts[0], parts[1]).cpu().numpy()
        before = dict(calls)
        M._accumulate(opt, model, net, 2 * step, batch)
        assert calls == before and opt.t == step     # nothing is exchanged by a micro-batch that does not close the step
        M._update(opt, model, net, 2 * step + 1, batch)
        per_step.append((calls['grad'] - before['grad'], calls['range'] - before['range']))
        assert opt.grad_scale == 1.0 / (2 * world) and opt.t == step + 1 and not opt._pending and opt._exchanged_from is None
    torch.cuda.synchronize()
    assert per_step == [(1, 1), (1, 1)], per_step       # exactly one all-reduce per step: the whole prefix, behind the close
    assert len(kept) == 2
    np.savez(os.path.join(outdir, 'after_%d.npz' % rank), **net.state_dict_chainer())
    np.save(os.path.join(outdir, 'seen_%d.npy' % rank), kept[0])
    np.save(os.path.join(outdir, 'local_%d.npy' % rank), local)
    comm.barrier()
    parallel.shutdown()


def test_two_ranks_exchange_one_accumulated_sum_per_step(tmp_path):
    out = str(tmp_path)
    mp.spawn(_worker, args=(WORLD, _free_port(), out), nprocs=WORLD, join=True)
    after = [dict(np.load(os.path.join(out, 'after_%d.npz' % r))) for r in range(WORLD)]
    moved = 0
    for k in after[0]:                                          # replicas stay in sync (BN running statistics are local)
        if 'avg_' not in k and not k.endswith('/N'):
            assert after[0][k].tobytes() == after[1][k].tobytes(), k
            moved += 1
    assert moved > 40
    seen = [np.load(os.path.join(out, 'seen_%d.npy' % r)) for r in range(WORLD)]
    local = [np.load(os.path.join(out, 'local_%d.npy' % r)) for r in range(WORLD)]
    assert seen[0].tobytes() == seen[1].tobytes()               # both ranks step on the same exchanged gradient
    assert local[0].tobytes() != local[1].tobytes() and np.isfinite(seen[0]).all()
    # ... which is the sum over the ranks of each rank's own (g1 + g2): one fp32 addition of two operands, the same in either order
    assert A.same_bits(seen[0], (local[0] + local[1]).astype(np.float32))
