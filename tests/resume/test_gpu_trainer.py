"""-m gpu: ``--checkpoint-interval`` / ``--resume`` of both trainers.

``train_imagenet.py``: a run stopped after 3 of 7 iterations and continued from
its checkpoint by a second ``run()`` with a fresh model is held against the straight 7-iteration run: the bookkeeping exactly
(iterations, epochs, rates, file names), the losses to the run-to-run spread of the straight run itself (tests/resume/util.py).
An epoch is 4 iterations, so stopping at 3 leaves the prefetch across the epoch boundary: it has already reshuffled and has
drawn crops for batches the stopped run never consumed.

``train_sheep_localizer.py``: the joint LoANs run -- two models, two AMSGrad optimisers, two iterators, ``rotation_dropout``
drawing from NumPy's global stream on every forward -- stopped after 3 of 6 iterations and continued by a second ``run()`` with
fresh models, against the straight 6-iteration run.  The configuration is the one of tests/test_gpu_trainer.py's 10-iteration
run in its smooth regime (batch 8 at 224 x 224, lr 1e-5)."""
import json
import os
import shutil

import numpy as np
import pytest

from tests.resume import util

pytestmark = pytest.mark.gpu

BASE = ['--use-resnet-18', '-b', '2', '--image-size', '64', '64', '--dataset-size', '8', '--validation-size', '4', '--seed', '0',
        '--log-interval', '1', '--flat-log-dir']
SGD = BASE + ['--augment', 'rrc', '--augment-seed', '3', '--optimizer', 'sgd', '--lr', '0.05', '--lr-drop-epochs', '1',
              '--warmup-epochs', '1']
BF16 = BASE + ['--augment', 'none', '--optimizer', 'adam', '--dtype', 'bf16']
# d0: the largest relative difference of the per-iteration `loss` (iterations 4..7) between two straight runs of the command,
# measured on an MI355X with the order-preserving kernels (fixture deterministic_forward), five runs of each command, the
# largest of the ten pairs.
#   sgd:  0.0687 (the pairs: 0.0042 .. 0.0687, median 0.029).  The fp32 weight gradients close with atomics; the runs part in
#         the 7th digit at iteration 2 and at lr 0.05 on batches of 2 that is two digits by iteration 5.  A wrong batch moves the
#         loss of iteration 4 by 0.8 (the negative control below).
#   bf16: 0 -- the five runs are bit-identical: the bf16 arm's kernels keep their order at these shapes
D0 = {'sgd': 0.0687, 'bf16': 0.0}


def run(argv, log_dir, *more):
    import train_imagenet as T
    lines = []
    entries, _ = T.run(T.parse_args(argv + list(more) + ['-l', log_dir]), log=lines.append)
    return entries, lines


def straight(argv, log_dir):
    run(argv, log_dir, '--iterations', '7')
    return util.read_log(log_dir)


def stopped_and_resumed(argv, log_dir):
    """(the log after 3 iterations, the log after the resumed run, what the resumed run printed)"""
    import train_imagenet as T
    run(argv, log_dir, '--iterations', '3', '--checkpoint-interval', '3')
    first = util.read_log(log_dir)
    assert sorted(n for n in os.listdir(log_dir) if n.startswith('checkpoint')) == ['checkpoint_3.npz']
    lines = []
    T.run(T.parse_args(argv + ['--resume', log_dir, '--iterations', '7']), log=lines.append)
    return first, util.read_log(log_dir), lines


def check_bookkeeping(first, resumed, want, log_dir, straight_dir):
    assert [e['iteration'] for e in resumed] == list(range(1, 8))
    for key in ('iteration', 'epoch', 'lr'):
        assert [e[key] for e in resumed] == [e[key] for e in want], key
    assert [e['epoch'] for e in resumed] == [0, 0, 0, 1, 1, 1, 1]
    assert resumed[:3] == first and 'batch_size' in resumed[0] and 'batch_size' not in resumed[3]
    times = [e['elapsed_time'] for e in resumed]
    assert times == sorted(times) and times[3] > times[2]
    assert 'SheepLocalizer_7.npz' in os.listdir(log_dir) and 'SheepLocalizer_7.npz' in os.listdir(straight_dir)
    assert not any(os.path.isdir(os.path.join(log_dir, n)) for n in os.listdir(log_dir))       # no new <time>_<name>


def test_sgd_rrc_run_continues(tmp_path, deterministic_forward):
    """Measured: d0 = 0.0687, so the bound is 0.275; the resumed run came out 0.021 from the straight one -- like a second
    straight run -- and the run resumed one batch behind 0.825."""
    import train_imagenet as T
    from loans_amd.common.datasets.shard import ShardedDataset
    from loans_amd.runtime import checkpoint, training
    import torch
    s_dir, r_dir, n_dir = (str(tmp_path / n) for n in 'SRN')
    want = straight(SGD, s_dir)
    first, resumed, lines = stopped_and_resumed(SGD, r_dir)
    check_bookkeeping(first, resumed, want, r_dir, s_dir)
    assert any('iterations was 3, is now 7' in l for l in lines) and any('checkpoint_interval was 3, is now 0' in l for l in lines)
    assert sum('iterations was' in l for l in lines) == 1 and not any('batch_size' in l for l in lines)
    tol = util.tolerance(D0['sgd'])
    spread = util.worst(resumed[3:], want[3:], ['loss'])
    print('resumed against straight, loss of iterations 4..7: %.3g (allowed %.3g)' % (spread, tol))
    assert spread <= tol, ([e['loss'] for e in resumed], [e['loss'] for e in want])

    # negative control: the same checkpoint with the training iterator's state of one batch earlier -- the data sequence is
    # wrong by one batch and the test must see it
    args = T.parse_args(SGD)
    train, _ = T.build_crop_datasets(args, torch.device('cuda', 0), 0)
    it = training.MultithreadIterator(ShardedDataset(train, 0, 1, pad=True), 2, shuffle=True, n_threads=args.loader_threads, device=0)
    for _ in range(2):
        next(it)
    earlier = it.state_dict()
    it.finalize()
    os.makedirs(n_dir)
    shutil.copy(os.path.join(r_dir, 'log'), n_dir)
    source = checkpoint.common_path(r_dir, 3)
    record = checkpoint.read_record(source)
    assert record['iterators']['main']['pos'] == 6 and earlier['pos'] == 4
    record['iterators']['main'] = earlier
    with np.load(source) as handle:
        arrays = {k: handle[k] for k in handle.files if k != 'rank' and not k.startswith('rank/')}
    arrays['rank'] = np.array(json.dumps(checkpoint.pack(record, 'rank', arrays)))
    checkpoint.write_atomic(checkpoint.common_path(n_dir, 3), arrays)
    T.run(T.parse_args(SGD + ['--resume', n_dir, '--iterations', '4']), log=lambda line: None)
    wrong = util.read_log(n_dir)
    assert [e['iteration'] for e in wrong] == [1, 2, 3, 4]
    off = util.rel(wrong[3]['loss'], want[3]['loss'])
    print('one batch behind, loss of iteration 4: off by %.3g' % off)
    assert off > tol, (wrong[3]['loss'], want[3]['loss'])


def test_adam_bf16_run_continues(tmp_path, deterministic_forward):
    """Measured: d0 = 0, so the floor of 1e-6 is the bound; the resumed run came out bit-identical to the straight one."""
    s_dir, r_dir = (str(tmp_path / n) for n in 'SR')
    want = straight(BF16, s_dir)
    first, resumed, _ = stopped_and_resumed(BF16, r_dir)
    check_bookkeeping(first, resumed, want, r_dir, s_dir)
    tol = util.tolerance(D0['bf16'])
    spread = util.worst(resumed[3:], want[3:], ['loss'])
    print('resumed against straight, loss of iterations 4..7: %.3g (allowed %.3g)' % (spread, tol))
    assert spread <= tol, ([e['loss'] for e in resumed], [e['loss'] for e in want])


# ---- the LoANs trainer ------------------------------------------------------------------------------------------------------------
# d0 between two straight runs of the command on an MI355X (order-preserving kernels, fixture deterministic_forward), five runs,
# the largest of the ten pairs: of loss_localizer / loss_dis / theta over iterations 4..6 (the pairs fall into two groups,
# 1.2e-6 .. 3.6e-6 and 1.47e-4: a rounding decides a pooling maximum or a ReLU one way or the other), and of the snapshots of
# iteration 6 (util.snapshot_spread; 4.0e-7 .. 2.26e-5)
LOANS_D0 = {'history': 1.474e-4, 'snapshots': 2.263e-5}
LOANS_KEYS = ('loss_localizer', 'loss_dis', 'theta')


def loans_argv():
    from tests.golden import make_golden as G
    return list(G.CONFIG1_SOFT_ARGV)


def loans_run(log_dir, *more):
    """(history, NumPy's global stream after the run)"""
    import train_sheep_localizer as T
    history, _, _ = T.run(T.parse_args(loans_argv() + list(more) + (['-l', log_dir] if log_dir else [])), log=lambda line: None)
    return history, np.random.get_state()


def snapshots(log_dir, iteration):
    return [os.path.join(log_dir, '%s_%d.npz' % (name, iteration)) for name in ('SheepLocalizer', 'ResnetAssessor')]


def test_joint_run_continues(tmp_path, deterministic_forward):
    """Measured: d0 = 1.474e-4 (history) and 2.263e-5 (snapshots), so the bounds are 5.9e-4 and 9.1e-5; the resumed run came out
    2.5e-7 and 7.1e-7 from the straight one."""
    s_dir, r_dir = (str(tmp_path / n) for n in 'SR')
    want, want_stream = loans_run(s_dir, '--iterations', '6')
    assert [h['iteration'] for h in want] == [1, 2, 3, 4, 5, 6]
    loans_run(r_dir, '--iterations', '3', '--checkpoint-interval', '3')
    assert 'checkpoint_3.npz' in os.listdir(r_dir)
    got, got_stream = loans_run(None, '--iterations', '6', '--resume', r_dir)
    assert [h['iteration'] for h in got] == [4, 5, 6] and [h['epoch'] for h in got] == [h['epoch'] for h in want[3:]]

    spread = util.worst(got, want[3:], LOANS_KEYS)
    print('resumed against straight, losses and theta of iterations 4..6: %.3g (allowed %.3g)' % (spread, util.tolerance(LOANS_D0['history'])))
    assert spread <= util.tolerance(LOANS_D0['history']), (got, want[3:])
    moved = [util.snapshot_spread(a, b) for a, b in zip(snapshots(r_dir, 6), snapshots(s_dir, 6))]
    print('snapshots of iteration 6 (localizer, assessor): %.3g %.3g (allowed %.3g)' % (moved[0], moved[1], util.tolerance(LOANS_D0['snapshots'])))
    assert max(moved) <= util.tolerance(LOANS_D0['snapshots'])

    # --resume freezes nothing: the assessor went on training after the checkpoint
    with np.load(snapshots(r_dir, 6)[1]) as late, np.load(snapshots(r_dir, 3)[1]) as early:
        assert any(not np.array_equal(late[k], early[k]) for k in late.files if k.endswith('/W'))

    # NumPy's global stream: rotation_dropout's draws of iterations 4..6 came out of the restored stream
    assert want_stream[0] == got_stream[0] and np.array_equal(want_stream[1], got_stream[1]) and want_stream[2:] == got_stream[2:]
    log = util.read_log(r_dir)
    times = [e['elapsed_time'] for e in log]
    assert [e['iteration'] for e in log] == [1, 2, 3, 4, 5, 6] and times == sorted(times)      # an epoch is one iteration: an entry each
