"""-m gpu: ``train_imagenet.py --gpus 2`` stopped after 2 of 4 iterations and resumed.  Two ranks on GPU 0 over gloo, as in
tests/imagenet_dp/test_gpu_parallel.py, each rank a process of its own under its own time limit (tests/resume/dp_worker.py);
one pair of processes makes the straight run, the stopped run and the resumed one.  An epoch is 2 iterations (8 examples, 2
ranks, batches of 2), so the run stops with the prefetch across the epoch boundary.  Every rank draws its crops from a stream of
its own: rank 1's record must be on disk beside rank 0's file and be the one rank 1 reads."""
import os
import socket
import subprocess
import sys

import pytest

from tests.resume import util

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
WORLD = 2
RUN = ['--use-resnet-18', '-b', '2', '--image-size', '64', '64', '--dataset-size', '8', '--validation-size', '4', '--seed', '0',
       '--log-interval', '1', '--flat-log-dir', '--augment', 'rrc', '--augment-seed', '3', '--optimizer', 'sgd', '--lr', '0.05',
       '--lr-drop-epochs', '1', '--warmup-epochs', '1', '--gpus', '2']
# d0: the largest relative difference of `loss` and `validation/loss` over iterations 3..4 between two straight two-rank runs
# of the command on an MI355X (order-preserving kernels), five runs, the largest of the ten pairs (5.3e-4 .. 5.74e-3)
D0 = 5.74e-3
LIMIT = 300         # seconds per rank process


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def launch(out, phases):
    """the WORLD rank processes, each under ``timeout``; returns when all have ended, asserts that all ended well"""
    port = str(_free_port())
    procs = [subprocess.Popen(['timeout', '-k', '10', str(LIMIT), sys.executable, os.path.join(HERE, 'dp_worker.py'),
                               str(rank), str(WORLD), port, out] + list(phases),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for rank in range(WORLD)]
    outputs = [p.communicate()[0] for p in procs]
    report = '\n'.join('--- rank %d ended with %s ---\n%s' % (rank, p.returncode, text[-3000:])
                       for rank, (p, text) in enumerate(zip(procs, outputs)))
    assert all(p.returncode == 0 for p in procs), report


def test_two_ranks_stop_and_resume(tmp_path, capsys):
    """Measured: d0 = 5.74e-3, so the bound is 0.023; the resumed run came out 1.8e-4 from the straight one."""
    import train_imagenet as T
    from loans_amd.runtime import checkpoint
    out = str(tmp_path)
    launch(out, ['straight:S', 'stopped:R', 'resumed:R'])
    want, got = util.read_log(os.path.join(out, 'S')), util.read_log(os.path.join(out, 'R'))
    assert [e['iteration'] for e in got] == [1, 2, 3, 4] and [e['epoch'] for e in got] == [0, 1, 1, 2]
    for key in ('iteration', 'epoch', 'lr', 'validation/rows'):
        assert [e[key] for e in got] == [e[key] for e in want], key
    assert got[0]['gpus'] == 2 and got[-1]['validation/rows'] == 4
    times = [e['elapsed_time'] for e in got]
    assert times == sorted(times)
    tol = util.tolerance(D0)
    spread = util.worst(got[2:], want[2:], ['loss', 'validation/loss'])
    with capsys.disabled():
        print('resumed against straight, two ranks, iterations 3..4: %.3g (allowed %.3g)' % (spread, tol))
    assert spread <= tol, (got, want)
    # the checkpoints: rank 0's common file and rank 1's record, of iteration 2 and of the last iteration of the resumed run
    names = sorted(os.listdir(os.path.join(out, 'R')))
    assert names == ['SheepLocalizer_2.npz', 'SheepLocalizer_4.npz', 'checkpoint_2.npz', 'checkpoint_2.rank1.npz', 'log'], names
    common = checkpoint.common_path(os.path.join(out, 'R'), 2)
    assert checkpoint.read_meta(common)['world_size'] == 2 and checkpoint.is_complete(common)[0]
    mine, theirs = (checkpoint.read_record(common, r)['iterators']['main'] for r in range(WORLD))
    assert mine['pos'] == theirs['pos'] == 0 and mine['epoch'] == theirs['epoch'] == 1
    assert mine['draw'] != theirs['draw']                   # augment_seed + 7919 r: a stream per rank

    # another world size is refused, with the documented message
    capsys.readouterr()
    with pytest.raises(SystemExit):
        T.parse_args(RUN[:-2] + ['--resume', os.path.join(out, 'R')])         # the same command without --gpus 2
    assert checkpoint.world_size_message(2, 1) in capsys.readouterr().err
    assert 'resume it with --gpus 2, not 1' in checkpoint.world_size_message(2, 1)
