"""-m gpu: ``train_imagenet.run`` with ``--drop-path 0.3 --drop-path-seed 3`` on the run of tests/imagenet_mix/test_gpu_trainer.py
(its sizes and its four iterations): the log and the argument record, two runs of one command, continuation from a checkpoint
and the refusal of a resume that changes the rate.  The runs are made with --dtype bf16 on the order-preserving kernels, for the
reason given there."""
import os

import numpy as np
import pytest

from tests.imagenet_mix.test_gpu_trainer import BITS, RUN
from tests.resume import util

pytestmark = pytest.mark.gpu

DROP = ['--drop-path', '0.3', '--drop-path-seed', '3']
ARGV = RUN + DROP + BITS
KEYS = ('iteration', 'epoch', 'lr', 'loss', 'accuracy', 'validation/loss', 'validation/accuracy')


def _run(log_dir, argv):
    import train_imagenet as T
    T.run(T.parse_args(argv + ['-l', log_dir]), log=lambda *a: None)
    return util.read_log(log_dir)


@pytest.fixture(scope='module')
def straight(tmp_path_factory):
    """(log, log directory) of the uninterrupted run, shared by the tests below"""
    from loans_amd import ops
    log_dir = str(tmp_path_factory.mktemp('drop_straight'))
    old, ops.SPLITK = ops.SPLITK, False
    try:
        return _run(log_dir, ARGV), log_dir
    finally:
        ops.SPLITK = old


def test_drop_path_run_logs_its_options(straight, deterministic_forward):
    log, log_dir = straight
    assert [e['iteration'] for e in log] == [1, 2, 3, 4]
    for e in log:
        assert np.isfinite(e['loss']) and np.isfinite(e['validation/loss']) and e['loss'] > 0
    assert (log[0]['drop_path'], log[0]['drop_path_seed']) == (0.3, 3)
    assert not {'drop_path', 'drop_path_seed'} & set(log[1])
    # a run without the option logs what it always logged, and is another trajectory from the second step on (the first
    # unit that drops has p > 0, so the first step's loss already differs where a sample was dropped)
    plain = _run(os.path.join(log_dir, 'plain'), RUN + BITS)
    assert not {'drop_path', 'drop_path_seed'} & set(plain[0])
    assert [e['loss'] for e in plain] != [e['loss'] for e in log]


def test_the_same_command_twice_gives_the_same_log(tmp_path, straight, deterministic_forward):
    want, _ = straight
    got = _run(str(tmp_path / 'again'), ARGV)
    for key in KEYS:
        assert [e[key] for e in got] == [e[key] for e in want], key


def test_drop_path_run_continues_from_its_checkpoint_bit_for_bit(tmp_path, straight, deterministic_forward, capsys):
    import train_imagenet as T
    from loans_amd.runtime import checkpoint
    want, s_dir = straight
    r_dir = str(tmp_path / 'R')
    argv = list(ARGV)
    argv[argv.index('--iterations') + 1] = '2'
    T.run(T.parse_args(argv + ['--checkpoint-interval', '2', '-l', r_dir]), log=lambda *a: None)
    assert sorted(n for n in os.listdir(r_dir) if n.startswith('checkpoint')) == ['checkpoint_2.npz']
    meta = checkpoint.read_meta(os.path.join(r_dir, 'checkpoint_2.npz'))
    assert (meta['args']['drop_path'], meta['args']['drop_path_seed']) == (0.3, 3)
    assert 'drop_path' in checkpoint.read_record(os.path.join(r_dir, 'checkpoint_2.npz'))['iterators']
    T.run(T.parse_args(ARGV + ['--resume', r_dir]), log=lambda *a: None)
    got = util.read_log(r_dir)
    assert [e['iteration'] for e in got] == [1, 2, 3, 4]
    for key in KEYS:
        assert [e[key] for e in got] == [e[key] for e in want], key
    with np.load(os.path.join(r_dir, 'SheepLocalizer_4.npz')) as a, np.load(os.path.join(s_dir, 'SheepLocalizer_4.npz')) as b:
        assert set(a.files) == set(b.files)
        for k in a.files:
            assert np.array_equal(a[k], b[k]), k
    # both options are fixed on resume
    capsys.readouterr()
    for other in (['--drop-path', '0.2', '--drop-path-seed', '3'], ['--drop-path', '0.3', '--drop-path-seed', '4'], []):
        with pytest.raises(SystemExit):
            T.parse_args(RUN + other + BITS + ['--resume', r_dir])
        assert 'drop_path' in capsys.readouterr().err
