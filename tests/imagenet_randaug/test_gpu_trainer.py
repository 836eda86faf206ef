"""-m gpu: ``train_imagenet.run`` with RandAugment and TrivialAugment on the run of tests/imagenet_photo/test_gpu_trainer.py: it
trains, repeats itself, validates on untouched frames, logs what it ran with -- and what it always logged without the options --
and continues from its checkpoint."""
import os

import numpy as np
import pytest

from loans_amd.runtime import checkpoint
from tests.resume import util

pytestmark = pytest.mark.gpu

RUN = ['--use-resnet-18', '-b', '2', '--image-size', '64', '64', '--augment', 'rrc', '--dataset-size', '8', '--validation-size', '4',
       '--synthetic-classes', '4', '--iterations', '4', '--log-interval', '1', '--no-shuffle', '--loader-threads', '1', '--flat-log-dir',
       '--seed', '0', '--augment-seed', '1']
RAND = ['--rand-augment', '2', '9', '--ra-seed', '3']
TRIVIAL = ['--trivial-augment', '--ra-seed', '3']
# equal bits are asked of the bf16 arm on the order-preserving kernels, as tests/imagenet_mix/test_gpu_trainer.py explains; the
# stage is fp32 in both arms
BITS = ['--dtype', 'bf16']
VOLATILE = ('elapsed_time', 'log_dir', 'resume', 'checkpoint_interval', 'iterations')
NEW = ('rand_augment', 'trivial_augment', 'ra_fill', 'ra_seed')


def _run(log_dir, extra):
    import train_imagenet as T
    T.run(T.parse_args(RUN + extra + ['-l', log_dir]), log=lambda *a: None)
    return util.read_log(log_dir)


def _stable(log):
    return [{k: v for k, v in e.items() if k not in VOLATILE} for e in log]


@pytest.mark.parametrize('options, logged', [(RAND, [[2, 9], False, [0.485, 0.456, 0.406], 3]), (TRIVIAL, [None, True, [0.485, 0.456, 0.406], 3])])
def test_trainer_with_the_stage_fp32(tmp_path, options, logged):
    log = _run(str(tmp_path / 'a'), options)
    assert [e['iteration'] for e in log] == [1, 2, 3, 4]
    for e in log:
        assert np.isfinite(e['loss']) and np.isfinite(e['validation/loss']) and e['loss'] > 0
        assert 0.0 <= e['accuracy'] <= 1.0 and 0.0 <= e['validation/accuracy'] <= 1.0
    assert [log[0][n] for n in NEW] == logged
    assert 'ra_seed' not in log[1] and os.path.exists(os.path.join(str(tmp_path / 'a'), 'SheepLocalizer_4.npz'))


@pytest.fixture(scope='module')
def straight(tmp_path_factory):
    """(log, log directory) of the bf16 run with RandAugment on, on the order-preserving kernels, shared by the two tests below"""
    from loans_amd import ops
    log_dir = str(tmp_path_factory.mktemp('ra_straight'))
    old, ops.SPLITK = ops.SPLITK, False
    try:
        return _run(log_dir, RAND + BITS), log_dir
    finally:
        ops.SPLITK = old


def test_runs_repeat_and_validate_on_untouched_frames(tmp_path, straight, deterministic_forward):
    from loans_amd import ops
    from loans_amd.common.datasets.classification_dataset import ResidentClassificationSource
    a, _ = straight
    # a second run: the same log.  The stage runs at most once per training batch the feed finishes, out of place, on frames of the
    # training size -- the validation set is not wrapped, so no validation batch can reach it
    staged, finished = [], []
    real_stage, real_finish = ops.rand_augment, ResidentClassificationSource.finish_batch

    def stage(x, jobs, out=None):
        staged.append((out is None, len(jobs), tuple(x.shape[1:])))
        return real_stage(x, jobs, out)

    def finish(self, *args, **kwargs):
        finished.append(self.train)
        return real_finish(self, *args, **kwargs)

    ops.rand_augment, ResidentClassificationSource.finish_batch = stage, finish
    try:
        b = _run(str(tmp_path / 'b'), RAND + BITS)
    finally:
        ops.rand_augment, ResidentClassificationSource.finish_batch = real_stage, real_finish
    assert _stable(a) == _stable(b)
    assert finished.count(False) >= 4 and finished.count(True) >= 4               # four validation passes, four training steps
    assert 3 <= len(staged) <= finished.count(True) and set(staged) == {(True, 2, (3, 64, 64))}
    # without the options: another run, which logs none of them
    plain = _run(str(tmp_path / 'p'), BITS)
    assert [e['loss'] for e in plain] != [e['loss'] for e in a]
    assert not set(NEW) & set(plain[0]) and set(a[0]) - set(plain[0]) == set(NEW)
    # a fill and a seed without a policy: the wrapper is not even built -- the plain bits, the options logged as given
    off = _run(str(tmp_path / 'o'), ['--ra-fill', '0', '0', '0', '--ra-seed', '9'] + BITS)
    for key in ('loss', 'accuracy', 'validation/loss', 'validation/accuracy'):
        assert [e[key] for e in off] == [e[key] for e in plain], key
    assert off[0]['ra_seed'] == 9
    # the validation entries of the first iteration depend on the first training batch alone, which the stage changed
    assert a[0]['validation/loss'] != plain[0]['validation/loss']


def test_run_continues_from_its_checkpoint(tmp_path, straight, deterministic_forward):
    import train_imagenet as T
    want, s_dir = straight
    r_dir = str(tmp_path / 'R')
    argv = list(RUN)
    argv[argv.index('--iterations') + 1] = '2'
    T.run(T.parse_args(argv + RAND + BITS + ['--checkpoint-interval', '2', '-l', r_dir]), log=lambda *a: None)
    assert sorted(n for n in os.listdir(r_dir) if n.startswith('checkpoint')) == ['checkpoint_2.npz']
    draw = checkpoint.read_record(checkpoint.common_path(r_dir, 2))['iterators']['main']['draw']
    assert isinstance(draw, tuple) and len(draw) == 2              # (the crop stream, the RandAugment stream)
    T.run(T.parse_args(RUN + RAND + BITS + ['--resume', r_dir]), log=lambda *a: None)
    got = util.read_log(r_dir)
    assert [e['iteration'] for e in got] == [1, 2, 3, 4]
    for key in ('iteration', 'epoch', 'lr'):
        assert [e[key] for e in got] == [e[key] for e in want], key
    tol = util.tolerance(0.0)           # two straight bf16 runs are bit-identical (D0 of tests/resume/test_gpu_trainer.py)
    spread = util.worst(got, want, ['loss', 'accuracy', 'validation/loss'])
    moved = util.snapshot_spread(os.path.join(r_dir, 'SheepLocalizer_4.npz'), os.path.join(s_dir, 'SheepLocalizer_4.npz'))
    print('resumed against straight: log %.3g, snapshot %.3g (allowed %.3g)' % (spread, moved, tol))
    assert spread <= tol and moved <= tol, ([e['loss'] for e in got], [e['loss'] for e in want])
    # the options are held against the checkpoint's: another seed is another data sequence, and so is the stage switched off
    with pytest.raises(SystemExit):
        T.parse_args(RUN + RAND[:-1] + ['4'] + BITS + ['--resume', r_dir])
    with pytest.raises(SystemExit):
        T.parse_args(RUN + BITS + ['--resume', r_dir])
    with pytest.raises(SystemExit):
        T.parse_args(RUN + TRIVIAL + BITS + ['--resume', r_dir])
