"""-m gpu: ``train_imagenet.run`` with the mix options on the run of tests/imagenet_rrc/test_gpu_input_path.py: both mixes,
repeatability, the plain bits of a run whose batches are never mixed, and continuation from a checkpoint."""
import os

import numpy as np
import pytest

from loans_amd.runtime import checkpoint
from tests.resume import util

pytestmark = pytest.mark.gpu

RUN = ['--use-resnet-18', '-b', '2', '--image-size', '64', '64', '--augment', 'rrc', '--dataset-size', '8', '--validation-size', '4',
       '--synthetic-classes', '4', '--iterations', '4', '--log-interval', '1', '--no-shuffle', '--loader-threads', '1', '--flat-log-dir',
       '--seed', '0', '--augment-seed', '1']
MIX = ['--mixup-alpha', '0.2', '--cutmix-alpha', '1.0', '--mix-seed', '3']
# Two straight fp32 runs of one command are not bit-identical on this GPU (the fp32 weight gradients close with atomics:
# tests/resume/util.py); the bf16 arm keeps its order at these shapes, and the head, the loss and the mix stay fp32 in it.  So
# the comparisons that ask for equal bits run the command with --dtype bf16 on the order-preserving kernels, as
# tests/resume/test_gpu_trainer.py does.
BITS = ['--dtype', 'bf16']
VOLATILE = ('elapsed_time', 'log_dir', 'resume', 'checkpoint_interval', 'iterations')


def _run(log_dir, extra):
    import train_imagenet as T
    T.run(T.parse_args(RUN + extra + ['-l', log_dir]), log=lambda *a: None)
    return util.read_log(log_dir)


def _stable(log):
    return [{k: v for k, v in e.items() if k not in VOLATILE} for e in log]


def test_trainer_with_both_mixes_fp32(tmp_path):
    log = _run(str(tmp_path / 'a'), MIX)
    assert [e['iteration'] for e in log] == [1, 2, 3, 4]
    for e in log:
        assert np.isfinite(e['loss']) and np.isfinite(e['validation/loss']) and e['loss'] > 0
        assert 0.0 <= e['accuracy'] <= 1.0 and 0.0 <= e['validation/accuracy'] <= 1.0
    first = log[0]
    assert (first['mixup_alpha'], first['cutmix_alpha'], first['mix_prob'], first['mix_switch_prob'], first['mix_seed']) == (0.2, 1.0, 1.0, 0.5, 3)
    assert 'mixup_alpha' not in log[1] and os.path.exists(os.path.join(str(tmp_path / 'a'), 'SheepLocalizer_4.npz'))


@pytest.fixture(scope='module')
def straight_mixed(tmp_path_factory):
    """(log, log directory) of the mixed bf16 run on the order-preserving kernels, shared by the two tests below"""
    from loans_amd import ops
    log_dir = str(tmp_path_factory.mktemp('mix_straight'))
    old, ops.SPLITK = ops.SPLITK, False
    try:
        return _run(log_dir, MIX + BITS), log_dir
    finally:
        ops.SPLITK = old


def test_mixed_runs_repeat_and_validate_on_the_plain_loss(tmp_path, straight_mixed, deterministic_forward):
    import loans_amd
    from loans_amd.functions import ops_small
    a, _ = straight_mixed
    # a second run: the same log; the two-label loss runs once per training step and never in a validation pass
    calls = []
    old = ops_small.SoftmaxCrossEntropyMixed.forward
    ops_small.SoftmaxCrossEntropyMixed.forward = lambda self, inputs: calls.append(loans_amd.config.train) or old(self, inputs)
    try:
        b = _run(str(tmp_path / 'b'), MIX + BITS)
    finally:
        ops_small.SoftmaxCrossEntropyMixed.forward = old
    assert calls == [True] * 4
    assert _stable(a) == _stable(b)
    assert all(np.isfinite(e['loss']) and np.isfinite(e['validation/loss']) for e in a)
    plain = _run(str(tmp_path / 'p'), BITS)
    assert [e['loss'] for e in plain] != [e['loss'] for e in a]
    # nothing mixed (--mix-prob 0): the wrapper, MixedLabels and the (1, 0) routes of both kernels end to end -- the plain bits
    off = _run(str(tmp_path / 'o'), ['--mixup-alpha', '0.4', '--mix-prob', '0'] + BITS)
    for key in ('loss', 'accuracy', 'validation/loss', 'validation/accuracy'):
        assert [e[key] for e in off] == [e[key] for e in plain], key
    assert off[0]['mix_prob'] == 0.0 and plain[0]['mixup_alpha'] == 0.0


def test_mixed_run_continues_from_its_checkpoint(tmp_path, straight_mixed, deterministic_forward):
    import train_imagenet as T
    want, s_dir = straight_mixed
    r_dir = str(tmp_path / 'R')
    argv = list(RUN)
    argv[argv.index('--iterations') + 1] = '2'
    T.run(T.parse_args(argv + MIX + BITS + ['--checkpoint-interval', '2', '-l', r_dir]), log=lambda *a: None)
    assert sorted(n for n in os.listdir(r_dir) if n.startswith('checkpoint')) == ['checkpoint_2.npz']
    draw = checkpoint.read_record(checkpoint.common_path(r_dir, 2))['iterators']['main']['draw']
    assert isinstance(draw, tuple) and len(draw) == 2              # (the crop stream, the mix stream)
    T.run(T.parse_args(RUN + MIX + BITS + ['--resume', r_dir]), log=lambda *a: None)
    got = util.read_log(r_dir)
    assert [e['iteration'] for e in got] == [1, 2, 3, 4]
    for key in ('iteration', 'epoch', 'lr'):
        assert [e[key] for e in got] == [e[key] for e in want], key
    tol = util.tolerance(0.0)           # two straight bf16 runs are bit-identical (D0 of tests/resume/test_gpu_trainer.py)
    spread = util.worst(got, want, ['loss', 'accuracy', 'validation/loss'])
    moved = util.snapshot_spread(os.path.join(r_dir, 'SheepLocalizer_4.npz'), os.path.join(s_dir, 'SheepLocalizer_4.npz'))
    print('resumed against straight: log %.3g, snapshot %.3g (allowed %.3g)' % (spread, moved, tol))
    assert spread <= tol and moved <= tol, ([e['loss'] for e in got], [e['loss'] for e in want])
    # the mix options are held against the checkpoint's: another seed is another data sequence
    with pytest.raises(SystemExit):
        T.parse_args(RUN + ['--mixup-alpha', '0.2', '--cutmix-alpha', '1.0', '--mix-seed', '4'] + BITS + ['--resume', r_dir])
