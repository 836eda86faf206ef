"""-m gpu: ``train_imagenet.run`` with ``--teacher`` on the run of tests/imagenet_mix/test_gpu_trainer.py (its sizes, a few
iterations): a run without the options writes the snapshot the second one distils from; the log, the resume rule, and the option
beside ``--accum-steps`` and ``--optimizer lamb``.  The ResNet-18 variant is student and teacher: the shapes are the smallest the
trainer runs at, and what differs with a ResNet-50 teacher is ``--teacher-arch`` alone."""
import os

import numpy as np
import pytest

from tests.imagenet_mix.test_gpu_trainer import BITS, RUN
from tests.resume import util

pytestmark = pytest.mark.gpu

NEW = ('teacher', 'teacher_arch', 'teacher_dtype', 'distill_alpha', 'distill_temperature')
KEYS = ('distill_loss', 'teacher_accuracy')
ARGV = RUN + BITS


def _argv(iterations):
    argv = list(ARGV)
    argv[argv.index('--iterations') + 1] = str(iterations)
    return argv


def _run(log_dir, argv):
    import train_imagenet as T
    T.run(T.parse_args(argv + ['-l', log_dir]), log=lambda *a: None)
    return util.read_log(log_dir)


@pytest.fixture(scope='module')
def plain(tmp_path_factory):
    """(log, snapshot) of a run without the options, with a weight average: its ``_ema_`` snapshot is the teacher below"""
    log_dir = str(tmp_path_factory.mktemp('distill_teacher'))
    log = _run(log_dir, _argv(2) + ['--ema-decay', '0.5'])
    return log, os.path.join(log_dir, 'SheepLocalizer_ema_2.npz')


def _distill(teacher):
    return ['--teacher', teacher, '--teacher-arch', 'resnet18', '--distill-temperature', '4']


def test_a_run_without_the_options_logs_none_of_them_and_writes_the_teacher(plain):
    log, snapshot = plain
    assert [e['iteration'] for e in log] == [1, 2] and os.path.exists(snapshot)
    for e in log:
        assert not (set(NEW) | set(KEYS)) & set(e)


def test_a_distilled_run_logs_its_options_once_and_its_metrics_on_every_entry_and_resumes(plain, tmp_path, deterministic_forward):
    import train_imagenet as T
    _, snapshot = plain
    recipe = _distill(snapshot) + ['--mixup-alpha', '0.2', '--mix-seed', '3', '--label-smoothing', '0.1', '--drop-path', '0.1', '--drop-path-seed', '5']
    log_dir = str(tmp_path / 'S')
    log = _run(log_dir, _argv(2) + recipe + ['--checkpoint-interval', '2'])
    assert [e['iteration'] for e in log] == [1, 2]
    for e in log:
        assert np.isfinite(e['loss']) and e['loss'] > 0 and np.isfinite(e['distill_loss']) and e['distill_loss'] >= 0
        assert 0.0 <= e['teacher_accuracy'] <= 1.0 and 0.0 <= e['accuracy'] <= 1.0 and np.isfinite(e['validation/loss'])
    first = log[0]
    assert tuple(first[n] for n in NEW) == (snapshot, 'resnet18', 'bf16', 0.5, 4.0)            # the defaults resolved: 0.5, the run's dtype
    assert not set(NEW) & set(log[1])
    # the snapshot and the checkpoint hold nothing of the teacher
    with np.load(os.path.join(log_dir, 'SheepLocalizer_2.npz')) as a, np.load(snapshot) as b:
        assert set(a.files) == set(b.files)
    with np.load(os.path.join(log_dir, 'checkpoint_2.npz')) as ck:
        assert not [k for k in ck.files if 'teacher' in k]
    # --resume with --teacher goes on distilling
    got = _run_resume(T, _argv(3) + recipe, log_dir)
    assert [e['iteration'] for e in got] == [1, 2, 3]
    assert all(k in got[2] and np.isfinite(got[2][k]) for k in KEYS)
    assert [e['loss'] for e in got[:2]] == [e['loss'] for e in log]
    # the options are not fixed on resume: without --teacher the checkpoint's arguments differ in lines, not in an error
    from loans_amd.runtime import checkpoint
    without = T.parse_args(_argv(3) + recipe[len(_distill(snapshot)):] + ['--resume', log_dir])
    _, changed = checkpoint.resolve_resume(without, T.RESUME_FIXED, lambda line: None, world=1, defaults=T.RESUME_DEFAULTS_WITH_ACCUM)
    assert 'resume: teacher was %r, is now None' % snapshot in changed


def _run_resume(T, argv, log_dir):
    T.run(T.parse_args(argv + ['--resume', log_dir]), log=lambda *a: None)
    return util.read_log(log_dir)


@pytest.mark.parametrize('extra', (['--accum-steps', '2'], ['--optimizer', 'lamb', '--lr', '0.01'], ['--teacher-dtype', 'fp32', '--distill-alpha', '1']),
                         ids=('accum', 'lamb', 'fp32-teacher'))
def test_one_iteration_beside_the_other_options(plain, tmp_path, extra):
    _, snapshot = plain
    log = _run(str(tmp_path / 'L'), _argv(1) + _distill(snapshot) + extra)
    assert [e['iteration'] for e in log] == [1]
    assert all(np.isfinite(log[0][k]) for k in ('loss',) + KEYS)
    if '--distill-alpha' in extra:
        assert log[0]['teacher_dtype'] == 'f32' and log[0]['distill_alpha'] == 1.0
        assert log[0]['loss'] == pytest.approx(log[0]['distill_loss'], rel=1e-6)              # alpha = 1: the loss is the KL term


def test_a_snapshot_of_another_architecture_is_refused(plain, tmp_path):
    import train_imagenet as T
    _, snapshot = plain
    with pytest.raises(ValueError, match='resnet50'):
        T.build_teacher(T.parse_args(ARGV + ['--teacher', snapshot]))
