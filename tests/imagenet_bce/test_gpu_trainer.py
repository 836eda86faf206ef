"""-m gpu: ``train_imagenet.run`` with ``--loss bce`` on the run of tests/imagenet_mix/test_gpu_trainer.py (its sizes and its four
iterations), with mixup, label smoothing and LAMB: the log, the validation loss against ``ClassificationMetrics`` on the snapshot,
and continuation from a checkpoint.  The runs are made with --dtype bf16 on the order-preserving kernels, for the reason given
there: the head and the loss stay fp32 in that arm."""
import os

import numpy as np
import pytest
import torch

from tests.imagenet_mix.test_gpu_trainer import BITS, RUN
from tests.resume import util

pytestmark = pytest.mark.gpu

BCE = ['--loss', 'bce', '--bce-target-thresh', '0.2']
RECIPE = ['--mixup-alpha', '0.2', '--mix-seed', '3', '--label-smoothing', '0.1', '--optimizer', 'lamb', '--lr', '0.01']
ARGV = RUN + BCE + RECIPE + BITS            # (RUN holds --augment rrc)


def _run(log_dir, argv):
    import train_imagenet as T
    T.run(T.parse_args(argv + ['-l', log_dir]), log=lambda *a: None)
    return util.read_log(log_dir)


@pytest.fixture(scope='module')
def straight(tmp_path_factory):
    """(log, log directory) of the uninterrupted run, shared by the tests below"""
    from loans_amd import ops
    log_dir = str(tmp_path_factory.mktemp('bce_straight'))
    old, ops.SPLITK = ops.SPLITK, False
    try:
        return _run(log_dir, ARGV), log_dir
    finally:
        ops.SPLITK = old


def test_bce_run_logs_its_options_and_validates_on_the_plain_cross_entropy(straight, deterministic_forward):
    import loans_amd
    import train_imagenet as T
    from loans_amd.common.datasets.shard import ShardedDataset
    from loans_amd.runtime import training
    log, log_dir = straight
    assert [e['iteration'] for e in log] == [1, 2, 3, 4]
    for e in log:
        assert np.isfinite(e['loss']) and np.isfinite(e['validation/loss']) and e['loss'] > 0
        assert 0.0 <= e['accuracy'] <= 1.0 and 0.0 <= e['validation/accuracy'] <= 1.0 and 'accuracy_top5' in e
    first = log[0]
    # (an entry's ``loss`` is the training loss, in the first entry too: the option of that name is logged as ``loss_function``)
    assert (first['loss_function'], first['bce_target_thresh'], first['bce_sum']) == ('bce', 0.2, False)
    assert not {'loss_function', 'bce_target_thresh', 'bce_sum'} & set(log[1])
    # the snapshot of iteration 4 under a plain Classifier, the validation frames of the run through ClassificationMetrics
    args = T.parse_args(ARGV)
    model = T.build_model(T.parse_args(RUN + BITS))
    assert model.loss_name == 'softmax'
    model.set_precision('bf16', 'bf16')
    model.to_gpu(0)
    loans_amd.load_npz(os.path.join(log_dir, 'SheepLocalizer_4.npz'), model.predictor)
    for name in T.Arguments._PIPELINE:
        setattr(args, name, getattr(args, name))
    _, validation = T.build_crop_datasets(args, torch.device('cuda', 0))
    batches = training.MultithreadIterator(ShardedDataset(validation, 0, 1, pad=False), 2, repeat=False, shuffle=False, n_threads=1, device=0)
    metrics = loans_amd.ClassificationMetrics(topk=5)
    for batch in batches:
        x, t = training.identity_converter(batch, 0)
        model.evaluate(x, t, metrics)
    total = metrics.result()
    last = log[-1]
    print('re-evaluated %.6f, logged %.6f' % (total['loss'], last['validation/loss']))
    assert total['rows'] == 4 and abs(total['loss'] - last['validation/loss']) <= 1e-4 * abs(total['loss'])
    assert total['accuracy'] == last['validation/accuracy']
    # a softmax cross-entropy over 1000 classes after four steps is of the order of log 1000; the training loss is a mean of
    # per-class binary losses, of the order of log 2
    assert last['validation/loss'] > 2.0 > last['loss']


def test_bce_run_continues_from_its_checkpoint_bit_for_bit(tmp_path, straight, deterministic_forward, capsys):
    import train_imagenet as T
    want, s_dir = straight
    r_dir = str(tmp_path / 'R')
    argv = list(ARGV)
    argv[argv.index('--iterations') + 1] = '2'
    T.run(T.parse_args(argv + ['--checkpoint-interval', '2', '-l', r_dir]), log=lambda *a: None)
    assert sorted(n for n in os.listdir(r_dir) if n.startswith('checkpoint')) == ['checkpoint_2.npz']
    T.run(T.parse_args(ARGV + ['--resume', r_dir]), log=lambda *a: None)
    got = util.read_log(r_dir)
    assert [e['iteration'] for e in got] == [1, 2, 3, 4]
    for key in ('iteration', 'epoch', 'lr', 'loss', 'accuracy', 'validation/loss'):
        assert [e[key] for e in got] == [e[key] for e in want], key
    with np.load(os.path.join(r_dir, 'SheepLocalizer_4.npz')) as a, np.load(os.path.join(s_dir, 'SheepLocalizer_4.npz')) as b:
        assert set(a.files) == set(b.files)
        for k in a.files:
            assert np.array_equal(a[k], b[k]), k
    # the loss is not fixed on resume: a changed value is a line of the resumed run, not an error
    capsys.readouterr()
    lines = []
    other = RUN + RECIPE + BITS
    T.check_loss_arguments(T.parse_args(other))
    from loans_amd.runtime import checkpoint
    checkpoint_args = T.parse_args(other + ['--resume', r_dir])
    _, changed = checkpoint.resolve_resume(checkpoint_args, T.RESUME_FIXED, lines.append, world=1, defaults=T.RESUME_DEFAULTS_WITH_LOSS)
    assert "resume: loss was 'bce', is now 'softmax'" in changed and "resume: bce_target_thresh was 0.2, is now None" in changed
