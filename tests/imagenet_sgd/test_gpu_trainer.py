"""-m gpu: ``train_imagenet.run`` with the recipe's options -- momentum SGD, a learning-rate step, label smoothing, top-5 -- on
the synthetic set, its snapshot as the starting point of a LoANs localizer, and a run without any of them."""
import json
import os

import numpy as np
import pytest

import loans_amd

pytestmark = pytest.mark.gpu

COMMON = ['--use-resnet-18', '-b', '2', '--image-size', '64', '64', '--seed', '0', '--dataset-size', '8', '--validation-size', '4',
          '--synthetic-classes', '4', '--snapshot-interval', '1000', '--no-shuffle', '--loader-threads', '1', '--flat-log-dir']
TODAYS_KEYS = {'iteration', 'epoch', 'loss', 'accuracy', 'validation/loss', 'validation/accuracy', 'elapsed_time'}


def _run(tmp_path, extra):
    import train_imagenet
    args = train_imagenet.parse_args(COMMON + ['-l', str(tmp_path)] + extra)
    entries, model = train_imagenet.run(args, log=lambda *a: None)
    with open(os.path.join(str(tmp_path), 'log')) as f:
        return json.load(f), args


def test_sgd_recipe_run_steps_the_rate_reports_top5_and_feeds_the_loans_trainer(tmp_path):
    import train_sheep_localizer
    log, args = _run(tmp_path, ['--iterations', '8', '--log-interval', '1', '--optimizer', 'sgd', '--lr', '0.05', '--lr-drop-epochs', '1',
                                '--label-smoothing', '0.1', '--topk', '5'])
    assert [e['iteration'] for e in log] == list(range(1, 9))          # 4 iterations per epoch
    for e in log:
        want = 0.05 if e['iteration'] <= 4 else 0.05 * 0.1                # the boundary: the first iteration of epoch 1
        assert e['lr'] == pytest.approx(want, rel=1e-12), e
        assert np.isfinite(e['loss']) and np.isfinite(e['validation/loss'])
        assert 0.0 <= e['accuracy'] <= e['accuracy_top5'] <= 1.0
        assert 0.0 <= e['validation/accuracy'] <= e['validation/accuracy_top5'] <= 1.0
        assert set(e) >= TODAYS_KEYS | {'lr', 'accuracy_top5', 'validation/accuracy_top5'}
    assert log[0]['lr'] == 0.05 and set(log[-1]) == TODAYS_KEYS | {'lr', 'accuracy_top5', 'validation/accuracy_top5'}
    assert log[0]['optimizer'] == 'sgd' and log[0]['label_smoothing'] == 0.1 and log[0]['lr_drop_epochs'] == [1]
    path = os.path.join(str(tmp_path), 'SheepLocalizer_8.npz')
    assert os.path.exists(path)
    with np.load(path) as h:
        assert h['feature_extractor/fc/W'].shape == (1000, 512) and h['feature_extractor/fc/b'].shape == (1000,)
        trained = {k: h[k] for k in h.files}
    assert all(np.isfinite(v).all() for v in trained.values())

    np.random.seed(1)
    loc = loans_amd.SheepLocalizer((75, 75))
    before = loc.state_dict_chainer()
    train_sheep_localizer.load_pretrained_model(path, loc)
    after = loc.state_dict_chainer()
    for k, v in after.items():
        if k.startswith('feature_extractor/'):
            np.testing.assert_array_equal(v, trained[k], err_msg=k)
        else:
            np.testing.assert_array_equal(v, before[k], err_msg=k)
    assert np.abs(after['feature_extractor/res5/1/conv2/W'] - before['feature_extractor/res5/1/conv2/W']).max() > 0


def test_a_run_without_the_new_options_logs_todays_keys_and_the_rate(tmp_path):
    log, args = _run(tmp_path, ['--iterations', '4', '--log-interval', '2'])
    assert [e['iteration'] for e in log] == [2, 4]
    assert set(log[-1]) == TODAYS_KEYS | {'lr'}
    assert all(e['lr'] == 0.001 for e in log)                           # Adam's alpha, untouched by the (empty) schedule
    # the first entry also carries every argument, as before: the new ones among them, at their inert defaults
    assert set(log[0]) == TODAYS_KEYS | {'lr', 'log_dir', 'image_size', 'localizer'} | set(vars(args))
    assert log[0]['optimizer'] == 'adam' and log[0]['topk'] is None and log[0]['label_smoothing'] == 0.0
