"""-m gpu: the datasets of the random-resized-crop feed against their own host reference (Pillow), the feeding iterator over
them, the HBM-resident source, and ``train_imagenet.run --augment rrc`` on the synthetic classes and on files."""
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

from loans_amd.common.datasets import crop_resize as CR
from loans_amd.common.datasets.classification_dataset import ClassificationImageDataset, ResidentClassificationSource
from loans_amd.runtime import training

pytestmark = pytest.mark.gpu

OUT = (24, 20)
TODAYS_KEYS = {'iteration', 'epoch', 'loss', 'accuracy', 'validation/loss', 'validation/accuracy', 'elapsed_time'}


def _write_set(folder, sizes, name):
    rng = np.random.RandomState(len(sizes))
    lines = []
    for n, (H, W) in enumerate(sizes):
        Image.fromarray(rng.randint(0, 256, (H, W, 3)).astype(np.uint8)).save(os.path.join(folder, '%s%d.png' % (name, n)))
        lines.append('%s%d.png\t%d' % (name, n, (3 * n + 1) % 4))
    path = os.path.join(folder, name + '.tsv')
    with open(path, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    return path


@pytest.fixture(scope='module')
def five_pngs(tmp_path_factory):
    folder = str(tmp_path_factory.mktemp('rrc_set'))
    return _write_set(folder, [(37, 53), (64, 48), (37, 53), (30, 91), (80, 33)], 'f'), folder


def _reference(ds, indices):
    examples = [ds.get_example(i) for i in indices]
    return np.stack([e[0] for e in examples]), np.array([e[1] for e in examples])


@pytest.mark.parametrize('train', [True, False], ids=['train', 'validation'])
def test_device_batch_equals_the_stacked_host_examples(five_pngs, train):
    path, folder = five_pngs
    ds = ClassificationImageDataset(path, folder, image_size=OUT, train=train, augment_seed=0)
    indices = [3, 0, 4, 1, 2]
    ds.reseed(11)
    frames, labels = ds.device_batch(indices, 'cuda')
    ds.reseed(11)
    want, want_labels = _reference(ds, indices)
    assert frames.is_cuda and frames.dtype == torch.float32 and tuple(frames.shape) == (5, 3) + OUT
    assert labels.is_cuda and labels.dtype == torch.int32
    np.testing.assert_array_equal(frames.cpu().numpy(), want)
    np.testing.assert_array_equal(labels.cpu().numpy(), want_labels)
    assert labels.cpu().tolist() == [(3 * i + 1) % 4 for i in indices]


def test_feeding_iterator_is_reproducible_and_redraws_every_epoch(five_pngs):
    path, folder = five_pngs
    ds = ClassificationImageDataset(path, folder, image_size=OUT, train=True)

    def two_epochs(seed):
        ds.reseed(seed)
        it = training.MultithreadIterator(ds, 2, shuffle=False, n_threads=2, device=torch.cuda.current_device())
        frames, labels = [], []
        try:
            for _ in range(5):                      # 10 examples = two passes over the five files
                x, t = training.identity_converter(next(it))
                assert x.is_cuda and tuple(x.shape) == (2, 3) + OUT and t.dtype == torch.int32
                frames.append(x.cpu().numpy())
                labels.append(t.cpu().numpy())
            assert it.epoch == 2
        finally:
            it.finalize()
        return np.concatenate(frames), np.concatenate(labels)

    a, la = two_epochs(5)
    b, lb = two_epochs(5)
    c, _ = two_epochs(6)
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(la, lb)
    assert la.tolist() == [(3 * i + 1) % 4 for i in range(5)] * 2
    assert not np.array_equal(a, c)
    for i in range(5):                              # the same file, another crop
        assert not np.array_equal(a[i], a[5 + i]), i
    ds.reseed(5)                                    # and what came out is what the host path makes of the same draws
    want, _ = _reference(ds, list(range(5)) * 2)
    np.testing.assert_array_equal(a, want)


@pytest.mark.parametrize('train', [True, False], ids=['train', 'validation'])
def test_resident_source_crops_in_place(train):
    rng = np.random.RandomState(3)
    frames = rng.randint(0, 256, (6, 40, 57, 3)).astype(np.uint8)
    labels = np.arange(6)[::-1].copy()
    src = ResidentClassificationSource(frames, labels, 'cuda', image_size=OUT, train=train, augment_seed=2)
    assert len(src) == 6 and src.frames.is_cuda and src.frames.dtype == torch.uint8
    indices = [4, 1, 5, 1]
    decoded = src.decode_batch(indices)
    x, t = src.finish_batch(decoded, 'cuda')
    want = np.stack([CR.crop_resize_host(frames[i], box, OUT, flip) for i, (box, flip) in zip(*decoded)])
    np.testing.assert_array_equal(x.cpu().numpy(), want)
    assert t.dtype == torch.int32 and t.cpu().tolist() == [1, 4, 0, 4]
    if train:
        assert len({box for box, _ in decoded[1]}) > 1
        src.reseed(2)
        assert src.decode_batch(indices)[1] == decoded[1]
    else:
        assert decoded[1] == [(CR.center_crop_box(40, 57, OUT), False)] * 4
    # the synthetic classes' conversion: k / 255 floats come back as k
    back = ResidentClassificationSource.from_float_chw(frames.transpose(0, 3, 1, 2).astype(np.float32) / 255, labels, 'cuda', image_size=OUT)
    np.testing.assert_array_equal(back.frames.cpu().numpy(), frames)


RUN = ['--use-resnet-18', '-b', '2', '--image-size', '64', '64', '--augment', 'rrc', '--dataset-size', '8', '--validation-size', '4',
       '--synthetic-classes', '4', '--iterations', '4', '--log-interval', '2', '--no-shuffle', '--loader-threads', '1', '--flat-log-dir',
       '--seed', '0', '--augment-seed', '1']


def _run(tmp_path, extra):
    import train_imagenet
    args = train_imagenet.parse_args(extra + RUN + ['-l', str(tmp_path / 'log')])
    train_imagenet.run(args, log=lambda *a: None)
    with open(os.path.join(str(tmp_path / 'log'), 'log')) as f:
        log = json.load(f)
    assert [e['iteration'] for e in log] == [2, 4]
    for e in log:
        assert np.isfinite(e['loss']) and np.isfinite(e['validation/loss'])
        assert 0.0 <= e['accuracy'] <= 1.0 and 0.0 <= e['validation/accuracy'] <= 1.0
    assert set(log[-1]) == TODAYS_KEYS | {'lr'}
    assert log[0]['augment'] == 'rrc' and log[0]['augment_seed'] == 1
    assert os.path.exists(os.path.join(str(tmp_path / 'log'), 'SheepLocalizer_4.npz'))


def test_trainer_with_rrc_on_the_synthetic_classes(tmp_path):
    _run(tmp_path, [])


def test_trainer_with_rrc_on_files(tmp_path):
    sizes = [(70, 90), (64, 64), (100, 61), (33, 47), (70, 90), (128, 96), (50, 75), (81, 80)]
    train = _write_set(str(tmp_path), sizes, 'train')
    val = _write_set(str(tmp_path), sizes[:4], 'val')
    _run(tmp_path, [train, val])
