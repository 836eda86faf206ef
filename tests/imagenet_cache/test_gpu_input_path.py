"""-m gpu: ``ClassificationImageDataset`` with a ``RaggedFrameCache`` against its own host reference (Pillow), through a shard
and on a second stream, and ``train_imagenet.run --frame-cache-gb``."""
import json
import os

import numpy as np
import pytest
import torch

from loans_amd.common.datasets import classification_dataset as CD
from loans_amd.common.datasets import crop_resize as CR
from loans_amd.common.datasets.classification_dataset import ClassificationImageDataset
from loans_amd.common.datasets.frame_cache import RaggedFrameCache
from loans_amd.common.datasets.shard import ShardedDataset

from ._files import nbytes, write_set

pytestmark = pytest.mark.gpu

OUT = (24, 20)


@pytest.fixture(scope='module')
def pngs(tmp_path_factory):
    folder = str(tmp_path_factory.mktemp('cache_set'))
    return write_set(folder), folder


def _reference(ds, indices):
    examples = [ds.get_example(i) for i in indices]
    return np.stack([e[0] for e in examples]), np.array([e[1] for e in examples])


def _no_decode(i):
    raise AssertionError('frame %d was decoded again' % i)


def _check(ds, ref, indices, seed):
    ds.reseed(seed)
    ref.reseed(seed)
    batch = ds.device_batch(indices, 'cuda')
    frames, labels = batch
    want, want_labels = _reference(ref, indices)
    assert frames.is_cuda and frames.dtype == torch.float32 and tuple(frames.shape) == (len(indices), 3) + OUT
    assert labels.is_cuda and labels.dtype == torch.int32
    np.testing.assert_array_equal(frames.cpu().numpy(), want)
    np.testing.assert_array_equal(labels.cpu().numpy(), want_labels)
    return batch


@pytest.mark.parametrize('where', ['device', 'host'])
@pytest.mark.parametrize('train', [True, False], ids=['train', 'validation'])
def test_the_second_epoch_decodes_nothing_and_equals_the_host_examples(pngs, train, where):
    path, folder = pngs
    cache = RaggedFrameCache(1 << 20, where, 'cuda', slab_bytes=1 << 16)
    ds = ClassificationImageDataset(path, folder, image_size=OUT, train=train, augment_seed=0, cache=cache)
    ref = ClassificationImageDataset(path, folder, image_size=OUT, train=train, augment_seed=0)
    first = _check(ds, ref, [3, 0, 4], 11)                          # epoch 1, in two batches
    _check(ds, ref, [1, 2], 12)
    assert (cache.hits, cache.misses, len(cache)) == (0, 5, 5) and cache.bytes == sum(nbytes(i) for i in range(5))
    assert (first.cache_hits, first.cache_misses) == (0, 3)
    if where == 'device':
        assert cache.allocated == 1 << 16 and len(cache.slabs) == 1 and cache.slabs[0].is_cuda
    ds._read_u8 = _no_decode                                        # epoch 2
    second = _check(ds, ref, [2, 4, 0, 3, 1], 13)
    _check(ds, ref, [0, 0, 3], 14)
    assert (cache.hits, cache.misses, len(cache)) == (8, 5, 5)
    assert (second.cache_hits, second.cache_misses) == (5, 0)
    if train:
        assert not torch.equal(first[0][1], second[0][2])           # frame 0 again: another crop


def test_a_batch_of_hits_stored_and_unstored_misses_is_one_launch(pngs, monkeypatch):
    path, folder = pngs
    calls = []
    real = CR.crop_resize_device_multi

    def counted(srcs, jobs, out_hw, out=None):
        calls.append(([int(s.numel()) for s in srcs], [j[6] for j in jobs]))
        return real(srcs, jobs, out_hw, out)

    monkeypatch.setattr(CD, 'crop_resize_device_multi', counted)
    monkeypatch.setattr(CD, 'crop_resize_device', _no_decode)
    # one slab of 6000 bytes: frames 0 (2139 B) and 1 (2040 B) go in with the first batch, of the second batch frame 3
    # (1800 B) fits what is left, frame 2 (12288 B) fits no slab and frame 4 (2871 B) has no room
    cache = RaggedFrameCache(6000, 'device', 'cuda', slab_bytes=6000)
    ds = ClassificationImageDataset(path, folder, image_size=OUT, train=True, augment_seed=0, cache=cache)
    ref = ClassificationImageDataset(path, folder, image_size=OUT, train=True, augment_seed=0)
    _check(ds, ref, [0, 1], 3)
    assert calls == [([6000], [0, 0])]
    assert (cache.hits, cache.misses, len(cache), cache.bytes, cache.allocated) == (0, 2, 2, nbytes(0) + nbytes(1), 6000)
    batch = _check(ds, ref, [0, 2, 1, 3, 4], 4)
    assert len(calls) == 2
    sizes, srcs = calls[1]
    assert sizes[0] == 6000 and len(sizes) == 2 and srcs == [0, 1, 0, 0, 1]       # the slab, and the upload of crop rows
    assert sizes[1] < nbytes(2) + nbytes(4)                                       # (rows of the crops, not whole frames)
    assert (batch.cache_hits, batch.cache_misses) == (2, 3)
    assert (cache.hits, cache.misses, len(cache), cache.bytes, cache.allocated) == (2, 5, 3, nbytes(0) + nbytes(1) + nbytes(3), 6000)
    assert cache.location(3) == (0, nbytes(0) + nbytes(1), 20, 30)
    # the slab holds the decoded frames byte for byte
    slab = cache.slabs[0].cpu().numpy()
    for i in (0, 1, 3):
        _, at, H, W = cache.location(i)
        np.testing.assert_array_equal(slab[at:at + H * W * 3].reshape(H, W, 3), ref._read_u8(i))
    _check(ds, ref, [3, 4, 2], 5)
    assert calls[2][1] == [0, 1, 1] and (cache.hits, cache.misses, len(cache)) == (3, 7, 3)


def test_a_shard_whose_batch_repeats_an_index(pngs):
    """rank 1 of 2 over five files holds base indices 1, 3, 0 (the last one by the padded wrap); a batch that runs over the
    shard's end into the next pass repeats index 1 before it is stored: neither occurrence is admitted"""
    path, folder = pngs
    cache = RaggedFrameCache(1 << 20, 'device', 'cuda', slab_bytes=1 << 16)
    ds = ShardedDataset(ClassificationImageDataset(path, folder, image_size=OUT, train=True, augment_seed=0, cache=cache), 1, 2, pad=True)
    ref = ShardedDataset(ClassificationImageDataset(path, folder, image_size=OUT, train=True, augment_seed=0), 1, 2, pad=True)
    assert [ds.base_index(i) for i in range(len(ds))] == [1, 3, 0]
    _check(ds, ref, [0, 1, 2, 0], 7)
    assert (cache.hits, cache.misses) == (0, 4) and sorted(cache.slots) == [0, 3]
    batch = _check(ds, ref, [0, 1, 2, 0], 8)
    assert (batch.cache_hits, batch.cache_misses) == (2, 2) and sorted(cache.slots) == [0, 3]
    _check(ds, ref, [2, 0], 9)
    assert (cache.hits, cache.misses) == (3, 7) and sorted(cache.slots) == [0, 1, 3]
    ds.dataset._read_u8 = _no_decode
    _check(ds, ref, [0, 1, 2, 0], 10)
    assert ds.cache is cache and cache.bytes == nbytes(0) + nbytes(1) + nbytes(3)


def test_a_second_stream_waits_for_the_stores(pngs):
    path, folder = pngs
    cache = RaggedFrameCache(1 << 20, 'device', 'cuda', slab_bytes=1 << 16)
    ds = ClassificationImageDataset(path, folder, image_size=OUT, train=True, augment_seed=0, cache=cache)
    ref = ClassificationImageDataset(path, folder, image_size=OUT, train=True, augment_seed=0)
    one, two = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(one):
        _check(ds, ref, [0, 1, 2, 3, 4], 1)
    assert list(cache._store_events) == [one]
    with torch.cuda.stream(two):
        _check(ds, ref, [4, 3, 2, 1, 0], 2)
    assert cache.hits == 5


# ---- the trainer ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('where', ['device', 'host'])
def test_trainer_with_a_frame_cache(tmp_path, where):
    import train_imagenet
    sizes = [(70, 90, 'RGB'), (64, 64, 'RGB'), (100, 61, 'RGB'), (33, 47, 'L'), (70, 90, 'RGB'), (128, 96, 'RGB'), (50, 75, 'RGB'), (81, 80, 'RGB')]
    train = write_set(str(tmp_path), sizes, 'train')
    val = write_set(str(tmp_path), sizes[:4], 'val')
    log_dir = str(tmp_path / 'log')
    args = train_imagenet.parse_args([train, val, '--use-resnet-18', '-b', '2', '--image-size', '64', '64', '--augment', 'rrc',
                                      '--num-epoch', '2', '--log-interval', '1000', '--no-shuffle', '--loader-threads', '1',
                                      '--flat-log-dir', '--seed', '0', '--augment-seed', '1', '--frame-cache-gb', '0.25',
                                      '--frame-cache-where', where, '-l', log_dir])
    train_imagenet.run(args, log=lambda *a: None)
    with open(os.path.join(log_dir, 'log')) as f:
        log = json.load(f)
    assert [(e['iteration'], e['epoch']) for e in log] == [(4, 1), (8, 2)]
    total = sum(H * W * 3 for H, W, _ in sizes)
    assert log[0]['frame_cache_gb'] == 0.25 and log[0]['frame_cache_where'] == where
    assert (log[0]['feed/cache_hits'], log[0]['feed/cache_misses']) == (0, 8)
    assert (log[1]['feed/cache_hits'], log[1]['feed/cache_misses']) == (8, 0)          # the shard's length, and no decode
    assert (log[0]['feed/val_cache_hits'], log[0]['feed/val_cache_misses']) == (0, 4)
    assert (log[1]['feed/val_cache_hits'], log[1]['feed/val_cache_misses']) == (4, 0)
    for e in log:
        assert (e['feed/cache_frames'], e['feed/cache_bytes']) == (8, total)
        assert np.isfinite(e['loss']) and np.isfinite(e['validation/loss'])
    assert os.path.exists(os.path.join(log_dir, 'SheepLocalizer_8.npz'))
