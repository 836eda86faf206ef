"""No GPU: the bookkeeping of ``RaggedFrameCache``, the per-source form of ``check_jobs``, the draw order of a partly cached
``decode_batch``, the launcher's argument checks and the trainer's options."""
import numpy as np
import pytest
import torch

from loans_amd.common.datasets import crop_resize as CR
from loans_amd.common.datasets.classification_dataset import ClassificationImageDataset
from loans_amd.common.datasets.frame_cache import CachedFrame, RaggedFrameCache
from loans_amd.common.datasets.resample import resample_coeffs
from loans_amd.common.datasets.shard import ShardedDataset

from ._files import SIZES, nbytes, write_set


# ---- the cache's bookkeeping ----------------------------------------------------------------------------------------------------
def test_slabs_are_sized_from_the_budget():
    assert RaggedFrameCache(1 << 30, device='cpu').slab_bytes == 64 << 20              # the floor
    assert RaggedFrameCache(64 << 30, device='cpu').slab_bytes == 2 << 30              # budget / 32
    small = RaggedFrameCache((64 << 20) - 1, device='cpu')                            # not even one slab fits
    assert small.reserve([(0, 10, 10)]) == [None] and small.allocated == 0 and small.slabs == []
    with pytest.raises(ValueError):
        RaggedFrameCache(1, where='disk')


def test_bump_allocation_across_slabs_within_the_budget():
    c = RaggedFrameCache(1000, 'device', 'cpu', slab_bytes=400)                        # two slabs of 400 fit 1000, a third not
    #        300 B        75 B (fits behind)  300 B: next slab  1200 B: over a slab   75 B         300 B: a third slab is over budget
    frames = [(10, 10, 10), (11, 5, 5), (12, 10, 10), (13, 20, 20), (14, 5, 5), (15, 10, 10)]
    got = c.reserve(frames)
    assert got == [(0, 0), (0, 300), (1, 0), None, (1, 300), None]
    assert c.allocated == 800 <= c.budget and len(c.slabs) == 2
    assert all(s.dtype == torch.uint8 and s.numel() == 400 and s.device.type == 'cpu' for s in c.slabs)
    # nothing is served before it is published
    assert len(c) == 0 and c.bytes == 0 and c.lookup(10) is None and (c.hits, c.misses) == (0, 1)
    c.publish([10, 11, 12, 14])
    assert len(c) == 4 and c.bytes == 300 + 75 + 300 + 75
    f = c.lookup(12)
    assert isinstance(f, CachedFrame) and f.index == 12 and f.shape == (10, 10, 3)
    assert c.location(12) == (1, 0, 10, 10) and c.location(11) == (0, 300, 5, 5)
    assert c.lookup(13) is None and c.lookup(15) is None and (c.hits, c.misses) == (1, 3)
    # a second store of an index is a no-op, published or only reserved; what is left of the last slab still serves
    assert c.reserve([(10, 10, 10), (12, 1, 1)]) == [None, None]
    assert c.reserve([(16, 2, 4)]) == [(1, 375)] and c.reserve([(16, 2, 4)]) == [None]
    assert c.reserve([(17, 1, 1)]) == [None]                                             # 1 B left: 3 do not fit
    assert c.allocated == 800 and len(c) == 4 and c.bytes == 750
    c.publish([16])
    assert len(c) == 5 and c.bytes == 750 + 24


def test_a_frame_never_straddles_two_slabs():
    c = RaggedFrameCache(10 ** 6, 'device', 'cpu', slab_bytes=1000)
    locs = c.reserve([(i, 7, 13) for i in range(40)])                                   # 273 B each: three per slab
    assert all(l is not None for l in locs)
    for slab, off in locs:
        assert off + 273 <= 1000
    assert [l[0] for l in locs[:7]] == [0, 0, 0, 1, 1, 1, 2] and c.allocated == 14 * 1000


def test_host_mode_keeps_arrays_within_the_budget():
    c = RaggedFrameCache(1000, 'host')
    a, b = np.zeros((10, 10, 3), np.uint8), np.ones((16, 16, 3), np.uint8)
    assert c.lookup(0) is None
    assert c.keep_host(0, a) and not c.keep_host(0, a)                                  # the second store: a no-op
    assert not c.keep_host(1, b)                                                        # 768 B more than the budget has left
    assert c.keep_host(2, a.copy())
    assert c.lookup(0) is a and c.lookup(1) is None and (c.hits, c.misses) == (1, 2)
    assert len(c) == 2 and c.bytes == 600 and c.allocated == 0
    assert c.reserve([(5, 2, 2)]) == [None]                                             # (device mode's calls do nothing here)
    assert not RaggedFrameCache(1000, 'device', 'cpu', slab_bytes=100).keep_host(0, a)


# ---- check_jobs ---------------------------------------------------------------------------------------------------------------------
def test_the_window_formula_is_the_tables_width():
    for out in (1, 2, 3, 4, 16, 31, 224, 225):
        for size in list(range(1, 300)) + [448, 449, 1000, 4001]:
            assert CR.bilinear_window(size, out) == resample_coeffs(size, out, 'bilinear')[2], (size, out)


def test_check_jobs_per_source_form():
    sizes = [40 * 50 * 3 + 10, 20 * 20 * 3, 40 * 50 * 3 + 10]
    ok = [(10, 150, 40, 50, (0, 0, 40, 50), False, 0), (0, 60, 20, 20, (3, 4, 10, 11), True, 1), (0, 150, 40, 50, (1, 1, 5, 5), False, 2)]
    CR.check_jobs(sizes, ok, (16, 16))
    CR.check_jobs(tuple(sizes), ok, (16, 16))
    for bad, what in [((0, 60, 20, 20, (0, 0, 5, 5), False, 3), 'source index'),               # out of range
                      ((0, 60, 20, 20, (0, 0, 5, 5), False, -1), 'source index'),
                      ((10, 150, 40, 50, (0, 0, 8, 8), False, 1), 'buffer'),                   # fits sources 0 and 2, not its own
                      ((11, 150, 40, 50, (0, 0, 8, 8), False, 2), 'buffer'),                   # ends one byte behind its source
                      ((1, 60, 20, 20, (0, 0, 8, 8), False, 1), 'buffer'),
                      ((0, 60, 20, 20, (0, 10, 10, 11), False, 1), 'box'),                     # leaves its frame on the right
                      ((0, 60, 20, 20, (11, 0, 10, 10), False, 1), 'box'),
                      ((0, 59, 20, 20, (0, 0, 8, 8), False, 1), 'pitch'),
                      ((0, 60, 20, 20, (0, 0, 8, 8), False), 'entries')]:                      # a job without its index
        with pytest.raises(ValueError, match=what):
            CR.check_jobs(sizes, ok + [bad], (16, 16))
    # a vertical window over the LDS capacity: out_w = 1024 holds 21 rows, 40 rows -> 2 have a window of 41
    with pytest.raises(ValueError, match='window'):
        CR.check_jobs(sizes, ok[:1], (2, 1024))
    with pytest.raises(ValueError):
        CR.check_jobs(sizes, [], (16, 16))
    # the single-source form is what it was
    CR.check_jobs(sizes[0], [j[:6] for j in ok[:1]], (16, 16))
    with pytest.raises(ValueError, match='buffer'):
        CR.check_jobs(sizes[0], [(11, 150, 40, 50, (0, 0, 8, 8), False)], (16, 16))


def test_the_multi_source_wrapper_validates_before_it_touches_a_gpu():
    bufs = [torch.zeros(40 * 50 * 3, dtype=torch.uint8), torch.zeros(20 * 20 * 3, dtype=torch.uint8)]     # host tensors
    ok = [(0, 150, 40, 50, (0, 0, 40, 50), False, 0), (0, 60, 20, 20, (0, 0, 20, 20), False, 1)]
    with pytest.raises(ValueError, match='source index'):
        CR.crop_resize_device_multi(bufs, ok + [(0, 60, 20, 20, (0, 0, 20, 20), False, 2)], (16, 16))
    with pytest.raises(ValueError, match='buffer'):
        CR.crop_resize_device_multi(bufs, [(0, 150, 40, 50, (0, 0, 40, 50), False, 1)], (16, 16))
    with pytest.raises(ValueError, match='uint8'):
        CR.crop_resize_device_multi([bufs[0].float()], ok[:1], (16, 16))
    with pytest.raises(ValueError):
        CR.crop_resize_device_multi([], ok[:1], (16, 16))
    with pytest.raises(ValueError, match='device'):                                      # everything in order but the buffers' home
        CR.crop_resize_device_multi(bufs, ok, (16, 16))


def test_launcher_rejects_a_missing_table_before_any_launch():
    import __graft_entry__
    __graft_entry__.build()
    from loans_amd import _lib
    fn = _lib.load().loans_crop_resize_srcs_u8_f32
    p = 4096                                                        # a non-null pointer value that nothing dereferences
    assert fn(0, p, 1, p, p, 1, p, 3, 16, 16, 0) == -1              # no pointer table
    assert fn(p, 0, 1, p, p, 1, p, 3, 16, 16, 0) == -1              # no index array
    assert fn(p, p, 0, p, p, 1, p, 3, 16, 16, 0) == -1              # nsrcs <= 0
    assert fn(p, p, -3, p, p, 1, p, 3, 16, 16, 0) == -1
    # and the shape checks of the single-source entry
    assert fn(p, p, 1, 0, p, 1, p, 3, 16, 16, 0) == -1
    assert fn(p, p, 1, p, 0, 1, p, 3, 16, 16, 0) == -1
    assert fn(p, p, 1, p, p, 1, 0, 3, 16, 16, 0) == -1
    assert fn(p, p, 1, p, p, 0, p, 3, 16, 16, 0) == -1
    assert fn(p, p, 1, p, p, 65536, p, 3, 16, 16, 0) == -1
    assert fn(p, p, 1, p, p, 1, p, 0, 16, 16, 0) == -1
    assert fn(p, p, 1, p, p, 1, p, 3, 0, 16, 0) == -1
    assert fn(p, p, 1, p, p, 1, p, CR.lds_row_capacity(224) + 1, 224, 224, 0) == -1
    assert fn(p, p, 1, p, p, 1, p, 1, 4, CR.CROP_LDS_BYTES, 0) == -1


# ---- the dataset's host half ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('where', ['device', 'host'])
def test_a_partly_cached_batch_draws_like_the_uncached_one(tmp_path, where):
    path = write_set(str(tmp_path))
    cache = RaggedFrameCache(10 ** 6, where, 'cpu', slab_bytes=10 ** 5)
    ds = ClassificationImageDataset(path, str(tmp_path), image_size=(16, 12), train=True, augment_seed=5, cache=cache)
    ref = ClassificationImageDataset(path, str(tmp_path), image_size=(16, 12), train=True, augment_seed=5)
    # frames 1 and 3 are in the cache
    if where == 'device':
        assert cache.reserve([(i,) + SIZES[i][:2] for i in (1, 3)]) == [(0, 0), (0, nbytes(1))]
        cache.publish([1, 3])
    else:
        for i in (1, 3):
            assert cache.keep_host(i, ref._read_u8(i))
    read = []
    real = ds._read_u8
    ds._read_u8 = lambda i: read.append(i) or real(i)
    indices = [4, 1, 0, 3, 2, 1]
    frames, draws, labels, carried, hits = ds.decode_batch(indices)
    assert read == [4, 0, 2] and carried == indices and hits == 3
    assert (cache.hits, cache.misses) == (3, 3)
    assert labels.tolist() == [(3 * i + 1) % 4 for i in indices]
    for i, f in zip(indices, frames):
        assert f.shape == SIZES[i][:2] + (3,)
        assert isinstance(f, CachedFrame) == (where == 'device' and i in (1, 3))
    want = ref.decode_batch(indices)
    assert draws == want[1] and len({d[0] for d in draws}) > 1
    assert ds._aug_rng.getstate() == ref._aug_rng.getstate()
    # ... which is the stream of get_example, one example after the other
    ref.reseed(5)
    ds.reseed(5)
    for i in indices:
        ref.get_example(i)
    ds.decode_batch(indices)
    assert ds._aug_rng.getstate() == ref._aug_rng.getstate()
    if where == 'host':                                             # the misses were kept as they were decoded
        assert len(cache) == 5 and cache.bytes == sum(nbytes(i) for i in range(5))


def test_without_a_cache_the_host_half_is_what_it_was(tmp_path):
    path = write_set(str(tmp_path))
    ds = ClassificationImageDataset(path, str(tmp_path), image_size=(16, 12), augment_seed=1)
    assert ds.cache is None and len(ds.decode_batch([0, 1])) == 3


def test_a_shard_hands_out_its_bases_cache(tmp_path):
    path = write_set(str(tmp_path))
    cache = RaggedFrameCache(10 ** 6, 'host')
    shard = ShardedDataset(ClassificationImageDataset(path, str(tmp_path), cache=cache), 1, 2, pad=True)
    assert shard.cache is cache
    shard.decode_batch([0, 1, 2])                                   # base indices 1, 3, 0: the cache is keyed by those
    assert cache.lookup(3) is not None and cache.lookup(2) is None
    assert not hasattr(ShardedDataset([1, 2, 3], 0, 1, pad=False), 'cache')


# ---- the trainer's options --------------------------------------------------------------------------------------------------------
def test_trainer_options():
    import train_imagenet as T
    new = ('frame_cache_gb', 'frame_cache_where')
    bare = T.parse_args([])
    assert not set(new) & set(vars(bare)) and (bare.frame_cache_gb, bare.frame_cache_where) == (0.0, 'device')
    assert set(T.Arguments._CACHE) == set(new)
    a = T.parse_args(['train.tsv', 'val.tsv', '--augment', 'rrc', '--frame-cache-gb', '1.5'])
    assert (a.frame_cache_gb, a.frame_cache_where) == (1.5, 'device')
    a = T.parse_args(['train.tsv', '--augment', 'rrc', '--frame-cache-gb', '200', '--frame-cache-where', 'host'])
    assert (a.frame_cache_gb, a.frame_cache_where) == (200.0, 'host')
    assert T.parse_args(['--frame-cache-where', 'host']).frame_cache_gb == 0.0         # off: nothing to reject
    for argv in (['train.tsv', 'val.tsv', '--frame-cache-gb', '1'],                     # no --augment rrc
                 ['train.tsv', 'val.tsv', '--augment', 'none', '--frame-cache-gb', '1'],
                 ['--augment', 'rrc', '--frame-cache-gb', '1'],                         # no files
                 ['train.tsv', '--augment', 'rrc', '--frame-cache-gb', '-1'],
                 ['train.tsv', '--augment', 'rrc', '--frame-cache-gb', '1', '--frame-cache-where', 'disk']):
        with pytest.raises(SystemExit):
            T.parse_args(argv)
    # a namespace that did not come from the command line is held to the same
    a = T.parse_args(['--augment', 'rrc'])
    a.frame_cache_gb = 2.0
    with pytest.raises(ValueError, match='train_file'):
        T.check_cache_arguments(a)
    a.train_file, a.augment = 'train.tsv', 'none'
    with pytest.raises(ValueError, match='--augment rrc'):
        T.check_cache_arguments(a)
    # the split of the budget: by the sets' numbers of examples, nothing lost
    assert T.cache_budgets(1300, 1200, 100) == (1200, 100) and T.cache_budgets(1000, 10, 0) == (1000, 0)
    assert sum(T.cache_budgets(10 ** 9 + 7, 1281167, 50000)) == 10 ** 9 + 7


def test_the_trainer_gives_each_set_a_cache_of_its_own(tmp_path):
    import train_imagenet as T
    train = write_set(str(tmp_path), name='train')
    val = write_set(str(tmp_path), SIZES[:2], name='val')
    args = T.parse_args([train, val, '--augment', 'rrc', '--frame-cache-gb', '0.7', '--frame-cache-where', 'host'])
    tr, va = T.build_crop_datasets(args, 'cpu')
    assert tr.cache is not va.cache and (tr.cache.where, va.cache.where) == ('host', 'host')
    assert (tr.cache.budget, va.cache.budget) == (500000000, 200000000)                 # 5 : 2 examples
    tr, va = T.build_crop_datasets(T.parse_args([train, val, '--augment', 'rrc']), 'cpu')
    assert tr.cache is None and va.cache is None
