"""Resumable training, the host side: iterator and draw-stream state round trips, the checkpoint files' protocol and the two
trainers' ``--resume`` argument checks.  No GPU."""
import json
import os
import random
import time

import numpy as np
import pytest

from loans_amd.common.datasets.shard import ShardedDataset
from loans_amd.runtime import checkpoint, training


# ---- 1. iterators -------------------------------------------------------------------------------------------------------------------
class Toy:
    """ten examples (index, one draw from the dataset's own stream), drawn in index order like the image datasets'"""

    def __init__(self, seed):
        self._aug_rng = random.Random(seed)

    def __len__(self):
        return 10

    def get_examples(self, indices, map_fn=map):
        return [(int(i), self._aug_rng.random()) for i in indices]

    def __getitem__(self, i):
        return self.get_examples([i])[0]

    def draw_state(self):
        return self._aug_rng.getstate()

    def set_draw_state(self, state):
        self._aug_rng.setstate(state)


def _make(kind, dataset, shuffle, n_prefetch, seed):
    if kind == 'serial':
        return training.SerialIterator(dataset, 4, shuffle=shuffle, seed=seed)
    return training.MultithreadIterator(dataset, 4, shuffle=shuffle, seed=seed, n_threads=2, n_prefetch=n_prefetch, device=None)


def _take(it, n):
    """n batches with everything they are handed out with"""
    out = []
    for _ in range(n):
        batch = next(it)
        out.append(([e[0] for e in batch], [e[1] for e in batch], it.epoch, it.is_new_epoch, it.epoch_detail))
    return out


def _ahead(it):
    """wait until the producer of a threaded iterator has filled its queue: it is then n_prefetch batches (and the ones in
    flight) ahead of the consumer"""
    if getattr(it, '_queue', None) is None:
        return
    deadline = time.time() + 5
    while not it._queue.full():
        assert time.time() < deadline, 'the producer never ran ahead'
        time.sleep(0.002)
    time.sleep(0.01)


def _through_a_file(state, tmp_path):
    """the state as a checkpoint's rank record keeps it: packed, written, read back"""
    path = str(tmp_path / 'record.npz')
    arrays = {}
    arrays['rank'] = np.array(json.dumps(checkpoint.pack(state, 'rank', arrays)))
    checkpoint.write_atomic(path, arrays)
    return checkpoint.read_record(path)


def _close(*iterators):
    for it in iterators:
        if hasattr(it, 'finalize'):
            it.finalize()


CASES = [('serial', 1)] + [('threads', p) for p in (1, 4)]


@pytest.mark.parametrize('k', [0, 1, 2, 3, 5])
@pytest.mark.parametrize('shuffle', [True, False], ids=['shuffle', 'in-order'])
@pytest.mark.parametrize('kind,n_prefetch', CASES, ids=['serial', 'threads-prefetch1', 'threads-prefetch4'])
def test_iterator_state_round_trip(kind, n_prefetch, shuffle, k, tmp_path):
    """batches of 4 over 10 examples straddle the epoch boundary (batch 3 ends epoch 1, batch 5 epoch 2); the state after k
    batches, loaded into a fresh iterator over a fresh dataset of another seed, continues with exactly the batches, draws and
    epoch values of the iterator that went on; the state after k - 1 batches does not"""
    a = _make(kind, Toy(1), shuffle, n_prefetch, seed=5)
    before = None
    if k > 0:
        _take(a, k - 1)
        _ahead(a)
        before = _through_a_file(a.state_dict(), tmp_path)
        _take(a, 1)
    elif kind == 'threads':
        assert a.state_dict()['pos'] == 0           # before any batch: the initial state
    _ahead(a)
    state = _through_a_file(a.state_dict(), tmp_path)
    want = _take(a, 6)

    b = _make(kind, Toy(99), shuffle, n_prefetch, seed=77)
    b.load_state_dict(state)
    assert (b.epoch, b.is_new_epoch) == ((0, False) if k == 0 else (k * 4 // 10, k in (3, 5)))
    got = _take(b, 6)
    assert got == want
    assert [w[2] for w in want] == [(k + j + 1) * 4 // 10 for j in range(6)]            # the epochs of an uninterrupted run

    if before is not None:
        c = _make(kind, Toy(99), shuffle, n_prefetch, seed=77)
        c.load_state_dict(before)
        wrong = _take(c, 6)
        assert [w[0] for w in wrong] != [w[0] for w in want] and [w[1] for w in wrong] != [w[1] for w in want]
        assert wrong[1:] == want[:5]                # one batch behind, and from there the same sequence
        _close(c)
    _close(a, b)


def test_threaded_iterator_refuses_a_load_while_it_runs():
    it = _make('threads', Toy(1), True, 2, seed=5)
    state = it.state_dict()
    next(it)
    with pytest.raises(RuntimeError, match='producer'):
        it.load_state_dict(state)
    it.reset()
    it.load_state_dict(state)
    short = training.SerialIterator(list(range(7)), 4)
    with pytest.raises(ValueError, match='order'):
        short.load_state_dict(state)
    _close(it)


# ---- 2. the crop / mirror draws --------------------------------------------------------------------------------------------------
def _crops(seed):
    from loans_amd.common.datasets.classification_dataset import ClassificationImageDataset
    rng = np.random.RandomState(0)
    frames = [rng.randint(0, 256, (37, 53, 3) if i % 2 else (64, 48, 3)).astype(np.uint8) for i in range(6)]

    class InMemory(ClassificationImageDataset):
        def _read_u8(self, i):
            return frames[i]

    return InMemory([('frame%d' % i, i) for i in range(6)], image_size=(32, 32), train=True, augment_seed=seed)


@pytest.mark.parametrize('sharded', [False, True], ids=['whole', 'rank1of2'])
def test_crop_draw_state_round_trip(sharded, tmp_path):
    def view(ds):
        return ShardedDataset(ds, 1, 2, pad=True) if sharded else ds

    a = view(_crops(3))
    n = len(a)
    a.decode_batch(list(range(n)))
    state = _through_a_file({'draw': a.draw_state()}, tmp_path)['draw']
    want = a.decode_batch(list(range(n)) + [0])[1]
    assert len({box for box, _ in want}) > 1 and all(len(box) == 4 for box, _ in want)
    b = view(_crops(11))
    assert b.decode_batch(list(range(n)) + [0])[1] != want
    b.set_draw_state(training._as_draw_state(state))
    assert b.decode_batch(list(range(n)) + [0])[1] == want
    assert hasattr(view(_crops(1)), 'draw_state') and not hasattr(ShardedDataset(list(range(4)), 0, 2, pad=True), 'draw_state')


def test_image_dataset_draw_state_covers_both_branches():
    from loans_amd.common.datasets.image_dataset import ImageDataset
    for imgaug in (True, False):
        a = ImageDataset(['a.png'], use_imgaug=imgaug, transform_probability=0.5, image_size=(8, 8), augment_seed=4)
        a._aug_rng.random()
        b = ImageDataset(['a.png'], use_imgaug=imgaug, transform_probability=0.5, image_size=(8, 8), augment_seed=9)
        b.set_draw_state(a.draw_state())
        frame = np.zeros((3, 20, 30), np.float32)
        for _ in range(4):
            got, want = b._augment(frame, imgaug_rows=True), a._augment(frame, imgaug_rows=True)
            assert got[0].shape == want[0].shape and np.array_equal(np.asarray(got[1]), np.asarray(want[1]))


# ---- 3. the files ----------------------------------------------------------------------------------------------------------------
META = {'epoch': 0, 'elapsed_time': 1.5, 'args': {'batch_size': 4}}


def _write(log_dir, iteration, world=1, keep=2, ranks=None):
    for rank in reversed(range(world) if ranks is None else ranks):          # rank 0 last, as behind the barrier
        checkpoint.write_checkpoint(str(log_dir), iteration, {'payload': np.arange(1000.0) + iteration},
                                    {'rank': rank, 'stream': (3, (1, 2, 3), None), 'order': np.arange(5)}, META, rank, world, keep)
    return checkpoint.common_path(str(log_dir), iteration)


def test_checkpoint_is_replaced_atomically_and_leftovers_are_ignored(tmp_path, monkeypatch):
    first = _write(tmp_path, 3)
    with open(str(tmp_path / 'checkpoint_9.npz.tmp4242'), 'wb') as f:      # what a process killed in mid-write leaves
        f.write(b'PK\x03\x04 half a file')
    assert checkpoint.resolve(str(tmp_path)) == first
    meta = checkpoint.read_meta(first)
    assert (meta['format'], meta['iteration'], meta['world_size'], meta['elapsed_time']) == (checkpoint.FORMAT, 3, 1, 1.5)
    record = checkpoint.read_record(first)
    assert record['stream'] == (3, (1, 2, 3), None) and np.array_equal(record['order'], np.arange(5))

    # killed between the write and the move: the previous checkpoint stays intact and loadable, and stays the newest
    def killed(src, dst):
        raise KeyboardInterrupt
    monkeypatch.setattr(os, 'replace', killed)
    with pytest.raises(KeyboardInterrupt):
        _write(tmp_path, 6)
    monkeypatch.undo()
    assert not os.path.exists(checkpoint.common_path(str(tmp_path), 6))
    assert checkpoint.resolve(str(tmp_path)) == first
    with np.load(first) as handle:
        assert np.array_equal(handle['payload'], np.arange(1000.0) + 3)


def test_keep_two_leaves_two(tmp_path):
    for iteration in (2, 4, 6, 8):
        _write(tmp_path, iteration, world=2)
    names = sorted(os.listdir(str(tmp_path)))
    assert names == ['checkpoint_6.npz', 'checkpoint_6.rank1.npz', 'checkpoint_8.npz', 'checkpoint_8.rank1.npz']
    _write(tmp_path, 10, keep=1)
    assert sorted(os.listdir(str(tmp_path))) == ['checkpoint_10.npz']


def test_directory_resolves_to_the_newest_complete_checkpoint(tmp_path):
    _write(tmp_path, 5, keep=5)
    _write(tmp_path, 10, keep=5)
    newest = _write(tmp_path, 15, keep=5)
    said = []
    assert checkpoint.resolve(str(tmp_path), said.append) == newest and not said
    assert checkpoint.resolve(newest) == newest
    # the newest one truncated: the one before it, and a word about it
    size = os.path.getsize(newest)
    with open(newest, 'r+b') as f:
        f.truncate(size // 2)
    assert checkpoint.resolve(str(tmp_path), said.append) == checkpoint.common_path(str(tmp_path), 10)
    assert len(said) == 1 and 'checkpoint_15.npz' in said[0] and 'falling back' in said[0]
    with pytest.raises(ValueError, match='not a complete checkpoint'):
        checkpoint.resolve(newest)
    with pytest.raises(ValueError, match='no such checkpoint'):
        checkpoint.resolve(str(tmp_path / 'nowhere'))
    os.makedirs(str(tmp_path / 'empty'))
    with pytest.raises(ValueError, match='no complete checkpoint'):
        checkpoint.resolve(str(tmp_path / 'empty'))


def test_a_missing_rank_record_makes_a_checkpoint_incomplete(tmp_path):
    whole = _write(tmp_path, 4, world=3, keep=5)
    assert checkpoint.is_complete(whole)[0]
    assert checkpoint.read_record(whole, 2)['rank'] == 2 and checkpoint.read_record(whole, 0)['rank'] == 0
    partial = _write(tmp_path, 8, world=3, keep=5, ranks=(0, 1))          # rank 2 never wrote
    ok, why = checkpoint.is_complete(partial)
    assert not ok and 'rank 2' in why
    said = []
    assert checkpoint.resolve(str(tmp_path), said.append) == whole and 'rank 2' in said[0]
    os.remove(checkpoint.rank_path(str(tmp_path), 4, 1))
    with pytest.raises(ValueError, match='no complete checkpoint'):
        checkpoint.resolve(str(tmp_path), said.append)


# ---- 4. the parsers --------------------------------------------------------------------------------------------------------------
def _trainer(name):
    import importlib
    return importlib.import_module(name)


@pytest.mark.parametrize('name', ['train_imagenet', 'train_sheep_localizer'])
def test_resume_arguments(name, tmp_path, capsys):
    T = _trainer(name)
    base = ['--use-resnet-18', '-b', '4', '--image-size', '64', '64', '--seed', '0']
    saved = T.parse_args(base + ['--num-epoch', '3', '--checkpoint-interval', '5'])
    assert (saved.checkpoint_interval, saved.checkpoint_keep, saved.resume) == (5, 2, None)
    assert (T.parse_args(base).checkpoint_interval, T.parse_args(base + ['--checkpoint-keep', '7']).checkpoint_keep) == (0, 7)
    log_dir = str(tmp_path / 'run')
    os.makedirs(log_dir)
    path = checkpoint.write_checkpoint(log_dir, 5, {}, {}, {'epoch': 0, 'elapsed_time': 2.0, 'args': checkpoint.plain_arguments(saved)})

    with pytest.raises(SystemExit):
        T.parse_args(base + ['--resume', str(tmp_path / 'nowhere')])
    assert 'nowhere' in capsys.readouterr().err

    with pytest.raises(SystemExit):
        T.parse_args(['--use-resnet-18', '-b', '8', '--image-size', '64', '64', '--seed', '0', '--dtype', 'bf16', '--resume', log_dir])
    err = capsys.readouterr().err
    line = [l for l in err.splitlines() if 'batch_size' in l]
    assert len(line) == 1 and 'dtype' in line[0], err                 # one error, both arguments, both values
    assert '4' in line[0] and '8' in line[0] and "'f32'" in line[0] and "'bf16'" in line[0]
    assert 'image_size' not in err and 'seed' not in line[0].replace('data_seed', '')

    with pytest.raises(SystemExit):
        T.parse_args(base + ['--gpus', '2', '--resume', log_dir])
    assert 'resume it with --gpus 1, not 2' in capsys.readouterr().err

    for where in (log_dir, path):                                       # a directory or the file itself; --num-epoch may change
        args = T.parse_args(base + ['--num-epoch', '7', '--iterations', '9', '--resume', where])
        assert args.resume == path and args.num_epoch == 7
    changed = checkpoint.check_arguments(checkpoint.plain_arguments(saved), args, T.RESUME_FIXED, checkpoint.SILENT)
    assert sorted(l.split()[1] for l in changed) == ['checkpoint_interval', 'iterations', 'num_epoch']
