"""-m gpu: ``RandAugmentBatches`` over an HBM-resident source behind the feeding iterator -- the device batch against
``ops.rand_augment`` of the cropped batch under a twin policy's jobs, the draw state of a checkpoint, and the photometric stage and
the mix behind it against those stages applied to its output."""
import json

import numpy as np
import pytest
import torch

from loans_amd import ops
from loans_amd.common.datasets import batch_mix as BM
from loans_amd.common.datasets import photometric as P
from loans_amd.common.datasets import rand_augment as RA
from loans_amd.common.datasets.classification_dataset import FeedBatch, ResidentClassificationSource
from loans_amd.common.datasets.shard import ShardedDataset
from loans_amd.mixed_labels import MixedLabels
from loans_amd.runtime import checkpoint, training
from tests.gpu_util import dev

pytestmark = pytest.mark.gpu

OUT = (32, 32)
BATCH = 3
PHOTO = dict(brightness=0.4, contrast=0.4, saturation=0.4, lighting_std=0.1, erase_prob=0.5)
MIX = dict(mixup_alpha=0.4, cutmix_alpha=1.0, prob=0.75, switch_prob=0.5)
RA_SEED, PHOTO_SEED, MIX_SEED = 11, 7, 5


def _policy(kind, seed=RA_SEED):
    return RA.RandAugmentPolicy(kind, 2, 9, seed=seed)


def _crops(augment_seed=2):
    rng = np.random.RandomState(3)
    frames = rng.randint(0, 256, (6, 40, 36, 3)).astype(np.uint8)
    source = ResidentClassificationSource(frames, np.array([4, 0, 3, 1, 5, 2]), 'cuda', image_size=OUT, train=True, augment_seed=augment_seed)
    return ShardedDataset(source, 0, 1, pad=True)


def _staged(kind, augment_seed=2, ra_seed=RA_SEED):
    return RA.RandAugmentBatches(_crops(augment_seed), _policy(kind, ra_seed))


def _take(dataset, n, states=None, load=None):
    it = training.MultithreadIterator(dataset, BATCH, shuffle=False, n_threads=1, device=torch.cuda.current_device())
    out = []
    try:
        if load is not None:
            it.load_state_dict(load)
        for _ in range(n):
            batch = next(it)
            x, labels = training.identity_converter(batch)
            assert isinstance(batch, (tuple, FeedBatch))
            assert x.is_cuda and x.dtype == torch.float32 and tuple(x.shape) == (BATCH, 3) + OUT and x.is_contiguous()
            out.append((x.cpu().numpy(), labels))
            if states is not None:
                states.append(it.state_dict())
    finally:
        it.finalize()
    return out


def _same(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize('kind', ['rand', 'trivial'])
def test_device_batches_equal_the_stage_on_the_cropped_batch_and_the_state_continues_them(kind):
    states = []
    got = _take(_staged(kind), 4, states)
    cropped = _take(_crops(), 4)
    twin, changed = _policy(kind), 0
    for n, ((x, labels), (crop, t)) in enumerate(zip(got, cropped)):
        assert labels.dtype == torch.int32 and torch.equal(labels, t)
        jobs = twin.draw_batch(BATCH, *OUT)
        want = ops.rand_augment(dev(crop), jobs).cpu().numpy()
        assert _same(x, want), n
        changed += int(not _same(x, crop))
    assert changed >= 3
    # two iterators, one pair of seeds: the same batches; another seed: the same crops, another stage
    again = _take(_staged(kind), 4)
    assert all(_same(a[0], b[0]) for a, b in zip(again, got))
    other = _take(_staged(kind, ra_seed=RA_SEED + 1), 4)
    assert not all(_same(a[0], b[0]) for a, b in zip(other, got))
    # the state behind batch 2, through a checkpoint's record, in a fresh iterator over fresh streams: batches 3 and 4
    arrays = {}
    packed = json.loads(json.dumps(checkpoint.pack(states[1], 'it', arrays)))
    arrays = {k: np.asarray(v) for k, v in arrays.items()}
    rest = _take(_staged(kind, augment_seed=None, ra_seed=None), 2, load=checkpoint.unpack(packed, arrays))
    assert all(_same(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(rest, got[2:]))


def test_the_photometric_stage_and_the_mix_behind_it_work_on_its_output():
    stack = BM.MixedBatches(P.PhotometricBatches(_staged('rand'), P.PhotoPolicy(seed=PHOTO_SEED, **PHOTO)), BM.MixPolicy(seed=MIX_SEED, **MIX))
    got = _take(stack, 4)
    cropped = _take(_crops(), 4)
    ra, photo, mix = _policy('rand'), P.PhotoPolicy(seed=PHOTO_SEED, **PHOTO), BM.MixPolicy(seed=MIX_SEED, **MIX)
    mixed = 0
    for n, ((x, labels), (crop, t)) in enumerate(zip(got, cropped)):
        frames = ops.rand_augment(dev(crop), ra.draw_batch(BATCH, *OUT))
        frames = ops.photometric(frames, photo.draw_batch(BATCH, *OUT))
        draw = mix.draw(*OUT)
        assert isinstance(labels, MixedLabels) and labels.lam == draw.weight
        np.testing.assert_array_equal(labels.t_a.cpu().numpy(), t.cpu().numpy())
        empty = draw.box[2] == draw.box[0] or draw.box[3] == draw.box[1]
        if not (empty and draw.oml32 == 0.0):
            frames = ops.batch_mix(frames, BM.SHIFT % BATCH, draw.lam32, draw.oml32, draw.box)
            mixed += 1
        assert _same(x, frames.cpu().numpy()), (n, draw)
    assert mixed > 0
