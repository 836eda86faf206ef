"""-m gpu: ``PhotometricBatches`` over an HBM-resident source behind the feeding iterator -- the device batch against
``apply_host`` of the dataset's own host examples under the same draws, the mix behind it against the host mix of that, and the
draw state of a checkpoint."""
import json

import numpy as np
import pytest
import torch

from loans_amd.common.datasets import batch_mix as BM
from loans_amd.common.datasets import photometric as P
from loans_amd.common.datasets.classification_dataset import FeedBatch, ResidentClassificationSource
from loans_amd.common.datasets.shard import ShardedDataset
from loans_amd.mixed_labels import MixedLabels
from loans_amd.runtime import checkpoint, training
from tests.imagenet_mix import reference as XM
from tests.imagenet_photo import reference as X

pytestmark = pytest.mark.gpu

OUT = (32, 32)
BATCH = 3
PHOTO = dict(brightness=0.4, contrast=0.4, saturation=0.4, lighting_std=0.1, erase_prob=0.5)
MIX = dict(mixup_alpha=0.4, cutmix_alpha=1.0, prob=0.75, switch_prob=0.5)
PHOTO_SEED, MIX_SEED = 7, 5


def _source(augment_seed):
    rng = np.random.RandomState(3)
    frames = rng.randint(0, 256, (6, 40, 36, 3)).astype(np.uint8)
    return ResidentClassificationSource(frames, np.array([4, 0, 3, 1, 5, 2]), 'cuda', image_size=OUT, train=True, augment_seed=augment_seed)


def _photo(augment_seed=2, photo_seed=PHOTO_SEED):
    return P.PhotometricBatches(ShardedDataset(_source(augment_seed), 0, 1, pad=True), P.PhotoPolicy(seed=photo_seed, **PHOTO))


def _mixed(augment_seed=2, photo_seed=PHOTO_SEED, mix_seed=MIX_SEED):
    return BM.MixedBatches(_photo(augment_seed, photo_seed), BM.MixPolicy(seed=mix_seed, **MIX))


def _iterator(dataset):
    return training.MultithreadIterator(dataset, BATCH, shuffle=False, n_threads=1, device=torch.cuda.current_device())


def _take(it, n, states=None):
    out = []
    for _ in range(n):
        batch = next(it)
        x, labels = training.identity_converter(batch)
        assert isinstance(batch, (tuple, FeedBatch))            # the inner dataset's own batch object, handed on
        assert x.is_cuda and x.dtype == torch.float32 and tuple(x.shape) == (BATCH, 3) + OUT and x.is_contiguous()
        out.append((x.cpu().numpy(), labels))
        if states is not None:
            states.append(it.state_dict())
    return out


def _host_batches(n):
    """(cropped stack, labels, jobs) of the first n batches from the host side of the same streams"""
    host, policy = _source(2), P.PhotoPolicy(seed=PHOTO_SEED, **PHOTO)
    for k in range(n):
        examples = [host.get_example((BATCH * k + j) % 6) for j in range(BATCH)]
        yield np.stack([e[0] for e in examples]), np.array([e[1] for e in examples], np.int32), policy.draw_batch(BATCH, *OUT)


def test_device_batches_equal_apply_host_of_the_cropped_batch_and_the_state_continues_them():
    states = []
    it = _iterator(_photo())
    try:
        got = _take(it, 4, states)
    finally:
        it.finalize()
    worst, erased, exact = 0.0, 0, 0
    for n, ((x, labels), (stack, t, jobs)) in enumerate(zip(got, _host_batches(4))):
        assert labels.dtype == torch.int32 and np.array_equal(labels.cpu().numpy(), t)
        want = P.apply_host(stack, jobs)
        out64, copies, bound = X.photo_ref(stack, jobs)
        assert np.array_equal(x.view(np.uint32)[copies], want.view(np.uint32)[copies]), n
        assert np.all(np.abs(x.astype(np.float64) - want.astype(np.float64)) <= bound), n       # against the restatement
        err = np.abs(x.astype(np.float64) - out64)
        assert np.all(err <= bound), n                                                          # against float64
        worst = max(worst, float((err[~copies] / bound[~copies]).max()))
        erased += int(copies.any())
        exact += int(np.array_equal(x.view(np.uint32), want.view(np.uint32)))
        assert not np.array_equal(x, stack), n                  # something was changed
    assert erased > 0
    print('worst error / bound %.3f; %d of 4 batches equal the restatement bit for bit' % (worst, exact))

    # two iterators, one pair of seeds: the same batches; another photo seed: the same crops, another stage
    it = _iterator(_photo())
    try:
        again = _take(it, 4)
    finally:
        it.finalize()
    assert all(np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) for a, b in zip(again, got))
    it = _iterator(_photo(photo_seed=PHOTO_SEED + 1))
    try:
        other = _take(it, 2)
    finally:
        it.finalize()
    assert not any(np.array_equal(a[0], b[0]) for a, b in zip(other, got))

    # the state behind batch 2, through a checkpoint's record, in a fresh iterator over fresh streams: batches 3 and 4
    arrays = {}
    packed = json.loads(json.dumps(checkpoint.pack(states[1], 'it', arrays)))
    arrays = {k: np.asarray(v) for k, v in arrays.items()}
    it = _iterator(_photo(augment_seed=None, photo_seed=None))
    try:
        it.load_state_dict(checkpoint.unpack(packed, arrays))
        rest = _take(it, 2)
    finally:
        it.finalize()
    assert all(np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and torch.equal(a[1], b[1]) for a, b in zip(rest, got[2:]))


def test_the_mix_behind_the_stage_equals_the_host_mix_of_the_restatement():
    """a mixed element is lam a + oml b of two elements of the stage's output: its bound is the mix's own (tests/imagenet_mix)
    on the float64 stage output plus what the two inputs bring along, lam e_a + oml e_b; a copy carries its source's bound"""
    it = _iterator(_mixed())
    try:
        got = _take(it, 4)
    finally:
        it.finalize()
    policy = BM.MixPolicy(seed=MIX_SEED, **MIX)
    modes = []
    for n, ((x, labels), (stack, t, jobs)) in enumerate(zip(got, _host_batches(4))):
        draw = policy.draw(*OUT)
        modes.append(draw.mode)
        assert isinstance(labels, MixedLabels) and labels.lam == draw.weight
        np.testing.assert_array_equal(labels.t_a.cpu().numpy(), t)
        np.testing.assert_array_equal(labels.t_b.cpu().numpy(), np.roll(t, 1))
        out64, copies, bound = X.photo_ref(stack, jobs)
        want, blended, mix_bound = XM.batch_mix_ref(out64, 1, draw.lam32, draw.oml32, draw.box)
        y0, x0, y1, x1 = draw.box
        inside = np.zeros(out64.shape, bool)
        inside[:, :, y0:y1, x0:x1] = True
        carried = np.where(inside, np.roll(bound, 1, axis=0),
                           bound if draw.oml32 == 0.0 else abs(draw.lam32) * bound + abs(draw.oml32) * np.roll(bound, 1, axis=0))
        err = np.abs(x.astype(np.float64) - want)
        assert np.all(err <= mix_bound + carried * (1 + 2 * X.U)), (n, draw)
        # and against the host mix of the fp32 restatement, where the stage's bits agree
        host = P.apply_host(stack, jobs)
        mixed, _, host_bound = XM.batch_mix_ref(host, 1, draw.lam32, draw.oml32, draw.box)
        assert np.all(np.abs(x.astype(np.float64) - mixed) <= host_bound + 2 * carried), (n, draw)
    assert {'mixup', 'cutmix'} <= set(modes), modes
