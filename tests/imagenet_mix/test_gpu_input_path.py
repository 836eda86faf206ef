"""-m gpu: ``MixedBatches`` over an HBM-resident source behind the feeding iterator -- the device batch against the same mix
made on the host in float64 from the dataset's own host examples, reproducibility, and the draw state of a checkpoint."""
import json

import numpy as np
import pytest
import torch

from loans_amd.common.datasets import batch_mix as BM
from loans_amd.common.datasets.classification_dataset import FeedBatch, ResidentClassificationSource
from loans_amd.common.datasets.shard import ShardedDataset
from loans_amd.mixed_labels import MixedLabels
from loans_amd.runtime import checkpoint, training
from tests.imagenet_mix import reference as X

pytestmark = pytest.mark.gpu

OUT = (16, 12)
BATCH = 3
POLICY = dict(mixup_alpha=0.4, cutmix_alpha=1.0, prob=0.75, switch_prob=0.5)
SEED = 5            # the first four draws of this stream: mixup, nothing, CutMix, CutMix


def _source(augment_seed):
    rng = np.random.RandomState(3)
    frames = rng.randint(0, 256, (6, 20, 16, 3)).astype(np.uint8)
    return ResidentClassificationSource(frames, np.array([4, 0, 3, 1, 5, 2]), 'cuda', image_size=OUT, train=True, augment_seed=augment_seed)


def _wrapped(augment_seed=2, mix_seed=SEED):
    return BM.MixedBatches(ShardedDataset(_source(augment_seed), 0, 1, pad=True), BM.MixPolicy(seed=mix_seed, **POLICY))


def _take(it, n, states=None):
    """n batches as (frames, t_a, t_b, label weight) on the host"""
    out = []
    for _ in range(n):
        batch = next(it)
        x, labels = training.identity_converter(batch)
        assert isinstance(batch, FeedBatch) and isinstance(labels, MixedLabels)
        assert x.is_cuda and x.dtype == torch.float32 and tuple(x.shape) == (BATCH, 3) + OUT and x.is_contiguous()
        assert labels.t_a.dtype == torch.int32 and labels.t_b.dtype == torch.int32 and labels.t_a.is_cuda
        out.append((x.cpu().numpy(), labels.t_a.cpu().numpy(), labels.t_b.cpu().numpy(), labels.lam))
        if states is not None:
            states.append(it.state_dict())
    return out


def _iterator(dataset):
    return training.MultithreadIterator(dataset, BATCH, shuffle=False, n_threads=1, device=torch.cuda.current_device())


def _same(a, b):
    return all(np.array_equal(p[0], q[0]) and np.array_equal(p[1], q[1]) and np.array_equal(p[2], q[2]) and p[3] == q[3]
               for p, q in zip(a, b)) and len(a) == len(b)


def test_device_batches_equal_the_host_mix_and_the_state_continues_them():
    states = []
    it = _iterator(_wrapped())
    try:
        got = _take(it, 4, states)
    finally:
        it.finalize()

    # the same draws on the host: the wrapped dataset's own examples, stacked, mixed in float64
    host, policy = _source(2), BM.MixPolicy(seed=SEED, **POLICY)
    modes, worst = [], 0.0
    for n, (x, ta, tb, weight) in enumerate(got):
        indices = [(BATCH * n + j) % 6 for j in range(BATCH)]
        examples = [host.get_example(i) for i in indices]
        draw = policy.draw(*OUT)
        modes.append(draw.mode)
        stack = np.stack([e[0] for e in examples])
        want, blended, bound = X.batch_mix_ref(stack, 1, draw.lam32, draw.oml32, draw.box)
        err = np.abs(x.astype(np.float64) - want)
        assert np.all(err <= bound), (n, draw)
        assert np.array_equal(x[~blended], want.astype(np.float32)[~blended]), (n, draw)
        if blended.any():
            worst = max(worst, float((err[blended] / bound[blended]).max()))
        labels = np.array([e[1] for e in examples], np.int32)
        np.testing.assert_array_equal(ta, labels)
        np.testing.assert_array_equal(tb, np.roll(labels, 1))
        assert weight == draw.weight
        if draw.mode is not None and draw.weight < 1.0:
            assert not np.array_equal(x, stack), n                      # something was mixed
        else:
            np.testing.assert_array_equal(x, stack)
    assert modes == ['mixup', None, 'cutmix', 'cutmix']
    print('worst blended error / bound %.3f' % worst)

    # two iterators, one pair of seeds: the same batches; another mix seed: the same crops, another mix
    it = _iterator(_wrapped())
    try:
        assert _same(_take(it, 4), got)
    finally:
        it.finalize()
    it = _iterator(_wrapped(mix_seed=SEED + 1))
    try:
        other = _take(it, 4)
    finally:
        it.finalize()
    assert all(np.array_equal(p[1], q[1]) for p, q in zip(other, got)) and not _same(other, got)

    # the state behind batch 2, through a checkpoint's record, in a fresh iterator over fresh streams: batches 3 and 4
    arrays = {}
    packed = json.loads(json.dumps(checkpoint.pack(states[1], 'it', arrays)))
    arrays = {k: np.asarray(v) for k, v in arrays.items()}
    it = _iterator(_wrapped(augment_seed=None, mix_seed=None))
    try:
        it.load_state_dict(checkpoint.unpack(packed, arrays))
        assert _same(_take(it, 2), got[2:])
    finally:
        it.finalize()
