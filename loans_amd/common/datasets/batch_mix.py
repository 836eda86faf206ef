"""mixup and CutMix for the device feed of the ImageNet pre-training arm: the draws on the host (``MixPolicy``), the pixels on
the GPU (``ops.batch_mix``, csrc/mix.hip), the wrapper that puts both between a dataset and ``MultithreadIterator``
(``MixedBatches``).  A batch is mixed with itself shifted by ONE row -- row b's partner is row b - 1, row 0's the last row --
with one draw per batch, and handed out as ``(frames, MixedLabels(t, roll(t, 1), weight of t))``.

THE DRAW of a batch of H x W frames, from the policy's own ``random.Random`` (not the crop stream: the crops of a run do not
depend on whether mixing is on), in this order:
  1. ``u = random()``;  ``u >= prob``: nothing is mixed -- image weights (1, 0), an empty box, label weight 1.
  2. the mode: with both alphas > 0 CutMix iff ``random() < switch_prob`` (else mixup); with one alpha > 0 that one, no draw.
  3. ``lam = betavariate(alpha, alpha)`` with the mode's alpha.
  4. mixup: image weights ``(float32(lam), float32(1 - float32(lam)))``, an empty box, label weight ``lam``.
  5. CutMix: ``r = sqrt(1 - lam)``, ``ch = int(H r)``, ``cw = int(W r)``; ``cy = randrange(H)``, then ``cx = randrange(W)``;
     the box ``y0 = max(cy - ch // 2, 0)``, ``y1 = min(cy + ch // 2, H)``, ``x0 = max(cx - cw // 2, 0)``, ``x1 = min(cx + cw // 2, W)``
     is the partner's; image weights (1, 0); label weight ``1 - (y1 - y0) (x1 - x0) / (H W)`` -- the share of the frame that
     stayed the row's own."""
import collections
import math
import random

import torch

from ... import ops
from ...mixed_labels import MixedLabels
from .classification_dataset import FeedBatch

SHIFT = 1
NO_BOX = (0, 0, 0, 0)

# mode: None (nothing mixed), 'mixup' or 'cutmix'; lam32 / oml32: the image weights; box: (y0, x0, y1, x1); weight: of the row's
# own label
MixDraw = collections.namedtuple('MixDraw', 'mode lam32 oml32 box weight')
UNMIXED = MixDraw(None, 1.0, 0.0, NO_BOX, 1.0)


def cutmix_box(lam, cy, cx, H, W):
    """step 5 above for a drawn ``lam`` and centre: ((y0, x0, y1, x1), label weight)"""
    r = math.sqrt(1.0 - lam)
    ch, cw = int(H * r), int(W * r)
    y0, y1 = max(cy - ch // 2, 0), min(cy + ch // 2, H)
    x0, x1 = max(cx - cw // 2, 0), min(cx + cw // 2, W)
    return (y0, x0, y1, x1), 1.0 - (y1 - y0) * (x1 - x0) / (H * W)


class MixPolicy:

    def __init__(self, mixup_alpha=0.0, cutmix_alpha=0.0, prob=1.0, switch_prob=0.5, seed=None):
        if mixup_alpha < 0 or cutmix_alpha < 0:
            raise ValueError('the alphas must not be negative, got %r and %r' % (mixup_alpha, cutmix_alpha))
        if not (0.0 <= prob <= 1.0 and 0.0 <= switch_prob <= 1.0):
            raise ValueError('the probabilities must lie in [0, 1], got %r and %r' % (prob, switch_prob))
        self.mixup_alpha, self.cutmix_alpha = float(mixup_alpha), float(cutmix_alpha)
        self.prob, self.switch_prob = float(prob), float(switch_prob)
        self._rng = random.Random(seed)

    @property
    def active(self):
        return self.mixup_alpha > 0 or self.cutmix_alpha > 0

    def reseed(self, seed):
        self._rng = random.Random(seed)

    def getstate(self):
        return self._rng.getstate()

    def setstate(self, state):
        self._rng.setstate(state)

    def draw(self, H, W):
        """the ``MixDraw`` of the next batch (the module docstring's five steps)"""
        rng = self._rng
        if not self.active or rng.random() >= self.prob:
            return UNMIXED
        if self.mixup_alpha > 0 and self.cutmix_alpha > 0:
            cutmix = rng.random() < self.switch_prob
        else:
            cutmix = self.cutmix_alpha > 0
        if not cutmix:
            lam = rng.betavariate(self.mixup_alpha, self.mixup_alpha)
            lam32, oml32 = MixedLabels.weights(lam)
            return MixDraw('mixup', lam32, oml32, NO_BOX, lam)
        lam = rng.betavariate(self.cutmix_alpha, self.cutmix_alpha)
        cy = rng.randrange(H)
        cx = rng.randrange(W)
        box, weight = cutmix_box(lam, cy, cx, H, W)
        return MixDraw('cutmix', 1.0, 0.0, box, weight)


def _image_size(dataset):
    """the output size of the (possibly wrapped) classification dataset"""
    while dataset is not None:
        size = dataset.__dict__.get('image_size') if hasattr(dataset, '__dict__') else None
        if size is not None:
            return int(size[0]), int(size[1])
        dataset = dataset.__dict__.get('dataset') if hasattr(dataset, '__dict__') else None
    raise ValueError('the dataset names no image_size: pass MixedBatches(..., image_size=(H, W))')


class MixedBatches:
    """``MixedBatches(dataset, policy)`` around the outermost dataset of a device feed (the ``ShardedDataset``): what
    ``MultithreadIterator(device=...)`` sees of a dataset, with the batch's mix draw taken behind its per-example draws on the
    decode thread and the mix launched behind the crop on the feed's stream."""

    def __init__(self, dataset, policy, image_size=None):
        self.dataset, self.policy = dataset, policy
        self.image_size = (int(image_size[0]), int(image_size[1])) if image_size is not None else _image_size(dataset)

    def __len__(self):
        return len(self.dataset)

    def __getattr__(self, name):
        if name == 'cache':             # the base's frame cache where it has one (hasattr() is False otherwise)
            return getattr(self.__dict__['dataset'], name)
        raise AttributeError(name)

    def decode_batch(self, indices, map_fn=map, farm=None):
        decoded = self.dataset.decode_batch(indices, map_fn) if farm is None else self.dataset.decode_batch(indices, map_fn, farm)
        return decoded, self.policy.draw(*self.image_size)

    def finish_batch(self, decoded, device, map_fn=map):
        inner, draw = decoded
        batch = self.dataset.finish_batch(inner, device, map_fn)
        frames, labels = batch
        if tuple(frames.shape[2:]) != self.image_size:
            raise ValueError('the draw was taken for %r frames, the batch holds %r' % (self.image_size, tuple(frames.shape[2:])))
        empty = draw.box[2] == draw.box[0] or draw.box[3] == draw.box[1]
        if not (empty and draw.oml32 == 0.0):           # (nothing mixed, a CutMix box of no area: the frames go through)
            frames = ops.batch_mix(frames, SHIFT % len(frames), draw.lam32, draw.oml32, draw.box)
        mixed = FeedBatch((frames, MixedLabels(labels, torch.roll(labels, SHIFT), draw.weight)))
        if isinstance(batch, FeedBatch):
            mixed.cache_hits, mixed.cache_misses = batch.cache_hits, batch.cache_misses
        return mixed

    def reseed(self, seed):
        self.dataset.reseed(seed)
        self.policy.reseed(seed)

    def draw_state(self):
        """(the wrapped dataset's draw stream, the policy's): what a checkpoint keeps"""
        return self.dataset.draw_state(), self.policy.getstate()

    def set_draw_state(self, state):
        inner, policy = state
        self.dataset.set_draw_state(inner)
        self.policy.setstate(policy)
