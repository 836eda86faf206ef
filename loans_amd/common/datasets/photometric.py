"""Colour jitter, AlexNet-style PCA lighting noise and random erasing for the device feed of the ImageNet pre-training arm -- the
"photometric" stage, between the crop and the mix, on training batches only: the draws on the host (``PhotoPolicy``), the pixels on
the GPU (``ops.photometric``, csrc/photo.hip), the wrapper that puts both between a dataset and ``MixedBatches`` /
``MultithreadIterator`` (``PhotometricBatches``), and the arithmetic restated in NumPy fp32 (``apply_host``).  Hue is not built.

THE ARITHMETIC.  Frames are fp32 [B][3][H][W] in [0, 1].  Every image of a batch has one job (``ops.PHOTO_JOB``, the mirror of
``loans_photo_job``): factors ``b``, ``c``, ``s`` (fp32) with ``omc = fl32(1 - c)`` and ``oms = fl32(1 - s)``, both rounded once
on the host the way ``MixedLabels.weights`` rounds; an order code 0..5 (``ORDERS``: a permutation of brightness, contrast,
saturation); an RGB addend ``add``; an erase box ``(y0, x0, y1, x1)``, possibly empty, with an RGB ``fill``.  One pixel's three
channels are worked on together, every multiply-add one fused operation:
    grey(r, g, b) = fma(0.299, r, fma(0.587, g, 0.114 * b))
    brightness      x = clamp01(b * x)
    saturation      x = clamp01(fma(s, x, oms * grey(pixel)))
    contrast        x = clamp01(fma(c, x, cm)),  cm = omc * m
where ``m`` is the image's mean grey AS IT STANDS WHEN CONTRAST IS REACHED -- after the operations that precede contrast in this
image's order --: the per-pixel greys summed in fp64 in a fixed order, divided by H W in fp64, rounded once to fp32.  A factor
that is exactly 1 skips its operation altogether: no clamp, the values are a bit copy.  After the three operations, if any addend
is non-zero, ``x = x + add[channel]`` with no clamp (the lighting noise, as in fb.resnet.torch).  Last, every pixel inside the
erase box becomes ``fill[channel]``, a bit copy.  An image with all three factors 1, a zero addend and an empty box leaves the
stage bit for bit.

THE DRAW of one example of an H x W batch, from the policy's own ``random.Random`` (the crops and the mix draws of a run do not
depend on whether this stage is on), in this order:
  1. the order: if any jitter strength is > 0, ONE ``shuffle`` of ``[0, 1, 2]`` (0 brightness, 1 contrast, 2 saturation); the
     order code is the permutation's index in ``ORDERS``.  Otherwise code 0, no draw.
  2. the factors: for each strength v > 0, in the order brightness, contrast, saturation, ``uniform(max(0, 1 - v), 1 + v)``,
     rounded to fp32; a strength of 0 is the factor 1, no draw.
  3. the lighting: if ``lighting_std > 0``, three ``gauss(0, std)`` values alpha; ``add = V (alpha * lambda)`` in fp64, rounded to
     fp32, with ``LIGHTING_EIGVAL`` and the rows of ``LIGHTING_EIGVEC``.
  4. the erase: if ``erase_prob > 0``, ``random()``; below ``erase_prob`` up to ten attempts, each drawing
     ``area = H W uniform(scale)``, ``ar = exp(uniform(log ratio))``, ``h = int(round(sqrt(area * ar)))``,
     ``w = int(round(sqrt(area / ar)))`` and, if ``h < H and w < W``, ``y = randint(0, H - h)`` then ``x = randint(0, W - w)`` --
     the box is ``(y, x, y + h, x + w)`` and the attempts end.  After ten failures there is no box (torchvision's
     ``RandomErasing``)."""
import math
import random

import numpy as np

from ... import ops
from ...ops import PHOTO_JOB
from .batch_mix import _image_size

# order code -> the operations in the order they are applied: 0 brightness, 1 contrast, 2 saturation
ORDERS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))
BRIGHTNESS, CONTRAST, SATURATION = 0, 1, 2
GREY = (0.299, 0.587, 0.114)
LIGHTING_EIGVAL = (0.2175, 0.0188, 0.0045)
LIGHTING_EIGVEC = ((-0.5675, 0.7192, 0.4009), (-0.5808, -0.0045, -0.8140), (-0.5836, -0.6948, 0.4203))
IMAGENET_MEAN = (0.485, 0.456, 0.406)
ERASE_ATTEMPTS = 10


def complement32(v):
    """(float32(v), float32(1 - float32(v))) as NumPy scalars: a factor and its complement, each rounded once"""
    v32 = np.float32(v)
    return v32, np.float32(1.0) - v32


def make_job(b=1.0, c=1.0, s=1.0, order=0, add=(0.0, 0.0, 0.0), box=(0, 0, 0, 0), fill=IMAGENET_MEAN):
    """one ``PHOTO_JOB`` record (a 0-d array) from plain numbers; the complements are formed here"""
    job = np.zeros((), PHOTO_JOB)
    job['b'] = np.float32(b)
    job['c'], job['omc'] = complement32(c)
    job['s'], job['oms'] = complement32(s)
    job['order'] = order
    job['add'] = np.asarray(add, np.float64).astype(np.float32)
    job['y0'], job['x0'], job['y1'], job['x1'] = box
    job['fill'] = np.asarray(fill, np.float64).astype(np.float32)
    return job


def lighting_addend(alpha):
    """step 3 above: ``V (alpha * lambda)`` in fp64, each row summed from the left; ``alpha``: three numbers, or [n][3] -> [n][3]"""
    alpha = np.asarray(alpha, np.float64)
    scaled = [alpha[..., k] * LIGHTING_EIGVAL[k] for k in range(3)]
    return np.stack([row[0] * scaled[0] + row[1] * scaled[1] + row[2] * scaled[2] for row in LIGHTING_EIGVEC], axis=-1)


class PhotoPolicy:

    def __init__(self, brightness=0.0, contrast=0.0, saturation=0.0, lighting_std=0.0, erase_prob=0.0, erase_scale=(0.02, 0.33),
                 erase_ratio=(0.3, 3.3), erase_value=IMAGENET_MEAN, seed=None):
        strengths = (brightness, contrast, saturation)
        if not all(v >= 0 for v in strengths) or not lighting_std >= 0:
            raise ValueError('the jitter strengths and the lighting deviation must not be negative, got %r and %r' % (strengths, lighting_std))
        if not 0.0 <= erase_prob <= 1.0:
            raise ValueError('the erase probability must lie in [0, 1], got %r' % (erase_prob,))
        for name, pair in (('scale', erase_scale), ('ratio', erase_ratio)):
            if len(pair) != 2 or not 0 < pair[0] <= pair[1]:
                raise ValueError('the erase %s must be a positive, ordered pair, got %r' % (name, tuple(pair)))
        if len(erase_value) != 3 or not all(math.isfinite(v) for v in erase_value):
            raise ValueError('the erase value must be three finite numbers, got %r' % (tuple(erase_value),))
        self.strengths = tuple(float(v) for v in strengths)
        self.lighting_std, self.erase_prob = float(lighting_std), float(erase_prob)
        self.erase_scale = (float(erase_scale[0]), float(erase_scale[1]))
        self.erase_ratio = (float(erase_ratio[0]), float(erase_ratio[1]))
        self.erase_value = tuple(float(v) for v in erase_value)
        self._rng = random.Random(seed)
        # what a draw reads, made once: the draws run beside the thread that enqueues the step
        self._ranges = tuple((k, max(0.0, 1.0 - v), 1.0 + v) for k, v in enumerate(self.strengths) if v > 0)
        self._log_ratio = (math.log(self.erase_ratio[0]), math.log(self.erase_ratio[1]))
        self._order_code = {perm: code for code, perm in enumerate(ORDERS)}

    @property
    def active(self):
        return any(v > 0 for v in self.strengths) or self.lighting_std > 0 or self.erase_prob > 0

    def reseed(self, seed):
        self._rng = random.Random(seed)

    def getstate(self):
        return self._rng.getstate()

    def setstate(self, state):
        self._rng.setstate(state)

    def erase_box(self, H, W):
        """step 4 above behind the ``random()`` that decided to erase: (y0, x0, y1, x1), or the empty box after ten failures"""
        rng = self._rng
        log_lo, log_hi = self._log_ratio
        for _ in range(ERASE_ATTEMPTS):
            area = H * W * rng.uniform(self.erase_scale[0], self.erase_scale[1])
            ar = math.exp(rng.uniform(log_lo, log_hi))
            h = int(round(math.sqrt(area * ar)))
            w = int(round(math.sqrt(area / ar)))
            if h < H and w < W:
                y = rng.randint(0, H - h)
                x = rng.randint(0, W - w)
                return y, x, y + h, x + w
        return 0, 0, 0, 0

    def _draw(self, H, W):
        """the module docstring's four steps in plain numbers: (order, b, c, s, alpha0, alpha1, alpha2, y0, x0, y1, x1)"""
        rng = self._rng
        order, factors, alpha, box = 0, [1.0, 1.0, 1.0], (0.0, 0.0, 0.0), (0, 0, 0, 0)
        if self._ranges:
            perm = [0, 1, 2]
            rng.shuffle(perm)
            order = self._order_code[tuple(perm)]
            for k, lo, hi in self._ranges:
                factors[k] = rng.uniform(lo, hi)
        if self.lighting_std > 0:
            std = self.lighting_std
            alpha = (rng.gauss(0.0, std), rng.gauss(0.0, std), rng.gauss(0.0, std))
        if self.erase_prob > 0 and rng.random() < self.erase_prob:
            box = self.erase_box(H, W)
        return (order, factors[0], factors[1], factors[2]) + alpha + box

    def draw(self, H, W):
        """the job of the next example: a 0-d ``PHOTO_JOB`` record"""
        return self.draw_batch(1, H, W)[0]

    def draw_batch(self, n, H, W):
        """the jobs of a batch of ``n`` examples, in batch order: n draws, the table filled a column at a time (the draws run on
        the feed's decode thread beside the thread that enqueues the step: a record at a time cost 40 ms of interpreter per batch
        of 256, this costs about one)"""
        jobs = np.zeros(n, PHOTO_JOB)
        if n == 0:
            return jobs
        rows = np.array([self._draw(H, W) for _ in range(n)], np.float64)          # (the integers among them are exact)
        factors = rows[:, 1:4].astype(np.float32)
        jobs['b'], jobs['c'], jobs['s'] = factors[:, BRIGHTNESS], factors[:, CONTRAST], factors[:, SATURATION]
        jobs['omc'], jobs['oms'] = np.float32(1.0) - factors[:, CONTRAST], np.float32(1.0) - factors[:, SATURATION]
        jobs['order'] = rows[:, 0].astype(np.int32)
        if self.lighting_std > 0:
            jobs['add'] = lighting_addend(rows[:, 4:7]).astype(np.float32)
        jobs['y0'], jobs['x0'], jobs['y1'], jobs['x1'] = (rows[:, k].astype(np.int32) for k in (7, 8, 9, 10))
        jobs['fill'] = np.asarray(self.erase_value, np.float64).astype(np.float32)
        return jobs


def _grey32(r, g, b):
    """grey() in fp32 with the kernel's rounding points: each fma rounds once (formed in fp64, which holds the exact product and,
    to well below half an fp32 ulp, the sum)"""
    f = np.float32
    t = (f(GREY[2]) * b).astype(f)
    t = (np.float64(f(GREY[1])) * g.astype(np.float64) + t.astype(np.float64)).astype(f)
    return (np.float64(f(GREY[0])) * r.astype(np.float64) + t.astype(np.float64)).astype(f)


def _fma32(a, x, t):
    return (np.float64(a) * x.astype(np.float64) + np.asarray(t, np.float64)).astype(np.float32)


def _clamp01(x):
    return np.minimum(np.maximum(x, np.float32(0)), np.float32(1))


def apply_host(frames, jobs):
    """the stage in NumPy fp32 with the module docstring's rounding points: frames [B][3][H][W] float32 and a ``PHOTO_JOB`` table
    -> a new array.  (An fma is formed in fp64 and rounded to fp32: the product of two fp32 numbers is exact there, and the
    second rounding of the sum moves the result only where the fp64 sum lies within 2^-29 ulp of an fp32 tie.)"""
    frames = np.asarray(frames)
    if frames.dtype != np.float32 or frames.ndim != 4 or frames.shape[1] != 3 or len(jobs) != len(frames):
        raise ValueError('frames must be float32 [B][3][H][W] with one job per image')
    f = np.float32
    out = frames.copy()
    H, W = frames.shape[2:]
    for n, j in enumerate(jobs):
        px = out[n]                                         # [3][H][W], changed in place
        for op in ORDERS[int(j['order'])]:
            if op == BRIGHTNESS and j['b'] != 1:
                px[:] = _clamp01((f(j['b']) * px).astype(f))
            elif op == SATURATION and j['s'] != 1:
                t = (f(j['oms']) * _grey32(px[0], px[1], px[2])).astype(f)
                px[:] = _clamp01(_fma32(j['s'], px, t[None]))
            elif op == CONTRAST and j['c'] != 1:
                m = f(_grey32(px[0], px[1], px[2]).astype(np.float64).sum() / float(H * W))
                cm = f(f(j['omc']) * m)
                px[:] = _clamp01(_fma32(j['c'], px, cm))
        if j['add'].any():
            px[:] = (px + j['add'].astype(f)[:, None, None]).astype(f)
        y0, x0, y1, x1 = (int(j[k]) for k in ('y0', 'x0', 'y1', 'x1'))
        if y1 > y0 and x1 > x0:
            px[:, y0:y1, x0:x1] = j['fill'].astype(f)[:, None, None]
    return out


class PhotometricBatches:
    """``PhotometricBatches(dataset, policy)`` around the ``ShardedDataset`` of a device feed, inside ``MixedBatches`` where the run
    mixes: what ``MultithreadIterator(device=...)`` sees of a dataset, with the batch's jobs drawn behind the inner dataset's
    per-example draws on the decode thread and the stage launched in place behind the crop on the feed's stream."""

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
        indices = list(indices)
        decoded = self.dataset.decode_batch(indices, map_fn) if farm is None else self.dataset.decode_batch(indices, map_fn, farm)
        return decoded, self.policy.draw_batch(len(indices), *self.image_size)

    def finish_batch(self, decoded, device, map_fn=map):
        inner, jobs = decoded
        batch = self.dataset.finish_batch(inner, device, map_fn)        # a FeedBatch with its cache_hits / cache_misses: handed on
        frames = batch[0]
        if tuple(frames.shape[2:]) != self.image_size:
            raise ValueError('the draws were taken for %r frames, the batch holds %r' % (self.image_size, tuple(frames.shape[2:])))
        if not ops.photo_identity(jobs).all():
            ops.photometric(frames, jobs, out=frames)       # in place: the crop wrote this tensor for this batch alone
        return batch

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
