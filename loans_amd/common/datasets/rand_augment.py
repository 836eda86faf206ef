"""RandAugment and TrivialAugmentWide for the device feed of the ImageNet pre-training arm, between the crop and the photometric
stage, on training batches only: the draws on the host (``RandAugmentPolicy``), the pixels on the GPU (``ops.rand_augment``,
csrc/randaug.hip), the wrapper that puts both between a dataset and ``PhotometricBatches`` / ``MixedBatches`` /
``MultithreadIterator`` (``RandAugmentBatches``), and the arithmetic restated in NumPy fp32 (``apply_host``).

THE OPERATIONS.  Frames are fp32 [B][3][H][W] in [0, 1].  Every image of a batch has one job (``ops.RA_JOB``, the mirror of
``loans_ra_job``) of 1..4 layers, each one of the fourteen ``OPS`` -- the op set of torchvision's ``RandAugment`` /
``TrivialAugmentWide`` -- applied one behind the other.  The magnitude of bin k (0..30) is ``hi * k / 30`` in Python fp64, negated
for a signed op where the sign draw says so:

     #  op            hi, RandAugment           hi, TrivialAugment       signed
     0  Identity
     1  ShearX        0.3                       0.99                     yes
     2  ShearY        0.3                       0.99                     yes
     3  TranslateX    150/331 W px, int()       32 px, int()             yes
     4  TranslateY    150/331 H px, int()       32 px, int()             yes
     5  Rotate        30 degrees                135 degrees              yes
     6  Brightness    0.9                       0.99                     yes
     7  Color         0.9                       0.99                     yes
     8  Contrast      0.9                       0.99                     yes
     9  Sharpness     0.9                       0.99                     yes
    10  Posterize     bits 8 - round(k / 7.5)   bits 8 - round(k / 5)
    11  Solarize      threshold fl32(1 - k / 30), both
    12  AutoContrast
    13  Equalize

GEOMETRIC (1-5): nearest-neighbour sampling with fixed-point coordinates -- an exact integer index map that the kernel, this module
and Pillow's ``Image.transform(size, AFFINE, coef, NEAREST)`` share.  The six fp64 coefficients (a, b, c, d, e, f) of the output ->
input map, with cx = W / 2, cy = H / 2 (``coefficients``):
    ShearX(v) (1, v, -v cy, 0, 1, 0)     ShearY(v) (1, 0, 0, v, 1, -v cx)     TranslateX(t) (1, 0, -t, 0, 1, 0)
    TranslateY(t) (1, 0, 0, 0, 1, -t)    Rotate(theta, c = cos, s = sin) (c, s, cx - c cx - s cy, -s, c, cy + s cx - c cy)
become six integers through FIX(v) = floor(v * 65536 + 0.5): a0 = FIX(a), a1 = FIX(b), a2 = FIX(c + a / 2 + b / 2), a3 = FIX(d),
a4 = FIX(e), a5 = FIX(f + d / 2 + e / 2); then xin = (a0 x + a1 y + a2) >> 16, yin = (a3 x + a4 y + a5) >> 16 in 64-bit integers
(an arithmetic shift).  The output pixel is a bit copy of src[yin][xin] in all three planes where that lies inside the frame, and
``fill[channel]`` otherwise.  A value of 0 gives the identity's coefficients and is skipped.

POINTWISE, with f = fl32(1 + v) and omf = fl32(1) - f, each rounded once on the host, every multiply-add one fused operation:
    grey(r, g, b) = fma(0.299, r, fma(0.587, g, 0.114 * b))
    Brightness      clamp01(f * x)
    Color           clamp01(fma(f, x, omf * grey(pixel)))
    Contrast        clamp01(fma(f, x, omf * m)), m the image's mean grey AS THIS LAYER FINDS IT: summed in fp64, divided by H W in
                    fp64, rounded once to fp32
    Sharpness       per channel; interior pixels: acc = the eight neighbours in row-major order, added from the left in fp32,
                    d = fma(5, x, acc) * fl32(1 / 13), clamp01(fma(f, x, omf * d)); the first / last row and column are bit copies,
                    an image with H < 3 or W < 3 is one altogether
    bin(x) = (int) min(max(fma(x, 255, 0.5), 0), 255)       (round half up; bin(fl32(u) / fl32(255)) == u for every byte u)
    Posterize       float(bin(x) & (0xFF << (8 - bits))) / 255   (one IEEE division)
    Solarize        x >= t ? 1 - x : x
    AutoContrast    per channel: lo, hi the exact extremes; hi > lo: clamp01((x - lo) * (1 / (hi - lo))), else a bit copy
    Equalize        per channel: h[k] the number of pixels with bin(x) == k; fewer than two non-zero counts: a bit copy; step =
                    (sum h - the last non-zero count) // 255; step == 0: a bit copy; else lut[i] = min(255, (step // 2 +
                    sum_{k < i} h[k]) // step) and float(lut[bin(x)]) / 255 (``PIL.ImageOps.equalize``'s table)
f == 1 skips its operation, and so do 8 bits.  A layer that is the identity for its image leaves it bit for bit.

THE DRAW of one example, from the policy's own ``random.Random`` (the crops, the photometric and the mix draws of a run do not
depend on whether this stage is on), per example in batch order:
  RandAugment N M: for each of the N layers ``op = randrange(14)``; if the op is signed, ``neg = randrange(2)`` -- also at M = 0.
  TrivialAugment:  ``op = randrange(14)``; if the op has a magnitude table (ops 1-11), ``k = randrange(31)``; if it is signed,
                   ``neg = randrange(2)``.
Nothing else is drawn."""
import math
import random

import numpy as np

from ... import ops
from ...ops import RA_JOB
from .batch_mix import _image_size
from .photometric import IMAGENET_MEAN, _clamp01, _fma32, _grey32

OPS = ('Identity', 'ShearX', 'ShearY', 'TranslateX', 'TranslateY', 'Rotate', 'Brightness', 'Color', 'Contrast', 'Sharpness',
       'Posterize', 'Solarize', 'AutoContrast', 'Equalize')
(IDENTITY, SHEAR_X, SHEAR_Y, TRANSLATE_X, TRANSLATE_Y, ROTATE, BRIGHTNESS, COLOR, CONTRAST, SHARPNESS, POSTERIZE, SOLARIZE,
 AUTOCONTRAST, EQUALIZE) = range(14)
SIGNED = tuple(1 <= op <= 9 for op in range(14))
HAS_MAGNITUDE = tuple(1 <= op <= 11 for op in range(14))
BINS = 31
MAX_LAYERS = 4
# hi of ops 1, 2, 5..9 (the shifts depend on the frame, ops 10 and 11 have tables of their own)
HI_RAND = {SHEAR_X: 0.3, SHEAR_Y: 0.3, ROTATE: 30.0, BRIGHTNESS: 0.9, COLOR: 0.9, CONTRAST: 0.9, SHARPNESS: 0.9}
HI_WIDE = {SHEAR_X: 0.99, SHEAR_Y: 0.99, ROTATE: 135.0, BRIGHTNESS: 0.99, COLOR: 0.99, CONTRAST: 0.99, SHARPNESS: 0.99}
WIDE_SHIFT = 32.0


def coefficients(op, v, H, W):
    """the six fp64 coefficients of the output -> input map of geometric op(s) ``op`` at value(s) ``v`` -- a shear, a shift in
    pixels, an angle in DEGREES -- on an H x W frame, in Pillow's ``AFFINE`` convention: arrays of ``op``'s shape + (6,)"""
    op, v = np.asarray(op), np.asarray(v, np.float64)
    cx, cy = W / 2, H / 2
    theta = v * math.pi / 180.0
    c, s = np.cos(theta), np.sin(theta)
    one, zero = np.ones(v.shape), np.zeros(v.shape)
    rows = {SHEAR_X: (one, v, -v * cy, zero, one, zero), SHEAR_Y: (one, zero, zero, v, one, -v * cx),
            TRANSLATE_X: (one, zero, -v, zero, one, zero), TRANSLATE_Y: (one, zero, zero, zero, one, -v),
            ROTATE: (c, s, cx - c * cx - s * cy, -s, c, cy + s * cx - c * cy)}
    out = np.stack([one, zero, zero, zero, one, zero], axis=-1)
    for code, row in rows.items():
        out = np.where((op == code)[..., None], np.stack(row, axis=-1), out)
    return out


def fixed_point(coef):
    """[..., 6] fp64 coefficients -> the six int64 of the index map (the module docstring's FIX)"""
    a, b, c, d, e, f = (coef[..., k] for k in range(6))
    parts = (a, b, c + a / 2 + b / 2, d, e, f + d / 2 + e / 2)
    return np.stack([np.floor(p * 65536.0 + 0.5) for p in parts], axis=-1).astype(np.int64)


def fill_layers(jobs, op, v, H, W):
    """the columns ``op``, ``a`` and ``f`` of the table ``jobs`` from [n][L] arrays: the op codes and their values -- a shear, a
    shift in pixels, an angle in degrees, the v of f = 1 + v, the bits, the threshold (ignored by ops 0, 12, 13)"""
    op, v = np.asarray(op, np.int32), np.asarray(v, np.float64)
    L = op.shape[1]
    geometric, factor = (op >= SHEAR_X) & (op <= ROTATE), (op >= BRIGHTNESS) & (op <= SHARPNESS)
    a = np.where(geometric[..., None], fixed_point(coefficients(op, np.where(geometric, v, 0.0), H, W)), 0)
    a[..., 0] = np.where(op == POSTERIZE, np.rint(v).astype(np.int64), a[..., 0])
    f = (1.0 + np.where(factor, v, 0.0)).astype(np.float32)
    pair = np.stack([f, np.float32(1.0) - f], axis=-1)
    pair = np.where(factor[..., None], pair, np.float32(0.0))
    pair[..., 0] = np.where(op == SOLARIZE, v.astype(np.float32), pair[..., 0])
    jobs['op'][:, :L], jobs['a'][:, :L], jobs['f'][:, :L] = op, a, pair
    return jobs


def make_job(layers=((IDENTITY, None),), H=1, W=1, fill=IMAGENET_MEAN):
    """one ``RA_JOB`` record (a 0-d array) for an H x W frame from 1..4 ``(op, value)`` pairs: the value is a shear, a shift in
    pixels, an angle in degrees, the v of f = 1 + v, the bits kept, the threshold; None for the ops without one"""
    layers = list(layers)
    if not 1 <= len(layers) <= MAX_LAYERS:
        raise ValueError('a job has 1 to %d layers, got %d' % (MAX_LAYERS, len(layers)))
    jobs = np.zeros(1, RA_JOB)
    jobs['layers'] = len(layers)
    jobs['fill'] = np.asarray(fill, np.float64).astype(np.float32)
    fill_layers(jobs, [[int(op) for op, _ in layers]], [[0.0 if v is None else float(v) for _, v in layers]], H, W)
    return jobs[0]


class RandAugmentPolicy:
    """``RandAugmentPolicy('rand', layers=N, magnitude=M)`` or ``RandAugmentPolicy('trivial')``, with the fill of the geometric ops
    and the seed of the stream"""

    def __init__(self, kind='rand', layers=2, magnitude=9, fill=IMAGENET_MEAN, seed=None):
        if kind not in ('rand', 'trivial'):
            raise ValueError('the policy is rand or trivial, got %r' % (kind,))
        if kind == 'trivial':
            layers, magnitude = 1, None
        elif not (isinstance(layers, int) and 1 <= layers <= MAX_LAYERS and isinstance(magnitude, int) and 0 <= magnitude < BINS):
            raise ValueError('RandAugment takes 1 to %d layers and a magnitude bin in [0, %d], got %r and %r'
                             % (MAX_LAYERS, BINS - 1, layers, magnitude))
        if len(fill) != 3 or not all(math.isfinite(v) for v in fill):
            raise ValueError('the fill must be three finite numbers, got %r' % (tuple(fill),))
        self.kind, self.layers, self.magnitude = kind, layers, magnitude
        self.fill = tuple(float(v) for v in fill)
        self._rng = random.Random(seed)

    def reseed(self, seed):
        self._rng = random.Random(seed)

    def getstate(self):
        return self._rng.getstate()

    def setstate(self, state):
        self._rng.setstate(state)

    def _draw(self, table):
        """the module docstring's draws of one example, appended to ``table`` as (op, k, neg) per layer"""
        rng = self._rng
        if self.kind == 'trivial':
            op = rng.randrange(14)
            k = rng.randrange(BINS) if HAS_MAGNITUDE[op] else 0
            table.append((op, k, rng.randrange(2) if SIGNED[op] else 0))
            return
        for _ in range(self.layers):
            op = rng.randrange(14)
            table.append((op, self.magnitude, rng.randrange(2) if SIGNED[op] else 0))

    def values(self, op, k, neg, H, W):
        """[n][L] op codes, magnitude bins and sign draws -> the values ``fill_layers`` takes"""
        wide = self.kind == 'trivial'
        hi = np.zeros(op.shape)
        for code, top in (HI_WIDE if wide else HI_RAND).items():
            hi = np.where(op == code, top, hi)
        hi = np.where(op == TRANSLATE_X, WIDE_SHIFT if wide else 150.0 / 331.0 * W, hi)
        hi = np.where(op == TRANSLATE_Y, WIDE_SHIFT if wide else 150.0 / 331.0 * H, hi)
        v = hi * k / 30
        v = np.where(neg == 1, -v, v)
        v = np.where((op == TRANSLATE_X) | (op == TRANSLATE_Y), np.trunc(v), v)
        v = np.where(op == POSTERIZE, 8 - np.rint(k / (5.0 if wide else 7.5)), v)
        return np.where(op == SOLARIZE, np.float32(1 - k / 30), v)

    def draw(self, H, W):
        """the job of the next example: a 0-d ``RA_JOB`` record"""
        return self.draw_batch(1, H, W)[0]

    def draw_batch(self, n, H, W):
        """the jobs of a batch of ``n`` examples, in batch order: the draws one example at a time -- nothing but ``randrange`` --,
        the table filled a column at a time"""
        jobs = np.zeros(n, RA_JOB)
        if n == 0:
            return jobs
        table = []
        for _ in range(n):
            self._draw(table)
        drawn = np.array(table, np.int64).reshape(n, self.layers, 3)
        op, k, neg = drawn[..., 0], drawn[..., 1], drawn[..., 2]
        jobs['layers'] = self.layers
        jobs['fill'] = np.asarray(self.fill, np.float64).astype(np.float32)
        return fill_layers(jobs, op, self.values(op, k, neg, H, W), H, W)


def _bin(x):
    """bin() of the module docstring on an fp32 array -> int32"""
    f = np.float32
    return np.minimum(np.maximum(_fma32(f(255), x, f(0.5)), f(0)), f(255)).astype(np.int32)


def gather_index(a, H, W):
    """(yin, xin, inside) of the fixed-point map ``a`` (six integers) over an H x W frame"""
    a = [int(v) for v in a]
    y, x = np.mgrid[0:H, 0:W].astype(np.int64)
    xin, yin = (a[0] * x + a[1] * y + a[2]) >> 16, (a[3] * x + a[4] * y + a[5]) >> 16
    return yin, xin, (xin >= 0) & (xin < W) & (yin >= 0) & (yin < H)


def equalize_table(h):
    """the module docstring's table of one channel's 256 counts: int32 [256], or None where the channel is a bit copy"""
    h = np.asarray(h, np.int64)
    nz = h[h > 0]
    if len(nz) < 2:
        return None
    step = (int(h.sum()) - int(nz[-1])) // 255
    if step == 0:
        return None
    before = np.concatenate([[0], np.cumsum(h)[:-1]])
    return np.minimum(255, (step // 2 + before) // step).astype(np.int32)


def apply_layer(px, op, a, pair, fill):
    """one layer on one image px [3][H][W] fp32 -> a new array, or ``px`` itself where the layer is the identity"""
    f32 = np.float32
    H, W = px.shape[1:]
    f, omf = f32(pair[0]), f32(pair[1])
    if SHEAR_X <= op <= ROTATE:
        if [int(v) for v in a] == [65536, 0, 32768, 0, 65536, 32768]:
            return px
        yin, xin, inside = gather_index(a, H, W)
        got = px[:, np.where(inside, yin, 0), np.where(inside, xin, 0)]
        return np.where(inside[None], got, np.asarray(fill, f32)[:, None, None]).astype(f32)
    if BRIGHTNESS <= op <= SHARPNESS:
        if f == 1:
            return px
        if op == BRIGHTNESS:
            return _clamp01((f * px).astype(f32))
        if op == COLOR:
            t = (omf * _grey32(px[0], px[1], px[2])).astype(f32)
            return _clamp01(_fma32(f, px, t[None]))
        if op == CONTRAST:
            m = f32(_grey32(px[0], px[1], px[2]).astype(np.float64).sum() / float(H * W))
            return _clamp01(_fma32(f, px, f32(omf * m)))
        if H < 3 or W < 3:
            return px
        out = px.copy()
        acc = (px[:, :-2, :-2] + px[:, :-2, 1:-1]).astype(f32)
        for part in (px[:, :-2, 2:], px[:, 1:-1, :-2], px[:, 1:-1, 2:], px[:, 2:, :-2], px[:, 2:, 1:-1], px[:, 2:, 2:]):
            acc = (acc + part).astype(f32)
        centre = px[:, 1:-1, 1:-1]
        d = (_fma32(f32(5), centre, acc) * (f32(1) / f32(13))).astype(f32)
        out[:, 1:-1, 1:-1] = _clamp01(_fma32(f, centre, (omf * d).astype(f32)))
        return out
    if op == POSTERIZE:
        bits = int(a[0])
        if bits == 8:
            return px
        return ((_bin(px) & ((0xFF << (8 - bits)) & 0xFF)).astype(f32) / f32(255)).astype(f32)
    if op == SOLARIZE:
        return np.where(px >= f, f32(1) - px, px).astype(f32)
    if op == AUTOCONTRAST:
        out = px.copy()
        for c in range(3):
            lo, hi = px[c].min(), px[c].max()
            if hi > lo:
                out[c] = _clamp01(((px[c] - lo).astype(f32) * (f32(1) / (hi - lo))).astype(f32))
        return out
    if op == EQUALIZE:
        out = px.copy()
        for c in range(3):
            k = _bin(px[c])
            lut = equalize_table(np.bincount(k.reshape(-1), minlength=256))
            if lut is not None:
                out[c] = (lut[k].astype(f32) / f32(255)).astype(f32)
        return out
    return px


def apply_host(frames, jobs):
    """the stage in NumPy fp32 with the module docstring's rounding points: frames [B][3][H][W] float32 and an ``RA_JOB`` table
    -> a new array.  (An fma is formed in fp64 and rounded to fp32, as in photometric.py.)"""
    frames = np.asarray(frames)
    if frames.dtype != np.float32 or frames.ndim != 4 or frames.shape[1] != 3 or len(jobs) != len(frames):
        raise ValueError('frames must be float32 [B][3][H][W] with one job per image')
    out = frames.copy()
    for n, j in enumerate(jobs):
        px = out[n]
        for l in range(int(j['layers'])):
            px = apply_layer(px, int(j['op'][l]), j['a'][l], j['f'][l], j['fill'])
        out[n] = px
    return out


class RandAugmentBatches:
    """``RandAugmentBatches(dataset, policy, image_size)`` around the ``ShardedDataset`` of a device feed, inside
    ``PhotometricBatches`` / ``MixedBatches`` where the run has them: what ``MultithreadIterator(device=...)`` sees of a dataset,
    with the batch's jobs drawn behind the inner dataset's per-example draws on the decode thread and the stage launched behind
    the crop on the feed's stream.  The stage writes a fresh tensor (out of place no layer order ever needs a copy launch,
    csrc/randaug.hip) and hands on a batch of the inner batch's type, with its cache counts, around it."""

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
        batch = self.dataset.finish_batch(inner, device, map_fn)
        frames = batch[0]
        if tuple(frames.shape[2:]) != self.image_size:
            raise ValueError('the draws were taken for %r frames, the batch holds %r' % (self.image_size, tuple(frames.shape[2:])))
        if ops.ra_identity(jobs, *self.image_size).all():
            return batch
        staged = type(batch)((ops.rand_augment(frames, jobs),) + tuple(batch[1:]))
        if hasattr(batch, '__dict__'):
            staged.__dict__.update(batch.__dict__)      # cache_hits / cache_misses of a FeedBatch
        return staged

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
