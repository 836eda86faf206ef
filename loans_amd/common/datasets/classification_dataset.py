"""The datasets of the ImageNet pre-training arm with the usual input pipeline: random-resized-crop + mirror for training,
a centre crop for validation, both finished on the GPU (crop_resize.py / csrc/croprs.hip: one launch per batch, the bytes of
Pillow's crop + BILINEAR resize).

``ClassificationImageDataset`` reads the ``path<TAB>class`` files ``LabeledImageDataset`` reads and decodes frames by
``ImageDataset._read_u8``'s convention, so the decode farm serves it unchanged; ``ResidentClassificationSource`` serves a set
that already lies in HBM as one uint8 [N][H][W][3] tensor -- its batches are cut straight out of that tensor, the only upload
is the job table.  Both offer ``get_example`` (the host reference: Pillow) and ``decode_batch`` / ``finish_batch`` in the
shape ``MultithreadIterator(device=...)`` expects; a finished batch is ``(frames [B][3][oh][ow] float32, labels [B] int32)``
on the device.

``ClassificationImageDataset(cache=RaggedFrameCache(...))`` decodes a file once: from the second epoch on a batch is cut out of
frames kept in HBM (or, in host mode, out of decoded arrays kept in host memory) -- only the draws change between epochs."""
import csv
import os
import random

import numpy
import torch
from PIL import Image

from .crop_resize import center_crop_box, crop_resize_device, crop_resize_device_multi, crop_resize_host, sample_rrc_box
from .frame_cache import CachedFrame


class _CropDraws:
    """the per-example draws: ``train`` -- the box, then the mirror, from the dataset's own stream, one example after the other
    in the order of the calls; otherwise the centre crop and no draw at all"""

    def _init_draws(self, image_size, train, scale, ratio, crop_pct, augment_seed):
        self.image_size = (int(image_size[0]), int(image_size[1]))
        self.train, self.scale, self.ratio, self.crop_pct = bool(train), tuple(scale), tuple(ratio), crop_pct
        self._aug_rng = random.Random(augment_seed)

    def reseed(self, seed):
        self._aug_rng = random.Random(seed)

    def draw_state(self):
        """where the draw stream stands (``random.Random.getstate()``): what a checkpoint keeps of this dataset"""
        return self._aug_rng.getstate()

    def set_draw_state(self, state):
        self._aug_rng.setstate(state)

    def _draw(self, H, W):
        """(box, flip) of the next example, an H x W frame"""
        if not self.train:
            return center_crop_box(H, W, self.image_size, self.crop_pct), False
        box = sample_rrc_box(self._aug_rng, H, W, self.scale, self.ratio)
        return box, self._aug_rng.random() < 0.5

    def __getitem__(self, i):
        return self.get_example(i)

    def device_batch(self, indices, device, map_fn=map):
        """``stack(get_example(i) for i in indices)`` finished on the GPU"""
        return self.finish_batch(self.decode_batch(indices, map_fn), device, map_fn)


class FeedBatch(tuple):
    """``(frames, labels)`` of a dataset with a frame cache, with what the cache did for it: ``cache_hits`` / ``cache_misses``
    -- counted where the batch is consumed, the lookups themselves run batches ahead"""
    cache_hits = cache_misses = 0


class ClassificationImageDataset(_CropDraws):

    def __init__(self, pairs, root='.', image_size=(224, 224), train=True, scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3),
                 crop_pct=0.875, augment_seed=None, cache=None):
        self.cache = cache          # a RaggedFrameCache (frame_cache.py) or None
        if isinstance(pairs, str):
            with open(pairs) as pairs_file:
                pairs = [(pair[0], int(pair[1])) for pair in csv.reader(pairs_file, delimiter='\t') if pair]
        self._pairs, self._root = list(pairs), root
        self._init_draws(image_size, train, scale, ratio, crop_pct, augment_seed)

    def __len__(self):
        return len(self._pairs)

    def _path(self, i):
        return os.path.join(self._root, self._pairs[i][0])

    def _read_u8(self, i):
        """decode only (no draws: safe on a pool thread): uint8 HWC RGB by ``ImageDataset``'s convention -- grey becomes three
        channels, otherwise the first three; a file that is not 8-bit is cut to uint8 the way ``astype`` cuts it"""
        with Image.open(self._path(i)) as f:
            image = numpy.asarray(f)
            if image.dtype != numpy.uint8:
                image = numpy.asarray(f, dtype=numpy.float32).astype(numpy.uint8)
        if image.ndim == 2:
            image = image[:, :, None]
        if image.shape[2] == 1:
            return numpy.repeat(image, 3, axis=2)
        if image.shape[2] < 3:
            raise ValueError('%s: neither grey nor at least three channels' % self._path(i))
        return numpy.ascontiguousarray(image[:, :, :3])

    def get_example(self, i):
        frame = self._read_u8(i)
        box, flip = self._draw(*frame.shape[:2])
        return crop_resize_host(frame, box, self.image_size, flip), numpy.int32(self._pairs[i][1])

    def _decode(self, indices, map_fn, farm):
        if farm is not None:
            frames = farm.decode([self._path(i) for i in indices], map_fn) if indices else []
            return [self._read_u8(i) if isinstance(f, int) else f for i, f in zip(indices, frames)]
        return list(map_fn(self._read_u8, indices))

    def decode_batch(self, indices, map_fn=map, farm=None):
        """Host half: ``map_fn`` (a thread pool's ``map``) or the decode farm decodes; the draws are taken afterwards in index
        order, so a pooled batch consumes the stream like ``[get_example(i) for i in indices]``.  With a cache every index is
        looked up first and only the misses are decoded: a frame resident in HBM is a ``CachedFrame`` placeholder of its shape,
        one kept on the host the array itself -- the draws see shapes alone, hit or miss -- and the indices travel with the
        result."""
        indices = list(indices)
        if self.cache is None:
            frames = self._decode(indices, map_fn, farm)
        else:
            frames = [self.cache.lookup(i) for i in indices]
            missing = [n for n, f in enumerate(frames) if f is None]
            for n, f in zip(missing, self._decode([indices[n] for n in missing], map_fn, farm)):
                frames[n] = f
                self.cache.keep_host(indices[n], f)
        draws = [self._draw(*f.shape[:2]) for f in frames]
        labels = numpy.array([self._pairs[i][1] for i in indices], numpy.int32)
        if self.cache is None:
            return frames, draws, labels
        return frames, draws, labels, indices, len(indices) - len(missing)

    def finish_batch(self, decoded, device, map_fn=map):
        """Device half.  Host cores are the scarce resource: per frame ONE contiguous copy -- rows y0 .. y0 + h at full width --
        into the pinned staging ring (``map_fn`` spreads the copies), one asynchronous upload with the labels behind the
        frames, one launch; the kernel gets x0 and the pitch."""
        from .resample import _staging
        device = torch.device(device)
        if len(decoded) > 3:
            return self._finish_cached(decoded, device, map_fn)
        frames, draws, labels = decoded
        jobs, spans, off = [], [], 0
        for f, ((y0, x0, h, w), flip) in zip(frames, draws):
            W = f.shape[1]
            jobs.append((off, 3 * W, h, W, (0, x0, h, w), flip))
            spans.append((off, f, y0, h))
            off += h * W * 3
        labels_at = (off + 3) & ~3
        total = labels_at + 4 * len(frames)
        ring, slot, host = _staging.get(total)
        host_np = host.numpy()

        def stage(span):
            o, f, y0, h = span
            W = f.shape[1]
            numpy.copyto(host_np[o:o + h * W * 3].reshape(h, W, 3), f[y0:y0 + h])

        list(map_fn(stage, spans))
        host_np[labels_at:total].view(numpy.int32)[:] = labels
        dev_all = host[:total].to(device, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(device))
        ring['events'][slot] = ev
        # (the labels are their own tensor: the upload buffer goes when the launch has read it)
        return crop_resize_device(dev_all[:off], jobs, self.image_size), dev_all[labels_at:total].view(torch.int32).clone()

    def _finish_cached(self, decoded, device, map_fn):
        """``finish_batch`` with a cache.  Three kinds of frames, ONE launch over several sources: hits are read where they lie
        in the cache's slabs; misses the cache admits are staged as WHOLE frames and uploaded, one asynchronous copy per
        touched slab, straight into the space reserved for them (no device-to-device copy), and read there; the other misses
        -- no room, an index that occurs twice in the batch before it is stored (a batch that runs over a shard's end), every miss in
        host mode -- go up as before: crop rows only, with the labels, as the last source."""
        from .resample import _staging
        frames, draws, labels, indices, hits = decoded
        cache = self.cache
        cur = torch.cuda.current_stream(device)
        missed = [n for n, f in enumerate(frames) if not isinstance(f, CachedFrame)]
        plan = {}
        if cache.where == 'device':
            if cache.device.type != device.type or None not in (cache.device.index, device.index) and cache.device.index != device.index:
                raise ValueError('the frame cache lives on %s, the batch is finished on %s' % (cache.device, device))
            cache.wait_for_stores(cur)
            times = {}
            for n in missed:
                times[indices[n]] = times.get(indices[n], 0) + 1
            once = [n for n in missed if times[indices[n]] == 1]
            plan = {n: loc for n, loc in zip(once, cache.reserve([(indices[n],) + frames[n].shape[:2] for n in once]))
                    if loc is not None}
        # the staging buffer: per touched slab the run of whole frames reserved in it, then the crop rows of the other misses,
        # then the labels
        runs = {}                                       # slab -> [first byte in the slab, bytes, offset in the staging buffer]
        for n, (slab, at) in plan.items():
            run = runs.setdefault(slab, [at, 0, 0])
            run[1] = at + frames[n].nbytes - run[0]     # (reserved in batch order: offsets ascend)
        off = 0
        for run in runs.values():
            run[2] = off
            off += run[1]
        rows_at = off = (off + 15) & ~15
        sources, source_of = [], {}

        def source(slab):
            if slab not in source_of:
                source_of[slab] = len(sources)
                sources.append(cache.slabs[slab])
            return source_of[slab]

        jobs, spans = [], []
        for n, (f, ((y0, x0, h, w), flip)) in enumerate(zip(frames, draws)):
            H, W = f.shape[:2]
            if isinstance(f, CachedFrame):
                slab, at = cache.location(f.index)[:2]
                jobs.append((at, 3 * W, H, W, (y0, x0, h, w), flip, source(slab)))
            elif n in plan:
                slab, at = plan[n]
                jobs.append((at, 3 * W, H, W, (y0, x0, h, w), flip, source(slab)))
                spans.append((runs[slab][2] + at - runs[slab][0], f, 0, H))
            else:
                jobs.append([off - rows_at, 3 * W, h, W, (0, x0, h, w), flip, None])
                spans.append((off, f, y0, h))
                off += h * W * 3
        labels_at = (off + 3) & ~3
        total = labels_at + 4 * len(frames)
        ring, slot, host = _staging.get(total)
        host_np = host.numpy()

        def stage(span):
            o, f, y0, h = span
            W = f.shape[1]
            numpy.copyto(host_np[o:o + h * W * 3].reshape(h, W, 3), f[y0:y0 + h])

        list(map_fn(stage, spans))
        host_np[labels_at:total].view(numpy.int32)[:] = labels
        for slab, (first, nbytes, at) in runs.items():
            cache.slabs[slab][first:first + nbytes].copy_(host[at:at + nbytes], non_blocking=True)
        dev_rest = host[rows_at:total].to(device, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(cur)
        ring['events'][slot] = ev
        if plan:
            cache.publish([indices[n] for n in plan], ev, cur)
        if off > rows_at:
            sources.append(dev_rest[:off - rows_at])
            jobs = [tuple(j[:6]) + (len(sources) - 1,) if j[6] is None else j for j in jobs]
        batch = FeedBatch((crop_resize_device_multi(sources, jobs, self.image_size),
                           dev_rest[labels_at - rows_at:total - rows_at].view(torch.int32).clone()))
        batch.cache_hits, batch.cache_misses = hits, len(frames) - hits
        return batch


class ResidentClassificationSource(_CropDraws):
    """a whole set resident in HBM: ``frames`` uint8 [N][H][W][3] (array or tensor), ``labels`` [N]; the kernel reads every
    crop in place through the frame's offset and the row pitch"""

    def __init__(self, frames, labels, device, image_size=(224, 224), train=True, scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3),
                 crop_pct=0.875, augment_seed=None):
        frames = torch.as_tensor(frames)
        if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3:
            raise ValueError('frames must be uint8 [N][H][W][3]')
        self.frames = frames.to(torch.device(device)).contiguous()
        self.labels = torch.as_tensor(numpy.asarray(labels).reshape(-1).astype(numpy.int32)).to(self.frames.device)
        if len(self.labels) != len(self.frames):
            raise ValueError('%d labels for %d frames' % (len(self.labels), len(self.frames)))
        self._init_draws(image_size, train, scale, ratio, crop_pct, augment_seed)

    @classmethod
    def from_float_chw(cls, x, labels, device, **kwargs):
        """from frames float [N][3][H][W] in [0, 1] (the synthetic classes: exactly k / 255), converted once"""
        u8 = numpy.rint(numpy.asarray(x) * 255).clip(0, 255).astype(numpy.uint8)
        return cls(numpy.ascontiguousarray(u8.transpose(0, 2, 3, 1)), labels, device, **kwargs)

    def __len__(self):
        return len(self.frames)

    def get_example(self, i):
        """the host reference of example i (copies the frame down)"""
        box, flip = self._draw(*self.frames.shape[1:3])
        return crop_resize_host(self.frames[i].cpu().numpy(), box, self.image_size, flip), numpy.int32(int(self.labels[i]))

    def decode_batch(self, indices, map_fn=map, farm=None):
        indices = [int(i) for i in indices]
        H, W = self.frames.shape[1:3]
        return indices, [self._draw(H, W) for _ in indices]

    def finish_batch(self, decoded, device, map_fn=map):
        indices, draws = decoded
        H, W = self.frames.shape[1:3]
        jobs = [(i * H * W * 3, 3 * W, H, W, box, flip) for i, (box, flip) in zip(indices, draws)]
        labels = self.labels[torch.as_tensor(indices, dtype=torch.int64).to(self.frames.device)]
        return crop_resize_device(self.frames.view(-1), jobs, self.image_size), labels
