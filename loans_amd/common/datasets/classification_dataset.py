"""The datasets of the ImageNet pre-training arm with the usual input pipeline: random-resized-crop + mirror for training,
a centre crop for validation, both finished on the GPU (crop_resize.py / csrc/croprs.hip: one launch per batch, the bytes of
Pillow's crop + BILINEAR resize).

``ClassificationImageDataset`` reads the ``path<TAB>class`` files ``LabeledImageDataset`` reads and decodes frames by
``ImageDataset._read_u8``'s convention, so the decode farm serves it unchanged; ``ResidentClassificationSource`` serves a set
that already lies in HBM as one uint8 [N][H][W][3] tensor -- its batches are cut straight out of that tensor, the only upload
is the job table.  Both offer ``get_example`` (the host reference: Pillow) and ``decode_batch`` / ``finish_batch`` in the
shape ``MultithreadIterator(device=...)`` expects; a finished batch is ``(frames [B][3][oh][ow] float32, labels [B] int32)``
on the device."""
import csv
import os
import random

import numpy
import torch
from PIL import Image

from .crop_resize import center_crop_box, crop_resize_device, crop_resize_host, sample_rrc_box


class _CropDraws:
    """the per-example draws: ``train`` -- the box, then the mirror, from the dataset's own stream, one example after the other
    in the order of the calls; otherwise the centre crop and no draw at all"""

    def _init_draws(self, image_size, train, scale, ratio, crop_pct, augment_seed):
        self.image_size = (int(image_size[0]), int(image_size[1]))
        self.train, self.scale, self.ratio, self.crop_pct = bool(train), tuple(scale), tuple(ratio), crop_pct
        self._aug_rng = random.Random(augment_seed)

    def reseed(self, seed):
        self._aug_rng = random.Random(seed)

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


class ClassificationImageDataset(_CropDraws):

    def __init__(self, pairs, root='.', image_size=(224, 224), train=True, scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3),
                 crop_pct=0.875, augment_seed=None):
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

    def decode_batch(self, indices, map_fn=map, farm=None):
        """Host half: ``map_fn`` (a thread pool's ``map``) or the decode farm decodes; the draws are taken afterwards in index
        order, so a pooled batch consumes the stream like ``[get_example(i) for i in indices]``."""
        indices = list(indices)
        if farm is not None:
            frames = farm.decode([self._path(i) for i in indices], map_fn) if indices else []
            frames = [self._read_u8(i) if isinstance(f, int) else f for i, f in zip(indices, frames)]
        else:
            frames = list(map_fn(self._read_u8, indices))
        draws = [self._draw(*f.shape[:2]) for f in frames]
        return frames, draws, numpy.array([self._pairs[i][1] for i in indices], numpy.int32)

    def finish_batch(self, decoded, device, map_fn=map):
        """Device half.  Host cores are the scarce resource: per frame ONE contiguous copy -- rows y0 .. y0 + h at full width --
        into the pinned staging ring (``map_fn`` spreads the copies), one asynchronous upload with the labels behind the
        frames, one launch; the kernel gets x0 and the pitch."""
        from .resample import _staging
        device = torch.device(device)
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
