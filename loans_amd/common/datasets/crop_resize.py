"""Random-resized-crop and centre crop of the ImageNet pre-training feed: the box arithmetic on the host, the pixels on the GPU.

A crop followed by Pillow's ``BILINEAR`` resize is the two integer passes resample.hip restates, with the tables
``resample_coeffs(crop size, output size, 'bilinear')`` -- so the reference implementation here is Pillow itself
(``crop_resize_host``) and the device path (``crop_resize_device``, csrc/croprs.hip) is held to its bytes, not to a tolerance.
The kernel reads each crop in place (frame origin, row pitch, box) from a staged upload or from frames resident in HBM, keeps
the intermediate of the two passes in LDS and writes ``/ 255`` float32 CHW: one launch per batch, no intermediate in HBM."""
import math

import numpy as np
import torch
from PIL import Image

from ... import _lib
from ...ops import _ptr, _stream, check
from . import resample
from .resample import resample_coeffs

# mirror of loans_crop_job (include/loans_hip.h)
CROP_JOB = np.dtype([('src_off', '<i8'), ('pitch', '<i4'), ('y0', '<i4'), ('x0', '<i4'), ('h', '<i4'), ('w', '<i4'),
                     ('hb_off', '<i4'), ('hk_off', '<i4'), ('hks', '<i4'), ('vb_off', '<i4'), ('vk_off', '<i4'), ('vks', '<i4'),
                     ('flip', '<i4')])
assert CROP_JOB.itemsize == 56
CROP_LDS_BYTES = 65536          # LOANS_CROP_LDS_BYTES: the kernel's LDS image of the horizontal pass, uint8 [rows][ow][3]
MAX_JOBS = 65535                # gridDim.y


def lds_row_capacity(out_w):
    """crop rows (after the horizontal pass: ``out_w`` pixels each) that fit the kernel's LDS; a vertical window (``vks`` of
    the crop's height) above it is the one shape the kernel cannot do"""
    return CROP_LDS_BYTES // (int(out_w) * 3)


def sample_rrc_box(rng, H, W, scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3)):
    """Random-resized-crop box ``(y0, x0, h, w)`` of an H x W frame, drawn from ``rng`` (a ``random.Random``): up to ten
    attempts at an area fraction uniform in ``scale`` and an aspect ratio log-uniform in ``ratio``; then the central crop
    clamped to the ratio bounds."""
    log_lo, log_hi = math.log(ratio[0]), math.log(ratio[1])
    for _ in range(10):
        area = H * W * rng.uniform(scale[0], scale[1])
        ar = math.exp(rng.uniform(log_lo, log_hi))
        w = int(round(math.sqrt(area * ar)))
        h = int(round(math.sqrt(area / ar)))
        if 0 < w <= W and 0 < h <= H:
            return rng.randint(0, H - h), rng.randint(0, W - w), h, w
    in_ratio = W / H
    if in_ratio < ratio[0]:
        w, h = W, int(round(W / ratio[0]))
    elif in_ratio > ratio[1]:
        h, w = H, int(round(H * ratio[1]))
    else:
        h, w = H, W
    h, w = max(1, min(h, H)), max(1, min(w, W))
    return (H - h) // 2, (W - w) // 2, h, w


def center_crop_box(H, W, out_hw, crop_pct=0.875):
    """the largest box of the output's aspect ratio that fits an H x W frame, scaled by ``crop_pct``, centred: ``(y0, x0, h, w)``
    in whole pixels, at least one a side"""
    oh, ow = int(out_hw[0]), int(out_hw[1])
    if W * oh <= H * ow:                    # the frame is the narrower one: the box takes its whole width
        w, h = float(W), W * oh / ow
    else:
        h, w = float(H), H * ow / oh
    h, w = max(1, min(H, int(h * crop_pct))), max(1, min(W, int(w * crop_pct)))
    return (H - h) // 2, (W - w) // 2, h, w


def crop_resize_host(frame_u8_hwc, box, out_hw, flip=False):
    """the reference: Pillow's crop, mirror and BILINEAR resize, then ``/ 255`` and CHW float32"""
    y0, x0, h, w = box
    image = Image.fromarray(np.ascontiguousarray(frame_u8_hwc[y0:y0 + h, x0:x0 + w]))
    if flip:
        image = image.transpose(Image.FLIP_LEFT_RIGHT)
    image = image.resize((int(out_hw[1]), int(out_hw[0])), Image.BILINEAR)
    return np.ascontiguousarray(np.asarray(image, dtype=np.float32).transpose(2, 0, 1) / 255, dtype=np.float32)


def bilinear_window(in_size, out_size):
    """``resample_coeffs(in_size, out_size, 'bilinear')[2]`` -- the width of the coefficient rows: the largest window of one
    output coordinate -- by that function's own arithmetic, without building the table (1 ms of Python apiece, and a batch of
    random-resized-crops from a cache has a few hundred distinct sizes: more than ``resample_coeffs`` memoises)"""
    filterscale = (float(in_size) - 0.0) / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    return int(math.ceil(resample.BILINEAR_SUPPORT * filterscale)) * 2 + 1


def check_jobs(nbytes, jobs, out_hw):
    """host-side validation of ``crop_resize_device``'s jobs against a source buffer of ``nbytes`` bytes: ValueError for a box
    that leaves its frame, a frame that leaves the buffer, a window that exceeds the LDS capacity.  Touches no GPU.

    The per-source form (``crop_resize_device_multi``): ``nbytes`` is the list of the sources' byte counts and a job carries
    the index of its source as a seventh entry -- an index that names no source is a ValueError, and a frame has to lie inside
    its OWN source."""
    oh, ow = int(out_hw[0]), int(out_hw[1])
    if oh <= 0 or ow <= 0:
        raise ValueError('output size must be positive, got %r' % (out_hw,))
    if not 0 < len(jobs) <= MAX_JOBS:
        raise ValueError('a launch takes 1 .. %d crops, got %d' % (MAX_JOBS, len(jobs)))
    multi = not isinstance(nbytes, (int, np.integer))
    sizes = [int(b) for b in nbytes] if multi else [int(nbytes)]
    cap = lds_row_capacity(ow)
    windows = {}
    for n, job in enumerate(jobs):
        if len(job) != (7 if multi else 6):
            raise ValueError('crop %d: a job of %d entries, %d expected' % (n, len(job), 7 if multi else 6))
        off, pitch, H, W, (y0, x0, h, w), _ = job[:6]
        s = job[6] if multi else 0
        if not (isinstance(s, (int, np.integer)) and 0 <= s < len(sizes)):
            raise ValueError('crop %d: source index %r of %d sources' % (n, s, len(sizes)))
        if H <= 0 or W <= 0 or pitch < 3 * W or pitch >= 1 << 31:
            raise ValueError('crop %d: a %d x %d frame with a row pitch of %d bytes' % (n, H, W, pitch))
        if off < 0 or off + (H - 1) * pitch + 3 * W > sizes[s]:
            raise ValueError('crop %d: the frame (offset %d, %d rows of pitch %d) does not lie inside the %d-byte buffer%s'
                             % (n, off, H, pitch, sizes[s], ' of source %d' % s if multi else ''))
        if h < 1 or w < 1 or y0 < 0 or x0 < 0 or y0 + h > H or x0 + w > W:
            raise ValueError('crop %d: box (y0 %d, x0 %d, h %d, w %d) does not lie inside its %d x %d frame' % (n, y0, x0, h, w, H, W))
        vks = windows.get(h)
        if vks is None:
            vks = windows[h] = bilinear_window(h, oh)
        if vks > cap:
            raise ValueError('crop %d: %d rows to %d need a vertical window of %d rows, the kernel holds %d rows of %d pixels'
                             % (n, h, oh, vks, cap, ow))


def crop_resize_device(dev_all, jobs, out_hw, out=None):
    """``jobs`` = [(byte offset of the frame in dev_all, row pitch in bytes, H, W, (y0, x0, h, w), flip)] in batch order, every
    frame uint8 RGB rows inside the device buffer ``dev_all``: ``crop_resize_host`` of each as ONE launch ->
    [N][3][oh][ow] float32 in that order (written into ``out`` where one is given)."""
    oh, ow = int(out_hw[0]), int(out_hw[1])
    jobs = list(jobs)
    if dev_all.dtype != torch.uint8 or not dev_all.is_contiguous():
        raise ValueError('the source must be a contiguous uint8 buffer')
    check_jobs(dev_all.numel(), jobs, (oh, ow))
    if not dev_all.is_cuda:
        raise ValueError('the source must be a device buffer')
    dev = dev_all.device
    if out is None:
        out = torch.empty((len(jobs), 3, oh, ow), device=dev, dtype=torch.float32)
    elif not (out.dtype == torch.float32 and out.device == dev and out.is_contiguous() and tuple(out.shape) == (len(jobs), 3, oh, ow)):
        raise ValueError('out must be a contiguous float32 [%d][3][%d][%d] tensor on %s' % (len(jobs), oh, ow, dev))
    # one arena per (device, stream), shared with resize_ragged: see there
    akey = (dev, torch.cuda.current_stream(dev).cuda_stream)
    arena = resample._arenas.get(akey)
    if arena is None:
        arena = resample._arenas[akey] = resample._TableArena(dev)
    at = arena.ensure({(job[4][3], ow, 'bilinear') for job in jobs} | {(job[4][2], oh, 'bilinear') for job in jobs})
    table = np.zeros(len(jobs), CROP_JOB)
    for n, (off, pitch, _, _, (y0, x0, h, w), flip) in enumerate(jobs):
        table[n] = (off, pitch, y0, x0, h, w) + at[(w, ow, 'bilinear')] + at[(h, oh, 'bilinear')] + (int(bool(flip)),)
    ring, slot, host = resample._staging.get(table.nbytes, kind='jobs')
    host[:table.nbytes].numpy()[:] = table.view(np.uint8)
    jobs_d = host[:table.nbytes].to(dev, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(dev))
    ring['events'][slot] = ev
    check(_lib.load().loans_crop_resize_u8_f32(_ptr(dev_all), _ptr(out), _ptr(jobs_d), len(jobs), _ptr(arena.buf),
                                               int(table['vks'].max()), oh, ow, _stream()), 'loans_crop_resize_u8_f32')
    return out


def crop_resize_device_multi(sources, jobs, out_hw, out=None):
    """``crop_resize_device`` for frames that lie in SEVERAL device buffers (slabs of a frame cache, an upload of this moment):
    ``sources`` is a list of contiguous uint8 device tensors on one device, a job is ``crop_resize_device``'s tuple plus the
    index of the source its byte offset refers to.  Still ONE launch, and one pinned staging upload for the job table, the
    index array and the table of the sources' addresses.  The sources have to stay alive until the launch has run: what the
    kernel is given are their addresses."""
    oh, ow = int(out_hw[0]), int(out_hw[1])
    sources, jobs = list(sources), list(jobs)
    if not sources:
        raise ValueError('at least one source buffer is needed')
    for s in sources:
        if s.dtype != torch.uint8 or not s.is_contiguous():
            raise ValueError('every source must be a contiguous uint8 buffer')
    check_jobs([s.numel() for s in sources], jobs, (oh, ow))
    dev = sources[0].device
    if not all(s.is_cuda and s.device == dev for s in sources):
        raise ValueError('the sources must be device buffers of one device')
    if out is None:
        out = torch.empty((len(jobs), 3, oh, ow), device=dev, dtype=torch.float32)
    elif not (out.dtype == torch.float32 and out.device == dev and out.is_contiguous() and tuple(out.shape) == (len(jobs), 3, oh, ow)):
        raise ValueError('out must be a contiguous float32 [%d][3][%d][%d] tensor on %s' % (len(jobs), oh, ow, dev))
    akey = (dev, torch.cuda.current_stream(dev).cuda_stream)
    arena = resample._arenas.get(akey)
    if arena is None:
        arena = resample._arenas[akey] = resample._TableArena(dev)
    at = arena.ensure({(job[4][3], ow, 'bilinear') for job in jobs} | {(job[4][2], oh, 'bilinear') for job in jobs})
    # [job table][index array][(padding to 8)][address table], staged and uploaded as one
    n = len(jobs)
    index_at = CROP_JOB.itemsize * n
    srcs_at = (index_at + 4 * n + 7) & ~7
    total = srcs_at + 8 * len(sources)
    ring, slot, host = resample._staging.get(total, kind='jobs')
    host_np = host[:total].numpy()
    table, index = host_np[:index_at].view(CROP_JOB), host_np[index_at:index_at + 4 * n].view(np.int32)
    max_vks = 0
    for k, (off, pitch, _, _, (y0, x0, h, w), flip, s) in enumerate(jobs):
        v = at[(h, oh, 'bilinear')]
        table[k] = (off, pitch, y0, x0, h, w) + at[(w, ow, 'bilinear')] + v + (int(bool(flip)),)
        index[k] = s
        max_vks = max(max_vks, v[2])
    host_np[srcs_at:total].view(np.int64)[:] = [s.data_ptr() for s in sources]
    staged = host[:total].to(dev, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(dev))
    ring['events'][slot] = ev
    check(_lib.load().loans_crop_resize_srcs_u8_f32(_ptr(staged[srcs_at:]), _ptr(staged[index_at:]), len(sources), _ptr(out),
                                                    _ptr(staged), n, _ptr(arena.buf), int(max_vks), oh, ow, _stream()),
          'loans_crop_resize_srcs_u8_f32')
    return out
