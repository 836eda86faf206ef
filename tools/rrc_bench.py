#!/usr/bin/env python
"""A/B of the random-resized-crop feed's GPU stage (development tool; needs a GPU).

Workload: 256 frames of 375 x 500 uint8 resident in HBM, one seeded ``sample_rrc_box`` crop (+ mirror) each, to 224 x 224.

  fused     loans_crop_resize_u8_f32: the crops read in place (offset, pitch, box), both passes in one launch, the
            intermediate in LDS (csrc/croprs.hip)
  two-pass  what the tree could do before: the crops copied out contiguously (NOT timed here), then
            loans_resize_ragged_u8_f32 with the bilinear tables -- two launches, the intermediate in HBM

Only the launches are timed (device events around ``--iters`` back-to-back calls on job tables that already lie on the
device); the two arms alternate within one process, ``--repeats`` windows each, and the spread over the windows is reported
with the medians.  The outputs of the two arms are compared first: they must be the same bytes.  The fused kernel's HBM bound
is the crop bytes read plus 12 oh ow bytes written per frame over the peak bandwidth."""
import argparse
import os
import random
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from loans_amd import _lib                                                  # noqa: E402
from loans_amd.common.datasets import crop_resize as CR                     # noqa: E402
from loans_amd.common.datasets import resample as RS                        # noqa: E402
from loans_amd.ops import _ptr, _stream, check                              # noqa: E402

HBM_PEAK = 8.0e12       # bytes / s, HBM3E spec


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--frames', type=int, default=256)
    ap.add_argument('--frame-size', type=int, nargs=2, default=(375, 500))
    ap.add_argument('--out-size', type=int, nargs=2, default=(224, 224))
    ap.add_argument('--iters', type=int, default=200, help='launches per timed window')
    ap.add_argument('--repeats', type=int, default=9, help='timed windows per arm, alternating')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--out', default=os.path.join('profiles', 'rrc_feed_ab.txt'))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('rrc_bench needs a GPU: a time from anything else says nothing')
    dev = torch.device('cuda', torch.cuda.current_device())
    lib = _lib.load()
    N, (H, W), (oh, ow) = a.frames, a.frame_size, a.out_size
    rng = random.Random(a.seed)
    draws = [(CR.sample_rrc_box(rng, H, W), rng.random() < 0.5) for _ in range(N)]
    frames = torch.randint(0, 256, (N, H, W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(a.seed)).to(dev)

    # the wrappers once: they make the tables resident and give the outputs to compare
    fused_jobs = [(n * H * W * 3, 3 * W, H, W, box, flip) for n, (box, flip) in enumerate(draws)]
    want = CR.crop_resize_device(frames.view(-1), fused_jobs, (oh, ow))
    crops = [frames[n, y0:y0 + h, x0:x0 + w].contiguous() for n, ((y0, x0, h, w), _) in enumerate(draws)]
    packed = torch.cat([c.view(-1) for c in crops])
    offs = np.cumsum([0] + [c.numel() for c in crops])[:-1]
    ragged = [(int(o), c.shape[0], c.shape[1], flip) for o, c, (_, flip) in zip(offs, crops, draws)]
    got = RS.resize_ragged(packed, ragged, (oh, ow), filt='bilinear')
    torch.cuda.synchronize()
    same = torch.equal(want, got)

    # job tables on the device, as the wrappers build them
    arena = RS._arenas[(dev, torch.cuda.current_stream(dev).cuda_stream)]
    at = arena.where
    ft = np.zeros(N, CR.CROP_JOB)
    rt = np.zeros(N, RS.RESAMPLE_JOB)
    tmp_off = 0
    for n, ((y0, x0, h, w), flip) in enumerate(draws):
        ft[n] = (n * H * W * 3, 3 * W, y0, x0, h, w) + at[(w, ow, 'bilinear')] + at[(h, oh, 'bilinear')] + (int(flip),)
        rt[n] = (int(offs[n]), tmp_off, h, w) + at[(w, ow, 'bilinear')] + at[(h, oh, 'bilinear')] + (int(flip), 0)
        tmp_off += (h * ow * 3 + 15) & ~15
    ft_d = torch.from_numpy(ft.view(np.uint8)).to(dev)
    rt_d = torch.from_numpy(rt.view(np.uint8)).to(dev)
    tmp = torch.empty(tmp_off, device=dev, dtype=torch.uint8)
    out_a, out_b = torch.empty_like(want), torch.empty_like(want)
    max_vks, max_h = int(ft['vks'].max()), max(h for (_, _, h, _), _ in draws)
    src_a = frames.view(-1)

    def fused():
        check(lib.loans_crop_resize_u8_f32(_ptr(src_a), _ptr(out_a), _ptr(ft_d), N, _ptr(arena.buf), max_vks, oh, ow, _stream()),
              'loans_crop_resize_u8_f32')

    def two_pass():
        check(lib.loans_resize_ragged_u8_f32(_ptr(packed), _ptr(tmp), _ptr(out_b), _ptr(rt_d), N, _ptr(arena.buf), max_h, oh, ow,
                                             _stream()), 'loans_resize_ragged_u8_f32')

    def window(fn):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(a.iters):
            fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) * 1e3 / a.iters         # microseconds per call

    for fn in (fused, two_pass):
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    same = same and torch.equal(out_a, want) and torch.equal(out_b, want)
    times = {'fused': [], 'two-pass': []}
    for _ in range(a.repeats):
        times['fused'].append(window(fused))
        times['two-pass'].append(window(two_pass))

    crop_bytes = sum(h * w * 3 for (_, _, h, w), _ in draws)
    bound_bytes = crop_bytes + 12 * oh * ow * N
    bound_us = bound_bytes / HBM_PEAK * 1e6
    med = {k: float(np.median(v)) for k, v in times.items()}
    lines = ['rrc feed A/B: %d frames of %d x %d -> %d x %d, boxes from sample_rrc_box(seed %d); %s' % (
                 N, H, W, oh, ow, a.seed, torch.cuda.get_device_name(dev)),
             'outputs of the two arms identical: %s' % same,
             '%d launches per window, %d windows per arm, alternating; microseconds per call' % (a.iters, a.repeats)]
    for k in ('fused', 'two-pass'):
        v = times[k]
        lines.append('%-9s median %8.1f   min %8.1f   max %8.1f   spread (max - min) %6.1f   windows %s' % (
            k, med[k], min(v), max(v), max(v) - min(v), ' '.join('%.1f' % t for t in v)))
    lines.append('two-pass / fused (medians): %.2f' % (med['two-pass'] / med['fused']))
    lines.append('fused HBM bound: %.1f MB crop bytes read + %.1f MB written = %.1f MB over %.1f TB/s = %.1f us; fused runs at %.1f %% of it (%.2f TB/s)'
                 % (crop_bytes / 1e6, 12 * oh * ow * N / 1e6, bound_bytes / 1e6, HBM_PEAK / 1e12, bound_us, 100 * bound_us / med['fused'],
                    bound_bytes / med['fused'] / 1e6))
    lines.append('(the two-pass arm is timed WITHOUT the copies that cut its crops out of the frames)')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)
    if not same:
        raise SystemExit('the two arms disagree')


if __name__ == '__main__':
    main()
