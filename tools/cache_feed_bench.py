#!/usr/bin/env python
"""The decode-once frame cache of ``train_imagenet.py --augment rrc`` measured (development tool; needs a GPU).

kernel   tools/rrc_bench.py's workload -- 256 seeded random-resized-crops of 375 x 500 frames to 224 x 224 -- as
         ``parent``    loans_crop_resize_u8_f32 of the library named by --parent-lib (build csrc/croprs.hip of the commit to
                       compare against into a shared library of its own; without it this arm is left out, and said so)
         ``single``    this tree's loans_crop_resize_u8_f32
         ``multi-1``   loans_crop_resize_srcs_u8_f32, all frames in one source
         ``multi-S``   the same launch with the frames spread over --slabs sources, consecutive jobs in different ones
         Only the launches are timed (device events around --iters calls on tables that lie on the device), the arms alternate
         in one process, --repeats windows each; all outputs must be the same bytes.
feed     files -> device batches through ``MultithreadIterator(device=...)`` over --files seeded JPEGs (sizes drawn around
         375 x 500), --processes decode processes on --cores cores (one rank's share of a node): frames/s of epoch 1 without a
         cache, of epoch 1 with one (whole frames uploaded) and of epoch 2 with it; the bytes each arm stages per epoch; and the
         host time per example of ``decode_batch`` + ``finish_batch`` on batches of hits."""
import argparse
import ctypes
import os
import random
import sys
import tempfile
import time

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from loans_amd import _lib                                                  # noqa: E402
from loans_amd.common.datasets import crop_resize as CR                     # noqa: E402
from loans_amd.common.datasets import resample as RS                        # noqa: E402
from loans_amd.ops import _ptr, _stream, check                              # noqa: E402


def kernel_part(a, dev, say):
    lib = _lib.load()
    N, (H, W), (oh, ow) = 256, (375, 500), (224, 224)
    rng = random.Random(a.seed)
    draws = [(CR.sample_rrc_box(rng, H, W), rng.random() < 0.5) for _ in range(N)]
    frames = torch.randint(0, 256, (N, H, W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(a.seed)).to(dev)
    per = H * W * 3
    jobs = [(n * per, 3 * W, H, W, box, flip) for n, (box, flip) in enumerate(draws)]
    want = CR.crop_resize_device(frames.view(-1), jobs, (oh, ow))
    S = a.slabs
    slabs = [frames[s::S].contiguous().view(-1) for s in range(S)]             # frame n: slab n % S, slot n // S
    spread = [((n // S) * per, 3 * W, H, W, box, flip, n % S) for n, (box, flip) in enumerate(draws)]
    same = torch.equal(want, CR.crop_resize_device_multi(slabs, spread, (oh, ow)))
    same = same and torch.equal(want, CR.crop_resize_device_multi([frames.view(-1)], [j + (0,) for j in jobs], (oh, ow)))

    arena = RS._arenas[(dev, torch.cuda.current_stream(dev).cuda_stream)]
    at = arena.where

    def table(offsets):
        t = np.zeros(N, CR.CROP_JOB)
        for n, ((y0, x0, h, w), flip) in enumerate(draws):
            t[n] = (offsets[n], 3 * W, y0, x0, h, w) + at[(w, ow, 'bilinear')] + at[(h, oh, 'bilinear')] + (int(flip),)
        return t, torch.from_numpy(t.view(np.uint8)).to(dev)

    flat, flat_d = table([n * per for n in range(N)])
    _, spread_d = table([(n // S) * per for n in range(N)])
    max_vks = int(flat['vks'].max())
    zeros_d = torch.zeros(N, dtype=torch.int32, device=dev)
    index_d = (torch.arange(N, dtype=torch.int32) % S).to(dev)
    one_d = torch.tensor([frames.data_ptr()], dtype=torch.int64).to(dev)
    many_d = torch.tensor([s.data_ptr() for s in slabs], dtype=torch.int64).to(dev)
    outs = {}

    def single_of(library):
        fn = library.loans_crop_resize_u8_f32
        fn.argtypes, fn.restype = [ctypes.c_void_p] * 3 + [ctypes.c_int32, ctypes.c_void_p] + [ctypes.c_int32] * 3 + [ctypes.c_void_p], ctypes.c_int
        return lambda out: check(fn(_ptr(frames), _ptr(out), _ptr(flat_d), N, _ptr(arena.buf), max_vks, oh, ow, _stream()), 'single')

    def multi_of(srcs_d, index, jobs_d, n):
        return lambda out: check(lib.loans_crop_resize_srcs_u8_f32(_ptr(srcs_d), _ptr(index), n, _ptr(out), _ptr(jobs_d), N,
                                                                   _ptr(arena.buf), max_vks, oh, ow, _stream()), 'multi')

    arms = {}
    if a.parent_lib:
        arms['parent'] = single_of(ctypes.CDLL(os.path.abspath(a.parent_lib)))
    arms['single'] = single_of(lib)
    arms['multi-1'] = multi_of(one_d, zeros_d, flat_d, 1)
    arms['multi-%d' % S] = multi_of(many_d, index_d, spread_d, S)
    for k, fn in arms.items():
        outs[k] = torch.empty_like(want)
        for _ in range(10):
            fn(outs[k])
    torch.cuda.synchronize()
    same = same and all(torch.equal(o, want) for o in outs.values())

    def window(k):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(a.iters):
            arms[k](outs[k])
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) * 1e3 / a.iters

    times = {k: [] for k in arms}
    for _ in range(a.repeats):
        for k in arms:
            times[k].append(window(k))
    say('kernel: %d crops of %d x %d -> %d x %d (sample_rrc_box, seed %d); %s' % (N, H, W, oh, ow, a.seed, torch.cuda.get_device_name(dev)))
    say('all outputs identical: %s;  %d launches per window, %d windows per arm, alternating; microseconds per launch' % (same, a.iters, a.repeats))
    med = {k: float(np.median(v)) for k, v in times.items()}
    for k, v in times.items():
        say('%-9s median %7.1f   min %7.1f   max %7.1f   spread %5.1f   windows %s' % (k, med[k], min(v), max(v), max(v) - min(v), ' '.join('%.1f' % t for t in v)))
    base = 'parent' if 'parent' in arms else 'single'
    if base != 'parent':
        say('(no --parent-lib: ratios are against THIS tree\'s single-source launch, not against the parent commit)')
    for k in arms:
        if k != base:
            say('%s / %s (medians): %.3f' % (k, base, med[k] / med[base]))
    if not same:
        raise SystemExit('the arms disagree')


def feed_part(a, dev, say):
    from loans_amd.common.datasets.classification_dataset import ClassificationImageDataset
    from loans_amd.common.datasets.frame_cache import RaggedFrameCache
    from loans_amd.datasets import synthetic
    from loans_amd.runtime import training
    root = tempfile.mkdtemp(prefix='loans_cache_feed_')
    gen = np.random.Generator(np.random.PCG64(a.seed))
    base = [np.asarray(synthetic.make_composite(gen, 560, 700)[0])[..., :3].astype(np.uint8) for _ in range(16)]
    pairs, frame_bytes = [], 0
    for i in range(a.files):
        H, W = int(gen.integers(300, 451)), int(gen.integers(400, 601))                # around 375 x 500
        y, x = int(gen.integers(0, 560 - H + 1)), int(gen.integers(0, 700 - W + 1))
        Image.fromarray(base[i % 16][y:y + H, x:x + W]).save(os.path.join(root, 'f%05d.jpg' % i), quality=90)
        pairs.append(('f%05d.jpg' % i, i % 1000))
        frame_bytes += H * W * 3
    batches = a.files // a.b
    say('feed: %d JPEGs (300..450 x 400..600, %.1f MB decoded), batches of %d -> 224 x 224, %d decode processes on %d cores'
        % (a.files, frame_bytes / 1e6, a.b, a.processes, len(os.sched_getaffinity(0))))

    def epochs(cache, count):
        ds = ClassificationImageDataset(pairs, root, train=True, augment_seed=1, cache=cache)
        it = training.MultithreadIterator(ds, a.b, shuffle=True, n_threads=a.threads, n_processes=a.processes, device=dev.index)
        rates = []
        try:
            for _ in range(count):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(batches):
                    next(it)
                torch.cuda.synchronize()
                rates.append(batches * a.b / (time.perf_counter() - t0))
        finally:
            it.finalize()
        return rates, ds

    epochs(None, 1)                                                     # the files into the page cache, the kernels loaded
    rows = {'epoch 1, no cache': [], 'epoch 1, cache': [], 'epoch 2, cache': []}
    for _ in range(a.feed_repeats):
        rows['epoch 1, no cache'].append(epochs(None, 1)[0][0])
        cache = RaggedFrameCache(int(a.cache_gb * 1e9), a.where, dev)
        (e1, e2), ds = epochs(cache, 2)
        rows['epoch 1, cache'].append(e1)
        rows['epoch 2, cache'].append(e2)
    for k, v in rows.items():
        say('%-18s frames/s  median %9.0f   windows %s' % (k, float(np.median(v)), ' '.join('%.0f' % r for r in v)))
    say('cache (%s): %d frames, %.1f MB kept, %.1f MB allocated; the last two epochs: %d hits, %d misses'
        % (a.where, len(cache), cache.bytes / 1e6, cache.allocated / 1e6, cache.hits, cache.misses))
    say('epoch 1 with the cache / without (medians): %.3f;  epoch 2 with the cache / epoch 1 without: %.2f' % (
        np.median(rows['epoch 1, cache']) / np.median(rows['epoch 1, no cache']),
        np.median(rows['epoch 2, cache']) / np.median(rows['epoch 1, no cache'])))
    # bytes through the pinned staging copy per epoch: whole frames against the rows of the crops (counted from the draws)
    plain = ClassificationImageDataset(pairs, root, train=True, augment_seed=1)
    rows_bytes = 0
    for i in sorted(cache.slots):
        H, W = cache.location(i)[2:]
        rows_bytes += plain._draw(H, W)[0][2] * W * 3
    if rows_bytes:
        say('staged per epoch 1: %.1f MB of whole frames with the cache, %.1f MB of crop rows without (one draw each): %.2f x'
            % (cache.bytes / 1e6, rows_bytes / 1e6, cache.bytes / rows_bytes))
    # host time of a batch of hits: decode_batch + finish_batch, the GPU work only enqueued
    order = list(range(a.files))
    random.Random(a.seed).shuffle(order)
    for warm in (True, False):
        t = 0.0
        for k in range(batches):
            idx = order[k * a.b:(k + 1) * a.b]
            t0 = time.perf_counter()
            ds.finish_batch(ds.decode_batch(idx), dev)
            t += time.perf_counter() - t0
        torch.cuda.synchronize()
    say('host time of decode_batch + finish_batch on batches of hits (%d batches of %d, one thread, launch enqueued only): %.1f us per example'
        % (batches, a.b, t / (batches * a.b) * 1e6))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--parent-lib', default='', help="shared library with the commit-to-compare-against's loans_crop_resize_u8_f32")
    ap.add_argument('--slabs', type=int, default=8)
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--files', type=int, default=4096)
    ap.add_argument('-b', type=int, default=256)
    ap.add_argument('--threads', type=int, default=8)
    ap.add_argument('--processes', type=int, default=8)
    ap.add_argument('--cores', type=int, default=8, help="pin to the first N cores: one rank's share of the host (0: leave)")
    ap.add_argument('--cache-gb', type=float, default=8.0)
    ap.add_argument('--where', default='device', choices=['device', 'host'])
    ap.add_argument('--feed-repeats', type=int, default=3)
    ap.add_argument('--skip', default='', choices=['', 'kernel', 'feed'])
    ap.add_argument('--out', default=os.path.join('profiles', 'imagenet_cache_feed.txt'))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('cache_feed_bench needs a GPU: a time from anything else says nothing')
    if a.cores:
        os.sched_setaffinity(0, set(sorted(os.sched_getaffinity(0))[:a.cores]))
    dev = torch.device('cuda', torch.cuda.current_device())
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    if a.skip != 'kernel':
        kernel_part(a, dev, say)
    if a.skip != 'feed':
        feed_part(a, dev, say)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
