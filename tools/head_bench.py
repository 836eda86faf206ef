#!/usr/bin/env python
"""What ``--head-dtype bf16`` buys (profiles/imagenet_head16.txt): each direction of the wide Linear alone -- forward, data gradient,
weight gradient -- at B = 256, K = 512 / 2048 and N = 1000 / 10450 / 21841, the bf16 entries (``loans_linear_wide16_*``) against the
fp32 entries of the same build, as a fraction of the HBM time of the direction's compulsory traffic (ops.ROOFLINE_HBM), and the
batch-256 ResNet-50 step of tools/imagenet_step.py at ``--dtype bf16 --num-classes 21841`` with and without the option.  Windows of
calls between device events, the arms alternating inside one sitting.

    python tools/head_bench.py --out imagenet_head16.txt
"""
import argparse
import contextlib
import io
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np      # noqa: E402
import torch            # noqa: E402

from loans_amd import ops       # noqa: E402

KS, NS = (512, 2048), (1000, 10450, 21841)


def window(fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / launches         # microseconds per call


def directions(B, K, N):
    """[(name, compulsory bytes, fn(compute))]"""
    g = torch.Generator().manual_seed(N + K)
    x, W, b, gy = (torch.randn(*s, generator=g).cuda() for s in ((B, K), (N, K), (N,), (B, N)))
    gW = torch.zeros(N, K, device='cuda')
    f = 4
    return [('forward', f * (N * K + B * K + B * N), lambda c: ops.linear_wide_fwd(x, W, b, compute=c)),
            ('data gradient', f * (N * K + B * N + B * K), lambda c: ops.linear_wide_bwd(x, W, gy, compute=c)),
            ('weight gradient', f * (2 * N * K + B * N + B * K), lambda c: ops.linear_wide_bwd(x, W, gy, gW=gW, need_gx=False, compute=c))]


def kernels(a, say):
    say('the wide Linear alone: B = %d; %s; %d windows per arm, alternating f32 / bf16, each window about %.2f s of calls; '
        'microseconds per call' % (a.batch_size, torch.cuda.get_device_name(0), a.windows, a.window_s))
    for K in KS:
        for N in NS:
            for name, nbytes, fn in directions(a.batch_size, K, N):
                times, launches = {}, {}
                for c in ('f32', 'bf16'):
                    window(lambda: fn(c), 3)
                    launches[c] = int(min(max(a.window_s * 1e6 / window(lambda: fn(c), 5), 5), 2000))
                    times[c] = []
                for _ in range(a.windows):
                    for c in ('f32', 'bf16'):
                        times[c].append(window(lambda: fn(c), launches[c]))
                hbm = nbytes / ops.ROOFLINE_HBM * 1e6
                m32, m16 = np.median(times['f32']), np.median(times['bf16'])
                spread = max(max(t) - min(t) for t in times.values())
                say('K %4d N %5d %-15s  f32 median %8.2f (min %8.2f max %8.2f)   bf16 median %8.2f (min %8.2f max %8.2f)   f32 / bf16 %5.2f   '
                    'gap %8.2f against a spread of %6.2f   HBM time %6.2f us: f32 %4.1f %%, bf16 %4.1f %% of it'
                    % (K, N, name, m32, min(times['f32']), max(times['f32']), m16, min(times['bf16']), max(times['bf16']), m32 / m16,
                       m32 - m16, spread, hbm, 100 * hbm / m32, 100 * hbm / m16))


def step(a, say):
    import imagenet_step
    base = ['-b', str(a.batch_size), '--steps', str(a.steps), '--warmup', str(a.warmup), '--resnet-50', '--dtype', 'bf16', '--num-classes', '21841']
    arms = [('fp32 head', base), ('bf16 head', base + ['--head-dtype', 'bf16'])]
    say('the step: tools/imagenet_step.py %s (ResNet-50 localizer, Adam, one resident batch) with and without --head-dtype bf16; %d runs '
        'per arm, alternating; ms per step, the median of %d steps between device events behind %d warm-up steps'
        % (' '.join(base), a.runs, a.steps, a.warmup))
    times = {name: [] for name, _ in arms}
    for _ in range(a.runs):
        for name, argv in arms:
            with contextlib.redirect_stdout(io.StringIO()):
                times[name].append(imagenet_step.main(argv)['step_ms_median'])
            torch.cuda.synchronize()
    for name, _ in arms:
        t = times[name]
        say('%-10s median %8.2f   min %8.2f   max %8.2f   spread %5.2f   runs %s'
            % (name, np.median(t), min(t), max(t), max(t) - min(t), ' '.join('%.2f' % x for x in t)))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--window-s', type=float, default=0.1, help='seconds of calls per window (5 .. 2000 calls)')
    ap.add_argument('-b', '--batch-size', type=int, default=256)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--no-step', action='store_true')
    ap.add_argument('--no-kernels', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args(argv)
    assert torch.cuda.is_available(), 'this measurement needs a GPU'
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)
        if a.out:
            with open(a.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')

    if not a.no_kernels:
        kernels(a, say)
    if not a.no_step:
        step(a, say)


if __name__ == '__main__':
    main()
