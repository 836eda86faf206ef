#!/usr/bin/env python
"""What the second half of the ImageNet recipe costs (profiles/imagenet_ema.txt): the segmented momentum SGD against the plain
kernel, the weight average's UPDATE (with and without the BN statistics jobs) and SWAP -- on the ResNet-50 classifier's own
arena, segment table and job table -- and the step of ``train_imagenet.py`` with and without ``--ema-decay 0.9999 --no-decay-1d``.
Windows of launches between device events, the arms alternating inside one sitting.

    python tools/ema_bench.py --out imagenet_ema.txt                              (kernels and step)
    python tools/ema_bench.py --no-step                                           (kernels only)
"""
import argparse
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np      # noqa: E402
import torch            # noqa: E402

import loans_amd        # noqa: E402
from loans_amd import ops       # noqa: E402


def window(fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / launches         # microseconds per launch


def kernels(a, say):
    import train_imagenet as T
    model = T.build_model(T.parse_args(['--seed', '0']))           # the ResNet-50 localizer under a Classifier
    model.to_gpu(0)
    arena = model.arena
    n = arena.numel
    arena.grad.normal_(0.0, 1e-3)
    opt = loans_amd.MomentumSGD(lr=1e-4, momentum=0.9, weight_decay_rate=1e-4, decay_exempt_1d=True).setup(model)
    opt._ensure_state()
    v = opt._state[0]
    table = opt._segment_table(arena, n)
    average = loans_amd.WeightAverage(model, 0.9999)
    arena_only = ops.AverageJobs([(average.avg, arena.data)])
    params = sum(p.size for p in arena.params)
    say('kernels: the ResNet-50 classifier: %d parameters, arena of %d floats (%.1f MB), %d decay segments, %d average jobs (%d units of %d floats); %s'
        % (params, n, n * 4 / 1e6, len(table), average._jobs.njobs, average._jobs.units, 4096, torch.cuda.get_device_name(0)))
    arms = [
        ('sgd plain', 20 * n, lambda: ops.momentum_sgd(arena.data, arena.grad, v, 1e-4, 0.9, 1e-4)),
        ('sgd segmented', 20 * n, lambda: ops.momentum_sgd_seg(arena.data, arena.grad, v, 1e-4, 0.9, 1e-4, table)),
        ('update, all jobs', 12 * sum(d.numel() for d, _ in average._jobs.pairs), lambda: ops.average_jobs(average._jobs, 'update', 1e-4)),
        ('update, arena only', 12 * n, lambda: ops.average_jobs(arena_only, 'update', 1e-4)),
        ('swap, all jobs', 16 * sum(d.numel() for d, _ in average._jobs.pairs), lambda: ops.average_jobs(average._jobs, 'swap')),
    ]
    for _, _, fn in arms:
        window(fn, 10)
    times = {name: [] for name, _, _ in arms}
    for _ in range(a.windows):
        for name, _, fn in arms:
            times[name].append(window(fn, a.launches))
    say('%d launches per window, %d windows per arm, alternating; microseconds per launch' % (a.launches, a.windows))
    med = {}
    for name, nbytes, _ in arms:
        t = times[name]
        med[name] = float(np.median(t))
        say('%-20s median %7.1f   min %7.1f   max %7.1f   spread %5.1f   %.2f TB/s of %d bytes per float' % (
            name, med[name], min(t), max(t), max(t) - min(t), nbytes / (med[name] * 1e-6) / 1e12, nbytes // n))
    spread = max(times['sgd plain']) - min(times['sgd plain'])
    say('sgd segmented - sgd plain (medians): %+.1f us; spread of the plain windows: %.1f us: %s' % (
        med['sgd segmented'] - med['sgd plain'], spread, 'not slower beyond it' if med['sgd segmented'] - med['sgd plain'] <= spread else 'SLOWER'))
    say('update, all jobs - arena only (medians): %+.1f us for the %d small jobs of the one-launch form' % (
        med['update, all jobs'] - med['update, arena only'], average._jobs.njobs - 1))
    del model, opt, average


def step(a, say):
    import train_imagenet as T
    base = ['-b', str(a.batch_size), '--optimizer', 'sgd', '--lr', '0.1', '--weight-decay', '1e-4', '--iterations', str(a.iterations),
            '--log-interval', '10', '--no-validation', '--seed', '0', '--dataset-size', str(2 * a.batch_size), '--synthetic-classes', '100',
            '--augment', 'rrc', '--augment-seed', '1', '--snapshot-interval', '100000', '--flat-log-dir']
    arms = [('plain', []), ('ema + no-decay-1d', ['--ema-decay', '0.9999', '--no-decay-1d'])]
    say('step: train_imagenet.py -b %d --optimizer sgd (ResNet-50 localizer, fp32, --augment rrc on the synthetic resident set), with and without --ema-decay 0.9999 --no-decay-1d' % a.batch_size)
    say('%d runs per arm, alternating; ms per step over iterations 11..%d of each run (host clock between two synchronising log entries)' % (a.runs, a.iterations))
    times = {name: [] for name, _ in arms}
    for _ in range(a.runs):
        for name, more in arms:
            with tempfile.TemporaryDirectory() as log_dir:          # (the run's final snapshots: 100 MB each)
                entries, model = T.run(T.parse_args(base + more + ['-l', log_dir]), log=lambda *x: None)
            at = {e['iteration']: e['elapsed_time'] for e in entries}
            times[name].append((at[a.iterations] - at[10]) / (a.iterations - 10) * 1e3)
            del model
            torch.cuda.synchronize()
            time.sleep(0.1)
    med = {}
    for name, _ in arms:
        t = times[name]
        med[name] = float(np.median(t))
        say('%-18s median %8.2f   min %8.2f   max %8.2f   runs %s' % (name, med[name], min(t), max(t), ' '.join('%.2f' % x for x in t)))
    say('ema + no-decay-1d - plain (medians): %+.2f ms (%.2f %%);  spread of the plain runs: %.2f ms' % (
        med['ema + no-decay-1d'] - med['plain'], (med['ema + no-decay-1d'] / med['plain'] - 1) * 100, max(times['plain']) - min(times['plain'])))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=50)
    ap.add_argument('--windows', type=int, default=9)
    ap.add_argument('-b', '--batch-size', type=int, default=256)
    ap.add_argument('--iterations', type=int, default=40)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--no-step', action='store_true')
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

    kernels(a, say)
    if not a.no_step:
        step(a, say)


if __name__ == '__main__':
    main()
