#!/usr/bin/env python
"""Timing of mixup / CutMix in the ImageNet feed (profiles/imagenet_mix.txt).

  kernel: loans_batch_mix_f32 at 256 x 3 x 224 x 224, mixup (three tensor-sized streams) and CutMix (two), beside a
          device-to-device copy (``clone``: two streams) of the same tensor -- windows of launches between device events, the arms
          alternating inside one process.
  step:   ms per step of ``train_imagenet.py -b 256 --augment rrc --optimizer sgd`` on the synthetic resident set with and without
          ``--mixup-alpha 0.2 --cutmix-alpha 1.0``, the runs alternating inside one process; per run the time between two log
          entries (each ends in a host synchronisation), the iterations before the first one being the warm-up.

usage: mix_bench.py [kernel|step|all] [--out FILE]"""
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from loans_amd import ops                                             # noqa: E402
from loans_amd.common.datasets.batch_mix import cutmix_box            # noqa: E402
from loans_amd.mixed_labels import MixedLabels                        # noqa: E402

SHAPE = (256, 3, 224, 224)
LAUNCHES, WINDOWS = 100, 9


def window(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(LAUNCHES):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / LAUNCHES           # microseconds per launch


def kernel(say):
    x = torch.rand(SHAPE, device='cuda')
    out = torch.empty_like(x)
    lam32, oml32 = MixedLabels.weights(0.3)
    box, weight = cutmix_box(0.5, 112, 112, 224, 224)     # a centred cut of half the frame's area
    nbytes = x.numel() * 4
    arms = {'clone': (lambda: out.copy_(x), 2),
            'mixup': (lambda: ops.batch_mix(x, 1, lam32, oml32, out=out), 3),
            'cutmix': (lambda: ops.batch_mix(x, 1, 1.0, 0.0, box, out=out), 2)}
    for fn, _ in arms.values():                           # warm-up: code objects, clocks
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in arms}
    for _ in range(WINDOWS):
        for name, (fn, _) in arms.items():
            times[name].append(window(fn))
    say('kernel: %d x %d x %d x %d fp32 (%.1f MB), shift 1, mixup weights (%.4f, %.4f), CutMix box %r (label weight %.3f); %s'
        % (SHAPE + (nbytes / 1e6, lam32, oml32, box, weight, torch.cuda.get_device_name(0))))
    say('%d launches per window, %d windows per arm, alternating; microseconds per launch' % (LAUNCHES, WINDOWS))
    med = {}
    for name, (_, streams) in arms.items():
        t = np.array(times[name])
        med[name] = float(np.median(t))
        say('%-7s median %7.1f   min %7.1f   max %7.1f   spread %5.1f   %.2f TB/s of %d tensor-sized streams   windows %s'
            % (name, med[name], t.min(), t.max(), t.max() - t.min(), streams * nbytes / med[name] / 1e6, streams,
               ' '.join('%.1f' % v for v in t)))
    spread = max(times['clone']) - min(times['clone'])
    for name in ('mixup', 'cutmix'):
        allowed = 1.5 * med['clone'] + spread
        say('%s / clone (medians): %.3f;  1.5 x clone + the clone windows\' spread = %.1f us: %s'
            % (name, med[name] / med['clone'], allowed, 'met' if med[name] <= allowed else 'MISSED'))


def step(say, runs=3, iterations=40, interval=10):
    import train_imagenet as T
    base = ['-b', '256', '--augment', 'rrc', '--optimizer', 'sgd', '--no-validation', '--iterations', str(iterations),
            '--log-interval', str(interval), '--snapshot-interval', '100000', '--flat-log-dir', '--seed', '0', '--augment-seed', '1']
    arms = {'plain': [], 'mixed': ['--mixup-alpha', '0.2', '--cutmix-alpha', '1.0', '--mix-seed', '3']}
    times = {name: [] for name in arms}
    for _ in range(runs):
        for name, extra in arms.items():
            with tempfile.TemporaryDirectory() as log_dir:
                log, _ = T.run(T.parse_args(base + extra + ['-l', log_dir]), log=lambda *a: None)
            stamps = {e['iteration']: e['elapsed_time'] for e in log if e['iteration'] % interval == 0}
            times[name].append((stamps[iterations] - stamps[interval]) * 1e3 / (iterations - interval))
    say('step: train_imagenet.py -b 256 --augment rrc --optimizer sgd (ResNet-50 localizer, fp32, synthetic resident set), '
        'with and without --mixup-alpha 0.2 --cutmix-alpha 1.0')
    say('%d runs per arm, alternating; ms per step over iterations %d..%d of each run (host clock between two synchronising log entries)'
        % (runs, interval + 1, iterations))
    for name, t in times.items():
        say('%-6s median %8.2f   min %8.2f   max %8.2f   runs %s' % (name, np.median(t), min(t), max(t), ' '.join('%.2f' % v for v in t)))
    say('mixed / plain (medians): %.4f;  spread of the plain runs: %.2f ms' % (
        np.median(times['mixed']) / np.median(times['plain']), max(times['plain']) - min(times['plain'])))


def main(argv):
    what = argv[0] if argv and not argv[0].startswith('-') else 'all'
    out = open(argv[argv.index('--out') + 1], 'a') if '--out' in argv else None

    def say(line):
        print(line, flush=True)
        if out is not None:
            out.write(line + '\n')
            out.flush()

    assert torch.cuda.is_available(), 'a measurement needs the GPU'
    if what in ('kernel', 'all'):
        kernel(say)
    if what in ('step', 'all'):
        step(say)


if __name__ == '__main__':
    main(sys.argv[1:])
