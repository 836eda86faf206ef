#!/usr/bin/env python
"""What ``--optimizer lamb`` costs (profiles/imagenet_lamb.txt): LAMB's three launches, separately and together, with their achieved
algorithmic bytes/s (24 bytes per parameter for the moments pass, 16 for the update) beside ``adam_kernel`` (28) and the LARS pair
whose streaming structures they are -- on the ResNet-50 classifier's own arena and segment tables -- and the step of
``train_imagenet.py`` with ``--optimizer lamb`` against ``--optimizer adam``.  Windows of launches between device events, the arms
alternating inside one sitting.

    python tools/lamb_bench.py --out imagenet_lamb.txt                            (kernels and step)
    python tools/lamb_bench.py --no-step                                          (kernels only)
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
    return e0.elapsed_time(e1) * 1e3 / launches         # microseconds per call


def kernels(a, say):
    import train_imagenet as T
    model = T.build_model(T.parse_args(['--seed', '0']))           # the ResNet-50 localizer under a Classifier
    model.to_gpu(0)
    arena = model.arena
    n = arena.numel
    arena.grad.normal_(0.0, 1e-3)
    lamb = loans_amd.LAMB(lr=1e-5, weight_decay_rate=5e-5, decay_exempt_1d=True).setup(model)
    lamb._ensure_state()
    m, v = lamb._state
    v.fill_(1e-6)
    table = lamb._segment_table(arena, n)
    units = table.workspace.numel() // 2
    params = sum(p.size for p in arena.params)
    say('kernels: the ResNet-50 classifier: %d parameters, arena of %d floats (%.1f MB), %d segments (%d units of %d floats); %s'
        % (params, n, n * 4 / 1e6, len(table), units, ops.LARS_UNIT, torch.cuda.get_device_name(0)))
    c1, c2 = 1.0 / (1.0 - 0.9 ** 100), 1.0 / (1.0 - 0.999 ** 100)
    hyper = (0.9, 0.999, c1, c2, 1e-6, 5e-5)

    def moments():
        ops.lamb_moments(arena.data, arena.grad, m, v, *hyper, table)

    def update():
        ops.lamb_update(arena.data, m, v, 1e-5, c1, c2, 1e-6, 5e-5, table)

    def whole():
        moments()
        ops.lamb_ratios(table)
        update()

    arms = [
        ('adam', 28 * n, lambda: ops.adam_amsgrad(arena.data, arena.grad, m, v, None, 1e-5, 0.9, 0.999, 1e-8, 1.0, 5e-5, 1.0)),
        ('lars ratios', 8 * n, lambda: ops.lars_ratios(arena.data, arena.grad, 5e-5, 0.001, 1e-8, table)),
        ('lars update', 20 * n, lambda: ops.lars_update(arena.data, arena.grad, m, 1e-5, 0.9, 5e-5, table)),
        ('lamb moments', 24 * n, moments),
        ('lamb fold', 16 * units, lambda: ops.lamb_ratios(table)),
        ('lamb update', 16 * n, update),
        ('lamb step', 40 * n, whole),
    ]
    for _, _, fn in arms:
        window(fn, 10)
    times = {name: [] for name, _, _ in arms}
    for _ in range(a.windows):
        for name, _, fn in arms:
            times[name].append(window(fn, a.launches))
    say('%d calls per window, %d windows per arm, alternating; microseconds per call (lars ratios: two launches per call, lamb step: three)'
        % (a.launches, a.windows))
    med, rate, spread = {}, {}, {}
    for name, nbytes, _ in arms:
        t = times[name]
        med[name], spread[name] = float(np.median(t)), max(t) - min(t)
        rate[name] = nbytes / (med[name] * 1e-6) / 1e12
        say('%-14s median %7.1f   min %7.1f   max %7.1f   spread %5.1f   %.2f TB/s of %s' % (
            name, med[name], min(t), max(t), spread[name], rate[name],
            '16 bytes per unit' if name == 'lamb fold' else '%d bytes per float' % (nbytes // n)))
    # a LAMB pass against the parent kernel whose streaming structure it is: algorithmic bytes/s, the margin the parent's own windows
    for mine, parent in (('lamb moments', 'lars ratios'), ('lamb update', 'lars update')):
        lo = rate[parent] * med[parent] / max(times[parent])
        say('%s %.2f TB/s against %s %.2f TB/s (its windows: %.2f .. %.2f): %s' % (
            mine, rate[mine], parent, rate[parent], lo, rate[parent] * med[parent] / min(times[parent]),
            'at or above its slowest window' if rate[mine] >= lo else 'BELOW its slowest window'))
    say('lamb step (medians): %.1f us for its three launches, %.1f us summed separately, against %.1f us for adam: %+.1f us' % (
        med['lamb step'], med['lamb moments'] + med['lamb fold'] + med['lamb update'], med['adam'], med['lamb step'] - med['adam']))
    del model, lamb


def step(a, say):
    import train_imagenet as T
    base = ['-b', str(a.batch_size), '--lr', '0.001', '--weight-decay', '5e-5', '--iterations', str(a.iterations),
            '--log-interval', '10', '--no-validation', '--seed', '0', '--dataset-size', str(2 * a.batch_size), '--synthetic-classes', '100',
            '--augment', 'rrc', '--augment-seed', '1', '--snapshot-interval', '100000', '--flat-log-dir']
    arms = [('adam', ['--optimizer', 'adam']), ('lamb', ['--optimizer', 'lamb'])]
    say('step: train_imagenet.py -b %d --weight-decay 5e-5 (ResNet-50 localizer, fp32, --augment rrc on the synthetic resident set), --optimizer adam against --optimizer lamb' % a.batch_size)
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
    say('lamb - adam (medians): %+.2f ms (%.2f %%);  spread of the adam runs: %.2f ms' % (
        med['lamb'] - med['adam'], (med['lamb'] / med['adam'] - 1) * 100, max(times['adam']) - min(times['adam'])))


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
