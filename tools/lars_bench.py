#!/usr/bin/env python
"""What ``--optimizer lars`` costs (profiles/imagenet_lars.txt): the ratios pass (norms of p and g per segment, two launches)
with its achieved bytes/s against the 8 bytes per parameter it has to read, the LARS update beside the segmented momentum SGD
it is modelled on -- on the ResNet-50 classifier's own arena and segment tables -- and the step of ``train_imagenet.py`` with
``--optimizer lars`` against ``--optimizer sgd --no-decay-1d``.  Windows of launches between device events, the arms alternating
inside one sitting.

    python tools/lars_bench.py --out imagenet_lars.txt                            (kernels and step)
    python tools/lars_bench.py --no-step                                          (kernels only)
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
    sgd = loans_amd.MomentumSGD(lr=1e-4, momentum=0.9, weight_decay_rate=5e-5, decay_exempt_1d=True).setup(model)
    sgd._ensure_state()
    v = sgd._state[0]
    decay_table = sgd._segment_table(arena, n)
    lars = loans_amd.LARS(lr=1e-4, momentum=0.9, weight_decay_rate=5e-5, decay_exempt_1d=True).setup(model)
    table = lars._segment_table(arena, n)
    units = table.workspace.numel() // 2
    params = sum(p.size for p in arena.params)
    say('kernels: the ResNet-50 classifier: %d parameters, arena of %d floats (%.1f MB), %d decay segments, %d LARS segments (%d units of %d floats); %s'
        % (params, n, n * 4 / 1e6, len(decay_table), len(table), units, ops.LARS_UNIT, torch.cuda.get_device_name(0)))
    arms = [
        ('sgd segmented', 20 * n, lambda: ops.momentum_sgd_seg(arena.data, arena.grad, v, 1e-4, 0.9, 5e-5, decay_table)),
        ('lars update', 20 * n, lambda: ops.lars_update(arena.data, arena.grad, v, 1e-4, 0.9, 5e-5, table)),
        ('lars ratios', 8 * n, lambda: ops.lars_ratios(arena.data, arena.grad, 5e-5, 0.001, 1e-8, table)),
    ]
    for _, _, fn in arms:
        window(fn, 10)
    times = {name: [] for name, _, _ in arms}
    for _ in range(a.windows):
        for name, _, fn in arms:
            times[name].append(window(fn, a.launches))
    say('%d calls per window, %d windows per arm, alternating; microseconds per call (lars ratios: two launches per call)' % (a.launches, a.windows))
    med = {}
    for name, nbytes, _ in arms:
        t = times[name]
        med[name] = float(np.median(t))
        say('%-20s median %7.1f   min %7.1f   max %7.1f   spread %5.1f   %.2f TB/s of %d bytes per float' % (
            name, med[name], min(t), max(t), max(t) - min(t), nbytes / (med[name] * 1e-6) / 1e12, nbytes // n))
    spread = max(times['sgd segmented']) - min(times['sgd segmented'])
    say('lars update - sgd segmented (medians): %+.1f us; spread of the sgd windows: %.1f us: %s' % (
        med['lars update'] - med['sgd segmented'], spread, 'equal within it' if abs(med['lars update'] - med['sgd segmented']) <= spread else 'DIFFERENT'))
    say('lars ratios + lars update (medians): %.1f us per step against %.1f us for sgd segmented' % (
        med['lars ratios'] + med['lars update'], med['sgd segmented']))
    del model, sgd, lars


def step(a, say):
    import train_imagenet as T
    base = ['-b', str(a.batch_size), '--lr', '0.1', '--weight-decay', '5e-5', '--no-decay-1d', '--iterations', str(a.iterations),
            '--log-interval', '10', '--no-validation', '--seed', '0', '--dataset-size', str(2 * a.batch_size), '--synthetic-classes', '100',
            '--augment', 'rrc', '--augment-seed', '1', '--snapshot-interval', '100000', '--flat-log-dir']
    arms = [('sgd', ['--optimizer', 'sgd']), ('lars', ['--optimizer', 'lars'])]
    say('step: train_imagenet.py -b %d --weight-decay 5e-5 --no-decay-1d (ResNet-50 localizer, fp32, --augment rrc on the synthetic resident set), --optimizer sgd against --optimizer lars' % a.batch_size)
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
    say('lars - sgd (medians): %+.2f ms (%.2f %%);  spread of the sgd runs: %.2f ms' % (
        med['lars'] - med['sgd'], (med['lars'] / med['sgd'] - 1) * 100, max(times['sgd']) - min(times['sgd'])))


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
