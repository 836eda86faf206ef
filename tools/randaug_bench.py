#!/usr/bin/env python
"""What the RandAugment stage costs (profiles/imagenet_randaug.txt): the launches of csrc/randaug.hip alone at 256 x 3 x 224 x 224
-- the statistics entry with every image taking Contrast, AutoContrast or Equalize; one apply layer of a pointwise op (Solarize),
of Rotate at 30 degrees and of Sharpness; the whole stage on the drawn jobs of ``--rand-augment 2 9`` -- in microseconds beside the
HBM bound of the bytes each has to move, and the step of ``train_imagenet.py`` with ``--rand-augment 2 9`` against the same command
without it, and against that command in a checkout of the parent commit (``--parent DIR``, its library built).  Windows of launches
between device events; the step arms are child processes that alternate inside one sitting.

    python tools/randaug_bench.py --out imagenet_randaug.txt --parent ../parent       (kernels and step)
    python tools/randaug_bench.py --no-step                                           (kernels only)
"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np      # noqa: E402
import torch            # noqa: E402

from loans_amd import _lib, ops                                 # noqa: E402
from loans_amd.common.datasets import rand_augment as RA        # noqa: E402

HBM_TBS = 8.0           # the MI355X's HBM3E peak, TB/s: the bound is the bytes below at this rate


def window(fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / launches         # microseconds per call


def kernels(a, say):
    B, H, W = a.batch_size, 224, 224
    rng = np.random.RandomState(0)
    x = torch.from_numpy((rng.randint(0, 256, (B, 3, H, W)).astype(np.float32) / np.float32(255))).cuda()
    out = torch.empty_like(x)
    lib = _lib.load()
    ws_bytes = int(lib.loans_ra_workspace_bytes(B, H, W))
    ws = torch.empty(ws_bytes, device='cuda', dtype=torch.uint8)
    batch_bytes = x.numel() * 4
    drawn = RA.RandAugmentPolicy('rand', 2, 9, seed=0).draw_batch(B, H, W)
    moving = [int(((drawn['op'][:, l] >= 1) & (drawn['op'][:, l] <= 5) | (drawn['op'][:, l] == 9)).sum()) for l in range(2)]
    counting = [int(np.isin(drawn['op'][:, l], (8, 12, 13)).sum()) for l in range(2)]
    say('kernels: %d x 3 x %d x %d fp32 (%.1f MB) on the byte grid; drawn jobs of RandAugmentPolicy(rand, 2, 9): gathers or Sharpness in %s, '
        'statistics in %s of %d images per layer; %s' % (B, H, W, batch_bytes / 1e6, moving, counting, B, torch.cuda.get_device_name(0)))
    st = ops._stream
    tables = {}

    def table(name, layers):
        jobs = np.array([RA.make_job(layers, H, W)] * B) if isinstance(layers, list) else layers
        tables[name] = (jobs, torch.from_numpy(jobs.view(np.uint8).copy()).cuda())
        return name

    def stats(name):
        jobs, jobs_d = tables[name]

        def fn():
            ops.check(lib.loans_ra_stats_f32(x.data_ptr(), B, 3, H, W, jobs_d.data_ptr(), jobs.ctypes.data, 0, ws.data_ptr(), ws_bytes, st()), name)
        return fn

    def stage(name):
        jobs, jobs_d = tables[name]

        def fn():           # out of place, as the feed runs it
            ops.check(lib.loans_ra_apply_f32(x.data_ptr(), out.data_ptr(), B, 3, H, W, jobs_d.data_ptr(), jobs.ctypes.data, ws.data_ptr(),
                                             ws_bytes, st()), name)
        return fn

    # bytes a call has to move: a statistics step reads the batch, an apply layer reads and writes it; the drawn stage has two
    # apply layers and reads the images that take a statistic once more
    drawn_bytes = 4 * batch_bytes + sum(counting) * (batch_bytes // B)
    arms = [('stats, Contrast', batch_bytes, stats(table('contrast', [(8, 0.27)]))),
            ('stats, AutoContrast', batch_bytes, stats(table('autocontrast', [(12, None)]))),
            ('stats, Equalize', batch_bytes, stats(table('equalize', [(13, None)]))),
            ('apply, Solarize', 2 * batch_bytes, stage(table('solarize', [(11, 0.7)]))),
            ('apply, Rotate 30', 2 * batch_bytes, stage(table('rotate', [(5, 30.0)]))),
            ('apply, Sharpness', 2 * batch_bytes, stage(table('sharpness', [(9, 0.27)]))),
            ('stage, drawn 2 9', drawn_bytes, stage(table('drawn', drawn)))]
    for _, _, fn in arms:
        window(fn, 5)
    times = {name: [] for name, _, _ in arms}
    for _ in range(a.windows):
        for name, _, fn in arms:
            times[name].append(window(fn, a.launches))
    say('%d calls per window, %d windows per arm, alternating; microseconds per call; bound = bytes / %.1f TB/s' % (a.launches, a.windows, HBM_TBS))
    for name, nbytes, _ in arms:
        t = times[name]
        med = float(np.median(t))
        bound = nbytes / (HBM_TBS * 1e12) * 1e6
        say('%-22s median %7.1f   min %7.1f   max %7.1f   spread %5.1f   %.2f TB/s of %.2f batch-sized streams   bound %.1f us: %.0f %% of it' % (
            name, med, min(t), max(t), max(t) - min(t), nbytes / (med * 1e-6) / 1e12, nbytes / batch_bytes, bound, 100 * bound / med))
    # the draws, on the host
    import time
    policy = RA.RandAugmentPolicy('rand', 2, 9, seed=1)
    t0 = time.perf_counter()
    for _ in range(20):
        policy.draw_batch(B, H, W)
    say('draw_batch(%d, %d, %d) of RandAugmentPolicy(rand, 2, 9): %.2f ms of interpreter per batch' % (B, H, W, (time.perf_counter() - t0) / 20 * 1e3))


CHILD = '''
import sys, tempfile
import train_imagenet as T
iterations = int(sys.argv[1])
with tempfile.TemporaryDirectory() as log_dir:
    entries, model = T.run(T.parse_args(sys.argv[2:] + ['-l', log_dir]), log=lambda *x: None)
at = {e['iteration']: e['elapsed_time'] for e in entries}
print('MS_PER_STEP %.4f' % ((at[iterations] - at[10]) / (iterations - 10) * 1e3))
'''


def step_time(tree, argv, iterations):
    """ms per step of ``train_imagenet.py`` in the checkout ``tree``, in a child process of its own"""
    text = subprocess.check_output([sys.executable, '-c', CHILD, str(iterations)] + argv, cwd=tree, timeout=600).decode()
    return float([line for line in text.splitlines() if line.startswith('MS_PER_STEP')][-1].split()[1])


def step(a, say):
    base = ['-b', str(a.batch_size), '--optimizer', 'sgd', '--lr', '0.1', '--weight-decay', '5e-5', '--iterations', str(a.iterations),
            '--log-interval', '10', '--no-validation', '--seed', '0', '--dataset-size', str(2 * a.batch_size), '--synthetic-classes', '100',
            '--augment', 'rrc', '--augment-seed', '1', '--snapshot-interval', '100000', '--flat-log-dir']
    ra = ['--rand-augment', '2', '9', '--ra-seed', '2']
    arms = [('plain', ROOT, []), ('rand-augment 2 9', ROOT, ra)]
    if a.parent:
        arms.insert(0, ('parent commit', os.path.abspath(a.parent), []))
    say('step: train_imagenet.py -b %d --optimizer sgd (ResNet-50 localizer, fp32, --augment rrc on the synthetic resident set), without and with %s%s'
        % (a.batch_size, ' '.join(ra[:3]), ', and the plain command in a checkout of the parent commit' if a.parent else ''))
    say('%d runs per arm, a process each, alternating; ms per step over iterations 11..%d of each run (host clock between two synchronising log entries)'
        % (a.runs, a.iterations))
    times = {name: [] for name, _, _ in arms}
    for _ in range(a.runs):
        for name, tree, more in arms:
            times[name].append(step_time(tree, base + more, a.iterations))
    med = {}
    for name, _, _ in arms:
        t = times[name]
        med[name] = float(np.median(t))
        say('%-18s median %8.2f   min %8.2f   max %8.2f   runs %s' % (name, med[name], min(t), max(t), ' '.join('%.2f' % x for x in t)))
    reference = 'parent commit' if a.parent else 'plain'
    spread = max(times[reference]) - min(times[reference])
    for name in [n for n, _, _ in arms if n != reference]:
        d = med[name] - med[reference]
        say('%s - %s (medians): %+.2f ms (%.2f %%);  spread of the %s runs: %.2f ms: %s' % (
            name, reference, d, (med[name] / med[reference] - 1) * 100, reference, spread, 'inside it' if abs(d) <= spread else 'OUTSIDE it'))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=30)
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('-b', '--batch-size', type=int, default=256)
    ap.add_argument('--iterations', type=int, default=40)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--parent', default=None, help='a checkout of the parent commit with its kernel library built: its step is timed too')
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
