#!/usr/bin/env python
"""What ``--num-classes`` above 8192 costs (profiles/imagenet_21k.txt): the launches of ``loans_softmax_xent_split_fwd_f32`` at
B = 256 and N = 10450 / 21841 against their HBM time (two reads and one write of the logits at ops.ROOFLINE_HBM), the mix entry at
N = 1000 in the same rotation (``--only-mix``: that arm alone, for a tree without the split entries), and the batch-256 ResNet-50
step of tools/imagenet_step.py with and without ``--num-classes 21841``.  Windows of calls between device events, the arms
alternating inside one sitting.

    python tools/split_xent_bench.py --out imagenet_21k.txt
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
from loans_amd.mixed_labels import MixedLabels      # noqa: E402

EPS, TOPK = 0.1, 5


def window(fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / launches         # microseconds per call


def kernels(a, say):
    lam, oml = MixedLabels.weights(0.3)
    arms = []
    for name, N, split in [('mix N 1000', 1000, False)] + ([] if a.only_mix else [('split N 10450', 10450, True), ('split N 21841', 21841, True),
                                                                                  ('split N 21841 one label', 21841, True)]):
        rng = np.random.RandomState(N)
        z = torch.from_numpy((3.0 * rng.standard_normal((a.batch_size, N))).astype(np.float32)).cuda()
        ta = torch.from_numpy(rng.randint(0, N, a.batch_size).astype(np.int32)).cuda()
        w = (1.0, 0.0) if 'one label' in name else (lam, oml)
        fwd = ops.softmax_xent_split_fwd if split else ops.softmax_xent_mix_fwd
        arms.append((name, N, (lambda fwd=fwd, z=z, ta=ta, tb=torch.roll(ta, 1), w=w: fwd(z, ta, tb, w[0], w[1], EPS, TOPK))))
    say('the loss alone: B = %d, eps %g, k %d, weights (%.9g, %.9g); %s' % (a.batch_size, EPS, TOPK, lam, oml, torch.cuda.get_device_name(0)))
    for _, _, fn in arms:
        window(fn, 20)
    times = {name: [] for name, _, _ in arms}
    for _ in range(a.windows):
        for name, _, fn in arms:
            times[name].append(window(fn, a.launches))
    say('%d calls per window, %d windows per arm, alternating; microseconds per call (three launches per split call, two per mix call)'
        % (a.launches, a.windows))
    for name, N, _ in arms:
        t, reads = times[name], 2 if name.startswith('split') else 1
        hbm = (reads + 1) * 4 * a.batch_size * N / ops.ROOFLINE_HBM * 1e6
        say('%-26s median %7.2f   min %7.2f   max %7.2f   spread %5.2f   HBM time of %d read(s) + 1 write: %6.2f us (%.0f %% of it)'
            % (name, np.median(t), min(t), max(t), max(t) - min(t), reads, hbm, 100 * hbm / np.median(t)))


def step(a, say):
    import imagenet_step
    base = ['-b', str(a.batch_size), '--steps', str(a.steps), '--warmup', str(a.warmup), '--label-smoothing', str(EPS), '--resnet-50']
    arms = [('1000 classes', base)] + ([] if a.only_mix else [('21841 classes', base + ['--num-classes', '21841'])])
    say('the step: tools/imagenet_step.py %s (ResNet-50 localizer, Adam, fp32, one resident batch); %d runs per arm, alternating; ms '
        'per step, the median of %d steps between device events behind %d warm-up steps' % (' '.join(base), a.runs, a.steps, a.warmup))
    times = {name: [] for name, _ in arms}
    for _ in range(a.runs):
        for name, argv in arms:
            with contextlib.redirect_stdout(io.StringIO()):
                times[name].append(imagenet_step.main(argv)['step_ms_median'])
            torch.cuda.synchronize()
    for name, _ in arms:
        t = times[name]
        say('%-14s median %8.2f   min %8.2f   max %8.2f   spread %5.2f   runs %s'
            % (name, np.median(t), min(t), max(t), max(t) - min(t), ' '.join('%.2f' % x for x in t)))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=2000)
    ap.add_argument('--windows', type=int, default=15)
    ap.add_argument('-b', '--batch-size', type=int, default=256)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--only-mix', action='store_true', help='the arms a tree without the split entries has: the mix entry, the 1000-class step')
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
