#!/usr/bin/env python
"""What ``--loss bce`` costs (profiles/imagenet_bce.txt): the two launches of ``loans_sigmoid_bce_fwd_f32`` beside the two of
``loans_softmax_xent_mix_fwd_f32`` at B = 256, N = 1000 with the same labels and weights -- both read the logits once and write
gz once -- with the spread the softmax launches show against themselves (a second softmax arm in the same rotation); and the
batch-256 ResNet-50 step of tools/imagenet_step.py with ``--loss bce`` beside the same command without it.  Windows of calls
between device events, the arms alternating inside one sitting.

    python tools/bce_bench.py --out imagenet_bce.txt                              (the loss and the step)
    python tools/bce_bench.py --no-step                                           (the loss only)
"""
import argparse
import contextlib
import io
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np      # noqa: E402
import torch            # noqa: E402

from loans_amd import ops       # noqa: E402
from loans_amd.mixed_labels import MixedLabels      # noqa: E402

EPS, TOPK, THRESH = 0.1, 5, 0.2


def window(fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / launches         # microseconds per call


def kernels(a, say):
    B, N = a.batch_size, a.classes
    rng = np.random.RandomState(0)
    z = torch.from_numpy((3.0 * rng.standard_normal((B, N))).astype(np.float32)).cuda()
    ta = torch.from_numpy(rng.randint(0, N, B).astype(np.int32)).cuda()
    tb = torch.roll(ta, 1)
    lam, oml = MixedLabels.weights(0.3)
    say('the loss alone: B = %d, N = %d, weights (%.9g, %.9g), eps %g, k %d; %s' % (B, N, lam, oml, EPS, TOPK, torch.cuda.get_device_name(0)))
    arms = [
        ('softmax mix', lambda: ops.softmax_xent_mix_fwd(z, ta, tb, lam, oml, EPS, TOPK)),
        ('sigmoid bce', lambda: ops.sigmoid_bce_fwd(z, ta, tb, lam, oml, EPS, TOPK)),
        ('softmax mix (again)', lambda: ops.softmax_xent_mix_fwd(z, ta, tb, lam, oml, EPS, TOPK)),
        ('sigmoid bce thresh %g' % THRESH, lambda: ops.sigmoid_bce_fwd(z, ta, tb, lam, oml, EPS, TOPK, THRESH)),
        ('sigmoid bce one label', lambda: ops.sigmoid_bce_fwd(z, ta, None, 1.0, 0.0, EPS, TOPK)),
    ]
    for _, fn in arms:
        window(fn, 20)
    times = {name: [] for name, _ in arms}
    for _ in range(a.windows):
        for name, fn in arms:
            times[name].append(window(fn, a.launches))
    say('%d calls per window, %d windows per arm, alternating; microseconds per call (two launches and five small allocations per call)'
        % (a.launches, a.windows))
    nbytes = 2 * 4 * B * N          # the logits read once, gz written once
    med = {}
    for name, _ in arms:
        t = times[name]
        med[name] = float(np.median(t))
        say('%-26s median %7.2f   min %7.2f   max %7.2f   spread %5.2f   (%.0f GB/s of %d bytes per call)'
            % (name, med[name], min(t), max(t), max(t) - min(t), nbytes / (med[name] * 1e-6) / 1e9, nbytes))
    both = times['softmax mix'] + times['softmax mix (again)']
    say('bce - softmax (medians): %+.2f us;  the two softmax arms against each other: %+.2f us (medians), %.2f us (all their windows, max - min)'
        % (med['sigmoid bce'] - med['softmax mix'], med['softmax mix (again)'] - med['softmax mix'], max(both) - min(both)))
    out = ops.sigmoid_bce_fwd(z, ta, tb, lam, oml, EPS, TOPK)[0].cpu().tolist()
    soft = ops.softmax_xent_mix_fwd(z, ta, tb, lam, oml, EPS, TOPK)[0].cpu().tolist()
    say('(what they computed: bce loss %.6f, softmax loss %.6f; accuracy %.4f / %.4f both)' % (out[0], soft[0], out[1], out[2]))
    assert out[1:] == soft[1:]


def step(a, say):
    import imagenet_step
    base = ['-b', str(a.batch_size), '--resnet-50', '--steps', str(a.steps), '--warmup', str(a.warmup), '--label-smoothing', str(EPS)]
    arms = [('softmax', []), ('bce thresh %g' % THRESH, ['--loss', 'bce', '--bce-target-thresh', str(THRESH)])]
    say('the step: tools/imagenet_step.py %s (ResNet-50 localizer, fp32, Adam, one resident batch), without and with --loss bce --bce-target-thresh %g'
        % (' '.join(base), THRESH))
    say('%d runs per arm, alternating; ms per step, the median of %d steps between device events behind %d warm-up steps' % (a.runs, a.steps, a.warmup))
    times = {name: [] for name, _ in arms}
    for _ in range(a.runs):
        for name, more in arms:
            with contextlib.redirect_stdout(io.StringIO()):
                res = imagenet_step.main(base + more)
            times[name].append(res['step_ms_median'])
            torch.cuda.synchronize()
            time.sleep(0.1)
    med = {}
    for name, _ in arms:
        t = times[name]
        med[name] = float(np.median(t))
        say('%-18s median %8.2f   min %8.2f   max %8.2f   runs %s' % (name, med[name], min(t), max(t), ' '.join('%.2f' % x for x in t)))
    plain, bce = arms[0][0], arms[1][0]
    say('bce - softmax (medians): %+.2f ms (%+.2f %%);  spread of the softmax runs: %.2f ms'
        % (med[bce] - med[plain], (med[bce] / med[plain] - 1) * 100, max(times[plain]) - min(times[plain])))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=2000)
    ap.add_argument('--windows', type=int, default=15)
    ap.add_argument('-b', '--batch-size', type=int, default=256)
    ap.add_argument('--classes', type=int, default=1000)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
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
