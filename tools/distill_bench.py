#!/usr/bin/env python
"""What ``--teacher`` costs (profiles/imagenet_distill.txt): the two launches of ``loans_softmax_distill_fwd_f32`` beside the two of
``loans_softmax_xent_mix_fwd_f32`` at B = 256, N = 1000 with the same labels and weights, with the spread the mix launches show
against themselves (a second mix arm in the same rotation); and the batch-256 ResNet-18 step of tools/imagenet_step.py under a
frozen ResNet-50 teacher beside (a) the same step without it and (b) the teacher's test-mode forward at that batch alone, in
each ``--dtype``.  Windows of calls between device events, the arms alternating inside one sitting.

    python tools/distill_bench.py --out imagenet_distill.txt                      (the loss and the step, both dtypes)
    python tools/distill_bench.py --no-step                                       (the loss only)
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

EPS, TOPK, ALPHA, TEMP = 0.1, 5, 0.5, 4.0


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
    zt = torch.from_numpy((3.0 * rng.standard_normal((B, N))).astype(np.float32)).cuda()
    ta = torch.from_numpy(rng.randint(0, N, B).astype(np.int32)).cuda()
    tb = torch.roll(ta, 1)
    lam, oml = MixedLabels.weights(0.3)
    say('the loss alone: B = %d, N = %d, weights (%.9g, %.9g), eps %g, k %d, alpha %g, T %g; %s'
        % (B, N, lam, oml, EPS, TOPK, ALPHA, TEMP, torch.cuda.get_device_name(0)))
    arms = [
        ('softmax mix', lambda: ops.softmax_xent_mix_fwd(z, ta, tb, lam, oml, EPS, TOPK)),
        ('distill', lambda: ops.softmax_distill_fwd(z, zt, ta, tb, lam, oml, EPS, TOPK, ALPHA, TEMP)),
        ('softmax mix (again)', lambda: ops.softmax_xent_mix_fwd(z, ta, tb, lam, oml, EPS, TOPK)),
        ('distill T 1', lambda: ops.softmax_distill_fwd(z, zt, ta, tb, lam, oml, EPS, TOPK, ALPHA, 1.0)),
        ('distill one label', lambda: ops.softmax_distill_fwd(z, zt, ta, ta, 1.0, 0.0, EPS, TOPK, ALPHA, TEMP)),
        ('distill alpha 0', lambda: ops.softmax_distill_fwd(z, None, ta, tb, lam, oml, EPS, TOPK, 0.0, TEMP)),
    ]
    for _, fn in arms:
        window(fn, 20)
    times = {name: [] for name, _ in arms}
    for _ in range(a.windows):
        for name, fn in arms:
            times[name].append(window(fn, a.launches))
    say('%d calls per window, %d windows per arm, alternating; microseconds per call (two launches per call -- three at alpha 0 -- and '
        'five (mix) or seven (distill) small allocations)' % (a.launches, a.windows))
    med = {}
    for name, _ in arms:
        t = times[name]
        nbytes = (3 if name.startswith('distill') and 'alpha 0' not in name else 2) * 4 * B * N      # logits read once each, gz written once
        med[name] = float(np.median(t))
        say('%-22s median %7.2f   min %7.2f   max %7.2f   spread %5.2f   (%.0f GB/s of %d bytes per call)'
            % (name, med[name], min(t), max(t), max(t) - min(t), nbytes / (med[name] * 1e-6) / 1e9, nbytes))
    both = times['softmax mix'] + times['softmax mix (again)']
    say('distill - mix (medians): %+.2f us;  the two mix arms against each other: %+.2f us (medians), %.2f us (all their windows, max - min)'
        % (med['distill'] - med['softmax mix'], med['softmax mix (again)'] - med['softmax mix'], max(both) - min(both)))
    out = ops.softmax_distill_fwd(z, zt, ta, tb, lam, oml, EPS, TOPK, ALPHA, TEMP)[0].cpu().tolist()
    soft = ops.softmax_xent_mix_fwd(z, ta, tb, lam, oml, EPS, TOPK)[0].cpu().tolist()
    say('(what they computed: distilled loss %.6f of which T^2 KL %.6f, mix loss %.6f; accuracy %.4f / %.4f both, teacher %.4f)'
        % (out[0], out[3], soft[0], out[1], out[2], out[4]))
    assert out[1:3] == soft[1:]


def step(a, say, dtype):
    import imagenet_step
    base = ['-b', str(a.batch_size), '--steps', str(a.steps), '--warmup', str(a.warmup), '--label-smoothing', str(EPS), '--dtype', dtype]
    distill = ['--teacher-arch', 'resnet50', '--distill-alpha', str(ALPHA), '--distill-temperature', str(TEMP)]
    arms = [('(a) student step', base), ('(b) teacher forward', base + ['--resnet-50', '--forward-only']), ('with the teacher', base + distill)]
    say('the step, --dtype %s: tools/imagenet_step.py %s (ResNet-18 localizer, Adam, one resident batch): (a) as it is, (b) the ResNet-50 '
        'localizer\'s test-mode forward at that batch alone (--resnet-50 --forward-only), and the step with %s' % (dtype, ' '.join(base), ' '.join(distill)))
    say('%d runs per arm, alternating; ms per step, the median of %d steps between device events behind %d warm-up steps' % (a.runs, a.steps, a.warmup))
    times = {name: [] for name, _ in arms}
    for _ in range(a.runs):
        for name, argv in arms:
            with contextlib.redirect_stdout(io.StringIO()):
                res = imagenet_step.main(argv)
            times[name].append(res['step_ms_median'])
            torch.cuda.synchronize()
            time.sleep(0.1)
    med = {}
    for name, _ in arms:
        t = times[name]
        med[name] = float(np.median(t))
        say('%-20s median %8.2f   min %8.2f   max %8.2f   runs %s' % (name, med[name], min(t), max(t), ' '.join('%.2f' % x for x in t)))
    plain, fwd, both = (name for name, _ in arms)
    spread = max(times[plain]) - min(times[plain])
    say('with the teacher - ((a) + (b)) (medians): %+.2f ms (%+.2f %% of (a) + (b));  spread of (a)\'s runs: %.2f ms;  the teacher adds %.1f %% to (a)'
        % (med[both] - med[plain] - med[fwd], (med[both] / (med[plain] + med[fwd]) - 1) * 100, spread, (med[both] / med[plain] - 1) * 100))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=2000)
    ap.add_argument('--windows', type=int, default=15)
    ap.add_argument('-b', '--batch-size', type=int, default=256)
    ap.add_argument('--classes', type=int, default=1000)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--dtypes', nargs='+', default=['f32', 'bf16'], choices=['f32', 'bf16'])
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
        for dtype in a.dtypes:
            step(a, say, dtype)


if __name__ == '__main__':
    main()
