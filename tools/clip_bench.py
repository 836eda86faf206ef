#!/usr/bin/env python
"""What ``--clip-grad-norm`` costs (profiles/imagenet_clip.txt): the norm pass (two launches) with its achieved bytes/s against the
4 bytes per parameter it has to read, beside the LARS ratios pass it is modelled on; the apply pass when it scales (8 bytes per
parameter) beside the segmented momentum SGD, and when ``k == 1`` (a launch, no traffic) -- on the ResNet-50 classifier's own arena
-- and the step of ``train_imagenet.py --optimizer lamb`` with and without ``--clip-grad-norm 1.0``.  Windows of launches between
device events, the arms alternating inside one sitting.

    python tools/clip_bench.py --out imagenet_clip.txt                            (kernels and step)
    python tools/clip_bench.py --no-step                                          (kernels only)
    make -C loans_amd/csrc exp SRCS=clip.hip && python tools/clip_bench.py --no-step --exp
                                                                                  (the four cache-hint arms of the apply kernel)
"""
import argparse
import ctypes
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np      # noqa: E402
import torch            # noqa: E402

import loans_amd        # noqa: E402
from loans_amd import _lib, ops       # noqa: E402

HINTS = {0: 'load cached, store cached', 1: 'load nt,     store cached', 2: 'load cached, store nt', 3: 'load nt,     store nt'}
NEAR_ONE = 1.0 - 2.0 ** -20         # a k that scales without draining the buffer over the thousands of calls of a sitting


def window(fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / launches         # microseconds per call


def exp_apply(hint):
    """loans_grad_clip_apply_f32 of the LOANS_EXPERIMENT build, which reads its cache hint from the environment on every call"""
    path = os.path.join(os.path.dirname(_lib.LIB_PATH), 'libloans_hip_exp.so')
    lib = ctypes.CDLL(path)
    fn = lib.loans_grad_clip_apply_f32
    fn.argtypes, fn.restype = _lib.SIGNATURES['loans_grad_clip_apply_f32'], ctypes.c_int

    def call(g, state):
        os.environ['LOANS_CLIP_HINT'] = str(hint)
        _lib.check(fn(g.data_ptr(), g.numel(), state.record.data_ptr(), ops._stream()), 'loans_grad_clip_apply_f32 (exp)')
    return call


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
    state = ops.GradClipState(n, arena.device)
    scaling, idle = ops.GradClipState(n, arena.device), ops.GradClipState(n, arena.device)
    scaling.record.copy_(torch.tensor([1.0, NEAR_ONE]))
    idle.record.copy_(torch.tensor([1.0, 1.0]))
    units = state.workspace.numel()
    say('kernels: the ResNet-50 classifier: arena of %d floats (%.1f MB), %d units of %d floats, %d partials per fold lane; %s'
        % (n, n * 4 / 1e6, units, ops.LARS_UNIT, -(-units // 64), torch.cuda.get_device_name(0)))
    g = arena.grad
    arms = [
        ('lars ratios', 8 * n, lambda: ops.lars_ratios(arena.data, g, 5e-5, 0.001, 1e-8, table)),
        ('sgd segmented', 20 * n, lambda: ops.momentum_sgd_seg(arena.data, g, v, 1e-4, 0.9, 5e-5, decay_table)),
        ('clip norm', 4 * n, lambda: ops.grad_norm(g, 1.0, state)),
        ('clip apply k<1', 8 * n, lambda: ops.grad_clip_apply(g, scaling)),
        ('clip apply k==1', 0, lambda: ops.grad_clip_apply(g, idle)),
    ]
    if a.exp:
        arms += [('apply ' + HINTS[h], 8 * n, (lambda f: lambda: f(g, scaling))(exp_apply(h))) for h in sorted(HINTS)]
    for _, _, fn in arms:
        window(fn, 10)
    times = {name: [] for name, _, _ in arms}
    for _ in range(a.windows):
        for name, _, fn in arms:
            times[name].append(window(fn, a.launches))
    say('%d calls per window, %d windows per arm, alternating; microseconds per call (lars ratios, clip norm: two launches per call)' % (a.launches, a.windows))
    med = {}
    for name, nbytes, _ in arms:
        t = times[name]
        med[name] = float(np.median(t))
        rate = '%.2f TB/s of %d bytes per float' % (nbytes / (med[name] * 1e-6) / 1e12, nbytes // n) if nbytes else 'no traffic'
        say('%-32s median %7.1f   min %7.1f   max %7.1f   spread %5.1f   %s' % (name, med[name], min(t), max(t), max(t) - min(t), rate))
    say('clip norm + clip apply k<1 (medians): %.1f us per clipping step, clip norm + clip apply k==1: %.1f us per step that does not clip'
        % (med['clip norm'] + med['clip apply k<1'], med['clip norm'] + med['clip apply k==1']))
    if a.exp:
        best = min(sorted(HINTS), key=lambda h: med['apply ' + HINTS[h]])
        say('cache hints of the apply kernel: the fastest median is "%s"' % HINTS[best].replace('     ', ' '))
    state_N, state_k = state.record.cpu().tolist()
    say('(the record of the norm arm: N %.6g, k %.6g; after the sitting |g| = %.6g)' % (state_N, state_k, float(g.double().norm())))
    del model, sgd, lars


def step(a, say):
    import train_imagenet as T
    base = ['-b', str(a.batch_size), '--optimizer', 'lamb', '--lr', '0.001', '--weight-decay', '5e-5', '--iterations', str(a.iterations),
            '--log-interval', '10', '--no-validation', '--seed', '0', '--dataset-size', str(2 * a.batch_size), '--synthetic-classes', '100',
            '--augment', 'rrc', '--augment-seed', '1', '--snapshot-interval', '100000', '--flat-log-dir']
    arms = [('lamb', []), ('lamb + clip 1.0', ['--clip-grad-norm', '1.0'])]
    say('step: train_imagenet.py -b %d --optimizer lamb --weight-decay 5e-5 (ResNet-50 localizer, fp32, --augment rrc on the synthetic resident set), without and with --clip-grad-norm 1.0' % a.batch_size)
    say('%d runs per arm, alternating; ms per step over iterations 11..%d of each run (host clock between two synchronising log entries)' % (a.runs, a.iterations))
    times = {name: [] for name, _ in arms}
    norms = []
    for _ in range(a.runs):
        for name, more in arms:
            with tempfile.TemporaryDirectory() as log_dir:          # (the run's final snapshots: 100 MB each)
                entries, model = T.run(T.parse_args(base + more + ['-l', log_dir]), log=lambda *x: None)
            at = {e['iteration']: e['elapsed_time'] for e in entries}
            times[name].append((at[a.iterations] - at[10]) / (a.iterations - 10) * 1e3)
            if more:
                norms = [e['grad_norm'] for e in entries]
            del model
            torch.cuda.synchronize()
            time.sleep(0.1)
    med = {}
    for name, _ in arms:
        t = times[name]
        med[name] = float(np.median(t))
        say('%-18s median %8.2f   min %8.2f   max %8.2f   runs %s' % (name, med[name], min(t), max(t), ' '.join('%.2f' % x for x in t)))
    say('clip - plain (medians): %+.2f ms (%.2f %%);  spread of the plain runs: %.2f ms' % (
        med['lamb + clip 1.0'] - med['lamb'], (med['lamb + clip 1.0'] / med['lamb'] - 1) * 100, max(times['lamb']) - min(times['lamb'])))
    say('grad_norm of the logged iterations of the last clipped run: %s' % ' '.join('%.4g' % x for x in norms))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=50)
    ap.add_argument('--windows', type=int, default=9)
    ap.add_argument('-b', '--batch-size', type=int, default=256)
    ap.add_argument('--iterations', type=int, default=40)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--no-step', action='store_true')
    ap.add_argument('--exp', action='store_true', help='also time the four cache-hint arms of the apply kernel (needs libloans_hip_exp.so)')
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
