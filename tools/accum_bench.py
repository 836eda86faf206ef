#!/usr/bin/env python
"""What ``--accum-steps`` costs (profiles/imagenet_accum.txt): the three modes of ``loans_grad_accum_f32`` -- STORE 8 bytes per
parameter, ADD and CLOSE 12 -- on the ResNet-50 classifier's own arena, beside ``loans_grad_clip_apply_f32`` scaling (8 bytes per
parameter: the yardstick for achieved bytes/s), each mode under its four cache-hint arms with ``--exp``; and the batch-128 iteration
of ``train_imagenet.py`` with ``--accum-steps 2`` beside the plain batch-128 and the plain batch-256 iteration.  Windows of launches
between device events, the arms alternating inside one sitting.

    python tools/accum_bench.py --out imagenet_accum.txt                          (kernels and step)
    python tools/accum_bench.py --no-step                                         (kernels only)
    make -C loans_amd/csrc exp SRCS=accum.hip && python tools/accum_bench.py --no-step --exp
                                                                                  (the four cache-hint arms of every mode)
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

from loans_amd import _lib, ops       # noqa: E402

HINTS = {0: 'loads cached, store cached', 1: 'loads nt,     store cached', 2: 'loads cached, store nt', 3: 'loads nt,     store nt'}
MODES = ('store', 'add', 'close')
BYTES = {'store': 8, 'add': 12, 'close': 12}
NEAR_ONE = 1.0 - 2.0 ** -20         # a k that scales without draining the buffer over the thousands of calls of a sitting


def window(fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / launches         # microseconds per call


def exp_accum(mode, hint):
    """loans_grad_accum_f32 of the LOANS_EXPERIMENT build, which reads its cache hint from the environment on every call"""
    path = os.path.join(os.path.dirname(_lib.LIB_PATH), 'libloans_hip_exp.so')
    lib = ctypes.CDLL(path)
    fn = lib.loans_grad_accum_f32
    fn.argtypes, fn.restype = _lib.SIGNATURES['loans_grad_accum_f32'], ctypes.c_int

    def call(acc, g):
        os.environ['LOANS_ACCUM_HINT'] = str(hint)
        _lib.check(fn(acc.data_ptr(), g.data_ptr(), g.numel(), ops.ACCUM_MODES[mode], ops._stream()), 'loans_grad_accum_f32 (exp)')
    return call


def kernels(a, say):
    import train_imagenet as T
    model = T.build_model(T.parse_args(['--seed', '0']))           # the ResNet-50 localizer under a Classifier
    model.to_gpu(0)
    arena = model.arena
    n = arena.numel
    g = arena.grad
    g.normal_(0.0, 1e-3)
    # ADD adds g into acc on every call of a sitting: zeros keep both buffers finite and cost what any other value costs
    zeros = torch.zeros_like(g)
    acc = torch.zeros_like(g)
    scaling = ops.GradClipState(n, arena.device)
    scaling.record.copy_(torch.tensor([1.0, NEAR_ONE]))
    say('kernels: the ResNet-50 classifier: arena of %d floats (%.1f MB), %d units of %d floats; %s'
        % (n, n * 4 / 1e6, -(-n // ops.LARS_UNIT), ops.LARS_UNIT, torch.cuda.get_device_name(0)))
    arms = [('clip apply k<1', 8 * n, lambda: ops.grad_clip_apply(g, scaling)),
            ('accum store', 8 * n, lambda: ops.grad_accum(acc, g, 'store')),
            ('accum add', 12 * n, lambda: ops.grad_accum(acc, zeros, 'add')),
            ('accum close', 12 * n, lambda: ops.grad_accum(zeros, g, 'close'))]
    if a.exp:
        pairs = {'store': (acc, g), 'add': (acc, zeros), 'close': (zeros, g)}
        for mode in MODES:
            arms += [('%-5s %s' % (mode, HINTS[h]), BYTES[mode] * n, (lambda f, p: lambda: f(*p))(exp_accum(mode, h), pairs[mode]))
                     for h in sorted(HINTS)]
    for _, _, fn in arms:
        window(fn, 10)
    times = {name: [] for name, _, _ in arms}
    for _ in range(a.windows):
        for name, _, fn in arms:
            times[name].append(window(fn, a.launches))
    say('%d calls per window, %d windows per arm, alternating; microseconds per call' % (a.launches, a.windows))
    med = {}
    for name, nbytes, _ in arms:
        t = times[name]
        med[name] = float(np.median(t))
        say('%-34s median %7.1f   min %7.1f   max %7.1f   spread %5.1f   %.2f TB/s of %d bytes per float'
            % (name, med[name], min(t), max(t), max(t) - min(t), nbytes / (med[name] * 1e-6) / 1e12, nbytes // n))
    say('a step of K micro-batches adds (medians): K = 2: %.1f us, K = 4: %.1f us, K = 8: %.1f us'
        % tuple(med['accum store'] + (K - 2) * med['accum add'] + med['accum close'] for K in (2, 4, 8)))
    if a.exp:
        for mode in MODES:
            best = min(sorted(HINTS), key=lambda h: med['%-5s %s' % (mode, HINTS[h])])
            say('cache hints of %s: the fastest median is "%s"' % (mode.upper(), HINTS[best].replace('     ', ' ')))
    say('(after the sitting |g| = %.6g, |acc| = %.6g)' % (float(g.double().norm()), float(acc.double().norm())))
    del model


def step(a, say):
    import train_imagenet as T
    b = a.batch_size

    def argv(batch, more):
        return ['-b', str(batch), '--optimizer', 'sgd', '--lr', '0.001', '--weight-decay', '5e-5', '--iterations', str(a.iterations),
                '--log-interval', '10', '--no-validation', '--seed', '0', '--dataset-size', str(4 * b), '--synthetic-classes', '100',
                '--augment', 'rrc', '--augment-seed', '1', '--snapshot-interval', '100000', '--flat-log-dir'] + more

    arms = [('plain b%d' % b, argv(b, [])), ('accum 2 b%d' % b, argv(b, ['--accum-steps', '2'])), ('plain b%d' % (2 * b), argv(2 * b, []))]
    say('step: train_imagenet.py --optimizer sgd --weight-decay 5e-5 (ResNet-50 localizer, fp32, --augment rrc on the synthetic resident '
        'set): -b %d, -b %d --accum-steps 2, -b %d' % (b, b, 2 * b))
    say('%d runs per arm, alternating; ms per iteration over iterations 11..%d of each run (host clock between two synchronising log entries)'
        % (a.runs, a.iterations))
    times = {name: [] for name, _ in arms}
    for _ in range(a.runs):
        for name, args in arms:
            with tempfile.TemporaryDirectory() as log_dir:          # (the run's final snapshot: 100 MB)
                entries, model = T.run(T.parse_args(args + ['-l', log_dir]), log=lambda *x: None)
            at = {e['iteration']: e['elapsed_time'] for e in entries}
            times[name].append((at[a.iterations] - at[10]) / (a.iterations - 10) * 1e3)
            del model
            torch.cuda.synchronize()
            time.sleep(0.1)
    med = {}
    for name, _ in arms:
        t = times[name]
        med[name] = float(np.median(t))
        say('%-16s median %8.2f   min %8.2f   max %8.2f   spread %6.2f   runs %s'
            % (name, med[name], min(t), max(t), max(t) - min(t), ' '.join('%.2f' % x for x in t)))
    plain, accum, double = (med[name] for name, _ in arms)
    say('accum 2 - 2 x plain b%d (medians): %+.2f ms (%+.2f %%);  accum 2 - plain b%d: %+.2f ms (%+.2f %%)'
        % (b, accum - 2 * plain, (accum / (2 * plain) - 1) * 100, 2 * b, accum - double, (accum / double - 1) * 100))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=50)
    ap.add_argument('--windows', type=int, default=9)
    ap.add_argument('-b', '--batch-size', type=int, default=128)
    ap.add_argument('--iterations', type=int, default=40)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--no-step', action='store_true')
    ap.add_argument('--exp', action='store_true', help='also time the four cache-hint arms of every mode (needs libloans_hip_exp.so)')
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
