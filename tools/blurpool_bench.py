#!/usr/bin/env python
"""What ``--blur-pool`` costs (profiles/imagenet_blurpool.txt): the kernels of csrc/blur.hip through the C ABI on preallocated
tensors, in one process, the arms of a shape alternating, at the batch-256 shapes of the strided stages -- the fused forward
``blur(relu(bn(x)))`` beside the composition it replaces (``loans_bn_apply_*``, then the plain arm on its output), the two
backward passes and the plain backward, each beside the time its bytes would take at the HBM roofline -- and the batch-256
ResNet-18 and ResNet-50 steps of tools/imagenet_step.py with ``--blur-pool`` beside the same command without it and, with
``--parent DIR``, beside a built checkout of the parent commit.

    python tools/blurpool_bench.py --parent ../parent --out imagenet_blurpool.txt
    python tools/blurpool_bench.py --no-step -b 32
"""
import argparse
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np      # noqa: E402
import torch            # noqa: E402

from droppath_bench import window             # noqa: E402
from loans_amd import _lib, ops               # noqa: E402

# (full-resolution H = W, C, what it is).  'stage': the conv output of a strided stage (BN + ReLU + blur: ResNet-18's conv1 of
# res3 .. res5 and ResNet-50's 1 x 1 conv1 have the same shapes); 'shortcut': a unit input (the plain arm)
SHAPES = ((56, 128, 'stage'), (28, 256, 'stage'), (14, 512, 'stage'),
          (56, 64, 'shortcut'), (28, 128, 'shortcut'), (14, 256, 'shortcut'),         # ResNet-18
          (56, 256, 'shortcut'), (28, 512, 'shortcut'), (14, 1024, 'shortcut'))       # ResNet-50


def arms_of(B, hw, C_, kind, bf16):
    """[(name, fn, bytes moved)] of one shape and storage type"""
    lib, p, s, ck = _lib.load(), ops._ptr, ops._stream(), ops.check
    dt = torch.bfloat16 if bf16 else torch.float32
    g = torch.Generator(device='cuda').manual_seed(C_)
    ho = ops.blur_outsize(hw)
    x = torch.randn((B, hw, hw, C_), device='cuda', generator=g).to(dt)
    gy = torch.randn((B, ho, ho, C_), device='cuda', generator=g).to(dt)
    y, gx = torch.empty_like(gy), torch.empty_like(x)
    eb = x.element_size()
    full, quarter = x.numel() * eb, gy.numel() * eb
    if kind == 'shortcut':
        arms = [('forward plain', lambda: ck(lib.loans_blur_fwd(p(x), 0, 0, p(y), B, hw, hw, C_, eb, eb, s), 'fwd'), full + quarter),
                ('backward plain +=', lambda: ck(lib.loans_blur_bwd_plain(p(gy), p(gx), p(gx), B, hw, hw, C_, eb, eb, s), 'plain'),
                 quarter + 2 * full)]
        return arms, (x, gy, y, gx)
    act = torch.empty_like(x)
    vec = lambda v: torch.full((C_,), v, device='cuda', dtype=torch.float32)           # noqa: E731
    mean, scale, shift, k = vec(0.0), vec(1.0), vec(0.0), torch.full((3, C_), 0.5, device='cuda')
    part = torch.empty((lib.loans_blur_bwd_records(B, hw, hw), 2, C_), device='cuda', dtype=torch.float64)
    sums = torch.zeros((ops.STATS_REPLICAS, 2, C_), device='cuda', dtype=torch.float64)
    apply_fn = lib.loans_bn_apply_bf16 if bf16 else lib.loans_bn_apply_f32

    def unfused():
        ck(apply_fn(p(x), p(scale), p(shift), 0, 0, 0, p(act), B * hw * hw, C_, 0, 1, s), 'bn_apply')
        ck(lib.loans_blur_fwd(p(act), 0, 0, p(y), B, hw, hw, C_, eb, eb, s), 'fwd')

    arms = [('forward fused', lambda: ck(lib.loans_blur_fwd(p(x), p(scale), p(shift), p(y), B, hw, hw, C_, eb, eb, s), 'fwd'), full + quarter),
            ('forward bn_apply + plain', unfused, 3 * full + quarter),
            ('backward reduce', lambda: ck(lib.loans_blur_bwd_reduce(p(gy), p(x), p(scale), p(shift), p(mean), p(part), p(sums), B, hw, hw, C_,
                                                                     eb, eb, s), 'reduce'), full + quarter),
            ('backward apply', lambda: ck(lib.loans_blur_bwd_apply(p(gy), p(x), p(scale), p(shift), p(k), p(gx), B, hw, hw, C_, eb, eb, s),
                                          'apply'), 2 * full + quarter)]
    return arms, (x, gy, y, gx, act, mean, scale, shift, k, part, sums)


def kernels(a, say):
    B = a.batch_size
    say('the blur-pool kernels: B = %d; %s' % (B, torch.cuda.get_device_name(0)))
    say('%d calls per window, %d windows per arm, the arms of one shape alternating; microseconds per call, median [min .. max]; '
        '"hbm" = the bytes the arm has to move at %.1f TB/s' % (a.launches, a.windows, ops.ROOFLINE_HBM / 1e12))
    total = {}
    for bf16 in (False, True):
        for hw, C_, kind in SHAPES:
            arms, keepalive = arms_of(B, hw, C_, kind, bf16)
            for _, fn, _ in arms:
                window(fn, 3)
            times = {name: [] for name, _, _ in arms}
            for _ in range(a.windows):
                for name, fn, _ in arms:
                    times[name].append(window(fn, a.launches))
            say('%d x %d x %d x %d %s (%s)' % (B, hw, hw, C_, 'bf16' if bf16 else 'fp32', kind))
            for name, _, nbytes in arms:
                t = times[name]
                m, hbm = float(np.median(t)), nbytes / ops.ROOFLINE_HBM * 1e6
                total[(bf16, hw, C_, name)] = m
                say('  %-26s %8.1f [%8.1f .. %8.1f]   hbm %7.1f (%3.0f %% of it)' % (name, m, min(t), max(t), hbm, hbm / m * 100))
            if kind == 'stage':
                f, u = (float(np.median(times[n])) for n in ('forward fused', 'forward bn_apply + plain'))
                say('  fused - composition: %+.1f us (%+.1f %%)' % (f - u, (f / u - 1) * 100))
            del arms, keepalive
            torch.cuda.empty_cache()
    return total


def blur_time(total, shortcuts):
    """ms of the new kernels alone in one fp32 step of a model: its three strided stages and its three shortcut inputs"""
    us = sum(v for (bf16, hw, C_, name), v in total.items()
             if not bf16 and name != 'forward bn_apply + plain' and (name.endswith(('fused', 'reduce', 'apply')) or (hw, C_) in shortcuts))
    return us / 1e3


def step(a, say, more, title):
    """tools/imagenet_step.py, a process per run, the arms alternating; returns the medians by arm"""
    here = os.path.dirname(os.path.abspath(__file__))
    base = ['-b', str(a.batch_size), '--steps', str(a.steps), '--warmup', str(a.warmup)] + more
    arms = [('without', os.path.join(here, 'imagenet_step.py'), []), ('--blur-pool', os.path.join(here, 'imagenet_step.py'), ['--blur-pool'])]
    if a.parent:
        arms.insert(0, ('parent commit', os.path.join(os.path.abspath(a.parent), 'tools', 'imagenet_step.py'), []))
    say('the step: tools/imagenet_step.py %s (%s localizer, fp32, Adam, one resident batch): %s'
        % (' '.join(base), title, ', '.join(name for name, _, _ in arms)))
    say('%d runs per arm, a process each, alternating; ms per step, the median of %d steps between device events behind %d warm-up steps'
        % (a.runs, a.steps, a.warmup))
    times = {name: [] for name, _, _ in arms}
    for _ in range(a.runs):
        for name, script, extra in arms:
            done = subprocess.run([sys.executable, script] + base + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
            if done.returncode != 0:
                raise RuntimeError('%s failed (%d): %s' % (script, done.returncode, done.stderr.decode()[-2000:]))
            times[name].append(json.loads(done.stdout.decode().strip().splitlines()[-1])['step_ms_median'])
    med = {}
    for name, _, _ in arms:
        t = times[name]
        med[name] = float(np.median(t))
        say('%-18s median %8.2f   min %8.2f   max %8.2f   runs %s' % (name, med[name], min(t), max(t), ' '.join('%.2f' % x for x in t)))
    line = 'with - without (medians): %+.2f ms (%+.2f %%)' % (med['--blur-pool'] - med['without'], (med['--blur-pool'] / med['without'] - 1) * 100)
    if a.parent:
        line += ';  without - parent: %+.2f ms (%+.2f %%)' % (med['without'] - med['parent commit'], (med['without'] / med['parent commit'] - 1) * 100)
    say(line + ';  spread of the runs: ' + ', '.join('%s %.2f ms' % (name, max(times[name]) - min(times[name])) for name, _, _ in arms))
    return med


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('-b', '--batch-size', type=int, default=256)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--no-step', action='store_true')
    ap.add_argument('--parent', default=None, help='a built checkout of the parent commit: a third arm of the step timing')
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

    total = kernels(a, say)
    if a.no_step:
        return
    for more, title, shortcuts in (([], 'ResNet-18', ((56, 64), (28, 128), (14, 256))),
                                   (['--resnet-50'], 'ResNet-50', ((56, 256), (28, 512), (14, 1024)))):
        med = step(a, say, more, title)
        blur = blur_time(total, shortcuts)
        say('of the %+.2f ms: %.2f ms are the blur kernels timed alone above (three strided stages, three shortcut inputs); the remaining '
            '%.2f ms are the convolutions, weight and data gradients and BN statistics that now run at full resolution'
            % (med['--blur-pool'] - med['without'], blur, med['--blur-pool'] - med['without'] - blur))


if __name__ == '__main__':
    main()
