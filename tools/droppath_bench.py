#!/usr/bin/env python
"""What ``--drop-path`` costs (profiles/imagenet_droppath.txt): each ``loans_bn_*_rows_*`` kernel beside the kernel it stands in
for -- ``loans_bn_apply_bits_*`` against ``loans_bn_apply_rows_*``, the sign-bit reduction and apply pass of the BN backward
against theirs -- through the C ABI on preallocated tensors, in one process, at one shape, the arms alternating, at the junction
shapes of a batch-256 ResNet-50 (256 x 56 x 56 x 256 down to 256 x 7 x 7 x 2048) in fp32 and bf16, with the time the bytes moved
would take at the HBM roofline beside them; and the batch-256 ResNet-50 step of tools/imagenet_step.py with ``--drop-path 0.05``
beside the same command without it and, with ``--parent DIR``, beside a built checkout of the parent commit -- a process per run,
the arms alternating.

    python tools/droppath_bench.py --parent ../parent --out imagenet_droppath.txt (the kernels and the three-way step)
    python tools/droppath_bench.py --no-step -b 32                                (the kernels only, a smaller batch)
"""
import argparse
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np      # noqa: E402
import torch            # noqa: E402

from loans_amd import _lib, ops       # noqa: E402

SHAPES = ((56, 256), (28, 512), (14, 1024), (7, 2048))         # (Ho = Wo, C) behind res2 .. res5
RATE = 0.05


def window(fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / launches         # microseconds per call


def arms_of(B, hw, C_, bf16):
    """[(name, fn, bytes moved)] of one shape and storage type: old / new of the forward, the reduction and the apply pass, in
    the identity-shortcut form (mode 1, single) and the convolution-shortcut form (mode 2, dual)"""
    lib, p, s = _lib.load(), ops._ptr, ops._stream()
    dt = torch.bfloat16 if bf16 else torch.float32
    rps, rows = hw * hw, B * hw * hw
    g = torch.Generator(device='cuda').manual_seed(C_)
    mk = lambda: torch.randn((B, hw, hw, C_), device='cuda', generator=g).to(dt)      # noqa: E731
    x, x2, gy = mk(), mk(), mk()
    y, gx, gx2 = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    bits = torch.empty(rows * C_ // 4, device='cuda', dtype=torch.uint8)
    vec = lambda v: torch.full((C_,), v, device='cuda', dtype=torch.float32)           # noqa: E731
    mean, rstd, scale, shift, k = vec(0.0), vec(1.0), vec(1.0), vec(0.0), vec(0.5)
    keep = (np.random.RandomState(0).random_sample(B) >= RATE).astype(np.float32) / np.float32(1 - RATE)
    r = torch.from_numpy(keep.astype(np.float32)).cuda()
    rep = ops.bn_units_ok(C_, bf16)             # the existing backward's replicated-accumulator path tiles this channel count
    sums = torch.zeros((ops.STATS_REPLICAS, 4, C_), device='cuda', dtype=torch.float64)
    sfx = 'bf16' if bf16 else 'f32'
    f = lambda name: getattr(lib, 'loans_%s_%s' % (name, sfx))          # noqa: E731
    ck = ops.check
    nb = x.numel() * x.element_size()
    nbits = bits.numel()
    out = []
    for dual in (False, True):
        mode, form = (2, 'dual') if dual else (1, 'single')
        sc2, sh2 = (p(scale), p(shift)) if dual else (0, 0)
        out.append(('apply bits mode %d' % mode, lambda mode=mode, sc2=sc2, sh2=sh2: ck(f('bn_apply_bits')(
            p(x), p(scale), p(shift), p(x2), sc2, sh2, p(y), p(bits), rows, C_, mode, 1, s), 'apply_bits'), 3 * nb + nbits))
        out.append(('apply rows mode %d' % mode, lambda mode=mode, sc2=sc2, sh2=sh2: ck(f('bn_apply_rows')(
            p(x), p(scale), p(shift), p(x2), sc2, sh2, p(r), p(y), p(bits), B, rps, C_, mode, s), 'apply_rows'), 3 * nb + nbits))
        w2, m2, r2 = (p(x2), p(mean), p(rstd)) if dual else (0, 0, 0)
        red_bytes = (3 if dual else 2) * nb + nbits
        if rep:
            out.append(('reduce bits %s' % form, lambda w2=w2, m2=m2, r2=r2: ck(f('bn_bwd_reduce_rep')(
                p(gy), p(bits), 3, p(x), p(mean), p(rstd), w2, m2, r2, 0, 0, p(sums), ops.STATS_REPLICAS, rows, C_, s), 'reduce_rep'), red_bytes))
        else:
            out.append(('reduce bits %s' % form, lambda w2=w2, m2=m2, r2=r2: ck(f('bn_bwd_reduce_bits')(
                p(gy), p(bits), p(x), p(mean), p(rstd), w2, m2, r2, p(sums), rows, C_, s), 'reduce_bits'), red_bytes))
        out.append(('reduce rows %s' % form, lambda w2=w2, m2=m2, r2=r2: ck(f('bn_bwd_reduce_rows')(
            p(gy), p(bits), p(r), p(x), p(mean), p(rstd), w2, m2, r2, p(sums), ops.STATS_REPLICAS, B, rps, C_, s), 'reduce_rows'), red_bytes))
        kb, g2 = (p(k), p(gx2)) if dual else (0, 0)
        app_bytes = (5 if dual else 3) * nb + nbits
        out.append(('bwd apply bits %s' % form, lambda w2=w2, kb=kb, g2=g2: ck(f('bn_bwd_apply_bits')(
            p(gy), p(bits), p(x), p(k), p(k), p(k), p(gx), w2, kb, kb, kb, g2, rows, C_, s), 'bwd_apply_bits'), app_bytes))
        out.append(('bwd apply rows %s' % form, lambda w2=w2, kb=kb, g2=g2: ck(f('bn_bwd_apply_rows')(
            p(gy), p(bits), p(r), p(x), p(k), p(k), p(k), p(gx), w2, kb, kb, kb, g2, B, rps, C_, s), 'bwd_apply_rows'), app_bytes))
    keepalive = (x, x2, gy, y, gx, gx2, bits, mean, rstd, scale, shift, k, r, sums)
    return out, keepalive


def kernels(a, say):
    B = a.batch_size
    say('the junction kernels: B = %d, keep table of p = %g (%s); %s' % (B, RATE, 'one seeded draw', torch.cuda.get_device_name(0)))
    say('%d calls per window, %d windows per arm, the arms of one shape alternating; microseconds per call; "hbm" = the bytes moved at %.1f TB/s'
        % (a.launches, a.windows, ops.ROOFLINE_HBM / 1e12))
    for bf16 in (False, True):
        for hw, C_ in SHAPES:
            arms, keepalive = arms_of(B, hw, C_, bf16)
            for _, fn, _ in arms:
                window(fn, 3)
            times = {name: [] for name, _, _ in arms}
            for _ in range(a.windows):
                for name, fn, _ in arms:
                    times[name].append(window(fn, a.launches))
            say('%d x %d x %d x %d %s' % (B, hw, hw, C_, 'bf16' if bf16 else 'fp32'))
            for i in range(0, len(arms), 2):
                (n0, _, nbytes), (n1, _, _) = arms[i], arms[i + 1]
                t0, t1 = times[n0], times[n1]
                m0, m1 = float(np.median(t0)), float(np.median(t1))
                say('  %-24s %8.1f [%8.1f .. %8.1f]   %-24s %8.1f [%8.1f .. %8.1f]   rows - bits %+7.1f (%+5.1f %%)   hbm %7.1f'
                    % (n0, m0, min(t0), max(t0), n1, m1, min(t1), max(t1), m1 - m0, (m1 / m0 - 1) * 100, nbytes / ops.ROOFLINE_HBM * 1e6))
            del arms, keepalive
            torch.cuda.empty_cache()


def step(a, say):
    """tools/imagenet_step.py, a process per run, the arms alternating: a checkout of the parent commit where ``--parent DIR``
    names one (built: its own tools/imagenet_step.py runs against its own library), this tree without the option, this tree
    with ``--drop-path``"""
    here = os.path.dirname(os.path.abspath(__file__))
    base = ['-b', str(a.batch_size), '--resnet-50', '--steps', str(a.steps), '--warmup', str(a.warmup)]
    arms = [('without', os.path.join(here, 'imagenet_step.py'), []),
            ('--drop-path %g' % RATE, os.path.join(here, 'imagenet_step.py'), ['--drop-path', str(RATE)])]
    if a.parent:
        arms.insert(0, ('parent commit', os.path.join(os.path.abspath(a.parent), 'tools', 'imagenet_step.py'), []))
    say('the step: tools/imagenet_step.py %s (ResNet-50 localizer, fp32, Adam, one resident batch): %s'
        % (' '.join(base), ', '.join(name for name, _, _ in arms)))
    say('%d runs per arm, a process each, alternating; ms per step, the median of %d steps between device events behind %d warm-up steps'
        % (a.runs, a.steps, a.warmup))
    times = {name: [] for name, _, _ in arms}
    for _ in range(a.runs):
        for name, script, more in arms:
            done = subprocess.run([sys.executable, script] + base + more, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
            if done.returncode != 0:
                raise RuntimeError('%s failed (%d): %s' % (script, done.returncode, done.stderr.decode()[-2000:]))
            times[name].append(json.loads(done.stdout.decode().strip().splitlines()[-1])['step_ms_median'])
    med = {}
    for name, _, _ in arms:
        t = times[name]
        med[name] = float(np.median(t))
        say('%-18s median %8.2f   min %8.2f   max %8.2f   runs %s' % (name, med[name], min(t), max(t), ' '.join('%.2f' % x for x in t)))
    plain, drop = 'without', '--drop-path %g' % RATE
    line = 'with - without (medians): %+.2f ms (%+.2f %%)' % (med[drop] - med[plain], (med[drop] / med[plain] - 1) * 100)
    if a.parent:
        line += ';  without - parent: %+.2f ms (%+.2f %%)' % (med[plain] - med['parent commit'], (med[plain] / med['parent commit'] - 1) * 100)
    say(line + ';  spread of the runs: ' + ', '.join('%s %.2f ms' % (name, max(times[name]) - min(times[name])) for name, _, _ in arms))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('-b', '--batch-size', type=int, default=256)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--no-step', action='store_true')
    ap.add_argument('--no-kernels', action='store_true')
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

    if not a.no_kernels:
        kernels(a, say)
    if not a.no_step:
        step(a, say)


if __name__ == '__main__':
    main()
