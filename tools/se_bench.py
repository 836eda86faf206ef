#!/usr/bin/env python
"""What ``--se-ratio`` costs (profiles/imagenet_se.txt): the streaming kernels of csrc/se.hip beside the ungated kernels of the
junction -- ``loans_se_squeeze_*`` (no counterpart: one read of the conv output), ``loans_bn_apply_gate_*`` against
``loans_bn_apply_rows_*``, ``loans_se_bwd_reduce_*`` against ``loans_bn_bwd_reduce_rows_*``, ``loans_bn_bwd_apply_gate_*`` against
``loans_bn_bwd_apply_rows_*`` -- and the two per-sample excitation launches, through the C ABI on preallocated tensors, in one
process, at one shape, the arms alternating, at the junction shapes of a batch-256 ResNet-50 in fp32 and bf16, each beside the
time its bytes would take at the HBM roofline; and the batch-256 ResNet-18 and ResNet-50 steps of tools/imagenet_step.py with
``--se-ratio 16`` beside the same command without it and, with ``--parent DIR``, beside a built checkout of the parent commit.

    python tools/se_bench.py --parent ../parent --out imagenet_se.txt     (the kernels and the three-way steps)
    python tools/se_bench.py --no-step -b 32                              (the kernels only, a smaller batch)
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

from droppath_bench import SHAPES, window     # noqa: E402
from loans_amd import _lib, ops               # noqa: E402

RATIO = 16


def arms_of(B, hw, C_, bf16):
    """[(name, fn, bytes moved)]: per form (identity shortcut = single, convolution shortcut = dual) rows / gate pairs of the
    forward, the reduction and the apply pass, then the squeeze and the two excitation launches on their own"""
    lib, p, s, ck = _lib.load(), ops._ptr, ops._stream(), ops.check
    dt = torch.bfloat16 if bf16 else torch.float32
    rps, hid = hw * hw, C_ // RATIO
    g = torch.Generator(device='cuda').manual_seed(C_)
    mk = lambda: torch.randn((B, hw, hw, C_), device='cuda', generator=g).to(dt)      # noqa: E731
    x, x2, gy = mk(), mk(), mk()
    y, gx, gx2 = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    bits = torch.empty(B * rps * C_ // 4, device='cuda', dtype=torch.uint8)
    vec = lambda v: torch.full((C_,), v, device='cuda', dtype=torch.float32)           # noqa: E731
    mean, rstd, scale, shift, k = vec(0.0), vec(1.0), vec(1.0), vec(0.0), vec(0.5)
    f32 = lambda *shape: torch.rand(shape, device='cuda', generator=g)                  # noqa: E731
    r, gate, t, S, h, q, da2, dh = f32(B), f32(B, C_), f32(B, C_), f32(B, C_), f32(B, hid), f32(B, C_), f32(B, C_), f32(B, hid)
    G, W1, b1, W2, b2 = f32(3, B, C_), f32(hid, C_), f32(hid), f32(C_, hid), f32(C_)
    gW1, gb1, gW2, gb2 = torch.zeros_like(W1), torch.zeros_like(b1), torch.zeros_like(W2), torch.zeros_like(b2)
    slabs = lib.loans_se_slabs(B, rps, C_, x.element_size())
    part = torch.empty((B, slabs, 3, C_), device='cuda', dtype=torch.float64)
    u = torch.empty((B, 2, C_), device='cuda', dtype=torch.float64)
    sums = torch.zeros((ops.STATS_REPLICAS, 4, C_), device='cuda', dtype=torch.float64)
    sfx = 'bf16' if bf16 else 'f32'
    f = lambda name: getattr(lib, 'loans_%s_%s' % (name, sfx))          # noqa: E731
    nb, nbits, tab = x.numel() * x.element_size(), bits.numel(), 4 * B * C_
    out = []
    for dual in (False, True):
        mode, form = (2, 'dual') if dual else (1, 'single')
        sc2, sh2 = (p(scale), p(shift)) if dual else (0, 0)
        out.append(('apply rows mode %d' % mode, lambda mode=mode, sc2=sc2, sh2=sh2: ck(f('bn_apply_rows')(
            p(x), p(scale), p(shift), p(x2), sc2, sh2, p(r), p(y), p(bits), B, rps, C_, mode, s), 'apply_rows'), 3 * nb + nbits))
        out.append(('apply gate mode %d' % mode, lambda mode=mode, sc2=sc2, sh2=sh2: ck(f('bn_apply_gate')(
            p(x), p(scale), p(shift), p(x2), sc2, sh2, p(gate), p(y), p(bits), B, rps, C_, mode, s), 'apply_gate'), 3 * nb + nbits + tab))
        w2, m2, r2, G2 = (p(x2), p(mean), p(rstd), p(G[2])) if dual else (0, 0, 0, 0)
        red_bytes = (3 if dual else 2) * nb + nbits
        out.append(('reduce rows %s' % form, lambda w2=w2, m2=m2, r2=r2: ck(f('bn_bwd_reduce_rows')(
            p(gy), p(bits), p(r), p(x), p(mean), p(rstd), w2, m2, r2, p(sums), ops.STATS_REPLICAS, B, rps, C_, s), 'reduce_rows'), red_bytes))
        out.append(('reduce gate %s' % form, lambda w2=w2, G2=G2: ck(f('se_bwd_reduce')(
            p(gy), p(bits), p(x), w2, p(G[0]), p(G[1]), G2, p(part), B, rps, C_, s), 'se_bwd_reduce'), red_bytes + (3 if dual else 2) * tab))
        kb, g2 = (p(k), p(gx2)) if dual else (0, 0)
        app_bytes = (5 if dual else 3) * nb + nbits
        out.append(('bwd apply rows %s' % form, lambda w2=w2, kb=kb, g2=g2: ck(f('bn_bwd_apply_rows')(
            p(gy), p(bits), p(r), p(x), p(k), p(k), p(k), p(gx), w2, kb, kb, kb, g2, B, rps, C_, s), 'bwd_apply_rows'), app_bytes))
        out.append(('bwd apply gate %s' % form, lambda w2=w2, kb=kb, g2=g2: ck(f('bn_bwd_apply_gate')(
            p(gy), p(bits), p(gate), p(t), p(x), p(k), p(k), p(k), p(gx), w2, kb, kb, kb, g2, B, rps, C_, s), 'bwd_apply_gate'), app_bytes + 2 * tab))
    solo = [('squeeze', lambda: ck(f('se_squeeze')(p(x), p(S), p(part), B, rps, C_, s), 'se_squeeze'), nb + tab),
            ('excite forward', lambda: ck(lib.loans_se_excite_fwd_f32(p(S), p(scale), p(shift), p(W1), p(b1), p(W2), p(b2), p(gate), p(h), p(q),
                                                                      B, rps, C_, hid, s), 'excite_fwd'), 4 * tab + 8 * C_ * hid),
            ('excite backward', lambda: ck(lib.loans_se_excite_bwd_f32(
                p(G[0]), p(G[1]), p(G[2]), p(S), p(scale), p(shift), p(mean), p(rstd), p(mean), p(rstd), p(gate), p(h), p(q), p(W1), p(W2),
                p(t), p(da2), p(dh), p(u), p(gW1), p(gb1), p(gW2), p(gb2), p(sums), B, rps, C_, hid, s), 'excite_bwd'), 12 * tab + 24 * C_ * hid)]
    keepalive = (x, x2, gy, y, gx, gx2, bits, mean, rstd, scale, shift, k, r, gate, t, S, h, q, da2, dh, G, W1, b1, W2, b2, gW1, gb1,
                 gW2, gb2, part, u, sums)
    return out, solo, keepalive


def kernels(a, say):
    B = a.batch_size
    say('the junction kernels: B = %d, R = %d; %s' % (B, RATIO, torch.cuda.get_device_name(0)))
    say('%d calls per window, %d windows per arm, the arms of one shape alternating; microseconds per call; "hbm" = the bytes moved at %.1f TB/s'
        % (a.launches, a.windows, ops.ROOFLINE_HBM / 1e12))
    for bf16 in (False, True):
        for hw, C_ in SHAPES:
            pairs, solo, keepalive = arms_of(B, hw, C_, bf16)
            arms = pairs + solo
            for _, fn, _ in arms:
                window(fn, 3)
            times = {name: [] for name, _, _ in arms}
            for _ in range(a.windows):
                for name, fn, _ in arms:
                    times[name].append(window(fn, a.launches))
            say('%d x %d x %d x %d %s' % (B, hw, hw, C_, 'bf16' if bf16 else 'fp32'))
            for i in range(0, len(pairs), 2):
                (n0, _, _), (n1, _, nbytes) = pairs[i], pairs[i + 1]
                t0, t1 = times[n0], times[n1]
                m0, m1 = float(np.median(t0)), float(np.median(t1))
                hbm = nbytes / ops.ROOFLINE_HBM * 1e6
                say('  %-24s %8.1f [%8.1f .. %8.1f]   %-24s %8.1f [%8.1f .. %8.1f]   gate - rows %+7.1f (%+5.1f %%)   hbm %7.1f (%3.0f %% of it)'
                    % (n0, m0, min(t0), max(t0), n1, m1, min(t1), max(t1), m1 - m0, (m1 / m0 - 1) * 100, hbm, hbm / m1 * 100))
            for name, _, nbytes in solo:
                t0 = times[name]
                m0, hbm = float(np.median(t0)), nbytes / ops.ROOFLINE_HBM * 1e6
                say('  %-24s %8.1f [%8.1f .. %8.1f]   hbm %7.1f (%3.0f %% of it)' % (name, m0, min(t0), max(t0), hbm, hbm / m0 * 100))
            del arms, pairs, solo, keepalive
            torch.cuda.empty_cache()


def step(a, say, more, title):
    """tools/imagenet_step.py, a process per run, the arms alternating: a checkout of the parent commit where ``--parent DIR``
    names one (built), this tree without the option, this tree with ``--se-ratio``"""
    here = os.path.dirname(os.path.abspath(__file__))
    base = ['-b', str(a.batch_size), '--steps', str(a.steps), '--warmup', str(a.warmup)] + more
    on = '--se-ratio %d' % RATIO
    arms = [('without', os.path.join(here, 'imagenet_step.py'), []), (on, os.path.join(here, 'imagenet_step.py'), ['--se-ratio', str(RATIO)])]
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
    line = 'with - without (medians): %+.2f ms (%+.2f %%)' % (med[on] - med['without'], (med[on] / med['without'] - 1) * 100)
    if a.parent:
        line += ';  without - parent: %+.2f ms (%+.2f %%)' % (med['without'] - med['parent commit'], (med['without'] / med['parent commit'] - 1) * 100)
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
        step(a, say, [], 'ResNet-18')
        step(a, say, ['--resnet-50'], 'ResNet-50')


if __name__ == '__main__':
    main()
