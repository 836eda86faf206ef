#!/usr/bin/env python
"""What the photometric stage costs (profiles/imagenet_photo.txt): the two launches of csrc/photo.hip alone at 256 x 3 x 224 x 224
with every stage on -- microseconds and the fraction of the HBM bound (one read of the batch for the grey pass, one read and one
write for the in-place apply pass) --, the fold launch of the grey entry against the other form that was tried, every apply block
folding its image's partials in its prologue (the LOANS_EXPERIMENT build of photo.hip, compiled here into tools/_bin/), and the step of ``train_imagenet.py`` with
``--color-jitter 0.4 0.4 0.4 --lighting-std 0.1 --random-erase-prob 0.25`` against the same command without them.  Windows of
launches between device events, the arms alternating inside one sitting.

    python tools/photo_bench.py --out imagenet_photo.txt                          (kernels and step)
    python tools/photo_bench.py --no-step                                         (kernels only)
"""
import argparse
import ctypes
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np      # noqa: E402
import torch            # noqa: E402

from loans_amd import _lib, ops                                 # noqa: E402
from loans_amd.common.datasets import photometric as P          # noqa: E402

HBM_TBS = 8.0           # the MI355X's HBM3E peak, TB/s: the bound is the bytes below at this rate
EXP_LIB = os.path.join(ROOT, 'tools', '_bin', 'libphoto_exp.so')


def window(fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / launches         # microseconds per call


def experiment_library():
    """photo.hip with -DLOANS_EXPERIMENT: the apply pass with the fold in its prologue (built once, kept out of git)"""
    if not os.path.exists(EXP_LIB):
        os.makedirs(os.path.dirname(EXP_LIB), exist_ok=True)
        csrc = os.path.join(ROOT, 'loans_amd', 'csrc')
        subprocess.check_call([os.environ.get('HIPCC', '/opt/rocm/bin/hipcc'), '-O3', '-std=c++17', '-fPIC', '--offload-arch=gfx950',
                               '-munsafe-fp-atomics', '-I' + os.path.join(ROOT, 'include'), '-DLOANS_EXPERIMENT', '-shared', '-o', EXP_LIB,
                               os.path.join(csrc, 'photo.hip')])
    lib = ctypes.CDLL(EXP_LIB)
    lib.loans_photo_exp_apply_prologue_f32.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_int32] * 3 + [ctypes.c_void_p] * 3
    return lib


def kernels(a, say):
    B, H, W = a.batch_size, 224, 224
    rng = np.random.RandomState(0)
    x = torch.from_numpy(rng.rand(B, 3, H, W).astype(np.float32)).cuda()
    jobs = P.PhotoPolicy(0.4, 0.4, 0.4, 0.1, 0.25, seed=0).draw_batch(B, H, W)
    jobs_d = torch.from_numpy(jobs.view(np.uint8).copy()).cuda()
    lib = _lib.load()
    ws_bytes = int(lib.loans_photo_workspace_bytes(B, H, W))
    ws = torch.empty(ws_bytes // 8, device='cuda', dtype=torch.float64)
    batch_bytes = x.numel() * 4
    say('kernels: %d x 3 x %d x %d fp32 (%.1f MB), jobs of PhotoPolicy(0.4, 0.4, 0.4, lighting 0.1, erase 0.25): %d of %d with a box, '
        '%d partials per image; %s' % (B, H, W, batch_bytes / 1e6, int(((jobs['y1'] > jobs['y0']) & (jobs['x1'] > jobs['x0'])).sum()), B,
                                      ws_bytes // 8 // B, torch.cuda.get_device_name(0)))
    host, st = jobs.ctypes.data, ops._stream
    exp = experiment_library()

    def grey():
        ops.check(lib.loans_photo_grey_means_f32(x.data_ptr(), B, 3, H, W, jobs_d.data_ptr(), host, ws.data_ptr(), ws_bytes, st()), 'grey')

    def apply():            # in place, as the feed runs it (the pixels drift towards the clamps over a window: the traffic does not)
        ops.check(lib.loans_photo_apply_f32(x.data_ptr(), x.data_ptr(), B, 3, H, W, jobs_d.data_ptr(), host, ws.data_ptr(), ws_bytes, st()), 'apply')

    def prologue_apply():   # the experiment build: the apply pass folding the partials in every block's prologue
        ops.check(exp.loans_photo_exp_apply_prologue_f32(x.data_ptr(), x.data_ptr(), B, H, W, jobs_d.data_ptr(), ws.data_ptr(), st()), 'prologue apply')

    def both():
        grey()
        apply()

    grey()
    arms = [('grey means + fold', batch_bytes, grey), ('apply', 2 * batch_bytes, apply),
            ('apply, prologue fold', 2 * batch_bytes, prologue_apply), ('grey + fold + apply', 3 * batch_bytes, both)]
    for _, _, fn in arms:
        window(fn, 10)
    times = {name: [] for name, _, _ in arms}
    for _ in range(a.windows):
        for name, _, fn in arms:
            times[name].append(window(fn, a.launches))
    say('%d calls per window, %d windows per arm, alternating; microseconds per call; bound = bytes / %.1f TB/s' % (a.launches, a.windows, HBM_TBS))
    med = {}
    for name, nbytes, _ in arms:
        t = times[name]
        med[name] = float(np.median(t))
        bound = nbytes / (HBM_TBS * 1e12) * 1e6
        say('%-24s median %7.1f   min %7.1f   max %7.1f   spread %5.1f   %.2f TB/s of %d batch-sized streams   bound %.1f us: %.0f %% of it' % (
            name, med[name], min(t), max(t), max(t) - min(t), nbytes / (med[name] * 1e-6) / 1e12, nbytes // batch_bytes, bound,
            100 * bound / med[name]))
    d = med['apply, prologue fold'] - med['apply']
    spread = max(times['apply']) - min(times['apply'])
    say('apply with the fold in its prologue - apply behind the fold launch (medians): %+.1f us; spread of the apply windows: %.1f us '
        '(the fold launch itself is inside "grey means + fold")' % (d, spread))


def step(a, say):
    import train_imagenet as T
    base = ['-b', str(a.batch_size), '--optimizer', 'sgd', '--lr', '0.1', '--weight-decay', '5e-5', '--iterations', str(a.iterations),
            '--log-interval', '10', '--no-validation', '--seed', '0', '--dataset-size', str(2 * a.batch_size), '--synthetic-classes', '100',
            '--augment', 'rrc', '--augment-seed', '1', '--snapshot-interval', '100000', '--flat-log-dir']
    photo = ['--color-jitter', '0.4', '0.4', '0.4', '--lighting-std', '0.1', '--random-erase-prob', '0.25', '--photo-seed', '2']
    arms = [('plain', []), ('photometric', photo)]
    say('step: train_imagenet.py -b %d --optimizer sgd (ResNet-50 localizer, fp32, --augment rrc on the synthetic resident set), without and with %s'
        % (a.batch_size, ' '.join(photo[:-2])))
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
    spread = max(times['plain']) - min(times['plain'])
    d = med['photometric'] - med['plain']
    say('photometric - plain (medians): %+.2f ms (%.2f %%);  spread of the plain runs: %.2f ms: %s' % (
        d, (med['photometric'] / med['plain'] - 1) * 100, spread, 'inside it' if abs(d) <= spread else 'OUTSIDE it'))


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
