#!/usr/bin/env python
"""Time one ImageNet pre-training step -- ``Classifier(SheepLocalizer(train_imagenet=True))``, Adam -- with device events, and
say what the head costs: the flop counts of the three head GEMMs against the backbone's (``ops`` class accounting).

    python tools/imagenet_step.py -b 256 --steps 20 --warmup 5             (step time, ms: median / min / max)
    python tools/imagenet_step.py -b 256 --resnet-50 --loss bce --bce-target-thresh 0.2
        (the ResNet-50 localizer, the sigmoid binary cross-entropy on the label-smoothed target: tools/bce_bench.py)
    python tools/imagenet_step.py -b 256 --resnet-50 --drop-path 0.05     (stochastic depth: tools/droppath_bench.py)
    python tools/imagenet_step.py -b 256 --teacher-arch resnet50           (a ResNet-18 student under a frozen ResNet-50 teacher)
    python tools/imagenet_step.py -b 256 --resnet-50 --forward-only        (the test-mode forward alone: what a teacher costs;
        tools/distill_bench.py)
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/imagenet_step.py -b 256 --steps 3 --warmup 2
        (per-kernel times: gemm_tile_kernel / colsum_ordered_kernel / softmax_xent_* are the head and the loss)
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np      # noqa: E402
import torch            # noqa: E402

import loans_amd        # noqa: E402
from loans_amd.datasets import synthetic        # noqa: E402
from loans_amd.runtime import training          # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('-b', '--batch-size', type=int, default=256)
    ap.add_argument('--image-size', type=int, nargs=2, default=(224, 224))
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--dtype', default='f32', choices=['f32', 'bf16'])
    ap.add_argument('--resnet-50', action='store_true', help='the ResNet-50 localizer instead of the ResNet-18 one')
    ap.add_argument('--loss', default='softmax', choices=['softmax', 'bce'])
    ap.add_argument('--bce-target-thresh', type=float, default=None)
    ap.add_argument('--label-smoothing', type=float, default=0.0)
    ap.add_argument('--drop-path', type=float, default=0.0, help='stochastic depth at this rate (tools/droppath_bench.py)')
    ap.add_argument('--teacher-arch', default=None, choices=['resnet18', 'resnet50'], help='distil from a frozen teacher of this architecture (random weights: the time does not depend on them)')
    ap.add_argument('--teacher-dtype', default=None, choices=['f32', 'bf16'], help='the teacher\'s arithmetic (default: --dtype)')
    ap.add_argument('--distill-alpha', type=float, default=0.5)
    ap.add_argument('--distill-temperature', type=float, default=1.0)
    ap.add_argument('--forward-only', action='store_true', help='time the test-mode forward without backprop instead of the step')
    ap.add_argument('--out', default=None, help='also write the JSON result here')
    a = ap.parse_args(argv)
    assert torch.cuda.is_available(), 'this measurement needs a GPU'
    B, (H, W) = a.batch_size, a.image_size

    np.random.seed(0)
    localizer = loans_amd.Resnet50SheepLocalizer if a.resnet_50 else loans_amd.SheepLocalizer
    options = dict(loss='bce', bce_target_threshold=a.bce_target_thresh) if a.loss == 'bce' else {}
    if a.teacher_arch is not None:
        teacher = (loans_amd.Resnet50SheepLocalizer if a.teacher_arch == 'resnet50' else loans_amd.SheepLocalizer)((75, 75), train_imagenet=True)
        want = a.teacher_dtype or a.dtype
        teacher.set_precision(want, want)
        options.update(teacher=teacher, distill_alpha=a.distill_alpha, distill_temperature=a.distill_temperature)
    model = loans_amd.Classifier(localizer((75, 75), train_imagenet=True), label_smoothing=a.label_smoothing, **options)
    if a.drop_path > 0:
        model.predictor.set_drop_path(a.drop_path, seed=0)
    if a.dtype == 'bf16':
        model.set_precision('bf16', 'bf16')
    x, t = synthetic.make_classification_set(0, min(B, 64), 1000, H, W)
    reps = -(-B // len(x))
    x = torch.from_numpy(np.concatenate([x] * reps)[:B]).cuda()
    t = torch.from_numpy(np.concatenate([t] * reps)[:B]).cuda()
    opt = loans_amd.Adam(alpha=1e-3)
    opt.setup(model)
    upd = training.StandardUpdater(training.DeviceBatchIterator([(x, t)]), opt, converter=training.identity_converter, device=0)
    if a.forward_only:
        metrics = loans_amd.ClassificationMetrics()
        upd.update = lambda: model.evaluate(x, t, metrics)
    for _ in range(a.warmup):
        upd.update()
    torch.cuda.synchronize()
    times = []
    for _ in range(a.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        upd.update()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    head_flop = 3 * 2 * B * (2048 if a.resnet_50 else 512) * 1000
    res = {'what': 'imagenet_forward' if a.forward_only else 'imagenet_step', 'dtype': a.dtype, 'teacher': a.teacher_arch, 'localizer': localizer.__name__, 'loss_function': a.loss, 'drop_path': a.drop_path, 'batch': B, 'image_size': [H, W], 'steps': a.steps,
           'step_ms_median': float(np.median(times)), 'step_ms_min': float(min(times)), 'step_ms_max': float(max(times)),
           'images_per_s': B / (float(np.median(times)) * 1e-3), 'head_gflop': head_flop / 1e9,
           'loss': float(loans_amd.reporter.observation.get('loss', float('nan'))),
           'accuracy': float(loans_amd.reporter.observation.get('accuracy', float('nan')))}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    return res


if __name__ == '__main__':
    main()
