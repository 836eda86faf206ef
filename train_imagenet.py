#!/usr/bin/env python
"""ImageNet pre-training of the localizer backbones (the ``train_imagenet=True`` arm of the reference's localizers,
sheep/sheep_localizer.py:20-49,122-152): ``Classifier(SheepLocalizer(train_imagenet=True))`` -- softmax cross-entropy over
the 1000-way head -- trained with Adam (the default) or with the recipe every ResNet is trained with: momentum SGD, weight
decay, a stepped learning rate, label smoothing, top-1 and top-5 accuracy.  The snapshot it writes is what
``train_sheep_localizer.py --rl`` starts a LoANs run from: ``load_pretrained_model`` is not strict, so the backbone is taken
and ``fc`` / ``fc6`` are ignored.

    python train_imagenet.py train.tsv val.tsv --use-resnet-18 -b 64
    python train_imagenet.py --use-resnet-18 -b 32 --iterations 20            (seeded synthetic classes)
    python train_imagenet.py train.tsv val.tsv -b 256 --optimizer sgd --lr 0.1 --weight-decay 1e-4 \
        --lr-drop-epochs 30 60 90 --label-smoothing 0.1 --topk 5
    python train_sheep_localizer.py --use-resnet-18 --rl <log dir>/SheepLocalizer_20.npz

``train_file`` / ``val_file`` hold one tab-separated ``path<TAB>class`` line per image, paths relative to the file; the
literal ``synthetic`` (the default) is a seeded set of low-frequency textures, one per class.

``--lr-drop-epochs`` multiplies the rate (``lr``, or Adam's ``alpha``) by ``--lr-drop-factor`` from the first iteration of
each listed epoch on -- a host-side assignment, like Chainer's ``ExponentialShift``.  Label smoothing applies to the training
loss only; the validation loss stays the plain cross-entropy.

``--augment rrc`` is the usual input pipeline, finished on the GPU: training frames are a random-resized-crop (area fraction
``--rrc-scale``, aspect ratio ``--rrc-ratio``) mirrored with probability one half, validation frames the centre crop
(``--val-crop-pct`` of the largest box of the output's aspect ratio), both Pillow's BILINEAR resize to ``--image-size`` byte
for byte.  uint8 frames go up as they are -- only the rows a crop needs -- and one kernel launch per batch, on the iterator's
own stream, crops, mirrors, resizes and writes ``/ 255`` float32 CHW (loans_amd/common/datasets/crop_resize.py,
csrc/croprs.hip); the synthetic classes are kept in HBM as uint8 and cropped in place.  ``--augment-seed`` seeds the draws.
``--augment none`` (the default) is the squash to ``--image-size`` on the host, as before.

``--gpus N`` trains data parallel on N GPUs of the node, one process per GPU (loans_amd/launch.py forks them; under a
launcher of your own -- ``RANK`` / ``WORLD_SIZE`` set -- the script is a rank).  Every rank builds the same dataset and takes
every N-th example of it (loans_amd/common/datasets/shard.py: the training share padded by wrapping, so that all ranks make the
same iterations; the validation share not, so that every example counts once); gradients are summed over the ranks and
averaged in the optimiser's kernel.  ``-b`` is the batch PER GPU -- a step sees N x b frames -- and ``--lr`` is the rate of the
whole run: nothing is scaled automatically.  ``--warmup-epochs E`` ramps the rate linearly from ``--warmup-start-factor`` times
the scheduled rate at the start to the scheduled rate at epoch E, the gradual warm-up large batches need.  Validation under
``--gpus N`` (and with ``--validation-sums`` in one process) sums loss and hits over all examples on the device
(``ClassificationMetrics``: no host synchronisation per batch, a ragged last batch weighs what it holds), after rank 0's BN
running statistics went to every rank; its entries also carry ``validation/rows`` and ``validation/valid`` under ``--gpus N``.
Rank 0 alone prints, logs and writes snapshots.

``--frame-cache-gb G`` (with ``--augment rrc`` on files; per rank) decodes every file once: the uint8 frames are kept -- whole,
at any size, packed into slabs in HBM (``--frame-cache-where device``, the default) or as arrays in host memory (``host``) --
and from the second epoch on a batch is cropped straight out of them, no decode and, in HBM, no upload
(loans_amd/common/datasets/frame_cache.py, ``RaggedFrameCache``; no eviction: what does not fit is decoded every epoch, as
before).  The training and the validation set have caches of their own, G split between them in proportion to their numbers
of examples.  The first epoch uploads whole frames where it would have uploaded the crops' rows.  Logged entries then carry
``feed/cache_frames`` and ``feed/cache_bytes`` (what the training cache holds) and ``feed/cache_hits`` / ``feed/cache_misses``
(training examples served from it / decoded since the previous entry), and the same four under ``feed/val_cache_`` for the
validation set.

``--mixup-alpha A`` and ``--cutmix-alpha A`` (with ``--augment rrc``; default 0: off) add the two batch-mixing regularisers on
top of label smoothing.  One draw per batch, from a stream of its own (``--mix-seed``; the crops do not depend on it): with
probability ``--mix-prob`` (default 1) the batch is mixed, by CutMix with probability ``--mix-switch-prob`` (default 0.5) where
both alphas are given, else by mixup.  Every row is mixed with the row before it (row 0 with the last one): mixup blends the two
frames with a weight drawn from Beta(A, A), CutMix pastes a box of the partner whose share of the frame is one minus such a
weight -- one streaming launch behind the crop on the iterator's stream (loans_amd/common/datasets/batch_mix.py, csrc/mix.hip) --
and the loss is taken against the two labels with the same weight (``MixedLabels``; csrc/classify.hip,
``loans_softmax_xent_mix_fwd_f32``).  Under ``--gpus N`` every rank mixes inside its own batch, with the draws of
``--mix-seed`` + 7919 r.  The logged ``accuracy`` (and top-k accuracy) of a mixed run is against each row's dominant label; the
validation entries are the plain loss on unmixed frames.  A batch that is not mixed runs the one-label loss bit for bit.

    python train_imagenet.py train.tsv val.tsv -b 256 --optimizer sgd --lr 0.1 --augment rrc --label-smoothing 0.1 \
        --mixup-alpha 0.2 --cutmix-alpha 1.0

``--color-jitter B C S``, ``--lighting-std`` and ``--random-erase-prob`` (with ``--augment rrc``; default 0: off) are the
photometric half of the augmentation, on training batches only, between the crop and the mix: brightness, contrast and saturation
factors drawn uniformly from ``[max(0, 1 - v), 1 + v]`` and applied in a random order per image (hue is not built), AlexNet-style
PCA lighting noise of that standard deviation, and random erasing of one box per image with that probability (area fraction
``--random-erase-scale``, aspect ratio ``--random-erase-ratio``, filled with ``--random-erase-value`` -- the ImageNet mean by
default: the frames are not mean-subtracted).  The draws come from a stream of their own (``--photo-seed``, rank r from seed +
7919 r; the crops and the mixes do not depend on it) on the host, the pixels are changed in place on the GPU: one small reduction
for the contrast means and one streaming pass, on the iterator's stream (loans_amd/common/datasets/photometric.py, csrc/photo.hip).
Validation frames are never touched.

    python train_imagenet.py train.tsv val.tsv -b 256 --optimizer sgd --lr 0.1 --augment rrc --label-smoothing 0.1 \
        --color-jitter 0.4 0.4 0.4 --lighting-std 0.1 --random-erase-prob 0.25

``--rand-augment N M`` and ``--trivial-augment`` (with ``--augment rrc``; one of the two; default: off) are the learned-policy-free
augmentations of the RandAugment family, on training batches only, between the crop and the photometric stage (crop -> RandAugment
-> jitter / lighting / erase -> mix): RandAugment applies N (1 to 4) operations per image, each drawn uniformly from torchvision's
fourteen (Identity, ShearX/Y, TranslateX/Y, Rotate, Brightness, Color, Contrast, Sharpness, Posterize, Solarize, AutoContrast,
Equalize), at the magnitude bin M (0 to 30) with a random sign; TrivialAugmentWide applies one operation at a magnitude bin drawn
uniformly from 0..30 of its wider ranges.  ``--ra-fill R G B`` is what a pixel becomes whose source lies outside the frame after a
shear, shift or rotation (the ImageNet mean by default).  The draws come from a stream of their own (``--ra-seed``, rank r from
seed + 7919 r; the crops, the photometric and the mix draws do not depend on it) on the host, one job per image; the pixels are
changed on the GPU on the iterator's stream: per layer one small statistics step where an image needs one (Contrast's mean,
AutoContrast's extremes, Equalize's histograms) and one apply launch (loans_amd/common/datasets/rand_augment.py,
csrc/randaug.hip).  Validation frames are never touched.

    python train_imagenet.py train.tsv val.tsv -b 256 --optimizer sgd --lr 0.1 --augment rrc --label-smoothing 0.1 \
        --rand-augment 2 9

``--ema-decay D`` (default 0: off) keeps an exponential moving average of the weights and the BN statistics
(loans_amd/runtime/average.py, ``WeightAverage``: one launch per step behind the optimiser's; update t uses the decay
``min(D, (1 + t) / (10 + t))``).  When validation runs it runs twice -- the live model first, as always, then the averaged one, whose
entries are ``validation/ema/loss``, ``validation/ema/accuracy`` and ``validation/ema/accuracy_top<k>`` -- and beside every
``<LocalizerClass>_<it>.npz`` the averaged model is written as ``<LocalizerClass>_ema_<it>.npz`` with the same keys: the model to
hand to ``train_sheep_localizer.py --rl`` after a long run.  The average is part of the checkpoints; a checkpoint written without
the option is not resumed with it, nor the reverse.  ``--lr-schedule cosine`` (default ``step``) takes the rate from ``--lr`` at the
end of the warm-up down half a cosine to ``--lr-min`` (default 0) at ``--num-epoch``; ``--lr-drop-epochs`` belongs to ``step``.
``--no-decay-1d`` (with ``--optimizer sgd``, ``lars`` or ``lamb``) exempts BN scales / shifts and biases from ``--weight-decay``.  The schedule and the
exemption may change on resume, like ``--weight-decay``.

    python train_imagenet.py train.tsv val.tsv -b 256 --optimizer sgd --lr 0.1 --weight-decay 5e-5 --no-decay-1d \
        --lr-schedule cosine --lr-min 1e-5 --warmup-epochs 5 --num-epoch 300 --ema-decay 0.9999

``--optimizer lars`` is momentum SGD with a trust ratio per parameter tensor (LARS, You et al. 2017: ``loans_amd.LARS``), for the
large-batch end of the recipe -- ``-b`` is the batch per GPU and ``--lr`` the rate of the whole run, so 8 GPUs at ``-b 512`` are a
global batch of 4096, where plain momentum SGD with a linearly scaled rate stops converging.  The rate of a tensor is ``--lr`` times
``--lars-eta`` (default 0.001) ``* |w| / (|g| + --weight-decay * |w| + --lars-eps)`` (default 1e-8); BN scales / shifts and biases
never adapt and, with ``--no-decay-1d``, take no weight decay.  ``--momentum``, ``--weight-decay``, the warm-up, both schedules and
``--ema-decay`` mean what they mean for ``sgd``; ``--lars-eta`` / ``--lars-eps`` may change on resume, like ``--momentum``.

    python train_imagenet.py train.tsv val.tsv --gpus 8 -b 512 --dtype bf16 --optimizer lars --lr 10 --weight-decay 5e-5 \
        --no-decay-1d --lr-schedule cosine --warmup-epochs 5 --num-epoch 90 --label-smoothing 0.1 --augment rrc

``--optimizer lamb`` is the Adam-shaped large-batch optimiser (LAMB, You et al. 2019, algorithm 2: ``loans_amd.LAMB``): Adam's
bias-corrected direction ``a = m^ / (sqrt(v^) + --lamb-eps)`` (``--lamb-beta1``, default 0.9; ``--lamb-beta2``, default 0.999;
``--lamb-eps``, default 1e-6) plus the decoupled decay ``--weight-decay * w``, stepped per parameter tensor by ``--lr * |w| / |u|``, so
that every adapting tensor moves by ``--lr`` of its own norm per step.  BN scales / shifts and biases never adapt and, with
``--no-decay-1d``, take no weight decay.  ``--lr``, ``--weight-decay``, the warm-up, both schedules, ``--ema-decay``, ``--gpus N``
and the checkpoints work as for ``lars``; the betas and ``--lamb-eps`` may change on resume, like ``--momentum``.  The recipe the
augmentation options above were built for:

    python train_imagenet.py train.tsv val.tsv --gpus 8 -b 256 --dtype bf16 --optimizer lamb --lr 5e-3 --weight-decay 0.02 \
        --no-decay-1d --lr-schedule cosine --lr-min 1e-6 --warmup-epochs 5 --num-epoch 300 --augment rrc --mixup-alpha 0.2 \
        --cutmix-alpha 1.0 --color-jitter 0.4 0.4 0.4 --random-erase-prob 0.25 --ema-decay 0.9999 --clip-grad-norm 1.0

``--clip-grad-norm C`` (``C > 0``) clips the gradient by its global L2 norm before every step, with every ``--optimizer``
(``loans_amd.GradientClipping``, added behind the data-parallel exchange): where the norm ``N`` of the gradient the optimiser is about
to apply exceeds ``C`` the whole gradient is multiplied by ``C / N``, on the device, with nothing returning to the host.  Every log
entry then holds ``grad_norm``, the norm before clipping of the step the entry belongs to (read at the entry's synchronisation
point; under ``--gpus N`` it is the exchanged gradient's, the same on every rank), and the logged arguments hold
``clip_grad_norm``.  ``inf`` logs the norm and clips nothing.  A non-finite norm is logged and the gradient left as it is; the step
is not skipped.  Without the option no hook is added and the log holds what it always held.  The threshold may change on resume.

``--loss bce`` trains with the per-class sigmoid binary cross-entropy of "ResNet strikes back" (timm's A1 - A3 procedures) instead
of the softmax cross-entropy, on the same target: the label-smoothed one-hot row, or the two-label row of a mixup / CutMix batch
(csrc/classify.hip, ``loans_sigmoid_bce_fwd_f32``; one pass over the logits, like the softmax loss).  The logged ``loss`` is the mean
over classes and rows, torch's ``binary_cross_entropy_with_logits``; ``--bce-sum`` sums over the classes instead (1000 times the
value and the gradient on ImageNet).  ``--bce-target-thresh T`` (``0 <= T < 1``) makes the target 0 / 1 by ``target > T``: at 0.2 both
labels of a mixed row whose weights exceed it become positives.  ``accuracy`` and the top-k accuracy are what they are for the
softmax loss (the sigmoid is monotone), and the validation loss stays the plain softmax cross-entropy, comparable between runs of
either loss.  The three options are logged where one of them is given -- ``--loss`` as ``loss_function``, an entry's ``loss`` being
the training loss -- and may change on resume.

    python train_imagenet.py train.tsv val.tsv --gpus 8 -b 256 --dtype bf16 --optimizer lamb --lr 5e-3 --weight-decay 0.02 \
        --no-decay-1d --lr-schedule cosine --lr-min 1e-6 --warmup-epochs 5 --num-epoch 300 --augment rrc --mixup-alpha 0.2 \
        --cutmix-alpha 1.0 --color-jitter 0.4 0.4 0.4 --random-erase-prob 0.25 --rand-augment 2 9 --ema-decay 0.9999 \
        --clip-grad-norm 1.0 --loss bce --bce-target-thresh 0.2

``--drop-path P`` (``0 <= P < 1``; default 0: off) is stochastic depth, the regulariser of the same procedures (A1 / A2: 0.05):
torchvision's ``StochasticDepth(mode='row')``, timm's ``drop_path``.  Residual unit l of the backbone's L (8 in the ResNet-18
variant, 16 in ResNet-50), in forward order, has the rate ``p_l = P l / (L - 1)``; in a training step every sample drops the
unit's main branch with that probability and a kept one is scaled by ``1 / (1 - p_l)``: ``relu(r_b * bn(conv(..)) + shortcut)``.
The BN statistics are taken over all samples as before, validation (the averaged model's too) drops nothing, and a unit whose
rate is 0 -- every unit without the option -- runs the launches it always ran.  The keep table of a step is drawn on the host
from a stream of its own (``--drop-path-seed``, rank r from seed + 7919 r: the ranks drop different samples) and goes up in one
asynchronous copy; the junction's three passes are kernels of their own (loans_amd/functions/drop_path.py, csrc/bn_pool.hip:
``loans_bn_*_rows_*``).  Works with every ``--optimizer``, ``--dtype``, ``--loss`` and ``--gpus N``; both options are fixed on resume,
and the stream's state is part of the checkpoint.

    python train_imagenet.py train.tsv val.tsv --gpus 8 -b 256 --dtype bf16 --optimizer lamb --lr 5e-3 --weight-decay 0.02 \
        --no-decay-1d --lr-schedule cosine --lr-min 1e-6 --warmup-epochs 5 --num-epoch 300 --augment rrc --mixup-alpha 0.2 \
        --cutmix-alpha 1.0 --color-jitter 0.4 0.4 0.4 --random-erase-prob 0.25 --rand-augment 2 9 --ema-decay 0.9999 \
        --clip-grad-norm 1.0 --loss bce --bce-target-thresh 0.2 --drop-path 0.05

``--accum-steps K`` (an integer >= 1; default 1: off) is gradient accumulation, the way to the global batches the ``lars`` and
``lamb`` lines are tuned for on fewer GPUs: an iteration draws K micro-batches of ``-b`` frames per GPU, sums their gradients -- one
streaming launch per micro-batch into an accumulator the size of the gradient arena (csrc/accum.hip; ``GradientMethod.accumulate``),
``((g1 + g2) + ..) + gK`` in fp32 -- and steps once on their mean, so a step sees ``--gpus`` x K x b frames.  ``-b`` stays the batch per
GPU and micro-batch; ``--lr``, ``--iterations``, the log, snapshot and checkpoint intervals and the warm-up count optimiser steps and
epochs as before, and nothing is scaled automatically, as for ``--gpus``.  The logged ``loss`` and accuracies of an iteration are
the means over its K micro-batches, and an iteration is logged and validated as an epoch's last where any of its micro-batches
crossed the boundary.  Works with every ``--optimizer``, ``--dtype``, ``--loss``, the mixes, ``--drop-path`` (draws per micro-batch),
``--ema-decay`` (one update per optimiser step), ``--clip-grad-norm`` (the norm of the averaged accumulated gradient) and ``--gpus N``
(one all-reduce per step, of the sum, behind the last micro-batch: the overlap of the exchange with the backward is given up).  The
BN statistics are taken per micro-batch, as everywhere else, so an accumulated step is NOT the step of one batch of K x b frames:
the gradients differ wherever a batch norm lies in front of them, and the running statistics move K times per step.  The option
is logged as ``accum_steps`` where given and is fixed on resume, like ``-b`` (a checkpoint from before the option ran at 1); a
checkpoint lies between steps and holds nothing of the accumulator.  Not built: accumulation inside a captured step, and
``train_sheep_localizer.py`` (two optimisers in one joint step).  The LARS line on one GPU:

    python train_imagenet.py train.tsv val.tsv -b 512 --accum-steps 8 --dtype bf16 --optimizer lars --lr 10 --weight-decay 5e-5 \
        --no-decay-1d --lr-schedule cosine --warmup-epochs 5 --num-epoch 90 --label-smoothing 0.1 --augment rrc

``--teacher PATH`` is knowledge distillation: the model is trained against the logits of a frozen, larger one as well as against
the labels (Hinton et al. 2015), ``loss = (1 - A) CE + A T^2 KL(softmax(teacher / T) || softmax(student / T))`` -- torch's
``kl_div(log_softmax(z / T), softmax(zt / T), reduction='batchmean') * T * T`` beside the cross-entropy.  ``PATH`` is a snapshot
as this script writes it, the ``_ema_`` one included; ``--teacher-arch {resnet18,resnet50}`` (default ``resnet50``) names the
localizer that wrote it, ``--teacher-dtype {fp32,bf16}`` the arithmetic of its forward (default: the run's ``--dtype``),
``--distill-alpha A`` (``0 < A <= 1``, default 0.5) the weight of the KL term and ``--distill-temperature T`` (``2^-6 <= T <= 2^6``,
default 1) the temperature.  Every rank loads the file itself, strictly (a file that lacks a parameter or a BN statistic of the
architecture is refused).  In a training step the teacher runs first, in test mode and without backprop, on the very batch the
student sees -- mixed by mixup / CutMix where those are on -- then the student, then one loss launch over both logit matrices
(csrc/classify.hip, ``loans_softmax_distill_fwd_f32``).  ``--label-smoothing`` smooths the hard part only, ``--drop-path`` drops in
the student only, the weight average is the student's.  The teacher is no part of the model: it has an arena of its own, takes
no gradient, and joins neither the optimiser, the data-parallel exchange, the weight average, the snapshots nor the
checkpoints.  Every log entry gains ``distill_loss`` (the ``T^2 KL`` term, the mean over the rows with a label) and
``teacher_accuracy`` (the teacher's top-1 accuracy on the training batches, against the dominant label of a mixed row); ``loss`` is
the whole training loss, and validation is what it always was -- the plain softmax cross-entropy of the student, the teacher not
run.  The five options are logged in the first entry where ``--teacher`` is given and are not fixed on resume: a checkpoint
holds nothing of the teacher, and ``--resume`` needs ``--teacher`` again if the run is to go on distilling.  Works with every
``--optimizer``, ``--gpus N``, ``--accum-steps`` (the means over the micro-batches are logged) and ``--ema-decay``; not with
``--loss bce``.  Not built: feature / hint losses, several teachers, teacher logits cached on disk, a teacher in
``train_sheep_localizer.py`` or in a captured step.  A ResNet-18 student under the averaged ResNet-50 of an earlier run:

    python train_imagenet.py train.tsv val.tsv --use-resnet-18 -b 256 --dtype bf16 --optimizer sgd --lr 0.1 --weight-decay 5e-5 \
        --no-decay-1d --lr-schedule cosine --warmup-epochs 5 --num-epoch 100 --augment rrc --label-smoothing 0.1 --ema-decay 0.9999 \
        --teacher imagenet_logs/<time>_r50/Resnet50SheepLocalizer_ema_<iteration>.npz --distill-alpha 0.5 --distill-temperature 4

``--checkpoint-interval N`` writes a full-state checkpoint, ``checkpoint_<iteration>.npz`` in the log directory, after every
N-th iteration and after the last one (default 0: none; ``--checkpoint-keep K``, default 2, keeps the newest K): the model with
its BN statistics, the optimiser's buffers and step count, the training iterator as of the batch the step consumed (shuffle
stream, order, position, the crop / mirror draw stream, the RandAugment, the photometric and the mix draw stream), the stochastic depth draw stream, NumPy's global stream and the run's arguments
(loans_amd/runtime/checkpoint.py; under ``--gpus N`` one small record per rank beside rank 0's file, which is written last).
``--resume PATH`` -- a checkpoint file, or a log directory, whose newest complete checkpoint is taken -- continues that run in
its log directory: the ``log`` file is read back and appended to, ``elapsed_time`` and the snapshot names count on.  Fixed on
resume (one error lists every one that differs): the architecture, ``--dtype``, ``--optimizer``, ``-b``, ``--gpus``,
``--image-size``, the dataset files or the synthetic sizes, classes and ``--data-seed``, ``--no-shuffle``, ``--augment`` /
``--rrc-*`` / ``--val-crop-pct`` / ``--augment-seed``, ``--mixup-alpha`` / ``--cutmix-alpha`` / ``--mix-*``, ``--color-jitter`` / ``--lighting-std`` / ``--random-erase-*`` / ``--photo-seed``, ``--rand-augment`` / ``--trivial-augment`` / ``--ra-fill`` / ``--ra-seed``, ``--drop-path`` / ``--drop-path-seed``, ``--accum-steps``, ``--ema-decay`` (a checkpoint from
before these options existed ran at their defaults), ``--seed``.  Taken from the new command line (each one that differs is
printed once): ``--num-epoch``, ``--iterations``, the log, snapshot and checkpoint intervals, ``--loader-threads``, the frame
cache options, ``--lr``, ``--weight-decay``, ``--momentum``, ``--lr-drop-*``, ``--lr-schedule``, ``--lr-min``, ``--no-decay-1d``, ``--lars-eta``, ``--lars-eps``, ``--lamb-beta1``, ``--lamb-beta2``, ``--lamb-eps``, ``--clip-grad-norm``, ``--warmup-*``, ``--label-smoothing``, ``--topk``, ``--loss``, ``--bce-target-thresh``, ``--bce-sum``, ``--teacher`` with ``--teacher-arch``, ``--teacher-dtype``, ``--distill-alpha`` and ``--distill-temperature``.  The
frame caches start empty after a resume and refill during the first epoch.

    python train_imagenet.py train.tsv val.tsv -b 256 --optimizer sgd --lr 0.1 --lr-drop-epochs 30 60 90 --checkpoint-interval 500
    python train_imagenet.py train.tsv val.tsv -b 256 --optimizer sgd --lr 0.1 --lr-drop-epochs 30 60 90 --checkpoint-interval 500 \
        --resume imagenet_logs/<time>_test

Not built (follow-ups): ``--use-graph``.
"""
import os

if __name__ == "__main__":
    # `--gpus N` (N > 1) outside a launcher: fork the N ranks as a child process group before anything touches the GPU; does
    # not return
    import importlib.util
    _spec = importlib.util.spec_from_file_location(
        '_loans_launch', os.path.join(os.path.dirname(os.path.abspath(__file__)), 'loans_amd', 'launch.py'))
    _launch = importlib.util.module_from_spec(_spec)
    _spec.loader.exec_module(_launch)
    _launch.launch_if_parent(os.path.abspath(__file__))

import argparse             # noqa: E402
import datetime             # noqa: E402
import json                 # noqa: E402
import math                 # noqa: E402
import time                 # noqa: E402

import numpy as np          # noqa: E402
import torch                # noqa: E402

import loans_amd            # noqa: E402
from loans_amd import parallel                                      # noqa: E402
from loans_amd.common.datasets.shard import ShardedDataset          # noqa: E402
from loans_amd.datasets import synthetic                            # noqa: E402
from loans_amd.runtime import checkpoint, training                  # noqa: E402

SYNTHETIC = 'synthetic'
# what --resume holds against the checkpoint's arguments: everything the data sequence and the model's shape depend on
RESUME_FIXED = ('use_resnet_18', 'dtype', 'optimizer', 'batch_size', 'gpus', 'image_size', 'train_file', 'val_file', 'dataset_size',
                'validation_size', 'synthetic_classes', 'data_seed', 'no_shuffle', 'augment', 'rrc_scale', 'rrc_ratio', 'val_crop_pct',
                'augment_seed', 'seed', 'mixup_alpha', 'cutmix_alpha', 'mix_prob', 'mix_switch_prob', 'mix_seed', 'ema_decay',
                'color_jitter', 'lighting_std', 'random_erase_prob', 'random_erase_scale', 'random_erase_ratio', 'random_erase_value',
                'photo_seed', 'rand_augment', 'trivial_augment', 'ra_fill', 'ra_seed', 'drop_path', 'drop_path_seed', 'accum_steps')


class SyntheticClasses:
    """``LabeledImageDataset`` stand-in: (float32 CHW RGB frame in [0,1], int32 class) pairs"""

    def __init__(self, n, classes, image_size, seed=0, split=0):
        self.x, self.t = synthetic.make_classification_set(seed, n, classes, image_size[0], image_size[1], split=split)

    def __len__(self):
        return len(self.x)

    def __getitem__(self, i):
        return self.x[i], self.t[i]

    get_example = __getitem__


class Arguments(argparse.Namespace):
    """The options of the input pipeline are read from here where the command line does not give them: a namespace parsed from
    a command line without them holds exactly the options of a ``--augment none`` run, and ``run`` writes the ones it ran with
    into it (and so into the first log entry, beside the other arguments)."""
    augment = 'none'
    rrc_scale = (0.08, 1.0)
    rrc_ratio = (3 / 4, 4 / 3)
    val_crop_pct = 0.875
    augment_seed = None

    # data parallel
    gpus = 1
    warmup_epochs = 0.0
    warmup_start_factor = 0.1
    validation_sums = False

    # decode-once frame cache of --augment rrc on files
    frame_cache_gb = 0.0
    frame_cache_where = 'device'

    # full-state checkpoints (loans_amd/runtime/checkpoint.py: FLAGS); logged only where the command line gives them
    checkpoint_interval = 0
    checkpoint_keep = 2
    resume = None

    # mixup / CutMix of the --augment rrc feed (loans_amd/common/datasets/batch_mix.py); both alphas 0: off
    mixup_alpha = 0.0
    cutmix_alpha = 0.0
    mix_prob = 1.0
    mix_switch_prob = 0.5
    mix_seed = None

    _PIPELINE = ('augment', 'rrc_scale', 'rrc_ratio', 'val_crop_pct', 'augment_seed')
    _PARALLEL = ('gpus', 'warmup_epochs', 'warmup_start_factor', 'validation_sums')
    _CACHE = ('frame_cache_gb', 'frame_cache_where')
    # weight average, cosine rate, decay-free 1-d parameters (loans_amd/runtime/average.py, optimizers.py); all off by default
    ema_decay = 0.0
    lr_schedule = 'step'
    lr_min = 0.0
    no_decay_1d = False

    # --optimizer lars (loans_amd/runtime/optimizers.py: LARS); logged with that optimiser only
    lars_eta = 0.001
    lars_eps = 1e-8

    # --optimizer lamb (loans_amd/runtime/optimizers.py: LAMB); logged with that optimiser only
    lamb_beta1 = 0.9
    lamb_beta2 = 0.999
    lamb_eps = 1e-6

    # colour jitter, lighting noise, random erasing of the --augment rrc feed (loans_amd/common/datasets/photometric.py); all off by
    # default, logged where one of them is given
    color_jitter = (0.0, 0.0, 0.0)
    lighting_std = 0.0
    random_erase_prob = 0.0
    random_erase_scale = (0.02, 0.33)
    random_erase_ratio = (0.3, 3.3)
    random_erase_value = (0.485, 0.456, 0.406)
    photo_seed = None

    # RandAugment / TrivialAugmentWide of the --augment rrc feed (loans_amd/common/datasets/rand_augment.py); off by default, logged
    # where one of them is given
    rand_augment = None
    trivial_augment = False
    ra_fill = (0.485, 0.456, 0.406)
    ra_seed = None
    _RA = ('rand_augment', 'trivial_augment', 'ra_fill', 'ra_seed')

    _MIX = ('mixup_alpha', 'cutmix_alpha', 'mix_prob', 'mix_switch_prob', 'mix_seed')
    _PHOTO = ('color_jitter', 'lighting_std', 'random_erase_prob', 'random_erase_scale', 'random_erase_ratio', 'random_erase_value',
              'photo_seed')
    _AVERAGE = ('ema_decay', 'lr_schedule', 'lr_min', 'no_decay_1d')
    _LARS = ('lars_eta', 'lars_eps')
    _LAMB = ('lamb_beta1', 'lamb_beta2', 'lamb_eps')

    # --clip-grad-norm (loans_amd/runtime/optimizers.py: GradientClipping); None: off, no hook, nothing logged
    clip_grad_norm = None
    _CLIP = ('clip_grad_norm',)

    # --loss bce (loans_amd/classifier.py, csrc/classify.hip: loans_sigmoid_bce_fwd_f32); logged only where given
    loss = 'softmax'
    bce_target_thresh = None
    bce_sum = False
    _LOSS = ('loss', 'bce_target_thresh', 'bce_sum')

    # --drop-path: stochastic depth in the residual units (loans_amd/functions/drop_path.py); 0: off, logged only where given
    drop_path = 0.0
    drop_path_seed = None
    _DROP = ('drop_path', 'drop_path_seed')

    # --accum-steps: gradient accumulation (loans_amd/runtime/optimizers.py: GradientMethod.accumulate); 1: off, logged only where given
    accum_steps = 1
    _ACCUM = ('accum_steps',)

    # --teacher: knowledge distillation from a frozen snapshot (loans_amd/classifier.py, csrc/classify.hip:
    # loans_softmax_distill_fwd_f32); None: nothing is loaded, launched or logged.  teacher_dtype None: the run's --dtype;
    # distill_alpha None: 0.5 with a teacher
    teacher = None
    teacher_arch = 'resnet50'
    teacher_dtype = None
    distill_alpha = None
    distill_temperature = 1.0
    _DISTILL = ('teacher', 'teacher_arch', 'teacher_dtype', 'distill_alpha', 'distill_temperature')


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description="ImageNet pre-training of a localizer backbone (MI355X-native)")
    parser.add_argument("train_file", nargs='?', default=SYNTHETIC, help="tab-separated `path<TAB>class` lines ('synthetic': seeded textures)")
    parser.add_argument("val_file", nargs='?', default=SYNTHETIC, help="validation file in the same format")
    parser.add_argument("--use-resnet-18", action='store_true', default=False, help="SheepLocalizer (ResNet-18 variant) instead of the ResNet-50 one")
    parser.add_argument("-b", "--batch-size", type=int, default=32, help="batch size")
    parser.add_argument("-g", "--gpu", type=int, default=-1, help="gpu id to use (-1: the current device)")
    parser.add_argument("--lr", "--learning-rate", dest="learning_rate", type=float, default=0.001, help="Adam's alpha / momentum SGD's, LARS's and LAMB's lr")
    parser.add_argument("--weight-decay", type=float, default=0.0, help="weight_decay_rate of the optimiser")
    parser.add_argument("--optimizer", default='adam', choices=['adam', 'sgd', 'lars', 'lamb'], help="Adam, SGD with momentum, LARS (momentum SGD with per-layer trust ratios) or LAMB (Adam with decoupled decay and per-layer trust ratios), the last two for large batches")
    parser.add_argument("--momentum", type=float, default=0.9, help="momentum of --optimizer sgd / lars")
    parser.add_argument("--lr-drop-epochs", type=int, nargs='+', default=(), help="epochs at whose first iteration the rate is multiplied by --lr-drop-factor")
    parser.add_argument("--lr-drop-factor", type=float, default=0.1, help="factor of each learning rate step")
    parser.add_argument("--label-smoothing", type=float, default=0.0, help="label smoothing of the training loss (uniform over all classes)")
    parser.add_argument("--topk", type=int, default=None, help="also report top-k accuracy (default: 5 with --optimizer sgd / lars / lamb, off with adam; 0: off)")
    parser.add_argument("--num-epoch", type=int, default=100, help="number of epochs to train")
    parser.add_argument("--iterations", type=int, default=None, help="stop after this many iterations (before --num-epoch epochs)")
    parser.add_argument("--image-size", type=int, nargs=2, default=(224, 224), help="input size")
    parser.add_argument("-l", "--log-dir", default='imagenet_logs', help="path to log dir")
    parser.add_argument("--ln", "--log-name", dest="ln", default="test", help="name of log")
    parser.add_argument("--log-interval", type=int, default=100, help="log interval")
    parser.add_argument("--snapshot-interval", type=int, default=1000, help="number of iterations after which a snapshot will be taken")
    parser.add_argument("--dtype", default='f32', choices=['f32', 'bf16'], help="f32, or bf16 activations and bf16 MFMA in the backbone (the head and the loss stay fp32)")
    parser.add_argument("--seed", type=int, default=None, help="seed NumPy's global RNG before the model is built (the initialisers draw from it)")
    parser.add_argument("--no-shuffle", action='store_true', help="iterate the training set in order")
    parser.add_argument("--no-validation", dest='validation', action='store_false', default=True, help="don't do validation")
    # the synthetic set
    parser.add_argument("--dataset-size", type=int, default=256, help="synthetic training examples")
    parser.add_argument("--validation-size", type=int, default=64, help="synthetic validation examples")
    parser.add_argument("--synthetic-classes", type=int, default=10, help="classes of the synthetic set (labels 0 .. n-1 of the 1000-way head)")
    parser.add_argument("--data-seed", type=int, default=10, help="seed of the synthetic set")
    parser.add_argument("--flat-log-dir", action='store_true', help="write into --log-dir itself (no <time>_<name> sub-directory)")
    parser.add_argument("--loader-threads", type=int, default=4, help="decode threads per iterator")
    # the input pipeline
    parser.add_argument("--augment", default=argparse.SUPPRESS, choices=['none', 'rrc'], help="none: squash every frame to --image-size on the host; rrc: random-resized-crop + mirror (training) and centre crop (validation) on the GPU")
    parser.add_argument("--rrc-scale", type=float, nargs=2, default=argparse.SUPPRESS, metavar=('LO', 'HI'), help="area fraction of a random-resized-crop (default 0.08 1)")
    parser.add_argument("--rrc-ratio", type=float, nargs=2, default=argparse.SUPPRESS, metavar=('LO', 'HI'), help="aspect ratio (width / height) of a random-resized-crop (default 3/4 4/3)")
    parser.add_argument("--val-crop-pct", type=float, default=argparse.SUPPRESS, help="side of the validation centre crop as a fraction of the largest fitting box (default 0.875)")
    parser.add_argument("--augment-seed", type=int, default=argparse.SUPPRESS, help="seed of the crop / mirror draws")
    # data parallel
    parser.add_argument("--gpus", type=int, default=argparse.SUPPRESS, help="train data parallel on this many GPUs of the node, one process each (-b is the batch per GPU)")
    parser.add_argument("--warmup-epochs", type=float, default=argparse.SUPPRESS, help="ramp the rate linearly up to the scheduled one over this many epochs (default 0: off)")
    parser.add_argument("--warmup-start-factor", type=float, default=argparse.SUPPRESS, help="fraction of the scheduled rate the warm-up starts from (default 0.1)")
    parser.add_argument("--validation-sums", action='store_true', default=argparse.SUPPRESS, help="validate by summing loss and hits over all examples on the device (always on with --gpus N)")
    # decode-once frame cache
    parser.add_argument("--frame-cache-gb", type=float, default=argparse.SUPPRESS, help="with --augment rrc on files: keep up to this many GB of decoded frames per rank and crop later epochs out of them (default 0: off)")
    parser.add_argument("--frame-cache-where", default=argparse.SUPPRESS, choices=['device', 'host'], help="keep the frames in HBM (default) or in host memory")
    # mixup / CutMix
    parser.add_argument("--mixup-alpha", type=float, default=argparse.SUPPRESS, help="with --augment rrc: mixup, the weight of a batch drawn from Beta(A, A) (default 0: off)")
    parser.add_argument("--cutmix-alpha", type=float, default=argparse.SUPPRESS, help="with --augment rrc: CutMix, the kept share of the frame drawn from Beta(A, A) (default 0: off)")
    parser.add_argument("--mix-prob", type=float, default=argparse.SUPPRESS, help="probability that a batch is mixed at all (default 1)")
    parser.add_argument("--mix-switch-prob", type=float, default=argparse.SUPPRESS, help="with both alphas: probability that a mixed batch takes CutMix, not mixup (default 0.5)")
    parser.add_argument("--mix-seed", type=int, default=argparse.SUPPRESS, help="seed of the mix draws (a stream of their own)")
    # colour jitter, lighting noise, random erasing
    parser.add_argument("--color-jitter", type=float, nargs=3, default=argparse.SUPPRESS, metavar=('B', 'C', 'S'), help="with --augment rrc: brightness, contrast and saturation factors uniform in [max(0, 1 - v), 1 + v], applied in a random order per image; hue is not built (default 0 0 0: off)")
    parser.add_argument("--lighting-std", type=float, default=argparse.SUPPRESS, help="with --augment rrc: standard deviation of the AlexNet-style PCA lighting noise (default 0: off)")
    parser.add_argument("--random-erase-prob", type=float, default=argparse.SUPPRESS, help="with --augment rrc: probability that a training image has one box erased (default 0: off)")
    parser.add_argument("--random-erase-scale", type=float, nargs=2, default=argparse.SUPPRESS, metavar=('LO', 'HI'), help="area fraction of the erased box (default 0.02 0.33)")
    parser.add_argument("--random-erase-ratio", type=float, nargs=2, default=argparse.SUPPRESS, metavar=('LO', 'HI'), help="aspect ratio (height / width) of the erased box, log-uniform (default 0.3 3.3)")
    parser.add_argument("--random-erase-value", type=float, nargs=3, default=argparse.SUPPRESS, metavar=('R', 'G', 'B'), help="what an erased pixel becomes (default 0.485 0.456 0.406, the ImageNet mean: the frames are not mean-subtracted)")
    parser.add_argument("--photo-seed", type=int, default=argparse.SUPPRESS, help="seed of the colour jitter / lighting / erase draws (a stream of their own)")
    # RandAugment / TrivialAugmentWide
    parser.add_argument("--rand-augment", type=int, nargs=2, default=argparse.SUPPRESS, metavar=('N', 'M'), help="with --augment rrc: RandAugment, N random operations (1 to 4) per training image at magnitude bin M (0 to 30), between the crop and the photometric stage (default: off)")
    parser.add_argument("--trivial-augment", action='store_true', default=argparse.SUPPRESS, help="with --augment rrc: TrivialAugmentWide, one random operation per training image at a random magnitude; not with --rand-augment (default: off)")
    parser.add_argument("--ra-fill", type=float, nargs=3, default=argparse.SUPPRESS, metavar=('R', 'G', 'B'), help="what a pixel becomes whose source lies outside the frame after a shear, shift or rotation (default 0.485 0.456 0.406, the ImageNet mean)")
    parser.add_argument("--ra-seed", type=int, default=argparse.SUPPRESS, help="seed of the RandAugment / TrivialAugment draws (a stream of their own)")
    # weight average, cosine rate, decay-free 1-d parameters
    parser.add_argument("--ema-decay", type=float, default=argparse.SUPPRESS, help="keep an exponential moving average of the weights with this decay (warmed up as (1 + t) / (10 + t)); validated and snapshotted beside the live model (default 0: off)")
    parser.add_argument("--lr-schedule", default=argparse.SUPPRESS, choices=['step', 'cosine'], help="step: --lr-drop-epochs; cosine: half a cosine from --lr down to --lr-min over --num-epoch, behind the warm-up (default step)")
    parser.add_argument("--lr-min", type=float, default=argparse.SUPPRESS, help="the rate --lr-schedule cosine ends at (default 0)")
    parser.add_argument("--no-decay-1d", action='store_true', default=argparse.SUPPRESS, help="with --optimizer sgd / lars / lamb: no weight decay on BN scales / shifts and on biases")
    # LARS
    parser.add_argument("--lars-eta", type=float, default=argparse.SUPPRESS, help="with --optimizer lars: the trust coefficient (default 0.001)")
    parser.add_argument("--lars-eps", type=float, default=argparse.SUPPRESS, help="with --optimizer lars: added to the trust ratio's denominator (default 1e-8)")
    # LAMB
    parser.add_argument("--lamb-beta1", type=float, default=argparse.SUPPRESS, help="with --optimizer lamb: decay of the first moment (default 0.9)")
    parser.add_argument("--lamb-beta2", type=float, default=argparse.SUPPRESS, help="with --optimizer lamb: decay of the second moment (default 0.999)")
    parser.add_argument("--lamb-eps", type=float, default=argparse.SUPPRESS, help="with --optimizer lamb: added to the root of the second moment (default 1e-6)")
    # gradient clipping
    parser.add_argument("--clip-grad-norm", type=float, default=argparse.SUPPRESS, metavar='C', help="clip the gradient to the global L2 norm C > 0 before every step and log its norm as grad_norm; inf: log the norm only (default: off)")
    # the training loss
    parser.add_argument("--loss", default=argparse.SUPPRESS, choices=['softmax', 'bce'], help="softmax cross-entropy (default) or the per-class sigmoid binary cross-entropy on the same smoothed / mixed target; the validation loss is the plain softmax cross-entropy either way")
    parser.add_argument("--bce-target-thresh", type=float, default=argparse.SUPPRESS, metavar='T', help="with --loss bce: make the target 0 / 1 by target > T, T in [0, 1) (default: the soft target)")
    parser.add_argument("--bce-sum", action='store_true', default=argparse.SUPPRESS, help="with --loss bce: sum the loss over the classes instead of averaging it (the mean over the rows either way)")
    # stochastic depth
    parser.add_argument("--drop-path", type=float, default=argparse.SUPPRESS, metavar='P', help="stochastic depth: in training, residual unit l of L drops its main branch per sample with probability P l / (L - 1) and scales the kept ones by 1 / (1 - p), P in [0, 1) (default 0: off)")
    parser.add_argument("--drop-path-seed", type=int, default=argparse.SUPPRESS, help="seed of the stochastic depth draws (a stream of their own)")
    # gradient accumulation
    parser.add_argument("--accum-steps", type=int, default=argparse.SUPPRESS, metavar='K', help="gradient accumulation: sum the gradients of K micro-batches of -b frames per GPU and step once on their mean; iterations, intervals, --lr and the warm-up count optimiser steps (default 1: off)")
    # knowledge distillation
    parser.add_argument("--teacher", default=argparse.SUPPRESS, metavar='PATH', help="distil from this frozen snapshot (a <Localizer>_<it>.npz or _ema_ file as this script writes it): loss = (1 - A) CE + A T^2 KL(teacher || student); every rank loads it itself (default: off)")
    parser.add_argument("--teacher-arch", default=argparse.SUPPRESS, choices=['resnet18', 'resnet50'], help="with --teacher: the localizer the snapshot was written by (default resnet50)")
    parser.add_argument("--teacher-dtype", default=argparse.SUPPRESS, choices=['fp32', 'f32', 'bf16'], help="with --teacher: the arithmetic of the teacher's forward (default: the run's --dtype)")
    parser.add_argument("--distill-alpha", type=float, default=argparse.SUPPRESS, metavar='A', help="with --teacher: the weight of the distillation term, A in (0, 1] (default 0.5)")
    parser.add_argument("--distill-temperature", type=float, default=argparse.SUPPRESS, metavar='T', help="with --teacher: the temperature both logit rows are divided by, T in [2^-6, 2^6] (default 1)")
    checkpoint.add_arguments(parser, argparse.SUPPRESS)
    args = parser.parse_args(argv, namespace=Arguments())
    try:
        check_cache_arguments(args)
        check_mix_arguments(args)
        check_photo_arguments(args)
        check_ra_arguments(args)
        check_average_arguments(args)
        check_lars_arguments(args)
        check_lamb_arguments(args)
        check_clip_arguments(args)
        check_loss_arguments(args)
        check_drop_arguments(args)
        check_accum_arguments(args)
        check_distill_arguments(args)
        if args.resume is not None:
            check_average_resume(args)
            world = os.environ.get('WORLD_SIZE')        # a rank under a launcher: the group's size, whatever --gpus says
            checkpoint.resolve_resume(args, RESUME_FIXED, world=None if world is None else int(world), defaults=RESUME_DEFAULTS_WITH_ACCUM)
    except ValueError as e:
        parser.error(str(e))
    return args


def check_cache_arguments(args):
    """ValueError where ``--frame-cache-gb`` is asked of a run that has nothing to cache"""
    gb = args.frame_cache_gb
    if gb < 0:
        raise ValueError('--frame-cache-gb must not be negative, got %r' % gb)
    if gb > 0 and args.augment != 'rrc':
        raise ValueError('--frame-cache-gb caches the frames the GPU crops: it needs --augment rrc')
    if gb > 0 and args.train_file == SYNTHETIC:
        raise ValueError('--frame-cache-gb caches decoded files: the synthetic classes already lie in HBM, give a train_file')


def check_mix_arguments(args):
    """ValueError for mix options that name no distribution, and where mixing is asked of a feed that is not on the device"""
    for name in ('mixup_alpha', 'cutmix_alpha'):
        if not getattr(args, name) >= 0:
            raise ValueError('--%s must not be negative, got %r' % (name.replace('_', '-'), getattr(args, name)))
    for name in ('mix_prob', 'mix_switch_prob'):
        if not 0.0 <= getattr(args, name) <= 1.0:
            raise ValueError('--%s is a probability: it must lie in [0, 1], got %r' % (name.replace('_', '-'), getattr(args, name)))
    if (args.mixup_alpha > 0 or args.cutmix_alpha > 0) and args.augment != 'rrc':
        raise ValueError('--mixup-alpha / --cutmix-alpha mix the batches the GPU crops: they need --augment rrc')


def photo_enabled(args):
    """whether any of the photometric stages is switched on"""
    return any(v > 0 for v in args.color_jitter) or args.lighting_std > 0 or args.random_erase_prob > 0


def check_photo_arguments(args):
    """ValueError for photometric options that name no distribution, and where a stage is asked of a feed that is not on the device"""
    if len(args.color_jitter) != 3 or not all(v >= 0 for v in args.color_jitter):
        raise ValueError('--color-jitter takes three strengths that must not be negative, got %r' % (tuple(args.color_jitter),))
    if not args.lighting_std >= 0:
        raise ValueError('--lighting-std must not be negative, got %r' % args.lighting_std)
    if not 0.0 <= args.random_erase_prob <= 1.0:
        raise ValueError('--random-erase-prob is a probability: it must lie in [0, 1], got %r' % args.random_erase_prob)
    for name in ('random_erase_scale', 'random_erase_ratio'):
        pair = tuple(getattr(args, name))
        if len(pair) != 2 or not 0 < pair[0] <= pair[1] < math.inf:
            raise ValueError('--%s takes a positive, ordered range, got %r' % (name.replace('_', '-'), pair))
    if len(args.random_erase_value) != 3 or not all(math.isfinite(v) for v in args.random_erase_value):
        raise ValueError('--random-erase-value takes three finite numbers, got %r' % (tuple(args.random_erase_value),))
    if photo_enabled(args) and args.augment != 'rrc':
        raise ValueError('--color-jitter / --lighting-std / --random-erase-prob change the batches the GPU crops: they need --augment rrc')


def ra_enabled(args):
    """whether RandAugment or TrivialAugment is switched on"""
    return args.rand_augment is not None or bool(args.trivial_augment)


def check_ra_arguments(args):
    """ValueError for a RandAugment that names no policy, for both policies at once, and where the stage is asked of a feed that is
    not on the device"""
    if args.rand_augment is not None:
        pair = tuple(args.rand_augment)
        if len(pair) != 2 or not all(isinstance(v, int) for v in pair) or not 1 <= pair[0] <= 4 or not 0 <= pair[1] <= 30:
            raise ValueError('--rand-augment takes N layers, 1 to 4, and a magnitude bin M, 0 to 30, got %r' % (pair,))
        if args.trivial_augment:
            raise ValueError('--rand-augment and --trivial-augment are two policies: give one of them')
    if len(args.ra_fill) != 3 or not all(math.isfinite(v) for v in args.ra_fill):
        raise ValueError('--ra-fill takes three finite numbers, got %r' % (tuple(args.ra_fill),))
    if ra_enabled(args) and args.augment != 'rrc':
        raise ValueError('--rand-augment / --trivial-augment change the batches the GPU crops: they need --augment rrc')


def check_average_arguments(args):
    """ValueError for an --ema-decay that is no decay, and for options that contradict each other"""
    if not 0.0 <= args.ema_decay < 1.0:
        raise ValueError('--ema-decay is a decay: it must lie in [0, 1), got %r' % args.ema_decay)
    if args.lr_schedule == 'cosine' and len(args.lr_drop_epochs) > 0:
        raise ValueError('--lr-drop-epochs belongs to --lr-schedule step: the cosine rate has no steps')
    if args.lr_min < 0:
        raise ValueError('--lr-min must not be negative, got %r' % args.lr_min)
    if args.no_decay_1d and args.optimizer not in ('sgd', 'lars', 'lamb'):
        raise ValueError('--no-decay-1d is built for --optimizer sgd: Adam\'s kernel applies one weight decay to every parameter')


def check_lars_arguments(args):
    """ValueError for a trust coefficient or an epsilon the kernel refuses, and for either given to another optimiser"""
    if not args.lars_eta > 0:
        raise ValueError('--lars-eta must be positive, got %r' % args.lars_eta)
    if not args.lars_eps >= 0:
        raise ValueError('--lars-eps must not be negative, got %r' % args.lars_eps)
    if args.optimizer != 'lars' and any(name in vars(args) for name in Arguments._LARS):
        raise ValueError('--lars-eta / --lars-eps belong to --optimizer lars')


def check_lamb_arguments(args):
    """ValueError for betas or an epsilon the kernels refuse, and for any of the three given to another optimiser"""
    for name in ('lamb_beta1', 'lamb_beta2'):
        if not 0 <= getattr(args, name) < 1:
            raise ValueError('--%s must lie in [0, 1), got %r' % (name.replace('_', '-'), getattr(args, name)))
    if not args.lamb_eps >= 0:
        raise ValueError('--lamb-eps must not be negative, got %r' % args.lamb_eps)
    if args.optimizer != 'lamb' and any(name in vars(args) for name in Arguments._LAMB):
        raise ValueError('--lamb-beta1 / --lamb-beta2 / --lamb-eps belong to --optimizer lamb')


def check_clip_arguments(args):
    """ValueError for a --clip-grad-norm that is no threshold"""
    c = args.clip_grad_norm
    if c is not None and not c > 0:
        raise ValueError('--clip-grad-norm is the largest gradient norm a step is taken with: it must be positive, or inf to log the '
                         'norm without clipping, got %r' % c)


def check_loss_arguments(args):
    """ValueError for a --bce-target-thresh that is no threshold, and for a BCE option given to the softmax loss"""
    if args.loss not in ('softmax', 'bce'):
        raise ValueError('--loss is softmax or bce, got %r' % (args.loss,))
    t = args.bce_target_thresh
    if t is not None and not 0.0 <= t < 1.0:
        raise ValueError('--bce-target-thresh is compared with a target in [0, 1]: it must lie in [0, 1), got %r' % t)
    if args.loss != 'bce' and (t is not None or args.bce_sum):
        raise ValueError('--bce-target-thresh / --bce-sum belong to --loss bce')


def check_drop_arguments(args):
    """ValueError for a --drop-path that is no probability below 1"""
    if not 0.0 <= args.drop_path < 1.0:
        raise ValueError('--drop-path is the largest drop probability of a residual unit: it must lie in [0, 1), got %r' % args.drop_path)


def check_accum_arguments(args):
    """ValueError for an --accum-steps that is no number of micro-batches"""
    k = args.accum_steps
    if isinstance(k, bool) or not isinstance(k, int) or k < 1:
        raise ValueError('--accum-steps is the number of micro-batches of one optimiser step: it must be an integer >= 1, got %r' % (k,))


DISTILL_T_RANGE = (2.0 ** -6, 2.0 ** 6)     # the temperatures loans_softmax_distill_fwd_f32 takes


def check_distill_arguments(args):
    """ValueError for a distillation option without --teacher, for a weight or a temperature outside the loss's limits, and for
    --loss bce with a teacher (not built)"""
    if args.teacher is None:
        given = [name for name in Arguments._DISTILL[1:] if name in vars(args)]
        if given:
            raise ValueError('--%s belongs to --teacher: give the snapshot to distil from' % given[0].replace('_', '-'))
        return
    if args.loss == 'bce':
        raise ValueError('--teacher with --loss bce is not built: distillation mixes the softmax cross-entropy with the KL term')
    if args.teacher_arch not in ('resnet18', 'resnet50'):
        raise ValueError('--teacher-arch is resnet18 or resnet50, got %r' % (args.teacher_arch,))
    if args.teacher_dtype not in (None, 'fp32', 'f32', 'bf16'):
        raise ValueError('--teacher-dtype is fp32 or bf16, got %r' % (args.teacher_dtype,))
    a = args.distill_alpha
    if a is not None and not 0.0 < a <= 1.0:
        raise ValueError('--distill-alpha is the weight of the distillation term: it must lie in (0, 1] (0 is a run without '
                         '--teacher), got %r' % a)
    t = args.distill_temperature
    if not DISTILL_T_RANGE[0] <= t <= DISTILL_T_RANGE[1]:
        raise ValueError('--distill-temperature must lie in [2^-6, 2^6], got %r' % t)


def distill_options(args):
    """(alpha, temperature, the teacher's dtype as --dtype spells it) of a run with --teacher, the defaults resolved"""
    dtype = args.dtype if args.teacher_dtype is None else {'fp32': 'f32'}.get(args.teacher_dtype, args.teacher_dtype)
    return (0.5 if args.distill_alpha is None else float(args.distill_alpha)), float(args.distill_temperature), dtype


def build_teacher(args):
    """the frozen teacher of --teacher: the localizer of --teacher-arch in its ``train_imagenet`` form with the snapshot's values,
    loaded strictly (every parameter and BN statistic of the architecture must be in the file); host side only"""
    localizer_class = loans_amd.SheepLocalizer if args.teacher_arch == 'resnet18' else loans_amd.Resnet50SheepLocalizer
    state = np.random.get_state()           # the initialisers' draws are overwritten: the student's --seed stream stays as it was
    try:
        teacher = localizer_class((75, 75), train_imagenet=True)
        loans_amd.Classifier(teacher).materialize()
    finally:
        np.random.set_state(state)
    try:
        loans_amd.load_npz(args.teacher, teacher, strict=True)
    except (KeyError, AssertionError) as e:
        raise ValueError('--teacher %s is no snapshot of a %s localizer: %r' % (args.teacher, args.teacher_arch, e))
    return teacher


AVERAGE_RESUME = {False: '--resume: the checkpoint was written without --ema-decay and holds no weight average: resume it without the option',
                  True: '--resume: the checkpoint was written with --ema-decay %g and holds a weight average: resume it with the option'}


def check_average_resume(args):
    """ValueError, a sentence, where a run with a weight average is to continue a checkpoint without one, or the reverse"""
    saved = float(checkpoint.read_meta(checkpoint.resolve(args.resume, log=lambda line: None))['args'].get('ema_decay', 0.0))
    if (saved > 0) != (args.ema_decay > 0):
        raise ValueError(AVERAGE_RESUME[True] % saved if saved > 0 else AVERAGE_RESUME[False])


# what a checkpoint written before an option existed is taken to have run with: the option's default
RESUME_DEFAULTS = {name: getattr(Arguments, name) for name in Arguments._MIX}
# ... and the same for the weight average, the cosine rate and --no-decay-1d (a table of its own: RESUME_DEFAULTS is the mix options')
RESUME_DEFAULTS_AVERAGE = {name: getattr(Arguments, name) for name in Arguments._AVERAGE}
ALL_RESUME_DEFAULTS = dict(RESUME_DEFAULTS, **RESUME_DEFAULTS_AVERAGE)
# ... and for --lars-eta / --lars-eps
RESUME_DEFAULTS_LARS = {name: getattr(Arguments, name) for name in Arguments._LARS}
RESUME_DEFAULTS_WITH_LARS = dict(ALL_RESUME_DEFAULTS, **RESUME_DEFAULTS_LARS)
# ... and for the photometric options
RESUME_DEFAULTS_PHOTO = {name: getattr(Arguments, name) for name in Arguments._PHOTO}
RESUME_DEFAULTS_WITH_PHOTO = dict(RESUME_DEFAULTS_WITH_LARS, **RESUME_DEFAULTS_PHOTO)
# ... and for --lamb-beta1 / --lamb-beta2 / --lamb-eps
RESUME_DEFAULTS_LAMB = {name: getattr(Arguments, name) for name in Arguments._LAMB}
RESUME_DEFAULTS_WITH_LAMB = dict(RESUME_DEFAULTS_WITH_PHOTO, **RESUME_DEFAULTS_LAMB)
# ... and for --clip-grad-norm
RESUME_DEFAULTS_CLIP = {name: getattr(Arguments, name) for name in Arguments._CLIP}
RESUME_DEFAULTS_WITH_CLIP = dict(RESUME_DEFAULTS_WITH_LAMB, **RESUME_DEFAULTS_CLIP)
# ... and for --loss / --bce-target-thresh / --bce-sum
RESUME_DEFAULTS_LOSS = {name: getattr(Arguments, name) for name in Arguments._LOSS}
RESUME_DEFAULTS_WITH_LOSS = dict(RESUME_DEFAULTS_WITH_CLIP, **RESUME_DEFAULTS_LOSS)
# ... and for --rand-augment / --trivial-augment / --ra-fill / --ra-seed
RESUME_DEFAULTS_RA = {name: getattr(Arguments, name) for name in Arguments._RA}
RESUME_DEFAULTS_WITH_RA = dict(RESUME_DEFAULTS_WITH_LOSS, **RESUME_DEFAULTS_RA)
# ... and for --drop-path / --drop-path-seed
RESUME_DEFAULTS_DROP = {name: getattr(Arguments, name) for name in Arguments._DROP}
RESUME_DEFAULTS_WITH_DROP = dict(RESUME_DEFAULTS_WITH_RA, **RESUME_DEFAULTS_DROP)
# ... and for --accum-steps (a checkpoint from before the option ran at 1); this is the table --resume uses
RESUME_DEFAULTS_ACCUM = {name: getattr(Arguments, name) for name in Arguments._ACCUM}
RESUME_DEFAULTS_WITH_ACCUM = dict(RESUME_DEFAULTS_WITH_DROP, **RESUME_DEFAULTS_ACCUM)


def cache_budgets(total_bytes, n_train, n_validation):
    """(training, validation) bytes of the frame caches: the budget split in proportion to the sets' numbers of examples --
    frames of one collection are of one size on average, so each set gets the same fraction of itself cached"""
    train = int(total_bytes) * n_train // max(n_train + n_validation, 1)
    return train, int(total_bytes) - train


def scheduled_lr(base, epoch, drop_epochs, factor):
    """the stepped rate of ``epoch``: ``base`` times ``factor`` once per listed epoch that has begun -- a pure function, so a
    resumed run and a fresh one agree"""
    return base * factor ** sum(1 for e in set(drop_epochs) if e <= epoch)


def cosine_lr(base, epoch_detail, num_epoch, warmup_epochs, lr_min):
    """the cosine rate at ``epoch_detail`` (epochs done, fractional): ``base`` until the warm-up ends, then half a cosine down to
    ``lr_min`` at ``num_epoch`` and ``lr_min`` from there on -- a pure function, like ``scheduled_lr``, whose place it takes;
    ``warmup_factor`` multiplies it the same way"""
    span = num_epoch - warmup_epochs
    progress = min(max((epoch_detail - warmup_epochs) / span, 0.0), 1.0) if span > 0 else 1.0
    return lr_min + (base - lr_min) * (1.0 + math.cos(math.pi * progress)) / 2.0


def warmup_factor(epoch_detail, warmup_epochs, start_factor):
    """the factor of the gradual warm-up at ``epoch_detail`` (epochs done, fractional): linear from ``start_factor`` at 0 to 1 at
    ``warmup_epochs``, 1 from there on and without a warm-up -- a pure function, like ``scheduled_lr``, which it multiplies"""
    if warmup_epochs <= 0 or epoch_detail >= warmup_epochs:
        return 1.0
    return start_factor + (1.0 - start_factor) * max(epoch_detail, 0.0) / warmup_epochs


def resolved_topk(args):
    """k of the reported top-k accuracy, or None: ``--topk`` where given (0: off), else 5 with SGD, LARS and LAMB and off with Adam"""
    if args.topk is None:
        return 5 if args.optimizer in ('sgd', 'lars', 'lamb') else None
    return args.topk if args.topk > 0 else None


def loss_options(args):
    """the ``Classifier`` arguments of ``--loss``; none for the softmax loss, which is built as it always was"""
    if args.loss != 'bce':
        return {}
    return dict(loss='bce', bce_target_threshold=args.bce_target_thresh, bce_sum=bool(args.bce_sum))


def build_model(args):
    """the localizer in its ``train_imagenet`` form under a ``Classifier``; host side only"""
    if args.seed is not None:
        np.random.seed(args.seed)
    localizer_class = loans_amd.SheepLocalizer if args.use_resnet_18 else loans_amd.Resnet50SheepLocalizer
    distill = {}
    if args.teacher is not None:
        alpha, temperature, teacher_dtype = distill_options(args)
        teacher = build_teacher(args)
        teacher.set_precision(*(('bf16', 'bf16') if teacher_dtype == 'bf16' else ('f32', 'f32')))
        distill = dict(teacher=teacher, distill_alpha=alpha, distill_temperature=temperature)
    model = loans_amd.Classifier(localizer_class((75, 75), train_imagenet=True), label_smoothing=args.label_smoothing,
                                 topk=resolved_topk(args), **loss_options(args), **distill)
    model.materialize()         # the ResNet-18 variant's lazily sized fc
    return model


def build_datasets(args):
    """(train, validation or None)"""
    from loans_amd.common.datasets.image_dataset import LabeledImageDataset

    def labelled(path):
        return LabeledImageDataset(path, os.path.dirname(path), dtype=np.float32, label_dtype=np.int32,
                                   image_size=tuple(args.image_size), return_dummy_scores=False)

    if args.train_file == SYNTHETIC:
        train = SyntheticClasses(args.dataset_size, args.synthetic_classes, args.image_size, seed=args.data_seed, split=0)
    else:
        train = labelled(args.train_file)
    validation = None
    if args.validation:
        if args.val_file == SYNTHETIC:
            validation = SyntheticClasses(args.validation_size, args.synthetic_classes, args.image_size, seed=args.data_seed, split=1)
        else:
            validation = labelled(args.val_file)
    return train, validation


def build_crop_datasets(args, device, rank=0):
    """(train, validation or None) of ``--augment rrc``: datasets that finish their batches on ``device``.  Rank r of a data
    parallel run draws its crops from the stream of ``--augment-seed`` + 7919 r."""
    from loans_amd.common.datasets.classification_dataset import ClassificationImageDataset, ResidentClassificationSource
    crops = dict(image_size=tuple(args.image_size), scale=tuple(args.rrc_scale), ratio=tuple(args.rrc_ratio),
                 crop_pct=args.val_crop_pct,
                 augment_seed=None if args.augment_seed is None else args.augment_seed + 7919 * rank)

    def dataset(path, n, split, train):
        if path == SYNTHETIC:
            x, t = synthetic.make_classification_set(args.data_seed, n, args.synthetic_classes, args.image_size[0], args.image_size[1], split=split)
            return ResidentClassificationSource.from_float_chw(x, t, device, train=train, **crops)
        return ClassificationImageDataset(path, os.path.dirname(path), train=train, **crops)

    train = dataset(args.train_file, args.dataset_size, 0, True)
    validation = dataset(args.val_file, args.validation_size, 1, False) if args.validation else None
    if getattr(args, 'frame_cache_gb', 0) > 0:
        # per rank: every rank keeps its own share of the sets (ShardedDataset hands it every N-th example)
        from loans_amd.common.datasets.frame_cache import RaggedFrameCache
        cached_validation = validation is not None and args.val_file != SYNTHETIC
        budgets = cache_budgets(args.frame_cache_gb * 1e9, len(train), len(validation) if cached_validation else 0)
        train.cache = RaggedFrameCache(budgets[0], args.frame_cache_where, device)
        if cached_validation:
            validation.cache = RaggedFrameCache(budgets[1], args.frame_cache_where, device)
    return train, validation


def converter(batch, device=None):
    """(frames (B,3,H,W) float32, labels (B,) int32) on the device; a label read from a file is a one-element row"""
    images, labels = training.concat_examples(batch, device)[:2]
    return images, labels.reshape(-1).to(torch.int32)


def run(args, log=print):
    """The training loop.  Returns (log entries, model)."""
    comm = parallel.init_from_env()
    if comm.size > 1:
        args.gpu = int(os.environ.get('LOCAL_RANK', '0')) % torch.cuda.device_count()
    elif args.gpu < 0:
        args.gpu = torch.cuda.current_device()
    torch.cuda.set_device(args.gpu)
    for name in Arguments._PIPELINE + Arguments._PARALLEL + Arguments._CACHE + Arguments._MIX:      # the values this run uses, logged with the other arguments
        setattr(args, name, getattr(args, name, getattr(Arguments, name)))
    # the _AVERAGE options are logged where one of them is given: a run without them logs what it always logged
    averaging = any(getattr(args, name) != getattr(Arguments, name) for name in Arguments._AVERAGE)
    # ... and so are the _PHOTO options
    photo_given = any((tuple(v) if isinstance(v, (list, tuple)) else v) != getattr(Arguments, name)
                      for name, v in ((name, getattr(args, name)) for name in Arguments._PHOTO))
    # ... and the _RA options
    ra_given = any((tuple(v) if isinstance(v, (list, tuple)) else v) != getattr(Arguments, name)
                   for name, v in ((name, getattr(args, name)) for name in Arguments._RA))
    # ... and the _DROP options
    drop_given = any(getattr(args, name) != getattr(Arguments, name) for name in Arguments._DROP)
    args.gpus = comm.size
    check_cache_arguments(args)
    check_mix_arguments(args)
    check_photo_arguments(args)
    check_ra_arguments(args)
    check_average_arguments(args)
    check_lars_arguments(args)
    check_lamb_arguments(args)
    check_clip_arguments(args)
    check_loss_arguments(args)
    check_drop_arguments(args)
    check_accum_arguments(args)
    check_distill_arguments(args)
    if args.teacher is not None:                # the values this run distils with, logged in the first entry
        args.distill_alpha, args.distill_temperature, args.teacher_dtype = distill_options(args)
        args.teacher_arch = args.teacher_arch
    chief = comm.rank == 0                     # prints, logs and writes snapshots

    # --augment rrc: the iterators hand out (frames, labels) already resident on the device
    feed, batch_converter = {}, converter
    if args.augment == 'rrc':
        train_dataset, validation_dataset = build_crop_datasets(args, torch.device('cuda', args.gpu), comm.rank)
        feed, batch_converter = {'device': args.gpu}, training.identity_converter
    else:
        train_dataset, validation_dataset = build_datasets(args)
    # the frame caches' work is counted where a batch is consumed (the lookups run batches ahead): [hits, misses] since the last
    # log entry, of the training and of the validation set
    caches = {'feed/cache_': [getattr(train_dataset, 'cache', None), 0, 0],
              'feed/val_cache_': [getattr(validation_dataset, 'cache', None), 0, 0]}
    caches = {k: v for k, v in caches.items() if v[0] is not None}

    def counting(prefix):
        if prefix not in caches:
            return batch_converter
        tally = caches[prefix]

        def convert(batch, device=None):
            tally[1] += getattr(batch, 'cache_hits', 0)
            tally[2] += getattr(batch, 'cache_misses', 0)
            return batch_converter(batch, device)
        return convert

    train_converter, validation_converter = counting('feed/cache_'), counting('feed/val_cache_')
    # every rank built the same sets and takes every comm.size-th example: the training share padded by wrapping (all ranks make
    # the same iterations and epochs), the validation share not (every example is counted once; shares may differ by one)
    train_dataset = ShardedDataset(train_dataset, comm.rank, comm.size, pad=True)
    if ra_enabled(args):
        # between the crop and the photometric stage, with draws of its own: the stream of --ra-seed + 7919 r
        from loans_amd.common.datasets.rand_augment import RandAugmentBatches, RandAugmentPolicy
        ra_seed = None if args.ra_seed is None else args.ra_seed + 7919 * comm.rank
        if args.trivial_augment:
            ra_policy = RandAugmentPolicy('trivial', fill=tuple(args.ra_fill), seed=ra_seed)
        else:
            ra_policy = RandAugmentPolicy('rand', int(args.rand_augment[0]), int(args.rand_augment[1]), tuple(args.ra_fill), ra_seed)
        train_dataset = RandAugmentBatches(train_dataset, ra_policy, tuple(args.image_size))
    if photo_enabled(args):
        # between the crop and the mix, with draws of its own: the stream of --photo-seed + 7919 r
        from loans_amd.common.datasets.photometric import PhotometricBatches, PhotoPolicy
        jitter = tuple(args.color_jitter)
        photo_policy = PhotoPolicy(jitter[0], jitter[1], jitter[2], args.lighting_std, args.random_erase_prob,
                                   tuple(args.random_erase_scale), tuple(args.random_erase_ratio), tuple(args.random_erase_value),
                                   None if args.photo_seed is None else args.photo_seed + 7919 * comm.rank)
        train_dataset = PhotometricBatches(train_dataset, photo_policy, tuple(args.image_size))
    if args.mixup_alpha > 0 or args.cutmix_alpha > 0:
        # every rank mixes inside its own batch, with draws of its own: the stream of --mix-seed + 7919 r, as for the crops
        from loans_amd.common.datasets.batch_mix import MixedBatches, MixPolicy
        policy = MixPolicy(args.mixup_alpha, args.cutmix_alpha, args.mix_prob, args.mix_switch_prob,
                           None if args.mix_seed is None else args.mix_seed + 7919 * comm.rank)
        train_dataset = MixedBatches(train_dataset, policy, tuple(args.image_size))
    if validation_dataset is not None:
        validation_dataset = ShardedDataset(validation_dataset, comm.rank, comm.size, pad=False)
    train_iter = training.MultithreadIterator(train_dataset, args.batch_size, shuffle=not args.no_shuffle, n_threads=args.loader_threads, **feed)

    model = build_model(args)
    localizer = model.predictor
    if args.dtype == 'bf16':
        model.set_precision('bf16', 'bf16')
    model.to_gpu(args.gpu)
    comm.bcast_data(model)
    drop = None
    if args.drop_path > 0:
        # every rank drops samples of its own batch, with draws of its own: the stream of --drop-path-seed + 7919 r
        drop = localizer.set_drop_path(args.drop_path, None if args.drop_path_seed is None else args.drop_path_seed + 7919 * comm.rank)

    if args.optimizer == 'lars':
        optimizer, rate_name = loans_amd.LARS(lr=args.learning_rate, momentum=args.momentum, weight_decay_rate=args.weight_decay,
                                              eta=args.lars_eta, eps=args.lars_eps, decay_exempt_1d=bool(args.no_decay_1d)), 'lr'
    elif args.optimizer == 'lamb':
        optimizer, rate_name = loans_amd.LAMB(lr=args.learning_rate, beta1=args.lamb_beta1, beta2=args.lamb_beta2, eps=args.lamb_eps,
                                              weight_decay_rate=args.weight_decay, decay_exempt_1d=bool(args.no_decay_1d)), 'lr'
    elif args.optimizer == 'sgd':
        exempt = {'decay_exempt_1d': True} if args.no_decay_1d else {}
        optimizer, rate_name = loans_amd.MomentumSGD(lr=args.learning_rate, momentum=args.momentum, weight_decay_rate=args.weight_decay, **exempt), 'lr'
    else:
        optimizer, rate_name = loans_amd.Adam(alpha=args.learning_rate, weight_decay_rate=args.weight_decay), 'alpha'
    optimizer.setup(model)
    parallel.create_multi_node_optimizer(optimizer, comm)
    clipping = None
    if args.clip_grad_norm is not None:
        # behind the communicator: the hook sees the exchanged gradient, the same on every rank
        clipping = loans_amd.GradientClipping(args.clip_grad_norm)
        optimizer.add_hook(clipping)
    topk ='accuracy_top%d' % model.topk if model.topk is not None else None
    train_keys = ('loss', 'accuracy') + ((topk,) if topk else ())
    if args.teacher is not None:
        train_keys += ('distill_loss', 'teacher_accuracy')
    # --accum-steps K: an update() draws K batches and steps once (1: the updater as it always was)
    updater = training.StandardUpdater(train_iter, optimizer, converter=train_converter, device=args.gpu, comm=comm,
                                       **({'accum_steps': args.accum_steps} if args.accum_steps > 1 else {}))
    # every rank keeps its own average: the parameters agree on all ranks (built after bcast_data), the BN statistics are local
    average = loans_amd.WeightAverage(model, args.ema_decay) if args.ema_decay > 0 else None

    evaluator = validate = None
    summed = comm.size > 1 or args.validation_sums
    if validation_dataset is not None:
        validation_iter = training.MultithreadIterator(validation_dataset, args.batch_size, repeat=False, shuffle=False,
                                                       n_threads=args.loader_threads, **feed)

        def eval_func(x, t):
            with loans_amd.using_config('train', False), loans_amd.using_config('enable_backprop', False):
                model(x, t)
            result = {'validation/loss': float(model.loss.data), 'validation/accuracy': float(model.accuracy.data)}
            if topk:
                result['validation/' + topk] = float(model.accuracy_topk.data)
            return result

        evaluator = training.Evaluator(validation_iter, model, converter=validation_converter, device=args.gpu, eval_func=eval_func)
        metrics = loans_amd.ClassificationMetrics(topk=model.topk, device=torch.device('cuda', args.gpu))

        def summed_validation():
            """loss and hits summed over every example of every share: rank 0's BN running statistics to all ranks (the ones
            its snapshot holds), one launch per batch into the five doubles, no collective inside the loop -- the shares may
            differ in length --, one all-reduce and one host synchronisation at the end"""
            comm.bcast_persistents(model)
            metrics.reset()
            validation_iter.reset()
            for batch in validation_iter:
                x, t = validation_converter(batch, args.gpu)
                model.evaluate(x, t, metrics)
            total = metrics.result(comm)
            result = {'validation/loss': total['loss'], 'validation/accuracy': total['accuracy']}
            if topk:
                result['validation/' + topk] = total[topk]
            if comm.size > 1:
                result.update({'validation/rows': total['rows'], 'validation/valid': total['valid']})
            return result

        validate = summed_validation if summed else evaluator.evaluate

    resumed = None
    if args.resume is not None:
        # the run continues in the checkpoint's log directory: no new <time>_<name>
        check_average_resume(args)
        resumed, changed = checkpoint.resolve_resume(args, RESUME_FIXED, log if chief else (lambda line: None), world=comm.size,
                                                     defaults=RESUME_DEFAULTS_WITH_ACCUM)
        args.log_dir = os.path.dirname(os.path.abspath(args.resume))
        for line in changed if chief else ():
            log(line)
    elif not args.flat_log_dir:
        stamp = datetime.datetime.now().isoformat() if comm.size == 1 else os.environ.get('TORCHELASTIC_RUN_ID', 'dp') + \
            '_' + datetime.datetime.now().strftime('%Y-%m-%dT%H')
        args.log_dir = os.path.join(args.log_dir, "{}_{}".format(stamp, args.ln))
    if chief:
        os.makedirs(args.log_dir, exist_ok=True)
    data_to_log = {'log_dir': args.log_dir, 'image_size': list(args.image_size), 'localizer': [localizer.__class__.__name__, 'localizer.py']}
    for argument in filter(lambda x: not x.startswith('_'), dir(args)):
        if argument in checkpoint.FLAGS and checkpoint.FLAGS[argument] == getattr(args, argument):
            continue        # a run without the checkpoint options logs what it always logged
        if argument in Arguments._AVERAGE and not averaging:
            continue
        if argument in Arguments._PHOTO and not photo_given:
            continue
        if argument in Arguments._RA and not ra_given:
            continue
        if argument in Arguments._DROP and not drop_given:
            continue
        if argument in Arguments._ACCUM and 'accum_steps' not in vars(args):
            continue        # logged where it is given
        if argument in Arguments._LARS and args.optimizer != 'lars':
            continue        # a run with another optimiser logs what it always logged
        if argument in Arguments._LAMB and args.optimizer != 'lamb':
            continue
        if argument in Arguments._CLIP and clipping is None:
            continue
        if argument in Arguments._LOSS and not any(name in vars(args) for name in Arguments._LOSS):
            continue        # logged where one of them is given
        if argument in Arguments._DISTILL and args.teacher is None:
            continue        # logged with a teacher only
        # (an entry's ``loss`` is the training loss: the option of that name is logged as ``loss_function``)
        data_to_log['loss_function' if argument == 'loss' else argument] = getattr(args, argument)
    log_entries = []
    state = dict(models={'model': model}, optimizers={'main': optimizer}, iterators={'main': train_iter}, comm=comm)
    if average is not None:
        state['optimizers']['ema'] = average    # the shape of an optimiser's record: class, t, hyperparam, state
    if drop is not None:
        state['iterators']['drop_path'] = drop  # the shape of an iterator's record: a rank's own draw stream

    def snapshot_path(it, tag=''):
        return os.path.join(args.log_dir, '%s_%s%d.npz' % (localizer.__class__.__name__, tag, it))

    def save_snapshots(it):
        loans_amd.save_npz(snapshot_path(it), localizer)
        if average is not None:     # the same keys, the averaged values: train_sheep_localizer.py --rl takes it as it is
            with average.applied():
                loans_amd.save_npz(snapshot_path(it, 'ema_'), localizer)

    t0 = time.time()
    it = 0
    if resumed is not None:
        # before the first step: model, optimiser, iterator and streams as they stood after iteration `resumed['iteration']`
        checkpoint.load_checkpoint(args.resume, **state)
        optimizer.hyperparam.weight_decay_rate = args.weight_decay      # the rates are the new command line's (--lr: set per step below)
        if args.optimizer == 'sgd':
            optimizer.hyperparam.decay_exempt_1d = bool(args.no_decay_1d)
        if args.optimizer == 'sgd':
            optimizer.hyperparam.momentum = args.momentum
        if args.optimizer == 'lars':
            optimizer.hyperparam.decay_exempt_1d, optimizer.hyperparam.momentum = bool(args.no_decay_1d), args.momentum
            optimizer.hyperparam.eta, optimizer.hyperparam.eps = args.lars_eta, args.lars_eps
        if args.optimizer == 'lamb':
            optimizer.hyperparam.decay_exempt_1d = bool(args.no_decay_1d)
            optimizer.hyperparam.beta1, optimizer.hyperparam.beta2, optimizer.hyperparam.eps = args.lamb_beta1, args.lamb_beta2, args.lamb_eps
        it = updater.iteration = int(resumed['iteration'])
        t0 -= float(resumed['elapsed_time'])
        log_entries = checkpoint.read_log(args.log_dir, it)
        if chief:
            log('resumed %s: iteration %d, epoch %d' % (args.resume, it, updater.epoch))
    while updater.epoch < args.num_epoch and (args.iterations is None or it < args.iterations):
        if args.lr_schedule == 'cosine':
            lr = cosine_lr(args.learning_rate, updater.epoch_detail, args.num_epoch, args.warmup_epochs, args.lr_min)
        else:
            lr = scheduled_lr(args.learning_rate, updater.epoch, args.lr_drop_epochs, args.lr_drop_factor)
        lr *= warmup_factor(updater.epoch_detail, args.warmup_epochs, args.warmup_start_factor)
        setattr(optimizer, rate_name, lr)
        updater.update()
        if average is not None:
            average.update()
        it = updater.iteration
        last = (args.iterations is not None and it == args.iterations) or updater.epoch >= args.num_epoch
        # LOCK STEP.  Everything below that holds a collective -- the mean of the training metrics, the validation pass -- and the
        # end of this loop depend on `iteration`, `epoch`, `is_new_epoch` and the arguments alone, and those are the same on
        # every rank: the padded training shares have one length, so every iterator makes the same (epoch, is_new_epoch)
        # sequence.  A condition that read anything a rank computed for itself (a loss, a clock) would leave a peer waiting.
        if updater.is_new_epoch or it % args.log_interval == 0 or last:
            # the only host synchronisation of an iteration
            obs = loans_amd.reporter.observation
            entry = {'iteration': it, 'epoch': updater.epoch}
            if comm.active:                     # equal batches per rank: the mean over ranks is the mean of the global batch
                mean = torch.stack([getattr(obs[k], 'data', obs[k]).detach().reshape(()).to(torch.float64) for k in train_keys])
                mean = (comm.allreduce_sum(mean) / comm.size).tolist()
                entry.update(dict(zip(train_keys, mean)))
            else:
                entry.update({k: float(obs[k]) for k in train_keys})
            entry['lr'] = lr                    # the rate this iteration was stepped with
            if clipping is not None:
                # the norm before clipping of this iteration's step, from the device record: local to the rank -- every rank
                # holds the same exchanged gradient --, so no collective and LOCK STEP holds
                entry['grad_norm'] = clipping.last_norm()
            if validate is not None:
                keep = {k: obs[k] for k in train_keys}
                entry.update({k: v for k, v in validate().items() if k.startswith('validation/')})
                if average is not None:
                    # the second pass: the same set through the averaged model (LOCK STEP: `average` depends on the arguments alone)
                    with average.applied():
                        entry.update({'validation/ema/' + k[len('validation/'):]: v for k, v in validate().items()
                                      if k in ('validation/loss', 'validation/accuracy', 'validation/' + str(topk))})
                loans_amd.report(keep)
            for prefix, tally in caches.items():
                entry.update({prefix + 'frames': len(tally[0]), prefix + 'bytes': tally[0].bytes,
                              prefix + 'hits': tally[1], prefix + 'misses': tally[2]})
                tally[1] = tally[2] = 0
            entry['elapsed_time'] = time.time() - t0
            top = '  top-%d %%.4f' % model.topk if topk else ''
            val = ''
            if 'validation/loss' in entry:
                val = '  validation loss %.5f accuracy %.4f' % (entry['validation/loss'], entry['validation/accuracy'])
                if topk:
                    val += top % entry['validation/' + topk]
            if 'validation/ema/loss' in entry:
                val += '  ema loss %.5f accuracy %.4f' % (entry['validation/ema/loss'], entry['validation/ema/accuracy'])
                if topk:
                    val += top % entry['validation/ema/' + topk]
            if chief:
                log('iteration %4d  epoch %d  lr %g  loss %.5f  accuracy %.4f%s%s  (%.1f s)' % (
                    it, updater.epoch, lr, entry['loss'], entry['accuracy'], top % entry[topk] if topk else '', val, entry['elapsed_time']))
            if not log_entries:
                entry.update(data_to_log)
            log_entries.append(entry)
            if chief:
                with open(os.path.join(args.log_dir, 'log'), 'w') as f:
                    json.dump(log_entries, f, indent=4, default=str)
        if chief and it % args.snapshot_interval == 0:
            save_snapshots(it)
        if checkpoint.due(it, args.checkpoint_interval, last):      # of `it` and the arguments alone: LOCK STEP holds (a barrier inside)
            checkpoint.save_checkpoint(args.log_dir, it, keep=args.checkpoint_keep, meta={
                'epoch': updater.epoch, 'elapsed_time': time.time() - t0, 'args': checkpoint.plain_arguments(args)}, **state)
    train_iter.finalize()
    if evaluator is not None:
        validation_iter.finalize()
    if chief:
        if not os.path.exists(snapshot_path(updater.iteration)):
            save_snapshots(updater.iteration)
        log('snapshot: %s' % snapshot_path(updater.iteration))
    return log_entries, model


def main(argv=None):
    run(parse_args(argv))
    parallel.shutdown()


if __name__ == "__main__":
    main()
