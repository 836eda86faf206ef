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

Not built (follow-ups): ``--gpus N``, ``--use-graph`` and cropping out of the decode-once frame cache.
"""
import argparse
import datetime
import json
import os
import time

import numpy as np
import torch

import loans_amd
from loans_amd.datasets import synthetic
from loans_amd.runtime import training

SYNTHETIC = 'synthetic'


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

    _PIPELINE = ('augment', 'rrc_scale', 'rrc_ratio', 'val_crop_pct', 'augment_seed')


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description="ImageNet pre-training of a localizer backbone (MI355X-native)")
    parser.add_argument("train_file", nargs='?', default=SYNTHETIC, help="tab-separated `path<TAB>class` lines ('synthetic': seeded textures)")
    parser.add_argument("val_file", nargs='?', default=SYNTHETIC, help="validation file in the same format")
    parser.add_argument("--use-resnet-18", action='store_true', default=False, help="SheepLocalizer (ResNet-18 variant) instead of the ResNet-50 one")
    parser.add_argument("-b", "--batch-size", type=int, default=32, help="batch size")
    parser.add_argument("-g", "--gpu", type=int, default=-1, help="gpu id to use (-1: the current device)")
    parser.add_argument("--lr", "--learning-rate", dest="learning_rate", type=float, default=0.001, help="Adam's alpha / momentum SGD's lr")
    parser.add_argument("--weight-decay", type=float, default=0.0, help="weight_decay_rate of the optimiser")
    parser.add_argument("--optimizer", default='adam', choices=['adam', 'sgd'], help="Adam, or SGD with momentum")
    parser.add_argument("--momentum", type=float, default=0.9, help="momentum of --optimizer sgd")
    parser.add_argument("--lr-drop-epochs", type=int, nargs='+', default=(), help="epochs at whose first iteration the rate is multiplied by --lr-drop-factor")
    parser.add_argument("--lr-drop-factor", type=float, default=0.1, help="factor of each learning rate step")
    parser.add_argument("--label-smoothing", type=float, default=0.0, help="label smoothing of the training loss (uniform over all classes)")
    parser.add_argument("--topk", type=int, default=None, help="also report top-k accuracy (default: 5 with --optimizer sgd, off with adam; 0: off)")
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
    return parser.parse_args(argv, namespace=Arguments())


def scheduled_lr(base, epoch, drop_epochs, factor):
    """the stepped rate of ``epoch``: ``base`` times ``factor`` once per listed epoch that has begun -- a pure function, so a
    resumed run and a fresh one agree"""
    return base * factor ** sum(1 for e in set(drop_epochs) if e <= epoch)


def resolved_topk(args):
    """k of the reported top-k accuracy, or None: ``--topk`` where given (0: off), else 5 with SGD and off with Adam"""
    if args.topk is None:
        return 5 if args.optimizer == 'sgd' else None
    return args.topk if args.topk > 0 else None


def build_model(args):
    """the localizer in its ``train_imagenet`` form under a ``Classifier``; host side only"""
    if args.seed is not None:
        np.random.seed(args.seed)
    localizer_class = loans_amd.SheepLocalizer if args.use_resnet_18 else loans_amd.Resnet50SheepLocalizer
    model = loans_amd.Classifier(localizer_class((75, 75), train_imagenet=True), label_smoothing=args.label_smoothing,
                                 topk=resolved_topk(args))
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


def build_crop_datasets(args, device):
    """(train, validation or None) of ``--augment rrc``: datasets that finish their batches on ``device``"""
    from loans_amd.common.datasets.classification_dataset import ClassificationImageDataset, ResidentClassificationSource
    crops = dict(image_size=tuple(args.image_size), scale=tuple(args.rrc_scale), ratio=tuple(args.rrc_ratio),
                 crop_pct=args.val_crop_pct, augment_seed=args.augment_seed)

    def dataset(path, n, split, train):
        if path == SYNTHETIC:
            x, t = synthetic.make_classification_set(args.data_seed, n, args.synthetic_classes, args.image_size[0], args.image_size[1], split=split)
            return ResidentClassificationSource.from_float_chw(x, t, device, train=train, **crops)
        return ClassificationImageDataset(path, os.path.dirname(path), train=train, **crops)

    train = dataset(args.train_file, args.dataset_size, 0, True)
    return train, (dataset(args.val_file, args.validation_size, 1, False) if args.validation else None)


def converter(batch, device=None):
    """(frames (B,3,H,W) float32, labels (B,) int32) on the device; a label read from a file is a one-element row"""
    images, labels = training.concat_examples(batch, device)[:2]
    return images, labels.reshape(-1).to(torch.int32)


def run(args, log=print):
    """The training loop.  Returns (log entries, model)."""
    if args.gpu < 0:
        args.gpu = torch.cuda.current_device()
    torch.cuda.set_device(args.gpu)
    for name in Arguments._PIPELINE:             # the values this run uses, logged with the other arguments
        setattr(args, name, getattr(args, name, getattr(Arguments, name)))

    # --augment rrc: the iterators hand out (frames, labels) already resident on the device
    feed, batch_converter = {}, converter
    if args.augment == 'rrc':
        train_dataset, validation_dataset = build_crop_datasets(args, torch.device('cuda', args.gpu))
        feed, batch_converter = {'device': args.gpu}, training.identity_converter
    else:
        train_dataset, validation_dataset = build_datasets(args)
    train_iter = training.MultithreadIterator(train_dataset, args.batch_size, shuffle=not args.no_shuffle, n_threads=args.loader_threads, **feed)

    model = build_model(args)
    localizer = model.predictor
    if args.dtype == 'bf16':
        model.set_precision('bf16', 'bf16')
    model.to_gpu(args.gpu)

    if args.optimizer == 'sgd':
        optimizer, rate_name = loans_amd.MomentumSGD(lr=args.learning_rate, momentum=args.momentum, weight_decay_rate=args.weight_decay), 'lr'
    else:
        optimizer, rate_name = loans_amd.Adam(alpha=args.learning_rate, weight_decay_rate=args.weight_decay), 'alpha'
    optimizer.setup(model)
    topk = 'accuracy_top%d' % model.topk if model.topk is not None else None
    train_keys = ('loss', 'accuracy') + ((topk,) if topk else ())
    updater = training.StandardUpdater(train_iter, optimizer, converter=batch_converter, device=args.gpu)

    evaluator = None
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

        evaluator = training.Evaluator(validation_iter, model, converter=batch_converter, device=args.gpu, eval_func=eval_func)

    if not args.flat_log_dir:
        args.log_dir = os.path.join(args.log_dir, "{}_{}".format(datetime.datetime.now().isoformat(), args.ln))
    os.makedirs(args.log_dir, exist_ok=True)
    data_to_log = {'log_dir': args.log_dir, 'image_size': list(args.image_size), 'localizer': [localizer.__class__.__name__, 'localizer.py']}
    for argument in filter(lambda x: not x.startswith('_'), dir(args)):
        data_to_log[argument] = getattr(args, argument)
    log_entries = []

    def snapshot_path(it):
        return os.path.join(args.log_dir, '%s_%d.npz' % (localizer.__class__.__name__, it))

    t0 = time.time()
    it = 0
    while updater.epoch < args.num_epoch and (args.iterations is None or it < args.iterations):
        lr = scheduled_lr(args.learning_rate, updater.epoch, args.lr_drop_epochs, args.lr_drop_factor)
        setattr(optimizer, rate_name, lr)
        updater.update()
        it = updater.iteration
        last = (args.iterations is not None and it == args.iterations) or updater.epoch >= args.num_epoch
        if updater.is_new_epoch or it % args.log_interval == 0 or last:
            # the only host synchronisation of an iteration
            obs = loans_amd.reporter.observation
            entry = {'iteration': it, 'epoch': updater.epoch}
            entry.update({k: float(obs[k]) for k in train_keys})
            entry['lr'] = lr                    # the rate this iteration was stepped with
            if evaluator is not None:
                keep = {k: obs[k] for k in train_keys}
                entry.update({k: v for k, v in evaluator.evaluate().items() if k.startswith('validation/')})
                loans_amd.report(keep)
            entry['elapsed_time'] = time.time() - t0
            top = '  top-%d %%.4f' % model.topk if topk else ''
            val = ''
            if 'validation/loss' in entry:
                val = '  validation loss %.5f accuracy %.4f' % (entry['validation/loss'], entry['validation/accuracy'])
                if topk:
                    val += top % entry['validation/' + topk]
            log('iteration %4d  epoch %d  lr %g  loss %.5f  accuracy %.4f%s%s  (%.1f s)' % (
                it, updater.epoch, lr, entry['loss'], entry['accuracy'], top % entry[topk] if topk else '', val, entry['elapsed_time']))
            if not log_entries:
                entry.update(data_to_log)
            log_entries.append(entry)
            with open(os.path.join(args.log_dir, 'log'), 'w') as f:
                json.dump(log_entries, f, indent=4, default=str)
        if it % args.snapshot_interval == 0:
            loans_amd.save_npz(snapshot_path(it), localizer)
    train_iter.finalize()
    if evaluator is not None:
        validation_iter.finalize()
    if not os.path.exists(snapshot_path(updater.iteration)):
        loans_amd.save_npz(snapshot_path(updater.iteration), localizer)
    log('snapshot: %s' % snapshot_path(updater.iteration))
    return log_entries, model


def main(argv=None):
    run(parse_args(argv))


if __name__ == "__main__":
    main()
