"""``Classifier(predictor)`` in the manner of ``chainer.links.Classifier``: ``__call__(x, t)`` runs the predictor, computes
``softmax_cross_entropy`` and ``accuracy`` from one pass over the logits, reports both under ``loss`` / ``accuracy`` and returns
the loss.  The ImageNet pre-training arm of the reference (train_imagenet=True localizers) is trained through it.
``label_smoothing`` smooths the training loss (``config.train``; the validation loss stays the plain one, comparable between
runs), ``topk=k`` also reports ``accuracy_top<k>``; with neither, the loss function and the reported keys are the plain ones.
``loss='bce'`` trains (``config.train``) with the per-class sigmoid binary cross-entropy on the same smoothed / mixed target,
under the same keys; its validation loss is the plain softmax cross-entropy too, by the same rule.
``teacher=`` (with ``distill_alpha > 0``) trains (``config.train``) against the logits of a frozen second predictor as well:
``loss = (1 - alpha) CE + alpha T^2 KL(softmax(teacher / T) || softmax(student / T))``, reported with ``distill_loss`` (the
``T^2 KL`` term) and ``teacher_accuracy``.  The teacher is NOT a child link: its parameters live in an arena of its own and join
neither the optimiser, the data-parallel exchange, EMA, snapshots nor checkpoints; it runs in test mode without backprop, which
leaves its parameters and BN statistics bit for bit.  In test mode and in ``evaluate`` the teacher does not run."""
import math

import torch

from . import ops
from .functions.ops_small import (DISTILL_T_MAX, DISTILL_T_MIN, _as_labels, sigmoid_binary_cross_entropy,
                                  softmax_cross_entropy_distilled, softmax_cross_entropy_mixed,
                                  softmax_cross_entropy_with_accuracy, softmax_cross_entropy_with_topk_accuracy)
from .mixed_labels import MixedLabels
from .runtime.core import Chain, Variable, config, report, using_config


def class_count(predictor):
    """the width of the classification head in ``predictor``'s tree (``ResNet(class_labels=K)``), or None where none is declared"""
    for link in predictor.links():
        if getattr(link, 'class_labels', None) is not None:
            return int(link.class_labels)
    return None


class Classifier(Chain):

    compute_accuracy = True

    def __init__(self, predictor, label_key=-1, label_smoothing=0.0, topk=None, loss='softmax', bce_target_threshold=None,
                 bce_sum=False, teacher=None, distill_alpha=0.0, distill_temperature=1.0):
        super().__init__()
        if label_key != -1:
            raise ValueError('the label is the last argument (label_key=-1)')
        if not 0.0 <= label_smoothing < 1.0:
            raise ValueError('label_smoothing must be in [0, 1)')
        if topk is not None and topk < 1:
            raise ValueError('topk must be at least 1')
        if loss not in ('softmax', 'bce'):
            raise ValueError('loss must be \'softmax\' or \'bce\', got %r' % (loss,))
        if bce_target_threshold is not None and not 0.0 <= bce_target_threshold < 1.0:
            raise ValueError('bce_target_threshold must be in [0, 1)')
        if loss != 'bce' and (bce_target_threshold is not None or bce_sum):
            raise ValueError('bce_target_threshold and bce_sum belong to loss=\'bce\'')
        if not (isinstance(distill_alpha, (int, float)) and 0.0 <= distill_alpha <= 1.0):          # (a NaN too)
            raise ValueError('distill_alpha must be in [0, 1]')
        if not (isinstance(distill_temperature, (int, float)) and math.isfinite(distill_temperature)
                and DISTILL_T_MIN <= distill_temperature <= DISTILL_T_MAX):
            raise ValueError('distill_temperature must be in [2^-6, 2^6]')
        if distill_alpha > 0.0 and teacher is None:
            raise ValueError('distill_alpha > 0 needs a teacher')
        if teacher is not None and loss == 'bce':
            raise ValueError('distillation under loss=\'bce\' is not built')
        if teacher is not None:
            want, have = class_count(predictor), class_count(teacher)
            if want is not None and have is not None and want != have:
                raise ValueError('the teacher has %d classes, the student %d' % (have, want))
        self.label_smoothing, self.topk = label_smoothing, topk
        self.loss_name, self.bce_target_threshold, self.bce_sum = loss, bce_target_threshold, bool(bce_sum)
        self.distill_alpha, self.distill_temperature = float(distill_alpha), float(distill_temperature)
        with self.init_scope():
            self.predictor = predictor
        # outside init_scope: no child link.  The teacher is run through a Classifier of its own, which sizes its head and gives
        # it an arena of its own exactly as this one does for the student.
        self.teacher = teacher
        self._teacher_model = Classifier(teacher) if teacher is not None else None
        self.distill_loss = self.teacher_accuracy = None
        self.y = self.loss = self.accuracy = self.accuracy_topk = None

    def materialize(self):
        """size every lazily sized head of the predictor's tree (``ResNet(class_labels=K).fc``): a parameter can only join the
        arena before it is finalised.  Host side only."""
        for link in self.predictor.links():
            if hasattr(link, 'materialize_head'):
                link.materialize_head()

    def _predict(self, *xs):
        if self._arena is None:
            self.materialize()
        first = xs[0].data if isinstance(xs[0], Variable) else xs[0]
        device = first.device if torch.is_tensor(first) and first.is_cuda else torch.device('cuda', torch.cuda.current_device())
        arena = self.finalize(device)
        for link in self.predictor.links():         # a predictor that finalises itself (the localizers do) finds this arena
            link.__dict__['_arena'] = arena
        self.y = self.predictor(*xs)
        return self.y

    def evaluate(self, x, t, metrics):
        """A test-mode forward without backprop whose logits go into ``metrics`` (``ClassificationMetrics.add``: one launch, no
        host synchronisation).  No loss function runs, no gradient is written, nothing is reported."""
        with using_config('train', False), using_config('enable_backprop', False):
            self._predict(x)
        metrics.add(self.y, t)

    def teacher_logits(self, *xs):
        """the teacher's logits on the same inputs and stream: a test-mode forward without backprop (no graph, no gradient, the
        BN statistics read and not written)"""
        with using_config('train', False), using_config('enable_backprop', False):
            zt = self._teacher_model._predict(*xs)
        return zt.data if isinstance(zt, Variable) else zt

    def __call__(self, *args):
        *xs, t = args
        if self.teacher is not None and self.distill_alpha > 0.0 and config.train:
            zt = self.teacher_logits(*xs)
            self._predict(*xs)
            if tuple(zt.shape) != tuple(self.y.shape):
                raise ValueError('the teacher gives logits of shape %s, the student %s' % (tuple(zt.shape), tuple(self.y.shape)))
            self.loss, self.accuracy, self.accuracy_topk, self.distill_loss, self.teacher_accuracy = softmax_cross_entropy_distilled(
                self.y, zt, t, self.label_smoothing, self.topk or 1, self.distill_alpha, self.distill_temperature)
            report({'loss': self.loss, 'accuracy': self.accuracy}, self)
            if self.topk is not None:
                report({'accuracy_top%d' % self.topk: self.accuracy_topk}, self)
            report({'distill_loss': self.distill_loss, 'teacher_accuracy': self.teacher_accuracy}, self)
            return self.loss
        self._predict(*xs)
        if self.loss_name == 'bce' and config.train:    # plain or mixed labels; in test mode the softmax paths below, as they are
            self.loss, self.accuracy, self.accuracy_topk = sigmoid_binary_cross_entropy(
                self.y, t, self.label_smoothing, self.topk or 1, self.bce_target_threshold, self.bce_sum)
            report({'loss': self.loss, 'accuracy': self.accuracy}, self)
            if self.topk is not None:
                report({'accuracy_top%d' % self.topk: self.accuracy_topk}, self)
            return self.loss
        if isinstance(t, MixedLabels):          # a mixup / CutMix batch: the same keys, the accuracies against the dominant label
            self.loss, self.accuracy, self.accuracy_topk = softmax_cross_entropy_mixed(
                self.y, t, self.label_smoothing if config.train else 0.0, self.topk or 1)
            report({'loss': self.loss, 'accuracy': self.accuracy}, self)
            if self.topk is not None:
                report({'accuracy_top%d' % self.topk: self.accuracy_topk}, self)
            return self.loss
        if self.label_smoothing == 0.0 and self.topk is None:
            self.loss, self.accuracy = softmax_cross_entropy_with_accuracy(self.y, t)
            report({'loss': self.loss, 'accuracy': self.accuracy}, self)
            return self.loss
        self.loss, self.accuracy, self.accuracy_topk = softmax_cross_entropy_with_topk_accuracy(
            self.y, t, self.label_smoothing if config.train else 0.0, self.topk or 1)
        report({'loss': self.loss, 'accuracy': self.accuracy}, self)
        if self.topk is not None:
            report({'accuracy_top%d' % self.topk: self.accuracy_topk}, self)
        return self.loss


class ClassificationMetrics:
    """Running sums of a classification pass in five doubles on the device: the sum of the row losses (plain cross-entropy), the
    top-1 hits, the top-``topk`` hits, the rows with a label and the rows.  ``add`` is one kernel call that synchronises nothing;
    ``result`` sums over the ranks of a communicator and reads the five numbers -- the only host synchronisation of a pass.
    Sums, not means of batch means: a ragged last batch and shards of different lengths weigh what they hold.  The loss divides
    by the rows with a label, the accuracies by all rows, as the loss kernels do per batch."""

    def __init__(self, topk=None, device=None):
        if topk is not None and topk < 1:
            raise ValueError('topk must be at least 1')
        self.topk, self.device, self.acc = topk, (torch.device(device) if device is not None else None), None

    def reset(self, device=None):
        if self.acc is None:
            device = self.device or device or torch.device('cuda', torch.cuda.current_device())
            self.acc = torch.zeros(5, device=device, dtype=torch.float64)
        else:
            self.acc.zero_()

    def add(self, logits, labels):
        z = logits.data if isinstance(logits, Variable) else logits
        if self.acc is None:
            self.reset(z.device)
        ops.softmax_xent_eval(z.contiguous(), _as_labels(z, labels).data.reshape(-1).contiguous(), self.acc, self.topk or 1)

    def result(self, comm=None):
        if self.acc is None:
            self.reset()
        total = self.acc
        if comm is not None and comm.active:
            total = comm.allreduce_sum(total.clone())
        loss, hits, hitsk, valid, rows = total.tolist()
        out = {'loss': loss / max(valid, 1), 'accuracy': hits / max(rows, 1)}
        if self.topk:
            out['accuracy_top%d' % self.topk] = hitsk / max(rows, 1)
        out['rows'], out['valid'] = int(rows), int(valid)
        return out
