"""``Classifier(predictor)`` in the manner of ``chainer.links.Classifier``: ``__call__(x, t)`` runs the predictor, computes
``softmax_cross_entropy`` and ``accuracy`` from one pass over the logits, reports both under ``loss`` / ``accuracy`` and returns
the loss.  The ImageNet pre-training arm of the reference (train_imagenet=True localizers) is trained through it.
``label_smoothing`` smooths the training loss (``config.train``; the validation loss stays the plain one, comparable between
runs), ``topk=k`` also reports ``accuracy_top<k>``; with neither, the loss function and the reported keys are the plain ones."""
import torch

from . import ops
from .functions.ops_small import softmax_cross_entropy_with_accuracy, softmax_cross_entropy_with_topk_accuracy
from .runtime.core import Chain, Variable, config, report


class Classifier(Chain):

    compute_accuracy = True

    def __init__(self, predictor, label_key=-1, label_smoothing=0.0, topk=None):
        super().__init__()
        if label_key != -1:
            raise ValueError('the label is the last argument (label_key=-1)')
        if not 0.0 <= label_smoothing < 1.0:
            raise ValueError('label_smoothing must be in [0, 1)')
        if topk is not None and topk < 1:
            raise ValueError('topk must be at least 1')
        self.label_smoothing, self.topk = label_smoothing, topk
        with self.init_scope():
            self.predictor = predictor
        self.y = self.loss = self.accuracy = self.accuracy_topk = None

    def materialize(self):
        """size every lazily sized head of the predictor's tree (``ResNet(class_labels=K).fc``): a parameter can only join the
        arena before it is finalised.  Host side only."""
        for link in self.predictor.links():
            if hasattr(link, 'materialize_head'):
                link.materialize_head()

    def __call__(self, *args):
        *xs, t = args
        if self._arena is None:
            self.materialize()
        first = xs[0].data if isinstance(xs[0], Variable) else xs[0]
        device = first.device if torch.is_tensor(first) and first.is_cuda else torch.device('cuda', torch.cuda.current_device())
        arena = self.finalize(device)
        for link in self.predictor.links():         # a predictor that finalises itself (the localizers do) finds this arena
            link.__dict__['_arena'] = arena
        self.y = self.predictor(*xs)
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
