"""Differentiable wrappers of the small kernels, named after the chainer.functions
the reference calls: ``_global_average_pooling_2d`` (sheep_localizer.py:58),
``L.Linear`` (:60), ``F.spatial_transformer_grid`` / ``_sampler`` (:62-63),
``F.mean_squared_error`` (sheep_updater.py:43,60), ``sigmoid(l4(relu(h)))``
(common/net.py:89-90)."""
import torch

from .. import ops
from ..mixed_labels import MixedLabels
from ..runtime.core import Function, Parameter, Variable, using_config


class GlobalAveragePooling2D(Function):
    """x: NHWC (B,H,W,C) -> (B,C)."""

    def forward(self, inputs):
        self.shape, self.dtype = tuple(inputs[0].shape), inputs[0].dtype
        return ops.gap_fwd(inputs[0])

    def backward(self, inputs, gys):
        return ops.gap_bwd(gys[0].contiguous(), self.shape, self.dtype)


def global_average_pooling_2d(x):
    return GlobalAveragePooling2D()(x)


class LinearFunction(Function):
    """y = act_out(act_in(x) W^T + b); accumulates gW / gb into the arena itself.  More than ``ops.LINEAR_SMALL_N`` outputs
    (the ImageNet heads) run on the GEMM kernels of classify.hip, which have no fused activations."""

    def __init__(self, act_in=False, act_out=False):
        self.act_in, self.act_out = act_in, act_out

    def forward(self, inputs):
        x, W = inputs[0], inputs[1]
        b = inputs[2] if len(inputs) > 2 else None
        self.wide = W.shape[0] > ops.LINEAR_SMALL_N
        if self.wide:
            if self.act_in or self.act_out:
                raise ValueError('a Linear layer with more than %d outputs has no fused activation' % ops.LINEAR_SMALL_N)
            return ops.linear_wide_fwd(x.contiguous(), W, b)
        self.y = ops.linear_fwd(x, W, b, self.act_in, self.act_out)
        return self.y

    def backward(self, inputs, gys):
        x, W = inputs[0], inputs[1]
        Wp = self.inputs[1]
        bp = self.inputs[2] if len(inputs) > 2 else None
        wgrad = Wp.update_rule.enabled or not getattr(Wp, 'skip_grad_when_disabled', False)
        if self.wide:
            gx = ops.linear_wide_bwd(x.contiguous(), W, gys[0].contiguous(), gW=Wp.grad_view if wgrad else None,
                                     gb=bp.grad_view if (bp is not None and wgrad) else None,
                                     need_gx=self.inputs[0].requires_grad)
            return (gx,) + (None,) * (len(inputs) - 1)
        gx = ops.linear_bwd(x, W, self.y, gys[0].contiguous(),
                            gW=Wp.grad_view if wgrad else None,
                            gb=bp.grad_view if (bp is not None and wgrad) else None,
                            need_gx=self.inputs[0].requires_grad, act_in=self.act_in, act_out=self.act_out)
        return (gx,) + (None,) * (len(inputs) - 1)

    def release(self):
        self.y = None


def linear(x, W, b=None):
    args = (x, W) if b is None else (x, W, b)
    return LinearFunction()(*args)


def sigmoid_linear_head(x, W):
    """sigmoid(Linear(relu(x))) fused (common/net.py:89-90)."""
    return LinearFunction(act_in=True, act_out=True)(x, W)


class SpatialTransformerGrid(Function):
    def __init__(self, output_shape):
        self.output_shape = tuple(output_shape)

    def forward(self, inputs):
        return ops.st_grid_fwd(inputs[0].contiguous(), self.output_shape)

    def backward(self, inputs, gys):
        return ops.st_grid_bwd(gys[0].contiguous())


def spatial_transformer_grid(theta, output_shape):
    return SpatialTransformerGrid(output_shape)(theta)


class SpatialTransformerSampler(Function):
    """images: NCHW leaf (B,3,H,W); grid (B,2,th,tw) -> rois as an NHWC4 buffer exposed
    through a (B,3,th,tw) view.  Only the grid gradient exists on this path (the frames
    are data, sheep_localizer.py:63)."""

    def forward(self, inputs):
        self.images, self.grid = inputs[0], inputs[1].contiguous()
        self.rois_nhwc4 = ops.st_sampler_fwd(self.images, self.grid)
        return self.rois_nhwc4

    def backward(self, inputs, gys):
        return None, ops.st_sampler_bwd_grid(self.images, self.grid, gys[0].contiguous())

    def release(self):
        self.images = self.grid = self.rois_nhwc4 = None


def spatial_transformer_sampler(images, grid):
    return SpatialTransformerSampler()(images, grid)


class MeanSquaredError(Function):
    def __init__(self, tconst=None):
        self.tconst = tconst

    def forward(self, inputs):
        y = inputs[0].contiguous()
        t = inputs[1].contiguous() if len(inputs) > 1 else None
        return ops.mse_fwd(y, t, 0.0 if self.tconst is None else self.tconst)

    def backward(self, inputs, gys):
        y = inputs[0].contiguous()
        t = inputs[1].contiguous() if len(inputs) > 1 else None
        g = ops.mse_bwd(y, gys[0], t, 0.0 if self.tconst is None else self.tconst)
        return (g,) if t is None else (g, None)


def mean_squared_error(x0, x1):
    """``F.mean_squared_error(y, t)``.  ``t`` may be a constant-filled array created with
    ``xp.full`` (sheep_updater.py:42); any array works."""
    return MeanSquaredError()(x0, x1)


class SoftmaxCrossEntropy(Function):
    """``F.softmax_cross_entropy(x, t, normalize=True, ignore_label=-1)`` and ``F.accuracy(x, t)`` from ONE pass over the
    logits: outputs (loss, accuracy), both 0-d device arrays.  t: int32 labels; a label outside [-1, N) is treated as ignored.
    The forward leaves ``(softmax - onehot) / count`` behind; the backward multiplies it by the upstream gradient."""

    def forward(self, inputs):
        x, t = inputs[0].contiguous(), inputs[1].contiguous()
        out, self.gz, _, _ = ops.softmax_xent_fwd(x, t)
        return out[0], out[1]

    def backward(self, inputs, gys):
        if gys[0] is None:          # only the accuracy was used: it has no gradient
            return None, None
        return ops.scale_by_scalar(self.gz, gys[0].reshape(1).contiguous()), None

    def release(self):
        self.gz = None


class SoftmaxCrossEntropyTopK(SoftmaxCrossEntropy):
    """The same against the label-smoothed target ``(1 - label_smoothing) onehot + label_smoothing / N`` (torch's convention),
    with the top-``topk`` accuracy as a third output: (loss, accuracy, accuracy_topk).  The backward is the parent's."""

    def __init__(self, label_smoothing, topk):
        self.label_smoothing, self.topk = float(label_smoothing), int(topk)

    def forward(self, inputs):
        x, t = inputs[0].contiguous(), inputs[1].contiguous()
        out, self.gz, _, _, _ = ops.softmax_xent_ls_fwd(x, t, self.label_smoothing, self.topk)
        return out[0], out[1], out[2]


class SoftmaxCrossEntropyMixed(SoftmaxCrossEntropyTopK):
    """The same against the target of a mixed batch, ``lam q(t_a) + oml q(t_b)`` with ``q`` the label-smoothed one-label target:
    inputs (x, t_a, t_b), outputs (loss, accuracy, accuracy_topk), the accuracies against the label of the larger weight.  The
    weights (1, 0) give ``SoftmaxCrossEntropyTopK``'s bits on (x, t_a).  The backward is the parent's."""

    def __init__(self, lam32, oml32, label_smoothing, topk):
        super().__init__(label_smoothing, topk)
        self.lam32, self.oml32 = float(lam32), float(oml32)

    def forward(self, inputs):
        x, ta, tb = (a.contiguous() for a in inputs)
        out, self.gz, _, _, _ = ops.softmax_xent_mix_fwd(x, ta, tb, self.lam32, self.oml32, self.label_smoothing, self.topk)
        return out[0], out[1], out[2]


class SigmoidBCE(SoftmaxCrossEntropyTopK):
    """The per-class sigmoid binary cross-entropy against the same target -- label-smoothed, one label or the two of a mixed batch,
    made 0 / 1 by ``target > target_threshold`` where a threshold is given -- from one pass over the logits: inputs (x, t_a) or
    (x, t_a, t_b), outputs (loss, accuracy, accuracy_topk).  The loss is the mean over classes and rows (``sum_classes``: the sum
    over classes, the mean over rows); the accuracies are the softmax ones, the sigmoid being monotone.  The backward is the
    parent's: the forward leaves ``(sigmoid - target) / denominator`` behind."""

    def __init__(self, lam32, oml32, label_smoothing, topk, target_threshold=None, sum_classes=False):
        super().__init__(label_smoothing, topk)
        self.lam32, self.oml32 = float(lam32), float(oml32)
        self.target_threshold, self.sum_classes = target_threshold, bool(sum_classes)

    def forward(self, inputs):
        x, ta, tb = (tuple(a.contiguous() for a in inputs) + (None,))[:3]
        out, self.gz, _, _, _ = ops.sigmoid_bce_fwd(x, ta, tb, self.lam32, self.oml32, self.label_smoothing, self.topk,
                                                    self.target_threshold, self.sum_classes)
        return out[0], out[1], out[2]


DISTILL_T_MIN, DISTILL_T_MAX = 2.0 ** -6, 2.0 ** 6       # the temperatures loans_softmax_distill_fwd_f32 takes


class SoftmaxDistill(SoftmaxCrossEntropyTopK):
    """The target of ``SoftmaxCrossEntropyMixed`` mixed with the KL divergence from a frozen teacher's logits at a temperature
    (Hinton's convention): inputs (x, teacher logits, t_a, t_b), outputs (loss, accuracy, accuracy_topk, distill_loss,
    teacher_accuracy) with loss = (1 - alpha) hard + alpha T^2 KL.  The teacher logits are a constant: no gradient flows to them.
    The backward is the parent's: the forward leaves the whole gradient with respect to ``x`` behind."""

    def __init__(self, lam32, oml32, label_smoothing, topk, alpha, temperature):
        super().__init__(label_smoothing, topk)
        self.lam32, self.oml32 = float(lam32), float(oml32)
        self.alpha, self.temperature = float(alpha), float(temperature)

    def forward(self, inputs):
        x, zt, ta, tb = (a.contiguous() for a in inputs)
        out, self.gz = ops.softmax_distill_fwd(x, zt, ta, tb, self.lam32, self.oml32, self.label_smoothing, self.topk,
                                               self.alpha, self.temperature)[:2]
        return out[0], out[1], out[2], out[3], out[4]

    def backward(self, inputs, gys):
        if gys[0] is None:
            return None, None, None, None
        return ops.scale_by_scalar(self.gz, gys[0].reshape(1).contiguous()), None, None, None


def _as_labels(x, t):
    import numpy as np
    if isinstance(t, Variable):
        t = t.data
    if isinstance(t, np.ndarray):
        t = torch.from_numpy(np.ascontiguousarray(t))
    device = x.data.device if isinstance(x, Variable) else x.device
    return Variable(t.to(device=device, dtype=torch.int32), requires_grad=False)


def softmax_cross_entropy_with_accuracy(x, t, ignore_label=-1):
    if ignore_label != -1:
        raise ValueError('only ignore_label=-1 (Chainer\'s default) is built')
    return SoftmaxCrossEntropy()(x, _as_labels(x, t))


def softmax_cross_entropy_with_topk_accuracy(x, t, label_smoothing=0.0, topk=1, ignore_label=-1):
    """(loss, accuracy, accuracy_topk): the label-smoothed loss, the top-1 and the top-``topk`` accuracy from one pass"""
    if ignore_label != -1:
        raise ValueError('only ignore_label=-1 (Chainer\'s default) is built')
    return SoftmaxCrossEntropyTopK(label_smoothing, topk)(x, _as_labels(x, t))


def softmax_cross_entropy_mixed(x, labels, label_smoothing=0.0, topk=1):
    """(loss, accuracy, accuracy_topk) of the logits ``x`` against ``labels``, a ``MixedLabels``: the loss of a mixup / CutMix
    batch.  The accuracies are against each row's dominant label."""
    return SoftmaxCrossEntropyMixed(labels.lam32, labels.oml32, label_smoothing, topk)(
        x, _as_labels(x, labels.t_a.reshape(-1)), _as_labels(x, labels.t_b.reshape(-1)))


def sigmoid_binary_cross_entropy(x, t, label_smoothing=0.0, topk=1, target_threshold=None, sum_classes=False):
    """(loss, accuracy, accuracy_topk) of the logits ``x`` under the per-class sigmoid binary cross-entropy (timm's
    ``BinaryCrossEntropy``): ``t`` is a label array or a ``MixedLabels``, the target the label-smoothed one of the softmax losses,
    made 0 / 1 by ``target > target_threshold`` where a threshold is given.  The loss is torch's
    ``binary_cross_entropy_with_logits`` -- the mean over classes and over the rows with a label -- or, with ``sum_classes``, its
    sum over the classes.  The accuracies are against each row's (dominant) label."""
    if target_threshold is not None and not 0.0 <= target_threshold < 1.0:
        raise ValueError('target_threshold must be in [0, 1)')
    if isinstance(t, MixedLabels):
        return SigmoidBCE(t.lam32, t.oml32, label_smoothing, topk, target_threshold, sum_classes)(
            x, _as_labels(x, t.t_a.reshape(-1)), _as_labels(x, t.t_b.reshape(-1)))
    return SigmoidBCE(1.0, 0.0, label_smoothing, topk, target_threshold, sum_classes)(x, _as_labels(x, t))


def softmax_cross_entropy_distilled(x, teacher_logits, t, label_smoothing=0.0, topk=1, alpha=0.5, temperature=1.0):
    """(loss, accuracy, accuracy_topk, distill_loss, teacher_accuracy) of the student logits ``x`` against the labels ``t`` (a
    label array or a ``MixedLabels``) and the logits of a frozen teacher: loss = (1 - alpha) CE(x, smoothed / mixed target)
    + alpha T^2 KL(softmax(teacher / T) || softmax(x / T)), the mean over the rows with a label.  ``distill_loss`` is the T^2 KL
    term alone, ``teacher_accuracy`` the teacher's top-1 accuracy against each row's (dominant) label.  The teacher logits are
    data: whatever graph made them is not walked."""
    if not 0.0 <= alpha <= 1.0:
        raise ValueError('alpha must be in [0, 1]')
    if not DISTILL_T_MIN <= temperature <= DISTILL_T_MAX:
        raise ValueError('temperature must be in [2^-6, 2^6]')
    zt = teacher_logits.data if isinstance(teacher_logits, Variable) else teacher_logits
    zt = Variable(zt, requires_grad=False)
    if isinstance(t, MixedLabels):
        return SoftmaxDistill(t.lam32, t.oml32, label_smoothing, topk, alpha, temperature)(
            x, zt, _as_labels(x, t.t_a.reshape(-1)), _as_labels(x, t.t_b.reshape(-1)))
    labels = _as_labels(x, t)
    return SoftmaxDistill(1.0, 0.0, label_smoothing, topk, alpha, temperature)(x, zt, labels, labels)


def softmax_cross_entropy(x, t, ignore_label=-1):
    """``F.softmax_cross_entropy(x, t)``: the mean loss over the rows whose label is not ``ignore_label``"""
    return softmax_cross_entropy_with_accuracy(x, t, ignore_label)[0]


def accuracy(y, t):
    """``F.accuracy(y, t)``: the share of ALL rows whose argmax (first index on a tie) equals the label; not differentiable"""
    with using_config('enable_backprop', False):
        return softmax_cross_entropy_with_accuracy(y, t)[1]


class GridLoss(Function):
    def __init__(self, kind, img_h=0.0, img_w=0.0, oob_scale=1.0):
        self.kind, self.img_h, self.img_w, self.oob_scale = kind, float(img_h), float(img_w), float(oob_scale)

    def forward(self, inputs):
        self.grid = inputs[0].contiguous()
        return ops.grid_loss_fwd(self.grid, self.kind, self.img_h, self.img_w, self.oob_scale)

    def backward(self, inputs, gys):
        return ops.grid_loss_bwd(self.grid, gys[0], self.kind, self.img_h, self.img_w, self.oob_scale)

    def release(self):
        self.grid = None


class ViewAsNHWC4(Function):
    """Re-interprets the NCHW *view* of an NHWC4 buffer (the localizer's ``rois``) as that
    buffer, and its gradient back; no data movement."""

    def forward(self, inputs):
        t = inputs[0]
        B, _, h, w = t.shape
        return torch.as_strided(t, (B, h, w, 4), (h * w * 4, w * 4, 4, 1))

    def backward(self, inputs, gys):
        return nchw_view(gys[0])


def nchw_view(nhwc4):
    """(B,h,w,4) buffer -> logical (B,3,h,w) view, the shape the reference exposes."""
    return nhwc4[..., :3].permute(0, 3, 1, 2)


class ExposeNCHW(Function):
    """NHWC4 -> logical (B,3,h,w) view (forward) and the inverse for the gradient."""

    def forward(self, inputs):
        return nchw_view(inputs[0])

    def backward(self, inputs, gys):
        g = gys[0]
        B, _, h, w = g.shape
        if g.stride() == (h * w * 4, 1, w * 4, 4):
            return torch.as_strided(g, (B, h, w, 4), (h * w * 4, w * 4, 4, 1))
        out = torch.zeros((B, h, w, 4), device=g.device, dtype=g.dtype)
        out[..., :3] = g.permute(0, 2, 3, 1)
        return out


class RoisToGrayscale(Function):
    """``0.299 * r + 0.587 * g + 0.114 * b`` with ``b, g, r = split_axis(rois, 3, axis=1)`` (reference
    sheep/sheep_localizer.py:65-68, ``transform_rois_to_grayscale=True``): (B,3,h,w) -> (B,1,h,w).  The rois are the NCHW
    view of the sampler's NHWC4 buffer; forward and backward are one streaming kernel each."""

    def forward(self, inputs):
        x = inputs[0]
        B, c, h, w = x.shape
        assert c == 3, "rois are not in RGB, can not convert them to grayscale"
        if x.stride() == (h * w * 4, 1, w * 4, 4):
            nhwc4 = torch.as_strided(x, (B, h, w, 4), (h * w * 4, w * 4, 4, 1))
        else:
            nhwc4 = ops.nchw3_to_nhwc4(x.contiguous())
        return ops.gray_fwd(nhwc4).view(B, 1, h, w)

    def backward(self, inputs, gys):
        g = gys[0].contiguous()
        B, _, h, w = g.shape
        return nchw_view(ops.gray_bwd(g.view(B, h, w)))


def rois_to_grayscale(rois):
    return RoisToGrayscale()(rois)
