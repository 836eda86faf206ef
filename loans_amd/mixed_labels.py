"""``MixedLabels(t_a, t_b, lam)``: the label of a mixup / CutMix batch -- two int32 label arrays on the device and the weight
of the first.  The feed (common/datasets/batch_mix.py) makes them, ``Classifier.__call__`` takes one in the place of the label
array and trains against ``lam q(t_a) + (1 - lam) q(t_b)`` (functions/ops_small.py, ``softmax_cross_entropy_mixed``)."""
import numpy as np


class MixedLabels:
    """The two fp32 weights the loss kernel is given are computed here, once: ``lam32 = float32(lam)`` and
    ``oml32 = float32(1 - lam32)`` -- so ``lam = 1`` is exactly (1, 0), the weights at which the loss is the one-label loss bit for
    bit."""

    def __init__(self, t_a, t_b, lam):
        if t_a.shape != t_b.shape:
            raise ValueError('the two label arrays differ in shape: %r and %r' % (tuple(t_a.shape), tuple(t_b.shape)))
        lam = float(lam)
        if not 0.0 <= lam <= 1.0:
            raise ValueError('lam must lie in [0, 1], got %r' % lam)
        self.t_a, self.t_b, self.lam = t_a, t_b, lam
        self.lam32, self.oml32 = self.weights(lam)

    @staticmethod
    def weights(lam):
        """(float32(lam), float32(1 - float32(lam))) as Python floats"""
        lam32 = np.float32(lam)
        return float(lam32), float(np.float32(1.0) - lam32)

    def __len__(self):
        return len(self.t_a)

    def record_stream(self, stream):
        """what ``MultithreadIterator`` asks of every member of a device batch it hands from the feed's stream to the step's"""
        self.t_a.record_stream(stream)
        self.t_b.record_stream(stream)
