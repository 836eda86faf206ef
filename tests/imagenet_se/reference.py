"""Test-side reference of the squeeze-and-excitation junction (csrc/se.hip): the formulas in NumPy, float64 as the reference and
float32 as the restatement the bound is taken from (tests/imagenet_droppath/reference.py: tol), and the oracle's basic units
with the gate at their junction for the model test.

x, second, gy: [B][P][C]; ``st`` / ``st2``: the fp32 vectors of the BN state, exact inputs; W1 [C/R][C], W2 [C][C/R].
    z = x scale + shift      q = mean_p z      h = relu(W1 q + b1)      s = sigmoid(W2 h + b2)      out = relu(s z + sc)
    g = gy (out > 0)         ds = sum_p g z    da2 = ds s (1 - s)       dh = (W2^T da2)(h > 0)      dq = W1^T dh
    gz = s g + dq / P  into the last BN (training mode: batch statistics of x),  g into the shortcut."""
import numpy as np

from oracle import chainer_ops as C
from oracle import model as M
from tests.imagenet import reference as R
from tests.imagenet_droppath.reference import _coeffs

SE_KEYS = ('se/down/W', 'se/down/b', 'se/up/W', 'se/up/b')


def _sigmoid(a):
    e = np.exp(-np.abs(a))
    return np.where(a >= 0, 1 / (1 + e), e / (1 + e)).astype(a.dtype)


def excite(q, W1, b1, W2, b2):
    """(h pre-activation, s) of q [B][C]"""
    a1 = q @ W1.T + b1
    return a1, _sigmoid(np.maximum(a1, 0) @ W2.T + b2)


def excite_bwd(ds, q, a1, s, W1, W2):
    """(gW1, gb1, gW2, gb2, dq) from ds [B][C]"""
    h = np.maximum(a1, 0)
    da2 = ds * s * (1 - s)
    dh = (da2 @ W2) * (a1 > 0)
    return dh.T @ q, dh.sum(0), da2.T @ h, da2.sum(0), dh @ W1


def junction_fwd(x, st, se, second, st2=None, dtype=np.float64, bf16=False):
    """dict(out, pre, a1, s, q): ``pre`` the final ReLU's input, ``a1`` the hidden layer's; bf16: the stored out rounded once"""
    t = lambda a: np.asarray(a).astype(dtype)       # noqa: E731
    z = t(x) * t(st['scale']) + t(st['shift'])
    sc = t(second) if st2 is None else t(second) * t(st2['scale']) + t(st2['shift'])
    q = z.mean(axis=1, dtype=dtype)
    a1, s = excite(q, *(t(w) for w in se))
    pre = s[:, None, :] * z + sc
    out = np.maximum(pre, dtype(0))
    return dict(out=C.round_bf16(out) if bf16 else out, pre=pre, a1=a1, s=s, q=q)


def junction_bwd(gy, mask, fwd, x, st, se, gamma, pre, x2=None, st2=None, gamma2=None, dtype=np.float64, bf16=False):
    """dict(gx, ggamma, gbeta, gW1, gb1, gW2, gb2[, gx2, ggamma2, gbeta2]); ``mask``: the forward's sign bits as bool [B][P][C];
    ``pre``: what the ten accumulators held, keyed like the result"""
    t = lambda a: np.asarray(a).astype(dtype)       # noqa: E731
    m, P = x.shape[0] * x.shape[1], x.shape[1]
    g = np.where(mask, t(gy), dtype(0))
    z = t(x) * t(st['scale']) + t(st['shift'])
    W1, _, W2, _ = (t(w) for w in se)
    gW1, gb1, gW2, gb2, dq = excite_bwd((g * z).sum(axis=1, dtype=dtype), fwd['q'], fwd['a1'], fwd['s'], W1, W2)
    gz = fwd['s'][:, None, :] * g + (dq / dtype(P))[:, None, :]
    xh = (t(x) - t(st['mean'])) * t(st['rstd'])
    db, dg = gz.sum(axis=(0, 1), dtype=dtype).astype(np.float64), (gz * xh).sum(axis=(0, 1), dtype=dtype).astype(np.float64)
    gg, gb, (k1, k2, k3) = _coeffs(db, dg, m, gamma, st, pre['ggamma'], pre['gbeta'], dtype)
    rnd = C.round_bf16 if bf16 else (lambda a: a)
    out = dict(gx=rnd(k1 * gz + k2 * t(x) + k3), ggamma=gg, gbeta=gb)
    for key, v in (('gW1', gW1), ('gb1', gb1), ('gW2', gW2), ('gb2', gb2)):
        out[key] = t(pre[key]) + v
    if x2 is not None:
        xh2 = (t(x2) - t(st2['mean'])) * t(st2['rstd'])
        db2, dg2 = g.sum(axis=(0, 1), dtype=dtype).astype(np.float64), (g * xh2).sum(axis=(0, 1), dtype=dtype).astype(np.float64)
        gg2, gb2_, (k1, k2, k3) = _coeffs(db2, dg2, m, gamma2, st2, pre['ggamma2'], pre['gbeta2'], dtype)
        out.update(gx2=rnd(k1 * g + k2 * t(x2) + k3), ggamma2=gg2, gbeta2=gb2_)
    return out


# ---- the oracle's basic units (NCHW) with the gate composed from its own operations -------------------------------------------------
class _Gate:
    """mixed into M._BasicA / M._BasicB: ``_gated(a)`` = s a on the forward, ``_ungate(gz, grads)`` the gradient into a"""

    def _gated(self, a):
        self.se = [self.c2.p[self.prefix + '/' + k] for k in SE_KEYS]
        self.a, self.q = a, a.mean(axis=(2, 3))
        self.a1, self.s = excite(self.q, *self.se)
        return self.s[:, :, None, None] * a

    def _ungate(self, gz, grads):
        got = excite_bwd((gz * self.a).sum(axis=(2, 3)), self.q, self.a1, self.s, self.se[0], self.se[2])
        for k, v in zip(SE_KEYS, got):
            M._acc(grads, self.prefix + '/' + k, v)
        return self.s[:, :, None, None] * gz + (got[4] / (gz.shape[2] * gz.shape[3]))[:, :, None, None]


class SEBasicA(M._BasicA, _Gate):
    def __init__(self, p, prefix, stride, train):
        super().__init__(p, prefix, stride, train)
        self.prefix = prefix

    def fwd(self, x):
        self.h1 = C.relu(self.c1.fwd(x))
        self.out = C.relu(self._gated(self.c2.fwd(self.h1)) + self.c3.fwd(x))
        return self.out

    def bwd(self, gy, grads):
        gz = gy * (self.out > 0)
        gx = self.c3.bwd(gz, grads)
        return gx + self.c1.bwd(self.c2.bwd(self._ungate(gz, grads), grads) * (self.h1 > 0), grads)


class SEBasicB(M._BasicB, _Gate):
    def __init__(self, p, prefix, train):
        super().__init__(p, prefix, train)
        self.prefix = prefix

    def fwd(self, x):
        self.h1 = C.relu(self.c1.fwd(x))
        self.out = C.relu(self._gated(self.c2.fwd(self.h1)) + x)
        return self.out

    def bwd(self, gy, grads):
        gz = gy * (self.out > 0)
        return gz + self.c1.bwd(self.c2.bwd(self._ungate(gz, grads), grads) * (self.h1 > 0), grads)


class SEResNet18Classifier(R.ResNet18Classifier):
    def forward(self, images, t):
        p, fe, train = self.p, self.fe, self.train
        self.stem = M._ConvBN(p, fe + 'conv1', fe + 'bn1', 2, 3, train)
        self.stem_relu = C.relu(self.stem.fwd(C.prepare_images(images)))
        h, self.pool_idx = C.max_pool_fwd(self.stem_relu, 3, 2, 0)
        self.blocks = []
        for name, _, stride in M.STAGES:
            for blk in (SEBasicA(p, fe + name + '/0', stride, train), SEBasicB(p, fe + name + '/1', train)):
                h = blk.fwd(h)
                self.blocks.append(blk)
        self.feat = h
        self.pooled = C.gap_fwd(h)
        self.logits = C.linear_fwd(self.pooled, p[fe + 'fc/W'], p[fe + 'fc/b'])
        self.t = t
        self.loss, self.accuracy, self.gz, _, _ = R.softmax_xent_ref(self.logits, t)
        return self.loss
