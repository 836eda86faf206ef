"""Test-side reference of stochastic depth in the residual units (loans_amd/functions/drop_path.py, the ``loans_bn_*_rows_*``
kernels of csrc/bn_pool.hip): the junction alone in float64 and as an fp32 NumPy restatement of the kernels, whole units as
subclasses of the oracle's with a per-sample factor at the junction, and a ResNet-18 classifier built from them on top of
tests/imagenet/reference.py (R).

THE JUNCTION.  x, second, gy: [B][P][C] (NHWC with the positions flattened), r: [B], 0 for a dropped sample and 1 / (1 - p)
for a kept one.  The fp32 vectors of the BN state (mean, rstd, scale, shift) and gamma are EXACT inputs, as the kernels take them.
    a   = x scale + shift                          (the last BN of the unit, its statistics over all samples)
    sc  = second  (mode 1)  or  second scale2 + shift2  (mode 2)
    out = relu(r_b a + sc);     a dropped sample is relu(sc), whatever x holds
    g   = gy (out > 0)          (the mask comes as sign bits: one byte per four channels)
    db = sum r_b g,  dg = sum r_b g xhat,  xhat = (x - mean) rstd        ggamma += dg,  gbeta += db
    k1 = gamma rstd,  k2 = -k1 rstd dg / m,  k3 = k1 (mean rstd dg - db) / m,   gx = k1 (r_b g) + k2 x + k3
    mode 2:  db2 = sum g,  dg2 = sum g xhat2,  gx2 = k1b g + k2b x2 + k3b         (the shortcut takes the unscaled gradient)
With mean / rstd the batch statistics of x this is the gradient of the junction through a training-mode BN
(test_droppath_cpu.py checks the units built from it against finite differences).

THE BOUND is the project's, max(5 |fp32 restatement - fp64|, 5e-4 |ref|, 1e-5), elementwise; on bf16 tensors the inputs are
rounded to bf16 first and the restatement rounds what the kernel stores (tests/bn_cases.py: NumpyImpl._out)."""
import numpy as np

from oracle import chainer_ops as C
from oracle import model as M
from tests.imagenet import reference as R

F = np.float32


def tol(r32, r64):
    """the project's form: max(5 |fp32 restatement - fp64|, 5e-4 |ref|, 1e-5)"""
    r32, r64 = np.asarray(r32, np.float64), np.asarray(r64, np.float64)
    return np.maximum(np.maximum(5 * np.abs(r32 - r64), 5e-4 * np.abs(r64)), 1e-5)


def bits_of(y):
    """one byte per four channels, bit e = (y[4 i + e] > 0)"""
    return ((np.asarray(y).reshape(-1, 4) > 0) * np.array([1, 2, 4, 8])).sum(axis=1).astype(np.uint8)


def mask_of(bits, shape):
    return ((np.asarray(bits)[:, None] >> np.arange(4)) & 1).astype(bool).reshape(shape)


def keep_factor(p):
    """fl32(1 / (1 - p)): what a kept sample is scaled by"""
    return F(1.0 / (1.0 - p))


def _rows(r, dtype):
    return np.asarray(r).astype(dtype)[:, None, None]


def junction_fwd(x, st, r, second, st2=None, dtype=np.float64, bf16=False):
    """out [B][P][C] in ``dtype`` (float64: the reference; float32: the kernel's operations one by one, every product rounded;
    ``bf16``: the stored result rounded once).  ``st`` / ``st2``: dicts of the fp32 vectors scale, shift (mean, rstd)."""
    t = lambda a: np.asarray(a).astype(dtype)       # noqa: E731
    a = t(x) * t(st['scale']) + t(st['shift'])
    sc = t(second) if st2 is None else t(second) * t(st2['scale']) + t(st2['shift'])
    rb = _rows(r, dtype)
    out = np.maximum(np.where(rb == 0, sc, rb * a + sc), dtype(0))
    assert out.dtype == dtype
    return C.round_bf16(out) if bf16 else out


def _coeffs(db, dg, m, gamma, st, gg0, gb0, dtype):
    rs, mu = st['rstd'].astype(np.float64), st['mean'].astype(np.float64)
    a = gamma.astype(np.float64) * rs
    k = (a, -a * rs * dg / m, a * (mu * rs * dg - db) / m)
    if dtype == F:      # the coefficient kernel: fp64 arithmetic on the fp64 sums, each result cast once
        return gg0 + dg.astype(F), gb0 + db.astype(F), tuple(v.astype(F) for v in k)
    return gg0.astype(np.float64) + dg, gb0.astype(np.float64) + db, k


def junction_bwd(gy, mask, r, x, st, gamma, gg0, gb0, x2=None, st2=None, gamma2=None, gg20=None, gb20=None, dtype=np.float64,
                 bf16=False):
    """dict(gx, ggamma, gbeta[, gx2, ggamma2, gbeta2]); ``mask``: bool [B][P][C], the sign bits of the forward's output;
    gg0 / gb0: what the accumulators held.  float32: sums in fp32 (NumPy's pairwise order), then the fp64 coefficient step."""
    t = lambda a: np.asarray(a).astype(dtype)       # noqa: E731
    m = x.shape[0] * x.shape[1]
    g = np.where(mask, t(gy), dtype(0))
    rg = _rows(r, dtype) * g
    xh = (t(x) - t(st['mean'])) * t(st['rstd'])
    db, dg = rg.sum(axis=(0, 1), dtype=dtype).astype(np.float64), (rg * xh).sum(axis=(0, 1), dtype=dtype).astype(np.float64)
    gg, gb, (k1, k2, k3) = _coeffs(db, dg, m, gamma, st, gg0, gb0, dtype)
    rnd = C.round_bf16 if bf16 else (lambda a: a)
    out = dict(gx=rnd(k1 * rg + k2 * t(x) + k3), ggamma=gg, gbeta=gb)
    if x2 is not None:
        xh2 = (t(x2) - t(st2['mean'])) * t(st2['rstd'])
        db2, dg2 = g.sum(axis=(0, 1), dtype=dtype).astype(np.float64), (g * xh2).sum(axis=(0, 1), dtype=dtype).astype(np.float64)
        gg2, gb2, (k1, k2, k3) = _coeffs(db2, dg2, m, gamma2, st2, gg20, gb20, dtype)
        out.update(gx2=rnd(k1 * g + k2 * t(x2) + k3), ggamma2=gg2, gbeta2=gb2)
    assert out['gx'].dtype == dtype
    return out


# ---- whole units: the oracle's (NCHW) with r at the junction --------------------------------------------------------------------
def _ex(r, like):
    return np.asarray(r).astype(like.dtype)[:, None, None, None]


class DropBasicA(M._BasicA):
    def __init__(self, p, prefix, stride, train, r=None):
        super().__init__(p, prefix, stride, train)
        self.r = r if train else None

    def fwd(self, x):
        if self.r is None:
            return super().fwd(x)
        self.h1 = M._q(C.relu(self.c1.fwd(x)))
        a = self.c2.fwd(self.h1)
        b = self.c3.fwd(x)
        self.out = M._q(C.relu(_ex(self.r, a) * a + b))
        return self.out

    def bwd(self, gy, grads):
        if self.r is None:
            return super().bwd(gy, grads)
        gz = gy * (self.out > 0)
        gx = M._q(self.c3.bwd(gz, grads))
        gh1 = M._q(self.c2.bwd(_ex(self.r, gz) * gz, grads))
        return M._q(gx + self.c1.bwd(gh1 * (self.h1 > 0), grads))


class DropBasicB(M._BasicB):
    def __init__(self, p, prefix, train, r=None):
        super().__init__(p, prefix, train)
        self.r = r if train else None

    def fwd(self, x):
        if self.r is None:
            return super().fwd(x)
        self.h1 = M._q(C.relu(self.c1.fwd(x)))
        a = self.c2.fwd(self.h1)
        self.out = M._q(C.relu(_ex(self.r, a) * a + x))
        return self.out

    def bwd(self, gy, grads):
        if self.r is None:
            return super().bwd(gy, grads)
        gz = gy * (self.out > 0)
        gh1 = M._q(self.c2.bwd(_ex(self.r, gz) * gz, grads))
        return M._q(gz + self.c1.bwd(gh1 * (self.h1 > 0), grads))


class DropResUnit(M._ResUnit):
    def __init__(self, p, stages, shortcut, train, r=None):
        super().__init__(p, stages, shortcut, train)
        self.r = r if train else None

    def fwd(self, x):
        if self.r is None:
            return super().fwd(x)
        self.hs = []
        h = x
        for i, st in enumerate(self.stages):
            h = st.fwd(h)
            if i < len(self.stages) - 1:
                h = M._q(C.relu(h))
                self.hs.append(h)
        sc = self.shortcut.fwd(x) if self.shortcut is not None else x
        self.out = M._q(C.relu(_ex(self.r, h) * h + sc))
        return self.out

    def bwd(self, gy, grads):
        if self.r is None:
            return super().bwd(gy, grads)
        gz = gy * (self.out > 0)
        gx = M._q(self.shortcut.bwd(gz, grads)) if self.shortcut is not None else gz
        g = _ex(self.r, gz) * gz
        for i in range(len(self.stages) - 1, 0, -1):
            g = M._q(self.stages[i].bwd(g, grads)) * (self.hs[i - 1] > 0)
        return M._q(gx + self.stages[0].bwd(g, grads))


class DropResNet18Classifier(R.ResNet18Classifier):
    """R.ResNet18Classifier with ``table`` = {unit index in forward order: r [B]} (a unit that is not in it runs the oracle's
    own code); test mode ignores the table"""

    def __init__(self, params, table, prefix='', train=True):
        super().__init__(params, prefix, train)
        self.table = table

    def forward(self, images, t):
        p, fe, train = self.p, self.fe, self.train
        x = M._q(C.prepare_images(images))
        self.stem = M._ConvBN(p, fe + 'conv1', fe + 'bn1', 2, 3, train)
        self.stem_relu = M._q(C.relu(self.stem.fwd(x)))
        h, self.pool_idx = C.max_pool_fwd(self.stem_relu, 3, 2, 0)
        self.blocks = []
        for name, _, stride in M.STAGES:
            for blk in (DropBasicA(p, fe + name + '/0', stride, train, self.table.get(len(self.blocks))),
                        DropBasicB(p, fe + name + '/1', train, self.table.get(len(self.blocks) + 1))):
                h = blk.fwd(h)
                self.blocks.append(blk)
        self.feat = h
        self.pooled = C.gap_fwd(h)
        self.logits = C.linear_fwd(self.pooled, p[fe + 'fc/W'], p[fe + 'fc/b'])
        self.t = t
        self.loss, self.accuracy, self.gz, _, _ = R.softmax_xent_ref(self.logits, t)
        return self.loss
