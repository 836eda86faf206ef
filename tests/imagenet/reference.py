"""Test-side reference of the ImageNet pre-training arm: the ResNet-18 classifier composed from the oracle's blocks, softmax
cross-entropy / accuracy in float64 NumPy (Chainer 4.1's ``F.softmax_cross_entropy(normalize=True, ignore_label=-1)`` and
``F.accuracy``), the case grid of the loss kernel, an fp32 NumPy restatement of that kernel's arithmetic, and the first-order
error bound the restatement and the kernel are both held to.

THE BOUND (u = 2^-24, the unit roundoff of fp32; everything first order in u, inflated by 1 %).  The kernel computes per row
    m = max z                                   exact
    d_i = fl(z_i - m)                           relative error u; exp(d_i (1 + delta)) = exp(d_i) (1 + d_i delta): |d_i| u
    e_i = expf(d_i)                             c_e u, c_e = 4: device expf and NumPy's float32 exp are 1-ulp functions (2u);
                                                two ulps are budgeted so that either side may be the one compared
    S = sum e_i                                 non-negative terms: relative error (adds on the longest path) u.  The tree is
                                                ceil(N / 256) serial adds per thread (element i goes to thread i % 256), six
                                                butterfly levels in a wave, (w0 + w1) + (w2 + w3): T = ceil(N / 256) + 8
  so S has relative error (T + c_e + sum_i p_i |d_i|) u, and sum_i p_i |d_i| = m - E_p[z] = H(p) - log S <= ln N.
    L = logf(S)                                 log S (1 + c_l u) + relerr(S), c_l = 4
    lse = fl(m + L), loss = fl(lse - z_t)       u |lse| + u |loss|
      |loss^ - loss| <= u (|lse| + |lse - z_t|) + (T + c_e + ln N + c_l |log S|) u
    p_i = e_i / S                               relative (|d_i| + 2 c_e + T + ln N + 1) u
    gz_i = fl(fl(p_i - o_i) / count)            2u |p_i - o_i| / count on top
The batch loss sums the non-negative row losses in the same tree over B (Tb = ceil(B / 256) + 8 adds) and divides once:
    |loss^ - loss| <= (sum_b bound_b + (Tb + 1) u sum_b loss_b) / count
Terms below 1e-37 (exp underflow) are covered by an absolute 1e-37."""
import numpy as np

from oracle import chainer_ops as C
from oracle import model as M

U = 2.0 ** -24
C_E = 4.0
C_L = 4.0
SLACK = 1.01


# ---- float64 reference --------------------------------------------------------------------------------------------------
def softmax_xent_ref(z, t, gy=1.0):
    """(loss, accuracy, gz, row_loss, argmax) in float64; a label outside [0, N) is an ignored row (-1 is Chainer's
    ignore_label, anything else out of range is the kernel's deliberate departure)"""
    z = np.asarray(z, np.float64)
    t = np.asarray(t, np.int64)
    B, N = z.shape
    valid = (t >= 0) & (t < N)
    count = max(int(valid.sum()), 1)
    m = z.max(axis=1, keepdims=True)
    e = np.exp(z - m)
    S = e.sum(axis=1, keepdims=True)
    lse = (m + np.log(S))[:, 0]
    tt = np.where(valid, t, 0)
    row_loss = np.where(valid, lse - z[np.arange(B), tt], 0.0)
    p = e / S
    onehot = np.zeros_like(p)
    onehot[np.arange(B), tt] = 1.0
    gz = np.where(valid[:, None], (p - onehot) / count, 0.0) * gy
    am = z.argmax(axis=1)               # first index on a tie
    acc = float((am == t).mean())
    return float(row_loss.sum() / count), acc, gz, row_loss, am


def row_bounds(z, t):
    """per-row loss bound (B,), per-element gz bound (B, N) for gy = 1, and the batch-loss bound, from the derivation above"""
    z = np.asarray(z, np.float64)
    t = np.asarray(t, np.int64)
    B, N = z.shape
    valid = (t >= 0) & (t < N)
    count = max(int(valid.sum()), 1)
    m = z.max(axis=1, keepdims=True)
    d = z - m
    e = np.exp(d)
    S = e.sum(axis=1, keepdims=True)
    p = e / S
    lse = (m + np.log(S))[:, 0]
    tt = np.where(valid, t, 0)
    loss = lse - z[np.arange(B), tt]
    T = -(-N // 256) + 8
    lnN = np.log(N)
    lb = U * (np.abs(lse) + np.abs(loss)) + (T + C_E + lnN + C_L * np.abs(np.log(S[:, 0]))) * U
    lb = np.where(valid, lb * SLACK + 1e-37, 0.0)
    onehot = np.zeros_like(p)
    onehot[np.arange(B), tt] = 1.0
    gb = U * (p * (np.abs(d) + 2 * C_E + T + lnN + 1) + 2 * np.abs(p - onehot)) / count
    gb = np.where(valid[:, None], gb * SLACK + 1e-37, 0.0)
    Tb = -(-B // 256) + 8
    batch = (lb.sum() + (Tb + 1) * U * np.where(valid, loss, 0.0).sum() * SLACK) / count
    return lb, gb, float(batch)


# ---- fp32 restatement of the kernel ---------------------------------------------------------------------------------------
def _tree256(partials):
    """(rows, 256) float32 -> (rows,): xor butterfly over 64 lanes (offsets 32 .. 1), then (w0 + w1) + (w2 + w3)"""
    v = partials.reshape(len(partials), 4, 64).astype(np.float32)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = (v + v[:, :, lane ^ o]).astype(np.float32)
    w = v[:, :, 0]
    return ((w[:, 0] + w[:, 1]).astype(np.float32) + (w[:, 2] + w[:, 3]).astype(np.float32)).astype(np.float32)


def _strided_partials(x):
    """(rows, n) float32 -> (rows, 256): thread j adds elements j, j + 256, ... in that order, starting from 0"""
    rows, n = x.shape
    pad = -(-n // 256) * 256
    xp = np.zeros((rows, pad), np.float32)
    xp[:, :n] = x
    acc = np.zeros((rows, 256), np.float32)
    for k in range(pad // 256):
        acc = (acc + xp[:, k * 256:(k + 1) * 256]).astype(np.float32)
    return acc


def softmax_xent_fp32(z, t):
    """the kernel's arithmetic, operation for operation, in NumPy float32: (loss, accuracy, gz, row_loss)"""
    z = np.asarray(z, np.float32)
    t = np.asarray(t, np.int64)
    B, N = z.shape
    valid = (t >= 0) & (t < N)
    count = np.float32(max(int(valid.sum()), 1))
    m = z.max(axis=1, keepdims=True)
    e = np.exp((z - m).astype(np.float32)).astype(np.float32)
    S = _tree256(_strided_partials(e))
    tt = np.where(valid, t, 0)
    lse = (m[:, 0] + np.log(S).astype(np.float32)).astype(np.float32)
    row_loss = np.where(valid, (lse - z[np.arange(B), tt]).astype(np.float32), np.float32(0))
    p = (e / S[:, None]).astype(np.float32)
    onehot = np.zeros_like(p)
    onehot[np.arange(B), tt] = 1
    gz = np.where(valid[:, None], ((p - onehot).astype(np.float32) / count).astype(np.float32), np.float32(0))
    hit = (z.argmax(axis=1) == t).astype(np.float32)
    loss = np.float32(_tree256(_strided_partials(row_loss[None, :]))[0] / count)
    acc = np.float32(_tree256(_strided_partials(hit[None, :]))[0] / np.float32(B))
    return float(loss), float(acc), gz, row_loss


# ---- the case grid ----------------------------------------------------------------------------------------------------------
XENT_N = (1, 2, 63, 64, 65, 1000, 1001)
XENT_B = (1, 5, 64, 257)
PROFILES = ('normal', 'pm80', 'equal', 'dominant', 'tie')
LABELS = ('first_last', 'third_ignored', 'all_ignored', 'one_out_of_range')


def make_logits(profile, B, N, rng):
    if profile == 'normal':
        z = rng.standard_normal((B, N))
    elif profile == 'pm80':                     # exp(80) overflows fp32 without the max shift
        z = np.where(rng.random((B, N)) < 0.5, 80.0, -80.0)
    elif profile == 'equal':                    # known answer: loss = log N, gz = (1/N - onehot) / count
        z = np.full((B, N), 0.75)
    elif profile == 'dominant':
        z = rng.standard_normal((B, N))
        z[np.arange(B), rng.integers(0, N, B)] += 30.0
    else:                                       # 'tie': two exactly equal maxima per row
        z = rng.standard_normal((B, N))
    return z.astype(np.float32)


def make_labels(kind, B, N, rng):
    t = np.where(np.arange(B) % 2 == 0, 0, N - 1).astype(np.int32)
    if kind == 'third_ignored':
        t[::3] = -1
    elif kind == 'all_ignored':
        t[:] = -1
    elif kind == 'one_out_of_range':
        t[B // 2] = N + 3 if (B // 2) % 2 == 0 else -7
    return t


def xent_cases(N):
    """every (B, profile, label set) of the grid at N classes: (name, z float32, t int32, tie expectations or None)"""
    for B in XENT_B:
        for profile in PROFILES:
            for kind in LABELS:
                rng = np.random.Generator(np.random.PCG64([N, B, PROFILES.index(profile), LABELS.index(kind)]))
                z = make_logits(profile, B, N, rng)
                t = make_labels(kind, B, N, rng)
                expect = None
                if profile == 'tie':
                    if N < 2 or kind != 'first_last':
                        continue
                    # row r: maxima at columns a < b; even rows carry the label on the first (correct), odd rows on the second
                    a = rng.integers(0, N - 1, B)
                    b = np.array([rng.integers(x + 1, N) for x in a])
                    top = (np.abs(z).max(axis=1) + 1.0).astype(np.float32)
                    z[np.arange(B), a] = top
                    z[np.arange(B), b] = top
                    t = np.where(np.arange(B) % 2 == 0, a, b).astype(np.int32)
                    expect = (np.arange(B) % 2 == 0)
                yield '%s-%s-B%d-N%d' % (profile, kind, B, N), z, t, expect


def argmax_margin_ok(z):
    """The logits are the kernel's INPUTS: the argmax compares them as they are, so their own rounding is zero and any two
    distinct fp32 values are ordered exactly.  A row is unambiguous when its maximum is unique, or when the tie is exact (the
    first index then wins on both sides).  True for every row whose top two are either bit-equal or at least one ulp apart --
    i.e. always for finite fp32 -- and the check below makes that explicit for the float64 copy the reference uses."""
    z64 = np.asarray(z, np.float64)
    if z64.shape[1] < 2:
        return True
    top2 = np.sort(z64, axis=1)[:, -2:]
    gap = top2[:, 1] - top2[:, 0]
    ulp = np.spacing(np.abs(np.asarray(z, np.float32)).max(axis=1)).astype(np.float64)
    return bool(np.all((gap == 0) | (gap >= ulp * 0.5)))


# ---- the classifier oracle ---------------------------------------------------------------------------------------------------
def init_fc(rng, classes, in_size=512):
    """Chainer's default Linear initialiser: LeCunNormal, zero bias"""
    return (rng.standard_normal((classes, in_size)) / np.sqrt(in_size)).astype(np.float32), np.zeros(classes, np.float32)


class ResNet18Classifier:
    """``Classifier(ResNet(18, class_labels=K))`` (prefix '') or ``Classifier(SheepLocalizer(train_imagenet=True))`` (prefix
    'feature_extractor/') on a parameter dict with Chainer's keys, composed from the oracle's blocks, in the dtype of the
    parameters"""

    def __init__(self, params, prefix='', train=True):
        self.p, self.fe, self.train = params, prefix, train

    def forward(self, images, t):
        p, fe, train = self.p, self.fe, self.train
        x = M._q(C.prepare_images(images))
        self.stem = M._ConvBN(p, fe + 'conv1', fe + 'bn1', 2, 3, train)
        self.stem_relu = M._q(C.relu(self.stem.fwd(x)))
        h, self.pool_idx = C.max_pool_fwd(self.stem_relu, 3, 2, 0)
        self.blocks = []
        for name, _, stride in M.STAGES:
            for blk in (M._BasicA(p, fe + name + '/0', stride, train), M._BasicB(p, fe + name + '/1', train)):
                h = blk.fwd(h)
                self.blocks.append(blk)
        self.feat = h
        self.pooled = C.gap_fwd(h)
        self.logits = C.linear_fwd(self.pooled, p[fe + 'fc/W'], p[fe + 'fc/b'])
        self.t = t
        self.loss, self.accuracy, self.gz, _, _ = softmax_xent_ref(self.logits, t)
        return self.loss

    def backward(self, grads):
        p, fe = self.p, self.fe
        gz = self.gz.astype(self.logits.dtype)
        gpooled, gW, gb = C.linear_bwd(self.pooled, p[fe + 'fc/W'], gz, True)
        M._acc(grads, fe + 'fc/W', gW)
        M._acc(grads, fe + 'fc/b', gb)
        g = M._q(C.gap_bwd(self.feat.shape, gpooled))
        for blk in reversed(self.blocks):
            g = blk.bwd(g, grads)
        g = C.max_pool_bwd(self.stem_relu.shape, self.pool_idx, g, 3, 2, 0)
        g = g * (self.stem_relu > 0)
        self.stem.bwd(g, grads, need_gx=False)
        return grads

    def step(self, images, t, optimizer):
        """forward, backward, one optimiser step (``oracle.model.AdamAMSGrad``); returns (loss, accuracy, logits, grads)"""
        loss = self.forward(images, t)
        grads = self.backward({})
        optimizer.update(grads)
        return loss, self.accuracy, self.logits, grads
