"""Test-side reference of mixup / CutMix in the ImageNet recipe: the two-label softmax cross-entropy in float64 NumPy, an fp32
NumPy restatement of the kernel (loans_amd/csrc/classify.hip, softmax_xent_mix_rows_kernel), the first-order bound both are
held to, the case grid, and the float64 mix of a batch with its shifted self with the bound of csrc/mix.hip.  What is not new
here is tests/imagenet/reference.py's (R) and tests/imagenet_sgd/reference.py's (S).

THE TARGET.  The two weights wa, wb are fp32 numbers and EXACT inputs (``MixedLabels`` rounds them once, on the host).  With
w_i = wa [i == ta] + wb [i == tb]  (ta == tb: wa + wb on that class)
    q = (1 - eps) w + eps / N,     loss = lse - (1 - eps) (wa z_ta + wb z_tb) - eps mean(z),     gz = (softmax(z) - q) / count
which is lam q(ta) + oml q(tb) of the one-label targets for weights that sum to one.  A row counts when both labels lie in
[0, N).  The weights (1, 0) and (0, 1) are the one-label loss on ta / on tb: the label of weight zero is not read, so it does
not decide whether a row counts, and the bound is S.ls_bounds itself.  Hits are taken against ta if wa >= wb, else tb.

THE BOUND for any other weights (u = 2^-24, first order, inflated by R.SLACK, plus 1e-37; E_lse, T as in S):
    zmix^ = fl(fl(wa z_ta) + fl(wb z_tb))           two products, one sum:  E_mix <= 2u (|wa z_ta| + |wb z_tb|)
    loss^ = fl(fl(lse^ - fl(omeps^ zmix^)) - fl(eps^ mean^))
      |loss^ - loss| <= E_lse + (1 - eps) E_mix + 2u |(1 - eps) zmix| + u |lse - (1 - eps) zmix|
                        + eps (T mean|z| + |mean z|) u + 2u |eps mean z| + u |loss|
    (S's smoothed bound with z_t replaced by zmix, plus the error zmix brings along; at eps = 0 the kernel skips the product
    with omeps = 1 and the mean, which only removes roundings)
    w^ = fl(wa + wb) where ta == tb, else exact;  q^ = fl(fl(omeps^ w^) + q_off^):  at most four roundings land on the
    (1 - eps) w part and two on eps / N:  |q^ - q| <= 4u q
    gz^ = fl(fl(p^ - q^) / count):  (p (|d| + 2 c_e + T + ln N + 1) + 4 q + 2 |p - q|) u / count
A contracted multiply-add skips the rounding of its product and nothing else: the bound holds for either code.  The batch
loss is R's tree over the row losses.  Hits are compared exactly.

THE MIX of a batch (csrc/mix.hip): a blended element is fl(fma(wa, a, fl(wb b))) or fl(fl(wa a) + fl(wb b)): at most two
roundings of the products and one of the sum, |out - ref| <= 2u (|wa a| + |wb b|); every other element is a bit copy."""
import numpy as np

from tests.imagenet import reference as R
from tests.imagenet_sgd import reference as S

U = R.U
LAMS = (1.0, 0.0, 0.5, float(np.float32(0.3)))
MIX_EPS = (0.0, 0.1)
PAIRS = ('different', 'equal', 'ta_ignored', 'tb_ignored', 'both_ignored')
GPU_N = (1, 2, 65, 1000)
GPU_B = (1, 5, 257)


def weights(lam):
    """(float32(lam), float32(1 - float32(lam))) as Python floats: what ``MixedLabels`` computes"""
    lam32 = np.float32(lam)
    return float(lam32), float(np.float32(1.0) - lam32)


def single_label(ta, tb, wa, wb):
    """the one label array that counts at the weights (1, 0) / (0, 1), else None"""
    if wa == 1.0 and wb == 0.0:
        return ta
    if wa == 0.0 and wb == 1.0:
        return tb
    return None


def _setup(z, ta, tb, wa, wb):
    z = np.asarray(z, np.float64)
    ta, tb = np.asarray(ta, np.int64), np.asarray(tb, np.int64)
    B, N = z.shape
    va, vb = (ta >= 0) & (ta < N), (tb >= 0) & (tb < N)
    one = single_label(ta, tb, wa, wb)
    valid = (va & vb) if one is None else ((one >= 0) & (one < N))
    # an index for every row; where a label is out of range the row is ignored or the label's weight is zero
    return z, np.where(va, ta, 0), np.where(vb, tb, 0), valid, max(int(valid.sum()), 1)


def mixed_ref(z, ta, tb, wa, wb, eps, k):
    """(loss, accuracy, accuracy_topk, gz, row_loss, hit, hitk) in float64 for the fp32 weights wa, wb taken as exact"""
    z, ia, ib, valid, count = _setup(z, ta, tb, wa, wb)
    B, N = z.shape
    rows = np.arange(B)
    m = z.max(axis=1, keepdims=True)
    e = np.exp(z - m)
    S_ = e.sum(axis=1, keepdims=True)
    lse = (m + np.log(S_))[:, 0]
    zmix = wa * z[rows, ia] + wb * z[rows, ib]
    row_loss = np.where(valid, lse - (1.0 - eps) * zmix - eps * z.mean(axis=1), 0.0)
    w = np.zeros_like(z)
    np.add.at(w, (rows, ia), wa)
    np.add.at(w, (rows, ib), wb)
    q = (1.0 - eps) * w + eps / N
    gz = np.where(valid[:, None], (e / S_ - q) / count, 0.0)
    dom = ia if wa >= wb else ib
    zd = z[rows, dom]
    hit = valid & (z.argmax(axis=1) == dom)
    j = np.arange(N)[None, :]
    rank = ((z > zd[:, None]) | ((z == zd[:, None]) & (j < dom[:, None]))).sum(axis=1)
    hitk = valid & (rank < k)
    return float(row_loss.sum() / count), float(hit.mean()), float(hitk.mean()), gz, row_loss, hit, hitk


def mixed_bounds(z, ta, tb, wa, wb, eps):
    """per-row loss bound (B,), per-element gz bound (B, N) for an upstream gradient of 1, and the batch-loss bound"""
    one = single_label(np.asarray(ta), np.asarray(tb), wa, wb)
    if one is not None:
        return S.ls_bounds(z, one, eps)
    z, ia, ib, valid, count = _setup(z, ta, tb, wa, wb)
    B, N = z.shape
    rows = np.arange(B)
    m = z.max(axis=1, keepdims=True)
    d = z - m
    e = np.exp(d)
    S_ = e.sum(axis=1, keepdims=True)
    p = e / S_
    lse = (m + np.log(S_))[:, 0]
    za, zb = z[rows, ia], z[rows, ib]
    zmix = wa * za + wb * zb
    mean = z.mean(axis=1)
    loss = lse - (1.0 - eps) * zmix - eps * mean
    T = -(-N // 256) + 8
    lnN = np.log(N)
    e_lse = U * np.abs(lse) + (T + R.C_E + lnN + R.C_L * np.abs(np.log(S_[:, 0]))) * U
    e_mix = 2 * U * (np.abs(wa * za) + np.abs(wb * zb))
    lb = e_lse + (1.0 - eps) * e_mix + 2 * U * np.abs((1.0 - eps) * zmix) + U * np.abs(lse - (1.0 - eps) * zmix) \
        + eps * (T * np.abs(z).mean(axis=1) + np.abs(mean)) * U + 2 * U * np.abs(eps * mean) + U * np.abs(loss)
    lb = np.where(valid, lb * R.SLACK + 1e-37, 0.0)
    w = np.zeros_like(z)
    np.add.at(w, (rows, ia), wa)
    np.add.at(w, (rows, ib), wb)
    q = (1.0 - eps) * w + eps / N
    gb = U * (p * (np.abs(d) + 2 * R.C_E + T + lnN + 1) + 4 * q + 2 * np.abs(p - q)) / count
    gb = np.where(valid[:, None], gb * R.SLACK + 1e-37, 0.0)
    Tb = -(-B // 256) + 8
    batch = (lb.sum() + (Tb + 1) * U * np.where(valid, np.abs(loss), 0.0).sum() * R.SLACK) / count
    return lb, gb, float(batch)


def mixed_fp32(z, ta, tb, wa, wb, eps, k):
    """the kernel's arithmetic, operation for operation, in NumPy float32 with every product rounded:
    (loss, accuracy, accuracy_topk, gz, row_loss).  The weights (1, 0) / (0, 1) ARE the label-smoothed kernels on one label."""
    one = single_label(np.asarray(ta), np.asarray(tb), wa, wb)
    if one is not None:
        return S.softmax_xent_ls_fp32(z, one, eps, k)
    f = np.float32
    z = np.asarray(z, f)
    _, ia, ib, valid, count = _setup(z, ta, tb, wa, wb)
    B, N = z.shape
    rows = np.arange(B)
    wa, wb, count = f(wa), f(wb), f(count)
    dom = ia if wa >= wb else ib
    zd = z[rows, dom]
    j = np.arange(N)[None, :]
    rank = ((z > zd[:, None]) | ((z == zd[:, None]) & (j < dom[:, None]))).sum(axis=1)
    hitk = (valid & (rank < k)).astype(f)
    hit = (valid & (z.argmax(axis=1) == dom)).astype(f)
    eps32, omeps, q_off = f(eps), f(1.0 - eps), f(eps / N)
    zmix = ((wa * z[rows, ia]).astype(f) + (wb * z[rows, ib]).astype(f)).astype(f)
    m = z.max(axis=1, keepdims=True)
    e = np.exp((z - m).astype(f)).astype(f)
    S_ = R._tree256(R._strided_partials(e))
    lse = (m[:, 0] + np.log(S_).astype(f)).astype(f)
    if eps == 0:
        row_loss = (lse - zmix).astype(f)
    else:
        mean = (R._tree256(R._strided_partials(z)) / f(N)).astype(f)
        row_loss = ((lse - (omeps * zmix).astype(f)).astype(f) - (eps32 * mean).astype(f)).astype(f)
    row_loss = np.where(valid, row_loss, f(0))
    p = (e / S_[:, None]).astype(f)
    w = (np.where(j == ia[:, None], wa, f(0)) + np.where(j == ib[:, None], wb, f(0))).astype(f)
    q = ((omeps * w).astype(f) + q_off).astype(f)
    gz = np.where(valid[:, None], ((p - q).astype(f) / count).astype(f), f(0))
    loss = f(R._tree256(R._strided_partials(row_loss[None, :]))[0] / count)
    acc = f(R._tree256(R._strided_partials(hit[None, :]))[0] / f(B))
    acck = f(R._tree256(R._strided_partials(hitk[None, :]))[0] / f(B))
    return float(loss), float(acc), float(acck), gz, row_loss


# ---- the case grid ----------------------------------------------------------------------------------------------------------
def label_pair(kind, t, N):
    """(ta, tb) from the label array ``t`` of an R case: ``different`` mirrors the class index (N = 1 has one class only)"""
    ta = t.copy()
    tb = (N - 1 - t).astype(np.int32) if kind != 'equal' else t.copy()
    if kind == 'ta_ignored':
        ta[::3] = -1
    elif kind == 'tb_ignored':
        tb[::2] = N + 3
    elif kind == 'both_ignored':
        ta[::2] = -1
        tb[::2] = -1
    return ta, tb


def mix_cases(N, batches=R.XENT_B):
    """(name, z, ta, tb, t, tie expectations or None) for every B, profile and label pair at N classes; ``t`` is the case's own
    label array (the one the tie expectations are stated for)"""
    for name, z, t, expect in R.xent_cases(N):
        if '-first_last-' not in name or len(t) not in batches:
            continue
        for kind in PAIRS:
            ta, tb = label_pair(kind, t, N)
            yield '%s-%s' % (name, kind), z, ta, tb, t, expect


# ---- the mix of a batch -----------------------------------------------------------------------------------------------------
def batch_mix_ref(x, shift, wa, wb, box):
    """(out float64, blended mask, bound) of mixing x [B][C][H][W] with itself shifted by ``shift`` rows; the weights are
    exact inputs.  Where ``blended`` is False the element is a copy: of the partner inside the box, else of x itself."""
    x64 = np.asarray(x, np.float64)
    partner = np.roll(x64, shift, axis=0)
    y0, x0, y1, x1 = box
    inside = np.zeros(x64.shape, bool)
    inside[:, :, y0:y1, x0:x1] = True
    if wb == 0.0:
        out = np.where(inside, partner, x64)
        return out, np.zeros(x64.shape, bool), np.zeros(x64.shape)
    out = np.where(inside, partner, wa * x64 + wb * partner)
    bound = np.where(inside, 0.0, 2 * U * (np.abs(wa * x64) + np.abs(wb * partner)) * R.SLACK + 1e-37)
    return out, ~inside, bound


class MixedClassifier(R.ResNet18Classifier):
    """R.ResNet18Classifier trained against mixed labels: its loss and gz replaced by the float64 mixed reference"""

    def __init__(self, params, tb, lam, label_smoothing=0.0, topk=1, prefix='', train=True):
        super().__init__(params, prefix, train)
        self.tb, self.w, self.label_smoothing, self.topk = tb, weights(lam), label_smoothing, topk

    def forward(self, images, t):
        super().forward(images, t)
        self.loss, self.accuracy, self.accuracy_topk, self.gz = mixed_ref(
            self.logits, t, self.tb, self.w[0], self.w[1], self.label_smoothing, self.topk)[:4]
        return self.loss
