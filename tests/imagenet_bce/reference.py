"""Test-side reference of the sigmoid binary cross-entropy of the ImageNet recipe (loans_amd/csrc/classify.hip,
sigmoid_bce_rows_kernel): the loss in float64 NumPy, an fp32 NumPy restatement of the kernel, the first-order bound both are held
to, and the case grid.  What is not new here is tests/imagenet/reference.py's (R) and tests/imagenet_mix/reference.py's (X).

THE LOSS.  The fp32 weights wa, wb, the fp32 constants omeps^ = fl(1 - eps), q_off^ = fl(eps / N) the launcher hands the kernel,
and the fp32 threshold are EXACT inputs.  With w_i = wa [i == ta] + wb [i == tb] (ta == tb: wa + wb on that class)
    q_i = omeps^ w_i + q_off^,    then q_i = [q_i > thresh] where a threshold is given (strictly greater)
    e_i = exp(-|z_i|),   l_i = max(z_i, 0) - z_i q_i + log1p(e_i),   s_i = z_i >= 0 ? 1 / (1 + e_i) : e_i / (1 + e_i)
    row_loss = sum_i l_i,   gz_i = (s_i - q_i) / denom,   loss = sum_b row_loss_b / denom
    denom = count N (the mean over classes: torch's binary_cross_entropy_with_logits) or count (sum_classes)
A row counts when both labels lie in [0, N); the weights (1, 0) / (0, 1) are the one-label loss on ta / on tb, where the label
of weight zero is not read and does not decide whether a row counts.  Hits are X's: against ta if wa >= wb, else tb.

THE BOUND (u = 2^-24, first order, inflated by R.SLACK; T = ceil(N / 256) + 8 adds on the longest path of the row tree, as in R).
    e^ = expf(-|z|)             the argument is exact: relative c_e u, c_e = R.C_E
    L^ = log1pf(e^)             d log1p(e) = de / (1 + e), and e / (1 + e) <= log1p(e):  |L^ - L| <= (c_e + c_1p) u L.
                                c_1p = 4: the HIP math API reference's table of single precision device functions gives log1pf a
                                maximum error of 1 ulp (= 2u, as for expf), and glibc's log1pf behind NumPy's float32 log1p is a
                                1-ulp function too; two ulps are budgeted so that either side may be the one compared, as for c_e
    q^ = fl(fl(omeps^ w^) + q_off^), w^ = fl(wa + wb) where ta == tb: |q^ - q| <= c_q u q, c_q = 4 (X's count of roundings);
                                with a threshold q^ is 0 or 1 and c_q = 0 (see THE THRESHOLD)
    l^ = fl(fl(max(z, 0) - fl(z q^)) + L^)
      |l^ - l| <= u ((c_q + 1) |z q| + |max(z, 0) - z q| + (c_e + c_1p) L + |l|)  =: E_i
    row_loss^ = the tree over l^:   |row_loss^ - row_loss| <= sum_i E_i + T u sum_i |l_i| + N 2^-126
      (every l_i is non-negative for q in [0, 1]; the last term lets each e_i, L_i below the smallest normal number be flushed)
    s^ = fl(num^ / fl(1 + e^)), num^ = 1 or e^:  relative (c_e + 2) u (d s / s <= d e / e on either branch, two roundings)
    denom^ = fl(count N): the integer product is at most 2^29 and is rounded to fp32 ONCE (count and N are exact): relative u
    gz^ = fl(fl(s^ - q^) / denom^):   |gz^ - gz| <= u (s (c_e + 2) + c_q q + 3 |s - q|) / denom    (+ 1e-37: flushed tails)
    loss^ = fl(tree_b(row_loss^) / denom^): (sum_b bound_b + (Tb + 2) u sum_b |row_loss_b|) / denom,  Tb = ceil(B / 256) + 8
A contracted multiply-add (z q, omeps^ w) skips the rounding of its product and nothing else: the bound holds for either code.
Since |s - q| <= 1 and rounding is monotone, |gz^| <= fl(1 / denom^) in fp32 for every finite z: `|gz| denom <= 1'.

THE THRESHOLD.  The comparison q > thresh is exact on both sides, so the 0 / 1 target of the kernel is the reference's unless the
roundings of q^ carry it across the threshold.  The kernel's q^ is one of two numbers -- the product rounded or contracted into
the add -- and ``threshold_ambiguous`` compares the reference's comparison with both: a case where they disagree anywhere would
have to be left out of the bound checks.  ``near_threshold`` is the first-order cover of the same thing, |q^ - thresh| <= 8u q
with q^ != q.  It names one configuration of the grid, N = 2, eps = 0.1, weights (0.5, 0.5) on two different labels,
thresh = 0.5: there q = 0.4999999888..., both roundings of it are 0.5 exactly, and all three are `not greater': the 0 / 1 targets
agree, nothing is left out, and the bound checks run on it like on every other case.  (thresh = 0.5 at eps = 0 with the weights
(0.5, 0.5) is q^ = q = 0.5 exactly: no rounding, both targets 0.)"""
import numpy as np

from tests.imagenet import reference as R
from tests.imagenet_mix import reference as X

U = R.U
C_1P = 4.0
TINY = 2.0 ** -126
BCE_N = (1, 2, 255, 256, 257, 1000)
BCE_B = (1, 5, 257)
BCE_EPS = (0.0, 0.1)
THRESH = (None, 0.2, 0.5)
EXTREMES = 'extremes'


def thresh32(thresh):
    """the threshold as the entry takes it (a float argument), or None"""
    return None if thresh is None else float(np.float32(thresh))


class Logits:
    """what depends on the logits alone, in float64 and in the kernel's fp32 arithmetic; the functions below take an array or this"""

    def __init__(self, z):
        f = np.float32
        self.z32 = np.asarray(z, f)
        self.z = self.z32.astype(np.float64)
        self.B, self.N = self.z.shape
        self.e = np.exp(-np.abs(self.z))
        self.L = np.log1p(self.e)
        self.relu = np.maximum(self.z, 0.0)
        self.s = np.where(self.z >= 0, 1.0, self.e) / (1.0 + self.e)
        self.e32 = np.exp(-np.abs(self.z32)).astype(f)
        self.L32 = np.log1p(self.e32).astype(f)
        self.relu32 = np.maximum(self.z32, f(0))
        self.s32 = (np.where(self.z32 >= 0, f(1), self.e32) / (f(1) + self.e32).astype(f)).astype(f)
        self._hits, self._parts = {}, None

    def hits(self, dom, valid, k):
        """(hit, hitk) of the rows that count against the label array ``dom``: R's argmax and X's rank, on the inputs as they are"""
        key = (dom.tobytes(), valid.tobytes(), k)
        if key not in self._hits:
            rows = np.arange(self.B)
            zd = self.z[rows, dom]
            j = np.arange(self.N)[None, :]
            rank = ((self.z > zd[:, None]) | ((self.z == zd[:, None]) & (j < dom[:, None]))).sum(axis=1)
            self._hits[key] = valid & (self.z.argmax(axis=1) == dom), valid & (rank < k)
        return self._hits[key]


def _logits(z):
    return z if isinstance(z, Logits) else Logits(z)


def _labels(N, ta, tb, wa, wb):
    """(ia, ib, valid, count): an index for every row, the rows that count and their number; at the one-label weights the array of
    weight zero is replaced by the other one, as the launcher does"""
    ta, tb = np.asarray(ta, np.int64), np.asarray(tb, np.int64)
    one = X.single_label(ta, tb, wa, wb)
    if one is not None:
        ta = tb = one
    va, vb = (ta >= 0) & (ta < N), (tb >= 0) & (tb < N)
    valid = va & vb
    return np.where(va, ta, 0), np.where(vb, tb, 0), valid, max(int(valid.sum()), 1)


def _denom(count, N, sum_classes):
    return count if sum_classes else count * N


def target64(N, ia, ib, wa, wb, eps, thresh):
    """the (B, N) target in float64 from the fp32 constants taken as exact"""
    omeps, q_off = float(np.float32(1.0 - eps)), float(np.float32(eps / N))
    rows = np.arange(len(ia))
    w = np.zeros((len(ia), N))
    w[rows, ia] = wa
    w[rows, ib] += wb
    q = omeps * w + q_off
    return q if thresh is None else (q > thresh32(thresh)).astype(np.float64)


def target32(N, ia, ib, wa, wb, eps, thresh, fused=False):
    """the kernel's target: the product rounded, or (``fused``) contracted into the add"""
    f = np.float32
    omeps, q_off = f(1.0 - eps), f(eps / N)
    rows = np.arange(len(ia))
    w = np.zeros((len(ia), N), f)
    w[rows, ia] = f(wa)
    w[rows, ib] += f(wb)                    # fl(wa + wb) where ta == tb, else 0 + wb
    if fused:       # (the product of two fp32 numbers is exact in float64; the sum is then rounded to fp32)
        q = (omeps.astype(np.float64) * w.astype(np.float64) + np.float64(q_off)).astype(f)
    else:
        q = ((omeps * w).astype(f) + q_off).astype(f)
    return q if thresh is None else (q > f(thresh)).astype(f)


def _target_kinds(N, ta, tb, wa, wb):
    """(ia, ib) of one row that counts per kind of row -- two different labels, one label twice: the values a target takes
    depend on nothing else"""
    ia, ib, valid, _ = _labels(N, ta, tb, wa, wb)
    keep = [rows[0] for rows in (np.flatnonzero(valid & (ia != ib)), np.flatnonzero(valid & (ia == ib))) if len(rows)]
    return ia[keep], ib[keep]


def threshold_ambiguous(N, ta, tb, wa, wb, eps, thresh):
    """whether a rounding of q^ carries an element of a row that counts across the threshold (see THE THRESHOLD)"""
    if thresh is None:
        return False
    ia, ib = _target_kinds(N, ta, tb, wa, wb)
    q = target64(N, ia, ib, wa, wb, eps, thresh)
    return any(not np.array_equal(q, target32(N, ia, ib, wa, wb, eps, thresh, fused).astype(np.float64)) for fused in (False, True))


def near_threshold(N, ta, tb, wa, wb, eps, thresh):
    """the number of target values (of one row per kind) whose rounding lies within 8u q of the threshold without being q itself"""
    if thresh is None:
        return 0
    ia, ib = _target_kinds(N, ta, tb, wa, wb)
    q = target64(N, ia, ib, wa, wb, eps, None)
    found = 0
    for fused in (False, True):
        q32 = target32(N, ia, ib, wa, wb, eps, None, fused).astype(np.float64)
        found = max(found, int(((np.abs(q32 - thresh32(thresh)) <= 8 * U * q) & (q32 != q)).sum()))
    return found


def _parts(c, ta, tb, wa, wb, eps, thresh):
    """what does not depend on the denominator, kept for the next call on the same case: labels, both targets, the elements' losses"""
    key = (np.asarray(ta).tobytes(), np.asarray(tb).tobytes(), wa, wb, eps, thresh)
    if c._parts is None or c._parts[0] != key:
        f = np.float32
        ia, ib, valid, count = _labels(c.N, ta, tb, wa, wb)
        q = target64(c.N, ia, ib, wa, wb, eps, thresh)
        zq = c.z * q
        q32 = target32(c.N, ia, ib, wa, wb, eps, thresh)
        l32 = ((c.relu32 - (c.z32 * q32).astype(f)).astype(f) + c.L32).astype(f)
        row32 = np.where(valid, R._tree256(R._strided_partials(l32)), f(0))
        c._parts = key, (ia, ib, valid, count, q, zq, c.relu - zq + c.L, q32, row32)
    return c._parts[1]


def bce_ref(z, ta, tb, wa, wb, eps, k, thresh=None, sum_classes=False):
    """(loss, accuracy, accuracy_topk, gz, row_loss, hit, hitk) in float64"""
    c = _logits(z)
    ia, ib, valid, count, q, _, l, _, _ = _parts(c, ta, tb, wa, wb, eps, thresh)
    denom = _denom(count, c.N, sum_classes)
    row_loss = np.where(valid, l.sum(axis=1), 0.0)
    gz = np.where(valid[:, None], (c.s - q) / denom, 0.0)
    hit, hitk = c.hits(ia if wa >= wb else ib, valid, k)
    return float(row_loss.sum() / denom), float(hit.mean()), float(hitk.mean()), gz, row_loss, hit, hitk


def bce_bounds(z, ta, tb, wa, wb, eps, thresh=None, sum_classes=False):
    """per-row loss bound (B,), per-element gz bound (B, N) for an upstream gradient of 1, and the batch-loss bound"""
    c = _logits(z)
    ia, ib, valid, count, q, zq, l, _, _ = _parts(c, ta, tb, wa, wb, eps, thresh)
    denom = _denom(count, c.N, sum_classes)
    c_q = 4.0 if thresh is None else 0.0
    T = -(-c.N // 256) + 8
    el = U * ((c_q + 1) * np.abs(zq) + np.abs(c.relu - zq) + (R.C_E + C_1P) * c.L + np.abs(l))
    lb = el.sum(axis=1) + T * U * np.abs(l).sum(axis=1) + c.N * TINY
    lb = np.where(valid, lb * R.SLACK + 1e-37, 0.0)
    gb = U * (c.s * (R.C_E + 2) + c_q * q + 3 * np.abs(c.s - q)) / denom
    gb = np.where(valid[:, None], gb * R.SLACK + 1e-37, 0.0)
    Tb = -(-c.B // 256) + 8
    batch = (lb.sum() + (Tb + 2) * U * np.where(valid, np.abs(l.sum(axis=1)), 0.0).sum() * R.SLACK) / denom
    return lb, gb, float(batch)


def bce_fp32(z, ta, tb, wa, wb, eps, k, thresh=None, sum_classes=False):
    """the kernel's arithmetic, operation for operation, in NumPy float32 with every product rounded:
    (loss, accuracy, accuracy_topk, gz, row_loss)"""
    f = np.float32
    c = _logits(z)
    # (_parts: q = target32, l = fl(fl(relu - fl(z q)) + L), row_loss = the tree over l)
    ia, ib, valid, count, _, _, _, q, row_loss = _parts(c, ta, tb, wa, wb, eps, thresh)
    denom = f(_denom(count, c.N, sum_classes))              # one rounding of the integer
    gz = np.where(valid[:, None], ((c.s32 - q).astype(f) / denom).astype(f), f(0))
    hit, hitk = c.hits(ia if f(wa) >= f(wb) else ib, valid, k)
    loss = f(R._tree256(R._strided_partials(row_loss[None, :]))[0] / denom)
    acc = f(R._tree256(R._strided_partials(hit.astype(f)[None, :]))[0] / f(c.B))
    acck = f(R._tree256(R._strided_partials(hitk.astype(f)[None, :]))[0] / f(c.B))
    return float(loss), float(acc), float(acck), gz, row_loss


def gz_limit(count, N, sum_classes):
    """fl(1 / denom^) in fp32: what no |gz| exceeds, whatever the logits"""
    return float(np.float32(1) / np.float32(_denom(count, N, sum_classes)))


# ---- the case grid ----------------------------------------------------------------------------------------------------------
def extreme_logits(B, N):
    """ordinary logits with +-100 and +-1e4 among them: exp(z) overflows fp32 at 100 and float64 at 1e4"""
    rng = np.random.Generator(np.random.PCG64([N, B, 99]))
    z = rng.standard_normal((B, N))
    flat = z.reshape(-1)
    for start, step, value in ((0, 5, 100.0), (1, 7, -100.0), (2, 11, 1e4), (3, 13, -1e4)):
        flat[start::step] = value
    return z.astype(np.float32)


def bce_cases(N, batches=BCE_B):
    """(name, Logits, ta, tb, t, tie expectations or None, extremes?) for every B, profile (R's and the extremes) and label pair"""
    last = None
    for name, z, ta, tb, t, expect in X.mix_cases(N, batches):
        if last is None or last[0] is not z:
            last = (z, Logits(z))
        yield name, last[1], ta, tb, t, expect, False
    for B in batches:
        c = Logits(extreme_logits(B, N))
        t = R.make_labels('first_last', B, N, None)
        for kind in X.PAIRS:
            ta, tb = X.label_pair(kind, t, N)
            yield '%s-first_last-B%d-N%d-%s' % (EXTREMES, B, N, kind), c, ta, tb, t, None, True


def profiles(N):
    """the number of logit profiles at N classes"""
    return (len(R.PROFILES) if N >= 2 else len(R.PROFILES) - 1) + 1


def lds_limit_case():
    """the one case at the LDS limit: (Logits, ta, tb) at N = 8192, B = 2"""
    N, B = 8192, 2
    rng = np.random.Generator(np.random.PCG64([N, B, 7]))
    z = (3.0 * rng.standard_normal((B, N))).astype(np.float32)
    ta = np.array([0, N - 1], np.int32)
    return Logits(z), ta, (N - 1 - ta).astype(np.int32)


# ---- the classifier oracle ---------------------------------------------------------------------------------------------------
class BceClassifier(R.ResNet18Classifier):
    """R.ResNet18Classifier trained with the sigmoid binary cross-entropy: its loss and gz replaced by the float64 reference.
    ``tb`` None: plain labels."""

    def __init__(self, params, tb=None, lam=1.0, label_smoothing=0.0, topk=1, thresh=None, sum_classes=False, prefix='', train=True):
        super().__init__(params, prefix, train)
        self.tb, self.w, self.label_smoothing, self.topk = tb, X.weights(lam), label_smoothing, topk
        self.thresh, self.sum_classes = thresh, sum_classes

    def forward(self, images, t):
        super().forward(images, t)
        self.loss, self.accuracy, self.accuracy_topk, self.gz = bce_ref(
            self.logits, t, t if self.tb is None else self.tb, self.w[0], self.w[1], self.label_smoothing, self.topk,
            self.thresh, self.sum_classes)[:4]
        return self.loss
