"""Test-side reference of knowledge distillation in the ImageNet recipe (loans_amd/csrc/classify.hip, softmax_distill_rows_kernel):
the loss in float64 NumPy, an fp32 NumPy restatement of the kernel, the first-order bound both are held to, and the case grid.
What is not new here is tests/imagenet/reference.py's (R), tests/imagenet_mix/reference.py's (X) and tests/imagenet_bce/reference.py's (Q).

THE LOSS.  EXACT inputs: the fp32 logits z, zt, the fp32 weights wa, wb, and the fp32 constants the launcher rounds once on the host,
invT^ = fl(1 / T), oma^ = fl(1 - alpha), alpha^ = fl(alpha), T2^ = fl(T T), aT^ = fl(alpha T) (all of them exact at the grid's powers
of two).  The SCALED logits zs = fl(z invT^), zts = fl(zt invT^) are fp32 numbers too, by the kernel's definition: the product is
rounded and never contracted, so the reference takes them as exact inputs as well.  Then, per row,
    y = softmax(z), s = softmax(zs), p = softmax(zts),      hard = X's two-label row loss, q = X's target
    kl = sum_i p_i ((zts_i - lse(zts)) - (zs_i - lse(zs))),     row_kl = T2^ kl,     row_loss = oma^ hard + alpha^ row_kl
    gz_i = (oma^ (y_i - q_i) + aT^ (s_i - p_i)) / count
(Hinton's convention: torch's kl_div(log_softmax(z / T), softmax(zt / T), 'batchmean') T T.)  A row counts when both labels lie in
[0, N); the weights (1, 0) / (0, 1) are the one-label loss, where the label of weight zero is not read.  Hits are X's, on z; the
teacher's hit is the argmax of zt (first index on a tie) against the dominant label.

THE BOUND (u = 2^-24, first order, inflated by R.SLACK; T_ = ceil(N / 256) + 8 adds on the longest path of the row tree, c_e = R.C_E,
c_l = R.C_L, as in R).  For either scaled row, with m its exact maximum (the scaled maximum: rounding is monotone) and d = fl(x - m):
    e^ = expf(d^)                relative (|d| + c_e) u
    S^ = tree(e^)                relative (T_ + c_e + ln N) u                                   (R: sum_i p_i |d_i| <= ln N)
    L^ = logf(S^)                |L^ - L| <= (c_l |L| + T_ + c_e + ln N) u  =: E_L
    a^ = fl(d^ - L^)             |a^ - a| <= u (|d| + |a|) + E_L                                 a = log p (teacher), b = log s
    D^ = fl(a^ - b^)             |D^ - D| <= err(a) + err(b) + u |D|
    p^ = fl(e^ / S^)             relative r_p = (|d| + 2 c_e + T_ + ln N + 1) u                  (R's softmax)
    t^ = fl(p^ D^)               |t^ - t| <= p err(D) + (r_p + u) p |D|                          (contracted into the sum: one rounding fewer)
    kl^ = tree(t^)               |kl^ - kl| <= sum_i err(t_i) + T_ u sum_i |t_i| + N 2^-126 (1 + max |D|)  =: E_kl
                                 (terms of either sign: the tree's roundings are held against sum |t|; the last term lets each p_i
                                 below the smallest normal number be flushed)
    row_kl^ = fl(T2^ kl^)        |.| <= T2 E_kl + u |row_kl|  =: E_rk
    row_loss^ = fl(fl(oma^ hard^) + fl(alpha^ row_kl^))
                                 |.| <= oma E_hard + alpha E_rk + u (|oma hard| + |alpha row_kl|) + u |row_loss|
                                 E_hard is X.mixed_bounds': the hard part is the mix kernel's expressions, operation for operation
    h^ = fl(y^ - q^)             |h^ - h| <= u (y (|d| + 2 c_e + T_ + ln N + 1) + 4 q + |y - q|)  =: E_h      (X's count of roundings)
    f^ = fl(s^ - p^)             |f^ - f| <= s r_s + p r_p + u |s - p|  =: E_f
    gz^ = fl(fl(fl(oma^ h^) + fl(aT^ f^)) / count)
                                 |.| <= (oma E_h + aT E_f + u (|oma h| + |aT f|) + u |oma h + aT f|) / count + u |gz|
    out[0]^, out[3]^             R's tree over the rows: (sum_b bound_b + (Tb + 1) u sum_b |row_b|) / count, Tb = ceil(B / 256) + 8
A contracted multiply-add skips the rounding of its product and nothing else: the bound holds for either code.  Hits are compared
exactly.  At alpha == 0 the entry IS the mix entry (its bits) and the teacher's outputs are zeros.

THE SPLIT.  What depends on (student, labels, weights, eps) -- ``Hard`` -- and what depends on (student, teacher, T) -- ``Soft`` -- are
computed once each and combined per alpha by ``combine`` / ``combine_fp32``, which use nothing but + - * / abs and sums: they run on
NumPy arrays and, unchanged, on float64 device tensors (the GPU test keeps the pieces on the device)."""
import numpy as np

from tests.imagenet import reference as R
from tests.imagenet_bce import reference as Q
from tests.imagenet_mix import reference as X

U = R.U
TINY = 2.0 ** -126
DISTILL_N = (1, 2, 255, 256, 257, 1000)
DISTILL_B = (1, 5, 257)
DISTILL_EPS = (0.0, 0.1)
ALPHAS = (0.5, 1.0)
TEMPERATURES = (0.5, 1.0, 4.0)
EXTREMES = Q.EXTREMES
PROFILES = R.PROFILES + (EXTREMES,)
f32 = np.float32


def constants(alpha, T):
    """(invT^, oma^, alpha^, T2^, aT^) as the launcher rounds them, as Python floats"""
    return (float(f32(1.0 / T)), float(f32(1.0 - alpha)), float(f32(alpha)), float(f32(T * T)), float(f32(alpha * T)))


def _T(N):
    return -(-N // 256) + 8


class Scaled:
    """softmax and log-softmax of the fp32 rows x in float64 and in the kernel's fp32 arithmetic"""

    def __init__(self, x32):
        self.x32 = np.ascontiguousarray(x32, f32)
        x = self.x32.astype(np.float64)
        self.B, self.N = x.shape
        m = x.max(axis=1, keepdims=True)
        self.d = x - m
        e = np.exp(self.d)
        S = e.sum(axis=1, keepdims=True)
        self.p = e / S
        self.L = np.log(S)
        self.logp = self.d - self.L
        self.r = (np.abs(self.d) + 2 * R.C_E + _T(self.N) + np.log(self.N) + 1) * U             # relative error of p^
        self.E_L = (R.C_L * np.abs(self.L) + _T(self.N) + R.C_E + np.log(self.N)) * U
        # fp32
        m32 = self.x32.max(axis=1, keepdims=True)
        self.d32 = (self.x32 - m32).astype(f32)
        self.e32 = np.exp(self.d32).astype(f32)
        self.S32 = R._tree256(R._strided_partials(self.e32))
        self.L32 = np.log(self.S32).astype(f32)
        self.m32 = m32[:, 0]
        self.p32 = (self.e32 / self.S32[:, None]).astype(f32)


class Logits:
    """a row set with its softmax at every scale asked for, kept"""

    def __init__(self, z):
        self.z32 = np.ascontiguousarray(z, f32)
        self.B, self.N = self.z32.shape
        self._scaled = {}

    def at(self, invT):
        """the rows times invT^, the product rounded to fp32"""
        if invT not in self._scaled:
            self._scaled[invT] = Scaled(self.z32 if invT == 1.0 else (self.z32 * f32(invT)).astype(f32))
        return self._scaled[invT]


def _labels(N, ta, tb, wa, wb):
    """(ta, tb) with the array of weight zero replaced by the other one at the one-label weights, as the launcher does"""
    ta, tb = np.asarray(ta, np.int64), np.asarray(tb, np.int64)
    one = X.single_label(ta, tb, wa, wb)
    return (one, one) if one is not None else (ta, tb)


class Hard:
    """what depends on (student, labels, weights, eps, k): X's two-label loss with its bound, h = y - q with its bound, the hits,
    and the same in the mix kernel's fp32 expressions (the general ones, also at the one-label weights: what the distill kernel runs)"""

    def __init__(self, c, ta, tb, wa, wb, eps, k):
        N, B = c.N, c.B
        y = c.at(1.0)
        ta, tb = _labels(N, ta, tb, wa, wb)
        ref = X.mixed_ref(c.z32, ta, tb, wa, wb, eps, k)
        self.hit, self.hitk = ref[5], ref[6]
        va, vb = (ta >= 0) & (ta < N), (tb >= 0) & (tb < N)
        self.valid = va & vb
        self.count = max(int(self.valid.sum()), 1)
        self.v = self.valid.astype(np.float64)
        ia, ib = np.where(va, ta, 0), np.where(vb, tb, 0)
        self.dom = ia if f32(wa) >= f32(wb) else ib
        self.loss = ref[4]                                                  # (B,), zero on rows that do not count
        self.E_loss = X.mixed_bounds(c.z32, ta, tb, wa, wb, eps)[0]         # (B,), slack included, zero on rows that do not count
        rows = np.arange(B)
        w = np.zeros((B, N))
        np.add.at(w, (rows, ia), wa)
        np.add.at(w, (rows, ib), wb)
        q = (1.0 - eps) * w + eps / N
        self.h = (y.p - q) * self.v[:, None]
        self.E_h = U * (y.p * y.r / U + 4 * q + np.abs(y.p - q)) * self.v[:, None]
        # fp32: softmax_xent_mix_rows_kernel's expressions with every product rounded
        z = c.z32
        fwa, fwb = f32(wa), f32(wb)
        eps32, omeps, q_off = f32(eps), f32(1.0 - eps), f32(eps / N)
        zmix = ((fwa * z[rows, ia]).astype(f32) + (fwb * z[rows, ib]).astype(f32)).astype(f32)
        lse = (y.m32 + y.L32).astype(f32)
        if eps == 0:
            loss32 = (lse - zmix).astype(f32)
        else:
            mean = (R._tree256(R._strided_partials(z)) / f32(N)).astype(f32)
            loss32 = ((lse - (omeps * zmix).astype(f32)).astype(f32) - (eps32 * mean).astype(f32)).astype(f32)
        self.loss32 = np.where(self.valid, loss32, f32(0))
        j = np.arange(N)[None, :]
        w32 = (np.where(j == ia[:, None], fwa, f32(0)) + np.where(j == ib[:, None], fwb, f32(0))).astype(f32)
        q32 = ((omeps * w32).astype(f32) + q_off).astype(f32)
        self.h32 = (y.p32 - q32).astype(f32)


class Soft:
    """what depends on (student, teacher, T): s - p and the row KL with their bounds, the teacher's argmax, and the fp32 restatement"""

    def __init__(self, c, ct, T):
        invT = constants(0.0, T)[0]
        s, p = c.at(invT), ct.at(invT)
        N = c.N
        self.f = s.p - p.p
        self.E_f = s.p * s.r + p.p * p.r + U * np.abs(self.f) + 2 * TINY
        D = p.logp - s.logp
        t = p.p * D
        self.kl = t.sum(axis=1)
        err_D = U * (np.abs(p.d) + np.abs(p.logp)) + p.E_L + U * (np.abs(s.d) + np.abs(s.logp)) + s.E_L + U * np.abs(D)
        err_t = p.p * err_D + (p.r + U) * np.abs(t)
        self.E_kl = err_t.sum(axis=1) + _T(N) * U * np.abs(t).sum(axis=1) + N * TINY * (1 + np.abs(D).max(axis=1))
        self.targmax = ct.z32.argmax(axis=1)
        # fp32
        D32 = ((p.d32 - p.L32[:, None]).astype(f32) - (s.d32 - s.L32[:, None]).astype(f32)).astype(f32)
        self.kl32 = R._tree256(R._strided_partials((p.p32 * D32).astype(f32)))
        self.f32 = (s.p32 - p.p32).astype(f32)


def combine(hard, soft, alpha, T, xp=None):
    """the float64 reference and its bounds of one case from its two halves -> a dict: gz, row_loss, row_kl (arrays), loss, kl
    (batch values), and the bounds gb, lb, kb, bb (batch loss), bkl (batch KL).  ``hard`` / ``soft``: objects with the attributes of
    ``Hard`` / ``Soft`` as NumPy arrays or as float64 device tensors (+ - * / abs and sums only)."""
    _, oma, a, T2, aT = constants(alpha, T)
    v, count = hard.v, hard.count
    row_kl = T2 * soft.kl * v
    E_rk = (T2 * soft.E_kl + U * abs(row_kl)) * v
    row_loss = oma * hard.loss + a * row_kl
    lb = oma * hard.E_loss + ((a * E_rk + U * (abs(oma * hard.loss) + abs(a * row_kl)) + U * abs(row_loss)) * R.SLACK + 1e-37) * v
    kb = (E_rk * R.SLACK + 1e-37) * v
    num = (oma * hard.h + aT * soft.f) * v[:, None]
    gz = num / count
    gb = (((oma * hard.E_h + aT * soft.E_f + U * (abs(oma * hard.h) + abs(aT * soft.f)) + U * abs(num)) / count + U * abs(gz)) * R.SLACK
          + 1e-37) * v[:, None]
    Tb = -(-len(v) // 256) + 8
    bb = (lb.sum() + (Tb + 1) * U * abs(row_loss).sum() * R.SLACK) / count
    bkl = (kb.sum() + (Tb + 1) * U * abs(row_kl).sum() * R.SLACK) / count
    return dict(gz=gz, row_loss=row_loss, row_kl=row_kl, loss=row_loss.sum() / count, kl=row_kl.sum() / count,
                gb=gb, lb=lb, kb=kb, bb=bb, bkl=bkl)


def hits(hard, soft):
    """(hit, hitk, thit) as bool arrays: X's on z, and the teacher's argmax against the dominant label, on rows that count"""
    return hard.hit, hard.hitk, hard.valid & (soft.targmax == hard.dom)


def combine_fp32(hard, soft, alpha, T):
    """the kernel's arithmetic, operation for operation, with every product rounded: gz, row_loss, row_kl, out[0..4]"""
    _, oma, a, T2, aT = (f32(x) for x in constants(alpha, T))
    valid, count = hard.valid, f32(hard.count)
    B = len(valid)
    rk = (T2 * soft.kl32).astype(f32)
    row_loss = ((oma * hard.loss32).astype(f32) + (a * rk).astype(f32)).astype(f32)
    row_loss, rk = np.where(valid, row_loss, f32(0)), np.where(valid, rk, f32(0))
    gz = (((oma * hard.h32).astype(f32) + (aT * soft.f32).astype(f32)).astype(f32) / count).astype(f32)
    gz = np.where(valid[:, None], gz, f32(0))
    hit, hitk, thit = hits(hard, soft)

    def tree(x):
        return R._tree256(R._strided_partials(np.asarray(x, f32)[None, :]))[0]
    out = [f32(tree(row_loss) / count), f32(tree(hit) / f32(B)), f32(tree(hitk) / f32(B)), f32(tree(rk) / count), f32(tree(thit) / f32(B))]
    return dict(gz=gz, row_loss=row_loss, row_kl=rk, out=[float(x) for x in out])


def distill_ref(z, zt, ta, tb, wa, wb, eps, k, alpha, T):
    """the whole loss in float64 from the arrays: a dict with loss, accuracy, accuracy_topk, distill_loss, teacher_accuracy, gz,
    row_loss, row_kl, hit, hitk, thit and the bounds of ``combine``.  alpha == 0: X's mix reference and zeros."""
    c = z if isinstance(z, Logits) else Logits(z)
    ct = zt if isinstance(zt, Logits) else Logits(zt)
    hard, soft = Hard(c, ta, tb, wa, wb, eps, k), Soft(c, ct, T)
    out = combine(hard, soft, alpha, T)
    hit, hitk, thit = hits(hard, soft)
    if alpha == 0:              # the entry does not read the teacher: zeros
        thit = np.zeros_like(thit)
        out.update(row_kl=np.zeros_like(out['row_kl']), kl=0.0, kb=np.zeros_like(out['kb']), bkl=0.0)
    out.update(hit=hit, hitk=hitk, thit=thit, accuracy=float(hit.mean()), accuracy_topk=float(hitk.mean()),
               teacher_accuracy=float(thit.mean()), distill_loss=float(out['kl']), loss=float(out['loss']), valid=hard.valid)
    return out


def distill_fp32(z, zt, ta, tb, wa, wb, eps, k, alpha, T):
    """the kernel's arithmetic from the arrays (``combine_fp32``); alpha == 0: X.mixed_fp32 and zeros, as the entry does"""
    if alpha == 0:
        loss, acc, acck, gz, row_loss = X.mixed_fp32(np.asarray(getattr(z, 'z32', z), f32), ta, tb, wa, wb, eps, k)
        return dict(gz=gz, row_loss=row_loss, row_kl=np.zeros(len(row_loss), f32), out=[loss, acc, acck, 0.0, 0.0])
    c = z if isinstance(z, Logits) else Logits(z)
    ct = zt if isinstance(zt, Logits) else Logits(zt)
    return combine_fp32(Hard(c, ta, tb, wa, wb, eps, k), Soft(c, ct, T), alpha, T)


# ---- the case grid ----------------------------------------------------------------------------------------------------------
def students(N, B):
    """(profile, Logits, t, tie expectations or None) of every profile at (N, B): R's with the first_last labels, and the extremes"""
    for name, z, t, expect in R.xent_cases(N):
        if '-first_last-' in name and len(t) == B:
            yield name.split('-')[0], Logits(z), t, expect
    yield EXTREMES, Logits(Q.extreme_logits(B, N)), R.make_labels('first_last', B, N, None), None


def teachers(N, B):
    """(profile, Logits) of every profile at (N, B), drawn from streams of their own: the teacher's rows are independent of the
    student's.  ``tie``: two exactly equal maxima per row, so the first index decides the teacher's hit."""
    for idx, profile in enumerate(PROFILES):
        rng = np.random.Generator(np.random.PCG64([N, B, idx, 4242]))
        if profile == EXTREMES:
            z = Q.extreme_logits(B, N)[::-1].copy() * f32(0.5)          # +-50 / +-5e3 among ordinary rows, in another order
        else:
            z = R.make_logits(profile, B, N, rng)
        if profile == 'tie':
            if N < 2:
                continue
            a = rng.integers(0, N - 1, B)
            b = np.array([rng.integers(x + 1, N) for x in a])
            top = (np.abs(z).max(axis=1) + 1.0).astype(f32)
            z[np.arange(B), a] = top
            z[np.arange(B), b] = top
        yield profile, Logits(z)


def profiles(N):
    """the number of logit profiles at N classes (N = 1 has no tie)"""
    return len(PROFILES) if N >= 2 else len(PROFILES) - 1


def lds_limit_case():
    """the one case at the LDS limit: (student Logits, teacher Logits, ta, tb) at N = 8192, B = 2"""
    c, ta, tb = Q.lds_limit_case()
    rng = np.random.Generator(np.random.PCG64([8192, 2, 11]))
    return Logits(c.z32), Logits((3.0 * rng.standard_normal((2, 8192))).astype(f32)), ta, tb


# ---- the classifier oracle ---------------------------------------------------------------------------------------------------
class DistilledClassifier(R.ResNet18Classifier):
    """R.ResNet18Classifier trained against a frozen teacher's logits: its loss and gz replaced by the float64 reference.
    ``tb`` None: plain labels."""

    def __init__(self, params, teacher_logits, alpha, temperature, tb=None, lam=1.0, label_smoothing=0.0, topk=1, prefix='', train=True):
        super().__init__(params, prefix, train)
        self.zt, self.alpha, self.temperature = teacher_logits, alpha, temperature
        self.tb, self.w, self.label_smoothing, self.topk = tb, X.weights(lam), label_smoothing, topk

    def forward(self, images, t):
        super().forward(images, t)
        ref = distill_ref(self.logits, self.zt, t, t if self.tb is None else self.tb, self.w[0], self.w[1], self.label_smoothing,
                          self.topk, self.alpha, self.temperature)
        self.loss, self.accuracy, self.accuracy_topk, self.gz = ref['loss'], ref['accuracy'], ref['accuracy_topk'], ref['gz']
        self.distill_loss, self.teacher_accuracy = ref['distill_loss'], ref['teacher_accuracy']
        return self.loss
