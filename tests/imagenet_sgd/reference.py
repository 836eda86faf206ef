"""Test-side reference of the ImageNet recipe: momentum SGD with weight decay (Chainer 4.1's ``MomentumSGDRule`` behind the
``WeightDecay`` hook) and label-smoothed softmax cross-entropy with top-k accuracy, both in float64 NumPy; fp32 NumPy
restatements of the two kernels; and the first-order error bounds restatement and kernel are both held to.  Everything that
is not new here -- the plain loss, its bound, the case grid, the 256-thread tree -- is tests/imagenet/reference.py's.

u = 2^-24, first order in u, inflated by 1 % (R.SLACK), plus an absolute 1e-37 for underflow, as there.

THE SGD BOUND.  The kernel takes lr, momentum, weight_decay_rate and grad_scale as doubles and rounds each to fp32 once:
a relative u on every hyperparameter.  Per element, with a = g gs, b = wd p, g' = a + b, c = mom v, d = lr g', v' = c - d:
    g'^ = fl(fl(g gs^) + fl(wd^ p))         two roundings on a, two on b, one on the sum:  E_g <= 3u (|a| + |b|)
    v'^ = fl(fl(mom^ v) - fl(lr^ g'^))      two roundings on c, two on d plus lr E_g, one on the difference:
                                            E_v <= 3u (|c| + |d|) + |lr| E_g
    p'^ = fl(p + v'^)                       E_p <= E_v + u |p'|
(three roundings that land on g', two multiplies and one subtraction on v, one addition on p).  A contracted multiply-add
skips the rounding of its product and nothing else, so every term above can only shrink: the bound holds for either code.
Several steps: the kernel's step k starts from its own p^, v^.  The update is linear in (p, v), so an incoming error
(e_p, e_v) goes through it as  E_g += |wd| e_p,  E_v += |mom| e_v,  E_p += e_p  -- `momentum_sgd_bound(..., ep, ev)`.

THE SMOOTHED LOSS BOUND.  With E_lse = u |lse| + (T + c_e + ln N + c_l |log S|) u the error of lse^ from R's derivation,
    loss^ = fl(fl(lse^ - fl(omeps^ z_t)) - fl(eps^ mean^)),    omeps^ = fl(1 - eps), eps^ = fl(eps)
    mean^ = fl(zsum^ / N),  zsum^ the signed sum of the row in the 256-thread tree: every term passes at most
            T = ceil(N / 256) + 8 additions, so |zsum^ - zsum| <= T u sum |z_i|;  N <= 8192 is exact in fp32
      |loss^ - loss| <= E_lse + 2u |(1 - eps) z_t| + u |lse - (1 - eps) z_t|
                        + eps (T mean|z| + |mean z|) u + 2u |eps mean z| + u |loss|
(the one signed sum and the two multiplies the smoothing adds; a contracted multiply-add again only removes a rounding).
    q_off^ = fl(eps / N) (one rounding of the double quotient), q_on^ = fl(omeps^ + q_off^):  |q^ - q| <= 2u q
    gz^ = fl(fl(p^ - q^) / count):  (p (|d| + 2 c_e + T + ln N + 1) + 2 q + 2 |p - q|) u / count
The batch loss is R's: the row losses (cross-entropies, non-negative) in the same tree over B, one division.
eps = 0 takes the kernel's plain expressions, so it is held to R.row_bounds itself.
Hits are integers summed in fp32 (B <= 65536 < 2^24: exact), one division by B: out[1], out[2] are compared exactly."""
import numpy as np

from oracle import model as M
from tests.imagenet import reference as R

U = R.U
EPS = (0.0, 0.1, 0.5)
TOPK = (1, 2, 5)


# ---- momentum SGD -------------------------------------------------------------------------------------------------------------
def momentum_sgd_ref(p, g, v, lr, momentum, weight_decay_rate, grad_scale=1.0):
    """one step in float64: (p', v')"""
    p, g, v = (np.asarray(a, np.float64) for a in (p, g, v))
    gp = g * grad_scale + weight_decay_rate * p
    v = momentum * v - lr * gp
    return p + v, v


def momentum_sgd_fp32(p, g, v, lr, momentum, weight_decay_rate, grad_scale=1.0):
    """the kernel's arithmetic in NumPy float32, every product rounded (no contraction): (p', v')"""
    f = np.float32
    p, g, v = (np.asarray(a, f) for a in (p, g, v))
    gp = ((g * f(grad_scale)).astype(f) + (f(weight_decay_rate) * p).astype(f)).astype(f)
    v = ((f(momentum) * v).astype(f) - (f(lr) * gp).astype(f)).astype(f)
    return (p + v).astype(f), v


def momentum_sgd_bound(p, g, v, lr, momentum, weight_decay_rate, grad_scale=1.0, ep=0.0, ev=0.0):
    """(bound on p', bound on v') per element for one step from (p, g, v), whose p and v carry the errors ep, ev"""
    p, g, v = (np.asarray(a, np.float64) for a in (p, g, v))
    a, b = np.abs(g * grad_scale), np.abs(weight_decay_rate * p)
    gp = g * grad_scale + weight_decay_rate * p
    c, d = np.abs(momentum * v), np.abs(lr * gp)
    p1, _ = momentum_sgd_ref(p, g, v, lr, momentum, weight_decay_rate, grad_scale)
    eg = 3 * U * (a + b) * R.SLACK + abs(weight_decay_rate) * ep
    evn = 3 * U * (c + d) * R.SLACK + abs(lr) * eg + abs(momentum) * ev + 1e-37
    epn = ep + evn + U * np.abs(p1) * R.SLACK + 1e-37
    return epn, evn


class MomentumSGD:
    """``oracle.model.AdamAMSGrad``-shaped: ``chainer.optimizers.MomentumSGD`` + ``WeightDecay`` over a parameter dict, in the
    dtype of the parameters"""

    def __init__(self, params, lr=0.01, momentum=0.9, weight_decay_rate=0.0):
        self.params, self.lr, self.momentum, self.weight_decay_rate, self.t = params, lr, momentum, weight_decay_rate, 0
        self.state = {k: np.zeros_like(v) for k, v in params.items() if M.is_trainable(k)}

    def update(self, grads):
        self.t += 1
        for k, v in self.state.items():
            p = self.params[k]
            g = grads.get(k)
            if g is None:                  # reallocate_cleared_grads -> zeros
                g = np.zeros_like(p)
            gp = g.astype(p.dtype, copy=False) + p.dtype.type(self.weight_decay_rate) * p
            v *= p.dtype.type(self.momentum)
            v -= p.dtype.type(self.lr) * gp
            p += v


# ---- label-smoothed softmax cross-entropy, top-k ------------------------------------------------------------------------------
def softmax_xent_ls_ref(z, t, eps, k):
    """(loss, accuracy, accuracy_topk, gz, row_loss, hit, hitk) in float64.  q = (1 - eps) onehot + eps / N; a label outside
    [0, N) is an ignored row (loss 0, gz 0, no hit); hitk = #{j : z_j > z_t or (z_j == z_t and j < t)} < k"""
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
    zt = z[np.arange(B), tt]
    row_loss = np.where(valid, lse - (1.0 - eps) * zt - eps * z.mean(axis=1), 0.0)
    p = e / S
    q = np.full_like(p, eps / N)
    q[np.arange(B), tt] += 1.0 - eps
    gz = np.where(valid[:, None], (p - q) / count, 0.0)
    hit = valid & (z.argmax(axis=1) == t)
    j = np.arange(N)[None, :]
    rank = ((z > zt[:, None]) | ((z == zt[:, None]) & (j < tt[:, None]))).sum(axis=1)
    hitk = valid & (rank < k)
    return float(row_loss.sum() / count), float(hit.mean()), float(hitk.mean()), gz, row_loss, hit, hitk


def ls_bounds(z, t, eps):
    """per-row loss bound (B,), per-element gz bound (B, N) for an upstream gradient of 1, and the batch-loss bound"""
    if eps == 0:
        return R.row_bounds(z, t)
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
    zt = z[np.arange(B), tt]
    mean = z.mean(axis=1)
    loss = lse - (1.0 - eps) * zt - eps * mean
    T = -(-N // 256) + 8
    lnN = np.log(N)
    e_lse = U * np.abs(lse) + (T + R.C_E + lnN + R.C_L * np.abs(np.log(S[:, 0]))) * U
    lb = e_lse + 2 * U * np.abs((1.0 - eps) * zt) + U * np.abs(lse - (1.0 - eps) * zt) \
        + eps * (T * np.abs(z).mean(axis=1) + np.abs(mean)) * U + 2 * U * np.abs(eps * mean) + U * np.abs(loss)
    lb = np.where(valid, lb * R.SLACK + 1e-37, 0.0)
    q = np.full_like(p, eps / N)
    q[np.arange(B), tt] += 1.0 - eps
    gb = U * (p * (np.abs(d) + 2 * R.C_E + T + lnN + 1) + 2 * q + 2 * np.abs(p - q)) / count
    gb = np.where(valid[:, None], gb * R.SLACK + 1e-37, 0.0)
    Tb = -(-B // 256) + 8
    batch = (lb.sum() + (Tb + 1) * U * np.where(valid, np.abs(loss), 0.0).sum() * R.SLACK) / count
    return lb, gb, float(batch)


def softmax_xent_ls_fp32(z, t, eps, k):
    """the kernel's arithmetic, operation for operation, in NumPy float32 with every product rounded:
    (loss, accuracy, accuracy_topk, gz, row_loss)"""
    f = np.float32
    z = np.asarray(z, f)
    t = np.asarray(t, np.int64)
    B, N = z.shape
    valid = (t >= 0) & (t < N)
    tt = np.where(valid, t, 0)
    zt = z[np.arange(B), tt]
    j = np.arange(N)[None, :]
    rank = ((z > zt[:, None]) | ((z == zt[:, None]) & (j < tt[:, None]))).sum(axis=1)
    hitk = (valid & (rank < k)).astype(f)
    acck = f(R._tree256(R._strided_partials(hitk[None, :]))[0] / f(B))
    if eps == 0:                # the plain expressions
        loss, acc, gz, row_loss = R.softmax_xent_fp32(z, t)
        return loss, acc, float(acck), gz, row_loss
    count = f(max(int(valid.sum()), 1))
    eps32, omeps, q_off = f(eps), f(1.0 - eps), f(eps / N)
    q_on = f(omeps + q_off)
    m = z.max(axis=1, keepdims=True)
    e = np.exp((z - m).astype(f)).astype(f)
    S = R._tree256(R._strided_partials(e))
    lse = (m[:, 0] + np.log(S).astype(f)).astype(f)
    mean = (R._tree256(R._strided_partials(z)) / f(N)).astype(f)
    row_loss = ((lse - (omeps * zt).astype(f)).astype(f) - (eps32 * mean).astype(f)).astype(f)
    row_loss = np.where(valid, row_loss, f(0))
    p = (e / S[:, None]).astype(f)
    q = np.full_like(p, q_off)
    q[np.arange(B), tt] = q_on
    gz = np.where(valid[:, None], ((p - q).astype(f) / count).astype(f), f(0))
    hit = (valid & (z.argmax(axis=1) == t)).astype(f)
    loss = f(R._tree256(R._strided_partials(row_loss[None, :]))[0] / count)
    acc = f(R._tree256(R._strided_partials(hit[None, :]))[0] / f(B))
    return float(loss), float(acc), float(acck), gz, row_loss


def rank_margin_ok(z, t):
    """The rank compares the kernel's INPUTS with z_t as they are (R.argmax_margin_ok): any two fp32 values are ordered exactly,
    so a row's rank is unambiguous when every z_j is either bit-equal to z_t or at least half an ulp (of the smaller of the two
    magnitudes) away from it -- always, for finite fp32; made explicit for the float64 copy the reference uses."""
    z32 = np.asarray(z, np.float32)
    z64 = z32.astype(np.float64)
    t = np.asarray(t, np.int64)
    B, N = z64.shape
    valid = (t >= 0) & (t < N)
    zt = z32[np.arange(B), np.where(valid, t, 0)]
    gap = np.abs(z64 - zt.astype(np.float64)[:, None])[valid]
    ulp = np.spacing(np.minimum(np.abs(z32), np.abs(zt)[:, None])).astype(np.float64)[valid]
    return bool(np.all((gap == 0) | (gap >= ulp * 0.5)))


def topk_tie_case(N=65, B=6, seed=0):
    """(z, t): in every row three columns a < b < c hold the same value, the row's largest, and the label is the middle one.
    One column ahead of the label and nothing greater: rank 1, so k = 1 misses, k = 2 and k = 3 hit."""
    rng = np.random.Generator(np.random.PCG64([N, B, seed]))
    z = rng.standard_normal((B, N)).astype(np.float32)
    t = np.zeros(B, np.int32)
    for r in range(B):
        a, b, c = np.sort(rng.choice(N, 3, replace=False))
        z[r, [a, b, c]] = np.float32(np.abs(z[r]).max() + 1.0)
        t[r] = b
    return z, t


def ls_cases(N):
    """R.xent_cases(N) and, at the sizes that can hold it, the top-k tie case: (name, z, t)"""
    for name, z, t, _ in R.xent_cases(N):
        yield name, z, t
    if N >= 3:
        z, t = topk_tie_case(N)
        yield 'topk-tie-B%d-N%d' % (len(t), N), z, t


class SmoothedClassifier(R.ResNet18Classifier):
    """R.ResNet18Classifier trained on the label-smoothed loss, with the top-k accuracy beside the top-1 one"""

    def __init__(self, params, label_smoothing, topk, prefix='', train=True):
        super().__init__(params, prefix, train)
        self.label_smoothing, self.topk = label_smoothing, topk

    def forward(self, images, t):
        super().forward(images, t)
        self.loss, self.accuracy, self.accuracy_topk, self.gz = softmax_xent_ls_ref(self.logits, t, self.label_smoothing, self.topk)[:4]
        return self.loss
