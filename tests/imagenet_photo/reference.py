"""Test-side reference of the photometric stage (loans_amd/common/datasets/photometric.py, loans_amd/csrc/photo.hip): the
arithmetic in float64 NumPy, a per-element first-order bound on what an fp32 implementation with the documented rounding points
may differ by, the mask of elements that are bit copies, the case grid of the kernel tests, and four wrong implementations
("mutants") the bound has to tell from the right one.

EXACT INPUTS.  The frames, the factors b, c, s, the complements omc, oms (the host rounds them once), the addend, the fill and the
three grey weights as fp32 numbers (0.299f, 0.587f, 0.114f) are fp32 numbers and enter the float64 reference as they are.

THE BOUND (u = 2^-24; every element carries its reference value v and a bound e on |computed - v|; inputs have e = 0).  Each
operation multiplies the incoming error by |factor| and adds its own roundings; terms of second order are kept where they are
one line and the whole is inflated by R.SLACK, plus 1e-37:
    grey^ = fl(w0 r^ + fl(w1 g^ + fl(w2 b^)))       three roundings, each of a partial sum of magnitude <= S = sum w_k |v_k| + E:
        E = sum w_k e_k,   e_grey = E + 3u (S)
    brightness  x' = fl(b x^):          e' = |b| e + u (|b v| + |b| e)
    saturation  t = fl(oms grey^), x' = fl(s x^ + t) (fused):  A = |s| e + |oms| e_grey
                                        e' = A + u (|oms G| + |oms| e_grey) + u (|s v| + |oms G| + A)
    contrast    m^ = fl32(mean in fp64 of grey^):  the mean's error is the mean of the grey errors, plus one fp32 rounding, plus
                the fp64 accumulation (H W additions of relative error 2^-53 each on a sum of |greys|):
                    e_m = mean(e_grey) + u (|m| + mean(e_grey)) + H W 2^-53 mean(|G| + e_grey)
                cm^ = fl(omc m^):       e_cm = |omc| e_m + u (|omc m| + |omc| e_m)
                x' = fl(c x^ + cm^):    e' = |c| e + e_cm + u (|c v| + |omc m| + |c| e + e_cm)
    every clamp is 1-Lipschitz:         e' = e
    addend      x' = fl(x^ + a):        e' = e + u (|v + a| + e)
An operation whose factor is exactly 1 is skipped: value and error go through unchanged.  A contracted or uncontracted
multiply-add differs from the above only by skipping or adding the rounding of a product that the bound already counts.

BIT COPIES: every element of an image whose three factors are 1 and whose addend is zero (outside its box: the input; a copy), and
every element inside an erase box (the fill)."""
import numpy as np

from loans_amd.common.datasets import photometric as P
from loans_amd.ops import PHOTO_JOB
from tests.imagenet import reference as R

U = R.U
W32 = tuple(float(np.float32(w)) for w in P.GREY)               # the grey weights as the kernel holds them
SHAPES = ((1, 1), (7, 5), (16, 12), (33, 65), (40, 64))
BATCHES = (1, 2, 5)
FACTORS = (0.0, 0.6, 1.0, 1.4)
MUTANTS = ('mean_of_input', 'grey_permuted', 'order_reversed', 'no_clamp')


def _grey(v, e, weights=W32):
    """(G, e_grey) of pixels v [3][H][W] carrying the errors e"""
    G = weights[0] * v[0] + weights[1] * v[1] + weights[2] * v[2]
    E = weights[0] * e[0] + weights[1] * e[1] + weights[2] * e[2]
    S = weights[0] * np.abs(v[0]) + weights[1] * np.abs(v[1]) + weights[2] * np.abs(v[2]) + E
    return G, E + 3 * U * S


def photo_ref(frames, jobs, mutant=None):
    """(out float64, copies mask, bound) of the stage on frames [B][3][H][W] under the ``PHOTO_JOB`` table ``jobs``.  ``mutant``:
    one of MUTANTS -- the same in float64 with that mistake built in (its bound is meaningless)."""
    x = np.asarray(frames, np.float64)
    B, C, H, W = x.shape
    assert C == 3 and len(jobs) == B
    out, bound, copies = x.copy(), np.zeros(x.shape), np.zeros(x.shape, bool)
    clamp = (lambda a: a) if mutant == 'no_clamp' else (lambda a: np.clip(a, 0.0, 1.0))
    weights = (W32[1], W32[2], W32[0]) if mutant == 'grey_permuted' else W32
    for n, j in enumerate(jobs):
        v, e = x[n].copy(), np.zeros(x[n].shape)
        b, c, s, omc, oms = (float(j[k]) for k in ('b', 'c', 's', 'omc', 'oms'))
        order = P.ORDERS[int(j['order'])]
        for op in (order[::-1] if mutant == 'order_reversed' else order):
            if op == P.BRIGHTNESS and b != 1.0:
                e = abs(b) * e + U * (np.abs(b * v) + abs(b) * e)
                v = clamp(b * v)
            elif op == P.SATURATION and s != 1.0:
                G, eg = _grey(v, e, weights)
                A = abs(s) * e + abs(oms) * eg[None]
                e = A + U * (np.abs(oms * G) + abs(oms) * eg)[None] + U * (np.abs(s * v) + np.abs(oms * G)[None] + A)
                v = clamp(s * v + (oms * G)[None])
            elif op == P.CONTRAST and c != 1.0:
                G, eg = _grey(x[n], np.zeros(x[n].shape), weights) if mutant == 'mean_of_input' else _grey(v, e, weights)
                m = G.mean()
                e_m = eg.mean() + U * (abs(m) + eg.mean()) + H * W * 2.0 ** -53 * (np.abs(G) + eg).mean()
                e_cm = abs(omc) * e_m + U * (abs(omc * m) + abs(omc) * e_m)
                e = abs(c) * e + e_cm + U * (np.abs(c * v) + abs(omc * m) + abs(c) * e + e_cm)
                v = clamp(c * v + omc * m)
        jitter = b != 1.0 or c != 1.0 or s != 1.0
        add = j['add'].astype(np.float64)
        if add.any():
            v = v + add[:, None, None]
            e = e + U * (np.abs(v) + e)
        copy = np.full(v.shape, not jitter and not add.any())
        y0, x0, y1, x1 = (int(j[k]) for k in ('y0', 'x0', 'y1', 'x1'))
        if y1 > y0 and x1 > x0:
            v[:, y0:y1, x0:x1] = j['fill'].astype(np.float64)[:, None, None]
            copy[:, y0:y1, x0:x1] = True
        out[n], copies[n] = v, copy
        bound[n] = np.where(copy, 0.0, e * R.SLACK + 1e-37)
    return out, copies, bound


def frames(B, H, W, seed=0):
    """[0, 1] pixels like the feed's, with negatives, values above 1, a zero and tiny magnitudes mixed in"""
    rng = np.random.RandomState(1000 * B + 10 * H + W + seed)
    x = rng.rand(B, 3, H, W).astype(np.float32)
    flat = x.reshape(-1)
    flat[::7] *= -1
    flat[::11] *= 3
    flat[::13] *= 1e-30
    flat[0] = 0.0
    return x


def boxes(H, W):
    """empty (twice: no rows, no columns), the whole frame, a single pixel, one box on each edge, and one whose left and right
    edges split a 16-byte unit (columns 1 .. 6 where the frame has them)"""
    y, x = H // 2, W // 2
    found = [(0, 0, 0, 0), (0, x, H, x), (0, 0, H, W), (y, x, y + 1, x + 1),
             (0, W // 3, max(1, H // 2), max(W // 3 + 1, 2 * W // 3)),          # top
             (H // 2, W // 3, H, max(W // 3 + 1, 2 * W // 3)),                  # bottom
             (H // 3, 0, max(H // 3 + 1, 2 * H // 3), max(1, W // 2)),          # left
             (H // 3, W // 2, max(H // 3 + 1, 2 * H // 3), W),                  # right
             (0, min(1, W - 1), max(1, H - 1), min(6, W))]                      # splits units
    return sorted(set(found))


def case_jobs(B, H, W, seed=0):
    """job tables for a batch of B images of H x W: together they cover all six orders with every factor triple out of FACTORS
    somewhere (the triple (1, 1, 1) among them), zero and non-zero addends and every box of ``boxes``"""
    triples = [(b, c, s) for b in FACTORS for c in FACTORS for s in FACTORS]            # 64, (1, 1, 1) among them
    bx = boxes(H, W)
    tables = []
    k = seed
    for t in range(0, len(triples) * 6, B):
        jobs = np.zeros(B, PHOTO_JOB)
        for n in range(B):
            i = t + n
            b, c, s = triples[i % len(triples)]
            order = (i // len(triples)) % 6
            add = (0.0, 0.0, 0.0) if k % 3 else (0.03, -0.02, 0.0 if k % 2 else 0.01)
            jobs[n] = P.make_job(b, c, s, order, add, bx[k % len(bx)], (0.485, 0.456, 0.406) if k % 5 else (0.0, 1.0, -0.25))
            k += 1
        tables.append(jobs)
    return tables


def fast_jobs(B, H, W):
    """a smaller set for the big shapes: a few tables that keep contrast on in the first, middle and last position of the order"""
    bx = boxes(H, W)
    picks = [(0.6, 1.4, 0.6, 0), (1.4, 0.6, 1.0, 3), (1.0, 1.4, 1.4, 5), (0.6, 0.6, 1.4, 4), (1.0, 1.0, 1.0, 0)]
    jobs = np.zeros(B, PHOTO_JOB)
    for n in range(B):
        b, c, s, order = picks[n % len(picks)]
        jobs[n] = P.make_job(b, c, s, order, (0.03, -0.02, 0.01) if n % 2 else (0, 0, 0), bx[(n + 4) % len(bx)])
    return jobs
