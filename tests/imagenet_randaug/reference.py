"""Test-side reference of the RandAugment stage (loans_amd/common/datasets/rand_augment.py, loans_amd/csrc/randaug.hip): the
continuous operations (6 Brightness, 7 Color, 8 Contrast, 9 Sharpness, 12 AutoContrast) in float64 NumPy with a per-element
first-order bound on what an fp32 implementation with the documented rounding points may differ by; the exact NumPy fp32 / integer
form of the others (the gathers, Posterize, Solarize, Equalize), which an implementation has to reproduce bit for bit; the mask of
elements that are bit copies; the case grid of the kernel tests; and seven wrong implementations ("mutants") the checks have to
tell from the right one.

A table may chain layers as long as at most the LAST layer that acts on an image is continuous: the exact layers before it hand on
fp32 numbers, which enter the float64 arithmetic as they are (chains of kernels are checked GPU against GPU).

EXACT INPUTS.  The frames, f, omf = fl32(1 - f), the threshold, the fill, the grey weights (0.299f, 0.587f, 0.114f) and fl32(1 / 13)
are fp32 numbers and enter the float64 reference as they are.

THE BOUND (u = 2^-24; the inputs of the continuous layer are exact; the whole is inflated by R.SLACK, plus 1e-37; every clamp is
1-Lipschitz and adds nothing).
    grey^ = fl(w0 r + fl(w1 g + fl(w2 b))): three roundings of partial sums of magnitude <= S = sum w_k |v_k|:   e_g = 3 u S
    Brightness  fl(f x):                                 e = u |f x|
    Color       t = fl(omf grey^), fl(f x + t) fused:    e_t = |omf| e_g + u (|omf G| + |omf| e_g)
                                                         e = e_t + u (|f x| + |omf G| + e_t)
    Contrast    m^ = fl32(fp64 mean of grey^):           e_m = mean(e_g) + u (|m| + mean(e_g)) + H W 2^-53 mean(|G| + e_g)
                cm^ = fl(omf m^):                        e_cm = |omf| e_m + u (|omf m| + |omf| e_m)
                fl(f x + cm^) fused:                     e = e_cm + u (|f x| + |omf m| + e_cm)
    Sharpness   acc^: seven fp32 additions, each rounding a partial sum of magnitude <= A = sum |neighbour|:  e_a = 7 u A (1 + 7 u)
                t^ = fl(5 x + acc^) fused:               e_t = e_a + u (|5 x| + A + e_a)
                d^ = fl(t^ c13):                         e_d = c13 e_t + u (|T c13| + c13 e_t)
                o^ = fl(omf d^):                         e_o = |omf| e_d + u (|omf D| + |omf| e_d)
                fl(f x + o^) fused:                      e = e_o + u (|f x| + |omf D| + e_o)
    AutoContrast lo, hi are exact (a minimum and a maximum round nothing); fl(hi - lo), fl(1 / .), fl(x - lo), fl(. * s): four
                roundings of relative error u each on the value (x - lo) / (hi - lo):   e = |v| ((1 + u)^4 - 1)
A contracted or uncontracted multiply-add differs from the above only by a rounding the bound already counts.

BIT COPIES: every element of an image whose acting layers are all exact comes out of the exact form and must be reproduced bit for
bit (the mask ``exact``); under Sharpness the border pixels, under AutoContrast a flat channel, are copies too."""
import numpy as np

from loans_amd.common.datasets import rand_augment as RA
from loans_amd.ops import RA_JOB
from tests.imagenet import reference as R

U = R.U
W32 = tuple(float(np.float32(w)) for w in (0.299, 0.587, 0.114))
C13 = float(np.float32(1) / np.float32(13))
SHAPES = ((1, 1), (7, 5), (16, 12), (33, 65), (40, 64))
BATCHES = (1, 2, 5)
CONTINUOUS = (6, 7, 8, 9, 12)
MUTANTS = ('bin_truncates', 'table_without_half_step', 'shear_on_the_wrong_axis', 'rotation_about_the_corner',
           'sharpness_blends_the_border', 'autocontrast_one_range_for_all_channels', 'contrast_mean_of_the_input')
SAME = [65536, 0, 32768, 0, 65536, 32768]


def _bin(x, mutant=None):
    """bin() on fp32 values -> int64; the product x * 255 is exact in float64"""
    t = (x.astype(np.float64) * 255.0 + (0.0 if mutant == 'bin_truncates' else 0.5)).astype(np.float32)
    return np.minimum(np.maximum(t, np.float32(0)), np.float32(255)).astype(np.int64)


def _table(h, mutant=None):
    nz = h[h > 0]
    if len(nz) < 2:
        return None
    step = (int(h.sum()) - int(nz[-1])) // 255
    if step == 0:
        return None
    half = 0 if mutant == 'table_without_half_step' else step // 2
    lut, before = [], 0
    for i in range(256):
        lut.append(min(255, (half + before) // step))
        before += int(h[i])
    return np.array(lut, np.int64)


def _exact_layer(px, op, a, thr, fill, mutant):
    """ops 1-5, 10, 11, 13 on fp32 px [3][H][W] -> fp32, bit for bit what an implementation must give"""
    f32 = np.float32
    H, W = px.shape[1:]
    if 1 <= op <= 5:
        a = [int(v) for v in a]
        if a == SAME:
            return px
        if mutant == 'shear_on_the_wrong_axis' and op in (1, 2):
            # ShearX(v) built as ShearY(v) and the reverse
            v = a[1] / 65536.0 if op == 1 else a[3] / 65536.0
            a = [int(c) for c in RA.fixed_point(RA.coefficients(3 - op, v, H, W))]
        if mutant == 'rotation_about_the_corner' and op == 5:
            a = a[:2] + [(a[0] + a[1] + 1) >> 1] + a[3:5] + [(a[3] + a[4] + 1) >> 1]       # no shift to the centre and back
        y, x = np.mgrid[0:H, 0:W].astype(np.int64)
        xin, yin = (a[0] * x + a[1] * y + a[2]) >> 16, (a[3] * x + a[4] * y + a[5]) >> 16
        inside = (0 <= xin) & (xin < W) & (0 <= yin) & (yin < H)
        out = np.empty_like(px)
        for c in range(3):
            out[c] = np.where(inside, px[c][np.clip(yin, 0, H - 1), np.clip(xin, 0, W - 1)], f32(fill[c]))
        return out
    if op == 10:
        bits = int(a[0])
        return px if bits == 8 else ((_bin(px, mutant) & ((0xFF << (8 - bits)) & 0xFF)).astype(f32) / f32(255)).astype(f32)
    if op == 11:
        return np.where(px >= f32(thr), f32(1) - px, px).astype(f32)
    assert op == 13
    out = px.copy()
    for c in range(3):
        k = _bin(px[c], mutant)
        lut = _table(np.bincount(k.reshape(-1), minlength=256), mutant)
        if lut is not None:
            out[c] = (lut[k].astype(f32) / f32(255)).astype(f32)
    return out


def _grey(v):
    G = W32[0] * v[0] + W32[1] * v[1] + W32[2] * v[2]
    S = W32[0] * np.abs(v[0]) + W32[1] * np.abs(v[1]) + W32[2] * np.abs(v[2])
    return G, 3 * U * S


def _continuous_layer(v, op, f, omf, first, mutant):
    """ops 6-9, 12 on float64 v [3][H][W] (exact fp32 numbers) -> (values, bound before the slack, copies)"""
    H, W = v.shape[1:]
    clamp = lambda t: np.clip(t, 0.0, 1.0)          # noqa: E731
    none = np.zeros(v.shape, bool)
    if op == 6:
        return clamp(f * v), U * np.abs(f * v), none
    if op == 7:
        G, eg = _grey(v)
        et = abs(omf) * eg + U * (np.abs(omf * G) + abs(omf) * eg)
        return clamp(f * v + (omf * G)[None]), et[None] + U * (np.abs(f * v) + np.abs(omf * G)[None] + et[None]), none
    if op == 8:
        G, eg = _grey(first if mutant == 'contrast_mean_of_the_input' else v)
        m = G.mean()
        em = eg.mean() + U * (abs(m) + eg.mean()) + H * W * 2.0 ** -53 * (np.abs(G) + eg).mean()
        ecm = abs(omf) * em + U * (abs(omf * m) + abs(omf) * em)
        return clamp(f * v + omf * m), ecm + U * (np.abs(f * v) + abs(omf * m) + ecm), none
    if op == 9:
        out, e, copies = v.copy(), np.zeros(v.shape), np.ones(v.shape, bool)
        if mutant == 'sharpness_blends_the_border':
            pad = np.pad(v, ((0, 0), (1, 1), (1, 1)), mode='edge')
            ys, xs = slice(0, H), slice(0, W)
        else:
            pad = v
            ys, xs = slice(1, H - 1), slice(1, W - 1)
        h, w = pad.shape[1] - 2, pad.shape[2] - 2
        nb = [pad[:, dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3) if (dy, dx) != (1, 1)]
        x = pad[:, 1:1 + h, 1:1 + w]
        acc, A = sum(nb), sum(np.abs(n) for n in nb)
        ea = 7 * U * A * (1 + 7 * U)
        T = 5 * x + acc
        et = ea + U * (np.abs(5 * x) + A + ea)
        D = T * C13
        ed = C13 * et + U * (np.abs(D) + C13 * et)
        eo = abs(omf) * ed + U * (np.abs(omf * D) + abs(omf) * ed)
        out[:, ys, xs] = clamp(f * x + omf * D)
        e[:, ys, xs] = eo + U * (np.abs(f * x) + np.abs(omf * D) + eo)
        copies[:, ys, xs] = False
        return out, e, copies
    assert op == 12
    out, e, copies = v.copy(), np.zeros(v.shape), np.ones(v.shape, bool)
    for c in range(3):
        lo, hi = (v.min(), v.max()) if mutant == 'autocontrast_one_range_for_all_channels' else (v[c].min(), v[c].max())
        if hi > lo:
            t = (v[c] - lo) / (hi - lo)
            out[c], e[c], copies[c] = clamp(t), np.abs(t) * ((1 + U) ** 4 - 1), False
    return out, e, copies


def acts(j, l, H, W):
    """whether layer l of job j changes an H x W image at all"""
    op = int(j['op'][l])
    if l >= int(j['layers']) or op == 0:
        return False
    if 1 <= op <= 5:
        return [int(v) for v in j['a'][l]] != SAME
    if 6 <= op <= 9:
        return float(j['f'][l][0]) != 1.0 and not (op == 9 and (H < 3 or W < 3))
    return not (op == 10 and int(j['a'][l][0]) == 8)


def ra_ref(frames, jobs, mutant=None):
    """(out float64, exact mask, bound) of the stage on frames [B][3][H][W] under the ``RA_JOB`` table ``jobs``: where ``exact``
    is set the element must equal ``out`` (an fp32 number) bit for bit, elsewhere within ``bound``.  ``mutant``: one of MUTANTS
    -- the same with that mistake built in."""
    x = np.asarray(frames, np.float32)
    B, C, H, W = x.shape
    assert C == 3 and len(jobs) == B
    out, bound, exact = x.astype(np.float64), np.zeros(x.shape), np.ones(x.shape, bool)
    for n, j in enumerate(jobs):
        px = x[n]
        live = [l for l in range(int(j['layers'])) if acts(j, l, H, W)]
        for l in live:
            op = int(j['op'][l])
            if op in CONTINUOUS:
                assert l == live[-1], 'a continuous layer must be the last one that acts'
                v, e, copies = _continuous_layer(px.astype(np.float64), op, float(j['f'][l][0]), float(j['f'][l][1]),
                                                 x[n].astype(np.float64), mutant)
                out[n], exact[n] = v, copies
                bound[n] = np.where(copies, 0.0, e * R.SLACK + 1e-37)
            else:
                px = _exact_layer(px, op, j['a'][l], j['f'][l][0], j['fill'], mutant)
                out[n] = px.astype(np.float64)
    return out, exact, bound


def holds(got, ref):
    """whether fp32 ``got`` passes the checks against ``ref`` = ra_ref(...): the exact elements bit for bit, the others inside the
    bound"""
    out64, exact, bound = ref
    got = np.asarray(got)
    if got.dtype != np.float32 or got.shape != out64.shape:
        return False
    if not np.array_equal(got.view(np.uint32)[exact], out64.astype(np.float32).view(np.uint32)[exact]):
        return False
    return bool(np.all(np.abs(got.astype(np.float64) - out64)[~exact] <= bound[~exact]))


def worst(got, ref):
    """the largest error / bound among the elements that are not exact (0 where there is none)"""
    out64, exact, bound = ref
    live = ~exact
    return float((np.abs(got.astype(np.float64) - out64)[live] / bound[live]).max()) if live.any() else 0.0


def frames(B, H, W, seed=0):
    """[0, 1] pixels like the feed's: three quarters of them on the byte grid u / 255 (so that bins repeat and the equalisation
    tables are real), with an exact 0 and 1, a few values outside [0, 1] and tiny magnitudes mixed in"""
    rng = np.random.RandomState(1000 * B + 10 * H + W + seed)
    x = rng.rand(B, 3, H, W).astype(np.float32)
    grid = (rng.randint(0, 256, x.shape).astype(np.float32) / np.float32(255)).astype(np.float32)
    x = np.where(rng.rand(*x.shape) < 0.75, grid, x).astype(np.float32)
    flat = x.reshape(-1)
    flat[::17] *= -1
    flat[::23] *= 1.5
    flat[::29] *= 1e-30
    flat[0] = 0.0
    flat[-1] = 1.0
    return x


def band_frames(B, H, W, seed=0):
    """byte-grid pixels in a narrow band of values, 100 .. 131: few bins, large counts"""
    rng = np.random.RandomState(7 + 1000 * B + 10 * H + W + seed)
    return (rng.randint(100, 132, (B, 3, H, W)).astype(np.float32) / np.float32(255)).astype(np.float32)


def values(op, H, W):
    """the sign and magnitude grid of one op: 0, the extremes of both policies with both signs, and one value in between"""
    if op in (1, 2):
        return (-0.99, -0.3, 0.0, 0.09, 0.3, 0.99)
    if op in (3, 4):
        t = int(150.0 / 331.0 * (W if op == 3 else H))
        return tuple(sorted({-32, -t, -1, 0, 1, t, 32}))
    if op == 5:
        return (-135.0, -30.0, 0.0, 9.0, 30.0, 90.0, 135.0)
    if 6 <= op <= 9:
        return (-0.99, -0.9, 0.0, 0.27, 0.9, 0.99)
    if op == 10:
        return (2, 3, 4, 5, 6, 7, 8)
    if op == 11:
        return tuple(float(np.float32(1 - k / 30)) for k in (0, 9, 15, 30))
    return (None,)


def combos(H, W):
    return [(op, v) for op in range(14) for v in values(op, H, W)]


FILLS = ((0.485, 0.456, 0.406), (0.0, 1.0, -0.25))


def case_jobs(B, H, W):
    """single-layer tables for a batch of B images of H x W: together they hold every op at every value of ``values``"""
    every = combos(H, W)
    tables = []
    for t in range(0, len(every), B):
        jobs = np.zeros(B, RA_JOB)
        for n in range(B):
            jobs[n] = RA.make_job([every[(t + n) % len(every)]], H, W, FILLS[(t + n) % 2])
        tables.append(jobs)
    return tables


def chain_jobs(B, H, W):
    """two- and three-layer tables whose last acting layer alone is continuous: Contrast, Sharpness and AutoContrast behind a
    gather, Solarize, Posterize -- the statistics are of the image as the layer finds it"""
    chains = [[(11, 0.5), (8, 0.9)], [(5, 30.0), (8, -0.9)], [(1, 0.3), (10, 4), (12, None)], [(3, 2), (9, 0.9)], [(11, 0.25), (0, None), (7, 0.5)]]
    jobs = np.zeros(B, RA_JOB)
    for n in range(B):
        jobs[n] = RA.make_job(chains[n % len(chains)], H, W, FILLS[n % 2])
    return [jobs, jobs[::-1].copy()]
