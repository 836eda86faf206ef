"""Cases, float64 references, derived bounds and fp32 restatements for the test-mode forward: BatchNormalization on running
statistics (``config.train`` false; csrc/bn_pool.hip: bn_eval_coeffs_kernel, functions/blocks.py: _ConvBN.forward).  Not collected
by pytest, as tests/bn_cases.py; tests/eval_mode/test_cases_cpu.py holds the restatements and the conditions on the inputs to what
is written here before any GPU run, test_gpu_kernels.py and test_gpu_model.py hold the device to it.

THE COEFFICIENTS.  Chainer's test-mode BN in float64 on the fp32 inputs (gamma, beta, running mean rm, running variance rv):
    rstd = 1 / sqrt(rv + eps)      scale = gamma rstd      shift = beta - rm scale
The kernel, one thread per channel (u = 2^-24, all first order, times 1 + 1e-3 for the second-order terms):
    s  = fl(rv + fl(eps))      eps cast once (u eps) and one addition (u s): 2 u relative at most
    q  = sqrtf(s)              correctly rounded (HIP's default): half of 2 u plus u = 2 u
    rs = fl(1 / q)             correctly rounded division: 3 u                                 -> rstd  within 3 u |rstd|
    sc = fl(gamma rs)          one product: 4 u                                                -> scale within 4 u |scale|
    sh = fl(beta - fl(rm sc))  the product carries sc's 4 u and its own u, the subtraction u of what it returns:
                               u |shift| + 5 u |rm scale|; contracted into one FMA the product is not rounded:
                               u |shift| + 4 u |rm scale|                                      -> shift within u (|shift| + 5 |rm scale|)
    mean = rm                  a copy: the same bits
gamma = 0 gives scale = +-0 and shift = beta exactly on both sides.  None of the figures was read off a kernel's output.

THE MODELS.  ``Classifier(SheepLocalizer((75, 75), train_imagenet=True, **options))`` with seeded parameters, every BN's running
statistics away from (0, 1) and from the batch statistics (avg_mean ~ N(0, 0.5^2), avg_var ~ U(0.5, 1.5)), on 64 x 64 frames; the
reference is ``RefNet``: the oracle's ResNet-18 composed from ``oracle.model._ConvBN`` with the squeeze-and-excitation gate of
tests/imagenet_se/reference.py and the blur of tests/imagenet_blurpool at the junctions (forward only -- test mode has no
backward, and the running averages of a training step are written by its forward).  Inside ``oracle.model.emulate_bf16_storage``
it rounds where the bf16 storage arm stores a tensor.  test_cases_cpu.py holds RefNet to the existing references bit for bit: plain,
SE alone and blur alone.  For SE and blur together no other reference exists; that composition is the same two junction changes in
one unit and is checked by nothing but the device tests themselves.

The issue asks for parameters as ``_randomize`` makes them.  Three tensors are scaled on top of that (CONV1_SCALE, SE_DOWN_SCALE,
FC_SCALE below, each with its reason): a departure from the issue, made so that its own conditions on the inputs can hold."""
import functools

import numpy as np

from oracle import chainer_ops as C
from oracle import model as M
from tests.bn_cases import U, _within
from tests.imagenet import reference as R
from tests.imagenet_droppath.reference import tol
from tests.imagenet_se import reference as S

F = np.float32

# ---- the coefficient grid ------------------------------------------------------------------------------------------------------
# one thread per channel, 256 per block: both sides of a block boundary, a ragged last block, one thread, eight blocks
COEFF_C = (1, 4, 63, 64, 96, 255, 256, 257, 2048)
N_VAR, N_MEAN, N_GAMMA = 5, 4, 4        # variance 0 / 1e-12 / ~eps / ~1 / ~1e6;  mean 0 / +60 / -60 / 1e4;  gamma ~1 / 1e-3 / < 0 / 0
N_PROFILES = N_VAR * N_MEAN * N_GAMMA   # every combination is a profile


def rotations(C_):
    """the rotations at which ``C_`` channels meet every profile"""
    return tuple(range(0, N_PROFILES, min(C_, N_PROFILES)))


def make_coeffs(C_, rot=0):
    """gamma, beta, running mean ``rm`` and variance ``rv`` (fp32).  Channel c has profile p = (c + rot) % 80: variance p % 5, mean
    p % 4 (the twenty pairs, by the Chinese remainder theorem), gamma (p // 20 + p) % 4 -- neighbouring channels differ in all three"""
    rng = np.random.RandomState(7000 + 97 * C_ + rot)
    p = (np.arange(C_) + rot) % N_PROFILES
    v, m, g = p % N_VAR, p % N_MEAN, (p // 20 + p) % N_GAMMA
    wob = lambda w: 1 + w * rng.uniform(-1, 1, C_)          # noqa: E731  (mantissas that round)
    rv = np.select([v == 0, v == 1, v == 2, v == 3], [0.0, 1e-12 * wob(0.25), C.BN_EPS * wob(0.25), wob(0.25)], 1e6 * wob(0.25))
    rm = np.select([m == 0, m == 1, m == 2], [0.0, 60 * wob(0.01), -60 * wob(0.01)], 1e4 * wob(0.01))
    one = 1 + 0.1 * rng.standard_normal(C_)
    gamma = np.select([g == 0, g == 1, g == 2], [one, 1e-3, -np.abs(one)], 0.0)
    beta = 0.1 * rng.standard_normal(C_)
    return dict(gamma=gamma.astype(F), beta=beta.astype(F), rm=rm.astype(F), rv=rv.astype(F), C=C_, profile=p)


def coeffs_ref(d):
    rv, rm, gamma, beta = (d[k].astype(np.float64) for k in ('rv', 'rm', 'gamma', 'beta'))
    rstd = 1.0 / np.sqrt(rv + C.BN_EPS)
    scale = gamma * rstd
    return dict(mean=rm, rstd=rstd, scale=scale, shift=beta - rm * scale)


def coeffs_bounds(ref):
    s = (1 + 1e-3) * U
    return dict(rstd=3 * s * ref['rstd'], scale=4 * s * np.abs(ref['scale']),
                shift=s * (np.abs(ref['shift']) + 5 * np.abs(ref['mean'] * ref['scale'])))


def coeffs_fp32(d, fma):
    """bn_eval_coeffs_kernel operation by operation in NumPy fp32; ``fma``: beta - rm sc as one fused multiply-add (the exact
    product of two fp32 values fits a double; the double's own rounding of the sum is 2^-29 of the one the cast then makes)"""
    rs = F(1) / np.sqrt(d['rv'] + F(C.BN_EPS))
    sc = d['gamma'] * rs
    if fma:
        sh = (d['beta'].astype(np.float64) - d['rm'].astype(np.float64) * sc.astype(np.float64)).astype(F)
    else:
        sh = d['beta'] - d['rm'] * sc
    assert rs.dtype == sc.dtype == sh.dtype == F
    return dict(mean=d['rm'].copy(), rstd=rs, scale=sc, shift=sh)


def check_coeffs(got, d, ratios):
    """``got``: dict(mean, rstd, scale, shift) of fp32 arrays"""
    ref = coeffs_ref(d)
    for key, bound in coeffs_bounds(ref).items():
        _within('coeffs.' + key, got[key], ref[key], bound, ratios)
    assert got['mean'].dtype == F and got['mean'].tobytes() == d['rm'].tobytes(), 'mean is not the running mean bit for bit'
    zero = d['gamma'] == 0
    assert not got['scale'][zero].any() and np.array_equal(got['shift'][zero], d['beta'][zero])


# ---- consumers of a test-mode state ----------------------------------------------------------------------------------------------
def far_state(x, seed):
    """gamma, beta, running mean / variance for the [..., C] tensor ``x``, deliberately far from its batch statistics: the mean
    off by two to four standard deviations to either side, the variance by a factor of 1/4 .. 4"""
    rng = np.random.RandomState(seed)
    flat = np.asarray(x, np.float64).reshape(-1, x.shape[-1])
    C_ = flat.shape[1]
    mean, std = flat.mean(0), flat.std(0) + 0.5
    rm = mean + std * rng.uniform(2, 4, C_) * np.where(rng.random_sample(C_) < 0.5, -1, 1)
    rv = std ** 2 * 4.0 ** rng.uniform(-1, 1, C_)
    return dict(gamma=(1 + 0.1 * rng.standard_normal(C_)).astype(F), beta=(0.1 * rng.standard_normal(C_)).astype(F),
                rm=rm.astype(F), rv=rv.astype(F), C=C_)


def apply_ref(x, st, dtype, relu=True, residual=None, x2=None, st2=None, bf16=False):
    """dict(y, pre) of bn_apply; ``st``: the fp32 vectors of the state, exact inputs (float32: one operation at a time)"""
    t = lambda a: np.asarray(a).astype(dtype)       # noqa: E731
    v = t(x) * t(st['scale']) + t(st['shift'])
    if residual is not None:
        v = v + t(residual)
    if x2 is not None:
        v = v + (t(x2) * t(st2['scale']) + t(st2['shift']))
    y = np.maximum(v, dtype(0)) if relu else v
    assert y.dtype == dtype
    return dict(y=C.round_bf16(y) if bf16 else y, pre=v)


def pool_ref(x4, st, dtype, bf16=False):
    """dict(y, idx, pre) of bn_relu_maxpool on NHWC ``x4``: 3 x 3 / stride 2 windows, cover_all, the first maximum wins"""
    from tests.bn_cases import _windows
    pre = np.asarray(x4).astype(dtype) * st['scale'].astype(dtype) + st['shift'].astype(dtype)
    win = _windows(np.maximum(pre, dtype(0)), -np.inf)
    y = win.max(axis=3).astype(dtype)
    return dict(y=C.round_bf16(y) if bf16 else y, idx=win.argmax(axis=3).astype(np.uint8), pre=pre, win=win)


def blur(a):
    """NCHW NumPy: reflect padding of one, the depthwise 3 x 3 binomial filter at stride 2 (the kernel test's torch reference)"""
    import torch
    from tests.imagenet_blurpool.test_gpu_kernels import _blur
    return _blur(torch.from_numpy(np.ascontiguousarray(a))).numpy()


def blur_ref(x4, st, dtype, bf16=False):
    """dict(y, pre) of blur_pool(x, st) on NHWC ``x4``"""
    pre = np.asarray(x4).astype(dtype) * st['scale'].astype(dtype) + st['shift'].astype(dtype)
    y = blur(np.maximum(pre, dtype(0)).transpose(0, 3, 1, 2)).transpose(0, 2, 3, 1)
    assert y.dtype == dtype
    return dict(y=C.round_bf16(y) if bf16 else y, pre=pre)


# ---- the models ------------------------------------------------------------------------------------------------------------------
FE = 'feature_extractor/'
VARIANTS = {'plain': {}, 'se': dict(se_ratio=16), 'blur': dict(blur_pool=True), 'se_blur': dict(se_ratio=16, blur_pool=True)}
BF16_ARMS = ('plain', 'se_blur')
H = W = 64
TOPK = 5
# A trained model's running statistics describe its activations.  With running variances near one nothing normalises the stem's
# output -- pixel values times a 7 x 7 x 3 HeNormal kernel: a few hundred, logits of a few thousand, whose fp32 rounding (1e-6 of
# the largest) is fifty times the absolute floor of the bound at every logit that happens to lie near zero.  conv1's weights are
# scaled so that its output has the unit order the running variances claim; the logits then are of order ten.  The squeeze is a
# mean that ReLUs and BN shifts keep away from zero, and behind a HeNormal ``down`` it saturates gates at 0 or 1 -- a test that
# cannot see the squeeze, and products gate * activation arbitrarily close to zero; ``down`` is scaled so that the gates of both
# modes spread over (1e-3, 1 - 1e-3) with some below 0.3 and above 0.7 in every unit (asserted on the CPU), as
# tests/imagenet_se/test_gpu_kernels.py arranges its gates.
SE_DOWN_SCALE = 1.0 / 4
CONV1_SCALE = 1.0 / 128
# Nothing normalises between the units either, so the pooled features still grow to some tens (more once a training step has mixed
# batch variances into the running ones).  A logit is a 512-term fp32 dot product: its rounding is a few u of the sum of the terms'
# magnitudes, about 1e-6 of the row's largest logit, whatever its own value -- and the bound's absolute floor, 1e-5, is all that
# covers a logit near zero.  The floor presumes logits of order one, as the training-mode tests have them; the head is scaled so
# that the test-mode logits are (largest logit times 1e-6 well below 1e-5).
FC_SCALE = 1.0 / 32
# named running averages of the state test: the stem, the BN of a blurred stage, a shortcut BN, the last BN of an SE unit
STATE_KEYS = (FE + 'bn1', FE + 'res3/0/bn1', FE + 'res3/0/bn3', FE + 'res4/0/bn2', FE + 'res5/1/bn2')


def randomize_running(link, rng):
    """avg_mean ~ N(0, 0.5^2), avg_var ~ U(0.5, 1.5) in every BN of a link that is still on the host"""
    for _, owner, name in link.namedpersistents():
        v = getattr(owner, name)
        if name == 'avg_mean':
            v[...] = 0.5 * rng.standard_normal(v.shape)
        elif name == 'avg_var':
            v[...] = rng.uniform(0.5, 1.5, v.shape)


def build_localizer(variant):
    """the seeded model of a variant, on the host: parameters as tests/imagenet/test_gpu_model._randomize makes them, the SE
    biases off zero (tests/imagenet_se/test_gpu_model.py), running statistics as above"""
    import loans_amd
    from tests.imagenet.test_gpu_model import _randomize
    np.random.seed(5)
    loc = loans_amd.SheepLocalizer((75, 75), train_imagenet=True, **VARIANTS[variant])
    loc.feature_extractor.materialize_head()
    rng = np.random.RandomState(105)
    _randomize(loc, rng)
    for key, p in loc.namedparams():
        if key.endswith(('se/down/b', 'se/up/b')):
            p.set_logical((0.5 * rng.standard_normal(p.logical_shape)).astype(F))
        elif key.endswith('se/down/W'):     # (see SE_DOWN_SCALE)
            p.set_logical((SE_DOWN_SCALE * p.get_logical()).astype(F))
        elif key == '/feature_extractor/conv1/W':       # (see CONV1_SCALE)
            p.set_logical((CONV1_SCALE * p.get_logical()).astype(F))
        elif key in ('/feature_extractor/fc/W', '/feature_extractor/fc/b'):     # (see FC_SCALE)
            p.set_logical((FC_SCALE * p.get_logical()).astype(F))
    randomize_running(loc, rng)
    return loc


BOTTLENECK = dict(B=4, H=9, W=10, cin=64, mid=64, cout=128)
BOTTLENECK_STAGES = [('conv1/conv', 'conv1/bn', 1, 0), ('conv2/conv', 'conv2/bn', 2, 1), ('conv3/conv', 'conv3/bn', 1, 0)]
BOTTLENECK_SHORTCUT = ('residual_conv/conv', 'residual_conv/bn', 2, 0)


def build_bottleneck(blur_pool):
    """(link on the host, x NCHW): one strided chainercv bottleneck as tests/imagenet_blurpool/test_gpu_model.py builds it"""
    import loans_amd
    from loans_amd.chainercv_resnet import Bottleneck
    from tests.imagenet.test_gpu_model import _randomize
    k = BOTTLENECK
    rng = np.random.RandomState(3)
    np.random.seed(4)
    blk = Bottleneck(k['cin'], k['mid'], k['cout'], 2, loans_amd.links.HeNormal(), residual_conv=True, blur_pool=blur_pool)
    _randomize(blk, rng)
    randomize_running(blk, rng)
    return blk, rng.standard_normal((k['B'], k['cin'], k['H'], k['W'])).astype(F)


class RefUnit:
    """relu(gate(bn_n(conv_n(... relu(bn_1(conv_1(x)))))) + shortcut(x)), forward only.  stages / shortcut = (conv key, bn key,
    stride, pad) as oracle.model._ResUnit takes them; ``blur``: every stride-2 convolution runs at stride 1, a strided stage hands
    blur(relu(bn(conv))) on, a strided shortcut reads blur(x); ``se``: the unit's key prefix, the gate of
    tests/imagenet_se/reference.py on the last BN's output.  ``pre`` collects every ReLU's input."""

    def __init__(self, p, stages, shortcut, train, blur=False, se=None):
        one = lambda t: (t[0], t[1], 1 if blur else t[2], t[3])     # noqa: E731
        self.stages = [M._ConvBN(p, *one(t), train) for t in stages]
        self.shortcut = None if shortcut is None else M._ConvBN(p, *one(shortcut), train)
        self.blurred = [bool(blur) and t[2] == 2 for t in stages]
        self.blur_sc = bool(blur) and shortcut is not None and shortcut[2] == 2
        self.se = None if se is None else [p[se + '/' + k] for k in S.SE_KEYS]
        assert not self.blurred[-1]

    def fwd(self, x):
        self.pre, h = [], x
        for st, blurred in zip(self.stages[:-1], self.blurred):
            a = st.fwd(h)
            self.pre.append(a)
            h = M._q(blur(C.relu(a)) if blurred else C.relu(a))     # (the full-resolution activation of a blurred stage is never stored)
        a = self.stages[-1].fwd(h)
        sc = x if self.shortcut is None else self.shortcut.fwd(M._q(blur(x)) if self.blur_sc else x)
        if self.se is not None:
            a1, s = S.excite(a.mean(axis=(2, 3)), *self.se)
            self.pre.append(a1)
            self.gate = s
            a = s[:, :, None, None] * a
        self.pre.append(a + sc)
        return M._q(C.relu(a + sc))


class RefNet:
    """the ResNet-18 classifier of a variant on a parameter dict with Chainer's keys, in the parameters' dtype; whether a unit has
    a gate is read off the keys"""

    def __init__(self, params, blur=False, prefix=FE, train=False):
        self.p, self.blur, self.fe, self.train = params, blur, prefix, train

    def forward(self, images, t=None):
        p, fe, train = self.p, self.fe, self.train
        self.stem = M._ConvBN(p, fe + 'conv1', fe + 'bn1', 2, 3, train)
        a = self.stem.fwd(M._q(C.prepare_images(images)))
        self.pre, self.gates = [a], []
        h, _ = C.max_pool_fwd(M._q(C.relu(a)), 3, 2, 0)
        for name, _, stride in M.STAGES:
            for i in (0, 1):
                u = fe + '%s/%d' % (name, i)
                se = u if (u + '/se/down/W') in p else None
                stages = [(u + '/conv1', u + '/bn1', stride if i == 0 else 1, 1), (u + '/conv2', u + '/bn2', 1, 1)]
                unit = RefUnit(p, stages, (u + '/conv3', u + '/bn3', stride, 1) if i == 0 else None, train, self.blur, se)
                h = unit.fwd(h)
                self.pre += unit.pre
                if se is not None:
                    self.gates.append(unit.gate)
        self.logits = C.linear_fwd(C.gap_fwd(h), p[fe + 'fc/W'], p[fe + 'fc/b'])
        if t is not None:
            self.loss, self.accuracy = R.softmax_xent_ref(self.logits, t)[:2]
        return self.logits

    def closest_to_zero(self):
        return min(float(np.abs(a).min()) for a in self.pre)


def run(params, variant, frames, train, dtype, bf16=False, t=None):
    """a RefNet after its forward, on a fresh cast of ``params`` (training mode writes the running statistics into ``.p``)"""
    net = RefNet(M.cast_params(dict(params), dtype), 'blur' in variant, train=train)
    if bf16:
        with M.emulate_bf16_storage():
            net.forward(frames.astype(dtype), t)
    else:
        net.forward(frames.astype(dtype), t)
    return net


FRAME_SEED = 2


@functools.lru_cache(maxsize=None)
def frames3():
    """three frames; the first two are ``synthetic.make_frames(2, 2, 64, 64)`` (the generator draws them one after the other).  The
    seed is one at which no ReLU input of a reference lies within 1e-6 of zero, in test or in training mode, in any variant."""
    from loans_amd.datasets import synthetic
    return synthetic.make_frames(FRAME_SEED, 3, H, W)


@functools.lru_cache(maxsize=None)
def start_params(variant):
    return build_localizer(variant).state_dict_chainer()


@functools.lru_cache(maxsize=None)
def reference(variant, kind, train=False):
    """the shared references of a variant (never changed by a test): ``kind`` 'f64', 'f32' or 'bf16' (fp32 with the storage
    emulation).  Test mode on all three frames -- a sample's logits do not depend on the batch it is in --, training mode on the
    first two."""
    fr = frames3() if not train else frames3()[:2]
    return run(start_params(variant), variant, fr, train, np.float64 if kind == 'f64' else F, kind == 'bf16')


def labels(variant):
    """int32 [3] from the float64 test-mode logits: the winner of the first row, one of the second to fourth of the second row,
    one of the sixth to tenth of the third -- accuracy 1/2 and top-5 accuracy 1 on the first two frames, 1/3 and 2/3 on all three.
    Among the candidates the class whose logit is furthest from every other logit of its row (label_margin)."""
    z = reference(variant, 'f64').logits
    order = np.argsort(-z, axis=1)
    lonely = lambda b, ranks: max((order[b, r] for r in ranks), key=lambda c: np.abs(np.delete(z[b], c) - z[b, c]).min())   # noqa: E731
    return np.array([order[0, 0], lonely(1, (1, 2, 3)), lonely(2, (5, 6, 7, 8, 9))], np.int32)


def metrics(logits, t, k=TOPK):
    """(loss, accuracy, top-k accuracy) in float64"""
    from tests.imagenet_sgd.reference import softmax_xent_ls_ref
    return softmax_xent_ls_ref(np.asarray(logits, np.float64), t, 0.0, k)[:3]


def tol_bf16(emulated, r64):
    """the bf16 arms: five times the distance of the emulated fp32 oracle from the float64 oracle on the same case, with the
    floors of the project's form.  The distance is ONE number per tensor, its largest element: two evaluations of a bf16 network
    differ by rounding that is as large at every logit, and where the emulation happens to land on the float64 value an
    elementwise distance would ask bf16 arithmetic for fp32 agreement."""
    emulated, r64 = np.asarray(emulated, np.float64), np.asarray(r64, np.float64)
    return np.maximum(np.maximum(5 * float(np.abs(emulated - r64).max()), 5e-4 * np.abs(r64)), 1e-5)


def model_tol(variant, bf16, rows=slice(None)):
    """(float64 logits, elementwise bound) of the test-mode forward"""
    r64 = reference(variant, 'f64').logits[rows]
    if bf16:
        return r64, tol_bf16(reference(variant, 'bf16').logits[rows], r64)
    return r64, tol(reference(variant, 'f32').logits[rows], r64)


def label_margin(variant, bf16, rows=2, k=TOPK):
    """How firmly the reference decides accuracy and top-k accuracy on the first ``rows`` frames, in bounds.  Only two boundaries of
    a row matter: the label is the winner or is not (its distance from the runner-up, or from the winner), and it is among the k
    largest or is not (its distance from the (k + 1)-th largest, or from the k-th).  Two logits that are each within the bound of
    the reference change order only if they are no more than two bounds apart, so above 2 the device's hits are the reference's."""
    z, bound = model_tol(variant, bf16, slice(0, rows))
    t = labels(variant)[:rows]
    worst = np.inf
    for b in range(rows):
        order = np.sort(z[b])[::-1]
        zt = z[b, t[b]]
        rank = int((z[b] > zt).sum())
        first = zt - order[1] if rank == 0 else order[0] - zt
        topk = zt - order[k] if rank < k else order[k - 1] - zt
        worst = min(worst, min(first, topk) / bound[b].max())
    return float(worst)


def separation(variant, kind):
    """the largest distance of a training-mode logit from its test-mode value on the first two frames, in references of ``kind``"""
    return float(np.abs(reference(variant, kind, train=True).logits - reference(variant, kind).logits[:2]).max())


# The fp32 bound is 5e-4 of a logit at the most, and the two modes differ by about the largest logit: well over a thousand bounds.
# The bf16 bound is five times the distance of the bf16 emulation from float64, which is about half a per cent of the largest logit
# behind seventeen bf16-stored layers: a bound of some 2.7 per cent, which a difference of the size of the logits themselves exceeds
# 30 to 45 times, never 100.  The factor that can be had is asserted (tests/eval_mode/test_cases_cpu.py).
BF16_SEPARATION = 30
