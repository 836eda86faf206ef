"""No GPU, no launch: the mix draws (loans_amd/common/datasets/batch_mix.py), the fp32 restatement of the two-label loss held to
the derived bound over the case grid, the trainer's options and their resume rules, and the two new entries' argument checks."""
import ctypes
import random

import numpy as np
import pytest

from loans_amd.common.datasets import batch_mix as BM
from loans_amd.mixed_labels import MixedLabels
from loans_amd.runtime import checkpoint
from tests.imagenet import reference as R
from tests.imagenet_mix import reference as X
from tests.imagenet_sgd import reference as S


# ---- the policy -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('lam, cy, cx, H, W, box, weight', [
    (0.75, 5, 5, 10, 10, (3, 3, 7, 7), 1 - 16 / 100),            # r = 0.5: a 5 x 5 cut, halves of 2 around the centre
    (0.75, 0, 5, 10, 10, (0, 3, 2, 7), 1 - 8 / 100),             # clipped at the top
    (0.75, 9, 5, 10, 10, (7, 3, 10, 7), 1 - 12 / 100),           # clipped at the bottom
    (0.75, 5, 0, 10, 10, (3, 0, 7, 2), 1 - 8 / 100),             # clipped at the left
    (0.75, 5, 9, 10, 10, (3, 7, 7, 10), 1 - 12 / 100),           # clipped at the right
    (0.0, 3, 4, 8, 6, (0, 1, 7, 6), 1 - 35 / 48),                # r = 1: the cut is the frame, clipped on every side it reaches
    (1.0, 3, 4, 8, 6, (3, 4, 3, 4), 1.0),                        # r = 0: no area, nothing of the partner
    (0.99, 0, 0, 7, 5, (0, 0, 0, 0), 1.0),                       # int(7 * 0.1) = 0: no area
    (0.36, 4, 11, 16, 12, (0, 7, 10, 12), 1 - 50 / 192),         # r = 0.8: 12 x 9, halves 6 and 4
])
def test_cutmix_box_known_answers(lam, cy, cx, H, W, box, weight):
    got_box, got_weight = BM.cutmix_box(lam, cy, cx, H, W)
    assert got_box == box
    assert got_weight == pytest.approx(weight, abs=1e-15)
    y0, x0, y1, x1 = got_box
    assert 0 <= y0 <= y1 <= H and 0 <= x0 <= x1 <= W


def test_prob_zero_never_mixes_and_prob_one_always_does():
    never = BM.MixPolicy(0.4, 1.0, prob=0.0, seed=1)
    assert all(never.draw(16, 12) == BM.UNMIXED for _ in range(50))
    always = BM.MixPolicy(0.4, 1.0, prob=1.0, seed=1)
    draws = [always.draw(16, 12) for _ in range(50)]
    assert all(d.mode in ('mixup', 'cutmix') for d in draws) and {d.mode for d in draws} == {'mixup', 'cutmix'}
    off = BM.MixPolicy(0.0, 0.0, seed=1)
    state = off.getstate()
    assert off.draw(16, 12) == BM.UNMIXED and off.getstate() == state             # both alphas 0: no draw is taken
    for bad in (dict(mixup_alpha=-0.1), dict(cutmix_alpha=-1), dict(prob=1.5), dict(switch_prob=-0.5)):
        with pytest.raises(ValueError):
            BM.MixPolicy(**bad)


def test_one_alpha_selects_its_mode_and_the_weights_are_the_documented_ones():
    for d in (BM.MixPolicy(0.3, 0.0, seed=2).draw(16, 12) for _ in range(20)):
        assert d.mode == 'mixup' and d.box == BM.NO_BOX
        assert (d.lam32, d.oml32) == X.weights(d.weight) == MixedLabels.weights(d.weight)
    for d in (BM.MixPolicy(0.0, 0.7, seed=2).draw(16, 12) for _ in range(20)):
        assert d.mode == 'cutmix' and (d.lam32, d.oml32) == (1.0, 0.0)
        y0, x0, y1, x1 = d.box
        assert d.weight == 1.0 - (y1 - y0) * (x1 - x0) / (16 * 12)


def test_the_stream_is_consumed_in_the_documented_order():
    """the policy against the same calls made by hand on a ``random.Random`` of the same seed"""
    H, W = 16, 12
    policy = BM.MixPolicy(0.4, 1.0, prob=0.7, switch_prob=0.4, seed=9)
    rng = random.Random(9)
    modes = set()
    for _ in range(200):
        got = policy.draw(H, W)
        if rng.random() >= 0.7:
            want = BM.UNMIXED
        elif rng.random() < 0.4:
            lam = rng.betavariate(1.0, 1.0)
            cy = rng.randrange(H)
            cx = rng.randrange(W)
            want = BM.MixDraw('cutmix', 1.0, 0.0, *BM.cutmix_box(lam, cy, cx, H, W))
        else:
            lam = rng.betavariate(0.4, 0.4)
            want = BM.MixDraw('mixup', *X.weights(lam), BM.NO_BOX, lam)
        assert got == want
        modes.add(got.mode)
    assert modes == {None, 'mixup', 'cutmix'}
    assert policy.getstate() == rng.getstate()

    a, b = BM.MixPolicy(0.4, 1.0, seed=5), BM.MixPolicy(0.4, 1.0, seed=5)
    first = [a.draw(H, W) for _ in range(7)]
    assert first == [b.draw(H, W) for _ in range(7)]
    state = a.getstate()
    rest = [a.draw(H, W) for _ in range(7)]
    c = BM.MixPolicy(0.4, 1.0, seed=None)
    c.setstate(state)
    assert [c.draw(H, W) for _ in range(7)] == rest
    a.reseed(5)
    assert [a.draw(H, W) for _ in range(7)] == first


class _Crops:
    """what the wrapper needs of a classification dataset, with the crop stream of ``_CropDraws``"""

    def __init__(self, seed):
        from loans_amd.common.datasets.classification_dataset import _CropDraws
        self.draws = _CropDraws()
        self.draws._init_draws((16, 12), True, (0.08, 1.0), (3 / 4, 4 / 3), 0.875, seed)
        self.image_size = self.draws.image_size

    def __len__(self):
        return 6

    def decode_batch(self, indices, map_fn=map):
        return list(indices), [self.draws._draw(20, 16) for _ in indices]

    def reseed(self, seed):
        self.draws.reseed(seed)

    def draw_state(self):
        return self.draws.draw_state()

    def set_draw_state(self, state):
        self.draws.set_draw_state(state)


def test_the_crop_stream_does_not_depend_on_the_wrapper_and_the_state_is_the_pair():
    from loans_amd.common.datasets.shard import ShardedDataset
    from loans_amd.runtime.training import _as_draw_state
    import json
    bare = _Crops(4)
    wrapped = BM.MixedBatches(ShardedDataset(_Crops(4), 0, 1, pad=True), BM.MixPolicy(0.4, 1.0, seed=8))
    assert len(wrapped) == 6 and wrapped.image_size == (16, 12) and not hasattr(wrapped, 'cache')
    batches = [[0, 1, 2], [3, 4, 5], [0, 1, 2], [3, 4, 5]]
    mixes = []
    for n, idx in enumerate(batches):
        if n == 2:
            state = wrapped.draw_state()
        inner, draw = wrapped.decode_batch(idx)
        assert inner == bare.decode_batch(idx)                  # the same crops, mixing or not
        mixes.append(draw)
    alone = BM.MixPolicy(0.4, 1.0, seed=8)
    assert mixes == [alone.draw(16, 12) for _ in batches]           # one mix draw per batch, from a stream of its own
    assert isinstance(state, tuple) and len(state) == 2
    # through a checkpoint's JSON and back: batches 3 and 4 again
    fresh = BM.MixedBatches(ShardedDataset(_Crops(None), 0, 1, pad=True), BM.MixPolicy(0.4, 1.0, seed=None))
    arrays = {}
    packed = json.loads(json.dumps(checkpoint.pack(state, 'draw', arrays)))
    fresh.set_draw_state(_as_draw_state(checkpoint.unpack(packed, arrays)))
    bare.reseed(4)
    for idx in batches[:2]:
        bare.decode_batch(idx)
    for n in (2, 3):
        inner, draw = fresh.decode_batch(batches[n])
        assert inner == bare.decode_batch(batches[n]) and draw == mixes[n]


def test_mixed_labels_round_their_weights_once():
    t = np.arange(4, dtype=np.int32)
    m = MixedLabels(t, np.roll(t, 1), 0.3)
    assert (m.lam32, m.oml32) == (float(np.float32(0.3)), float(np.float32(1) - np.float32(0.3))) and len(m) == 4
    assert (MixedLabels(t, t, 1.0).lam32, MixedLabels(t, t, 1.0).oml32) == (1.0, 0.0)
    with pytest.raises(ValueError):
        MixedLabels(t, t[:3], 0.5)
    with pytest.raises(ValueError):
        MixedLabels(t, t, 1.5)


# ---- reference, restatement and bound -----------------------------------------------------------------------------------------
def test_float64_reference_known_answers():
    # equal logits: softmax is 1 / N, lse = c + log N whatever the target; the target sums to one
    N, B = 5, 3
    z = np.full((B, N), 0.75)
    ta, tb = np.array([0, 1, 2]), np.array([4, 1, -1])
    wa, wb = X.weights(0.3)
    loss, acc, acck, gz, row_loss, hit, hitk = X.mixed_ref(z, ta, tb, wa, wb, 0.1, 2)
    want = (0.75 + np.log(N)) - 0.9 * (wa + wb) * 0.75 - 0.1 * 0.75
    np.testing.assert_allclose(row_loss, [want, want, 0.0], rtol=1e-14)
    assert loss == pytest.approx(want, rel=1e-14)                 # two rows count
    q0 = np.full(N, 0.02)
    q0[0] += 0.9 * wa
    q0[4] += 0.9 * wb
    np.testing.assert_allclose(gz[0], (0.2 - q0) / 2, rtol=1e-13)
    q1 = np.full(N, 0.02)
    q1[1] += 0.9 * (wa + wb)                                     # ta == tb: both weights on the class
    np.testing.assert_allclose(gz[1], (0.2 - q1) / 2, rtol=1e-13)
    assert not gz[2].any()
    # the dominant label is tb (wa < wb); all logits tie, so the argmax is column 0 and the rank of class c is c
    assert hit.tolist() == [False, False, False] and hitk.tolist() == [False, True, False]
    # the one-label weights are the label-smoothed reference on that label, and the other label is not read
    for w, t in (((1.0, 0.0), ta), ((0.0, 1.0), tb)):
        zz = np.random.RandomState(0).standard_normal((B, N))
        got = X.mixed_ref(zz, ta, tb, w[0], w[1], 0.1, 2)
        ref = S.softmax_xent_ls_ref(zz, t, 0.1, 2)
        for g, r in zip(got, ref):
            np.testing.assert_allclose(np.asarray(g, np.float64), np.asarray(r, np.float64), rtol=1e-13, atol=1e-16)


@pytest.mark.parametrize('N', R.XENT_N)
def test_restatement_is_inside_the_bound_over_the_grid(N):
    worst = {'loss': 0.0, 'gz': 0.0, 'batch': 0.0}
    cases = 0
    for name, z, ta, tb, t, expect in X.mix_cases(N):
        assert R.argmax_margin_ok(z), name
        for lam in X.LAMS:
            wa, wb = X.weights(lam)
            for eps in X.MIX_EPS:
                loss, acc, acck, gz, row_loss, hit, hitk = X.mixed_ref(z, ta, tb, wa, wb, eps, 2)
                lb, gb, bb = X.mixed_bounds(z, ta, tb, wa, wb, eps)
                f_loss, f_acc, f_acck, f_gz, f_row = X.mixed_fp32(z, ta, tb, wa, wb, eps, 2)
                err = np.abs(f_row.astype(np.float64) - row_loss)
                gerr = np.abs(f_gz.astype(np.float64) - gz)
                tag = (name, lam, eps)
                assert np.all(err <= lb), tag + (float((err - lb).max()),)
                assert np.all(gerr <= gb), tag + (float((gerr - gb).max()),)
                assert abs(f_loss - loss) <= bb, tag + (f_loss, loss, bb)
                assert f_acc == float(np.float32(acc)) and f_acck == float(np.float32(acck)), tag
                valid = lb > 0
                if valid.any():
                    worst['loss'] = max(worst['loss'], float((err[valid] / lb[valid]).max()))
                    worst['gz'] = max(worst['gz'], float((gerr[valid] / gb[valid]).max()))
                    worst['batch'] = max(worst['batch'], abs(f_loss - loss) / bb)
                else:
                    assert f_loss == 0.0 and not f_gz.any()
                if expect is not None and np.array_equal(ta if wa >= wb else tb, t):
                    # the tie expectations, against the dominant label: the first of two equal maxima is the hit
                    np.testing.assert_array_equal(hit, expect & (lb > 0), err_msg=name)
                cases += 1
    assert cases == len(R.XENT_B) * (len(R.PROFILES) if N >= 2 else len(R.PROFILES) - 1) * len(X.PAIRS) * len(X.LAMS) * len(X.MIX_EPS)
    print('N=%d worst error / bound: row loss %.3f, gz %.3f, batch loss %.3f' % (N, worst['loss'], worst['gz'], worst['batch']))


@pytest.mark.parametrize('N', (2, 65, 1001))
def test_restatement_with_one_label_is_the_label_smoothed_restatement_bit_for_bit(N):
    for name, z, ta, tb, t, _ in X.mix_cases(N, batches=(5, 257)):
        for eps in X.MIX_EPS:
            for w, one in (((1.0, 0.0), ta), ((0.0, 1.0), tb)):
                got = X.mixed_fp32(z, ta, tb, w[0], w[1], eps, 2)
                want = S.softmax_xent_ls_fp32(z, one, eps, 2)
                assert got[:3] == want[:3], (name, eps, w)
                np.testing.assert_array_equal(got[3], want[3])
                np.testing.assert_array_equal(got[4], want[4])
        assert X.weights(1.0) == (1.0, 0.0) and X.weights(0.0) == (0.0, 1.0)


def test_batch_mix_reference_known_answers():
    x = np.arange(2 * 1 * 2 * 3, dtype=np.float32).reshape(2, 1, 2, 3)
    out, blended, bound = X.batch_mix_ref(x, 1, 1.0, 0.0, (0, 1, 1, 3))
    assert out[0, 0].tolist() == [[0, 7, 8], [3, 4, 5]] and out[1, 0].tolist() == [[6, 1, 2], [9, 10, 11]]
    assert not blended.any() and not bound.any()
    out, blended, bound = X.batch_mix_ref(x, 1, 0.5, 0.5, (0, 0, 0, 0))
    assert blended.all() and np.all(out[0] == out[1]) and out[0, 0, 0, 0] == 3.0
    out, _, _ = X.batch_mix_ref(x, 0, 0.5, 0.5, (0, 0, 0, 0))
    np.testing.assert_array_equal(out, x)


# ---- the trainer's options ----------------------------------------------------------------------------------------------------
NEW = ('mixup_alpha', 'cutmix_alpha', 'mix_prob', 'mix_switch_prob', 'mix_seed')


def test_the_mix_options_parse_and_leave_the_default_namespace_alone():
    import train_imagenet as T
    bare = T.parse_args([])
    assert not set(NEW) & set(vars(bare))                                     # class-level defaults, not parsed values
    assert tuple(getattr(bare, n) for n in NEW) == (0.0, 0.0, 1.0, 0.5, None)
    args = T.parse_args(['--augment', 'rrc', '--mixup-alpha', '0.2', '--cutmix-alpha', '1.0', '--mix-prob', '0.5',
                         '--mix-switch-prob', '0.25', '--mix-seed', '3'])
    assert tuple(getattr(args, n) for n in NEW) == (0.2, 1.0, 0.5, 0.25, 3)
    assert set(vars(args)) == set(vars(bare)) | set(NEW) | {'augment'}
    assert set(T.Arguments._MIX) == set(NEW) and set(NEW) <= set(T.RESUME_FIXED)
    T.check_mix_arguments(bare)
    T.check_mix_arguments(args)


@pytest.mark.parametrize('argv', [
    ['--mixup-alpha', '0.2'],                                   # mixing needs the device feed
    ['--cutmix-alpha', '1.0', '--augment', 'none'],
    ['--augment', 'rrc', '--mixup-alpha', '-0.1'],
    ['--augment', 'rrc', '--cutmix-alpha', '-1'],
    ['--augment', 'rrc', '--mixup-alpha', '0.2', '--mix-prob', '1.5'],
    ['--augment', 'rrc', '--mixup-alpha', '0.2', '--mix-prob', '-0.1'],
    ['--augment', 'rrc', '--mixup-alpha', '0.2', '--mix-switch-prob', '2'],
    ['--mix-prob', 'nan'],
])
def test_the_mix_options_are_refused_by_the_parser_and_by_the_check(argv, capsys):
    import train_imagenet as T
    with pytest.raises(SystemExit):
        T.parse_args(argv)
    capsys.readouterr()
    # the same values on a namespace that never went through the parser (``run`` calls the check too)
    args = T.Arguments()
    pairs = dict(zip(argv[::2], argv[1::2]))
    for flag, value in pairs.items():
        name = flag[2:].replace('-', '_')
        setattr(args, name, value if name == 'augment' else float(value))
    with pytest.raises(ValueError):
        T.check_mix_arguments(args)


def test_a_checkpoint_from_before_the_options_resumes_at_their_defaults_only():
    import train_imagenet as T
    args = T.parse_args(['--augment', 'rrc'])
    saved = {k: v for k, v in checkpoint.plain_arguments(args).items() if k not in NEW}
    fixed = [k for k in T.RESUME_FIXED if k != 'gpus']
    assert checkpoint.check_arguments(saved, args, fixed, checkpoint.SILENT, T.RESUME_DEFAULTS) == []
    mixed = T.parse_args(['--augment', 'rrc', '--mixup-alpha', '0.2'])
    with pytest.raises(ValueError, match='mixup_alpha'):
        checkpoint.check_arguments(saved, mixed, fixed, checkpoint.SILENT, T.RESUME_DEFAULTS)
    # a checkpoint that holds the keys is compared as it is, and without the defaults an absent key still differs from a value
    now = checkpoint.plain_arguments(mixed)
    assert checkpoint.check_arguments(now, mixed, fixed, checkpoint.SILENT, T.RESUME_DEFAULTS) == []
    with pytest.raises(ValueError, match='mix_seed'):
        checkpoint.check_arguments(now, T.parse_args(['--augment', 'rrc', '--mixup-alpha', '0.2', '--mix-seed', '1']), fixed,
                                   checkpoint.SILENT, T.RESUME_DEFAULTS)
    assert T.RESUME_DEFAULTS == {'mixup_alpha': 0.0, 'cutmix_alpha': 0.0, 'mix_prob': 1.0, 'mix_switch_prob': 0.5, 'mix_seed': None}


# ---- the two entries without a GPU ----------------------------------------------------------------------------------------------
def test_mix_entry_checks_its_arguments_before_any_hip_call():
    from loans_amd import _lib
    f = _lib.load().loans_batch_mix_f32
    buf = ctypes.create_string_buffer(256)
    x = ctypes.addressof(buf)
    o = x + 128
    good = dict(x=x, out=o, B=2, C=1, H=2, W=2, shift=1, lam=0.5, oml=0.5, y0=0, x0=0, y1=1, x1=2)
    order = ('x', 'out', 'B', 'C', 'H', 'W', 'shift', 'lam', 'oml', 'y0', 'x0', 'y1', 'x1')
    inf, nan = float('inf'), float('nan')
    bad = [dict(x=0), dict(out=0), dict(out=x), dict(B=0), dict(C=0), dict(H=-1), dict(W=0), dict(shift=-1), dict(shift=2),
           dict(y0=-1), dict(y0=2, y1=1), dict(y1=3), dict(x0=-1), dict(x0=2, x1=1), dict(x1=3), dict(lam=nan), dict(lam=inf),
           dict(oml=nan), dict(oml=-inf)]
    for change in bad:
        args = dict(good, **change)
        assert f(*[args[n] for n in order], 0) == -1, change
    assert f(x, o, 1, 1 << 10, 1 << 10, 1 << 10, 0, 1.0, 0.0, 0, 0, 0, 0, 0) == -2          # a row of the batch past 32-bit indexing
    assert bytes(buf) == bytes(256)


def test_mixed_loss_entry_checks_its_arguments_before_any_hip_call():
    from loans_amd import _lib
    f = _lib.load().loans_softmax_xent_mix_fwd_f32
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)

    def call(ptrs=None, lam=0.5, oml=0.5, B=4, N=8, eps=0.1, k=1):
        z, ta, tb, gz, rl, rh, rhk, out = ptrs or [p] * 8
        return f(z, ta, tb, lam, oml, gz, rl, rh, rhk, out, B, N, eps, k, 0)

    for weights in ((0.5, 0.5), (1.0, 0.0), (0.0, 1.0)):          # the general kernel and the two one-label routes
        lam, oml = weights
        for missing in range(8):
            ptrs = [p] * 8
            ptrs[missing] = 0
            assert call(ptrs, lam, oml) == -1, (weights, missing)
        assert call(lam=lam, oml=oml, k=0) == -1
        assert call(lam=lam, oml=oml, B=0) == -1 and call(lam=lam, oml=oml, N=0) == -1 and call(lam=lam, oml=oml, B=-3) == -1
        assert call(lam=lam, oml=oml, eps=1.0) == -1 and call(lam=lam, oml=oml, eps=-0.1) == -1
        assert call(lam=lam, oml=oml, eps=float('nan')) == -1
        assert call(lam=lam, oml=oml, N=8193) == -2 and call(lam=lam, oml=oml, B=65537) == -2
    for lam, oml in ((float('nan'), 0.5), (0.5, float('inf')), (float('-inf'), 0.0)):
        assert call(lam=lam, oml=oml) == -1
    assert bytes(buf) == bytes(64)
