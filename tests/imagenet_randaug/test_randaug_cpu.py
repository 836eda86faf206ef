"""No GPU, no launch: the RandAugment / TrivialAugment draws (loans_amd/common/datasets/rand_augment.py), the fp32 restatement held
to the reference over the case grid, the checks' power to tell seven wrong implementations from the right one, Pillow cross-checks
of the gathers, Equalize and Posterize, the trainer's options and their resume rules, the job struct's layout and the entries'
argument checks."""
import ctypes
import json
import os
import random
import subprocess

import numpy as np
import pytest
from PIL import Image, ImageOps

from loans_amd.common.datasets import batch_mix as BM
from loans_amd.common.datasets import photometric as P
from loans_amd.common.datasets import rand_augment as RA
from loans_amd.ops import RA_JOB
from loans_amd.runtime import checkpoint
from tests.imagenet_randaug import reference as X

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
f32 = np.float32


# ---- reference and restatement ------------------------------------------------------------------------------------------------
def _grid():
    for H, W in X.SHAPES:
        for B in X.BATCHES:
            for x in (X.frames(B, H, W), X.band_frames(B, H, W)):
                for jobs in X.case_jobs(B, H, W) + X.chain_jobs(B, H, W):
                    yield (H, W, B), x, jobs


def test_reference_known_answers():
    x = np.zeros((1, 3, 3, 3), f32)
    x[0, 0], x[0, 1], x[0, 2] = 0.5, 0.25, 1.0
    x[0, :, 1, 1] = (0.75, 0.5, 0.0)
    one = lambda *layers: np.array([RA.make_job(layers, 3, 3, fill=(0.1, 0.2, 0.3))])           # noqa: E731
    out, exact, bound = X.ra_ref(x, one((0, None)))
    assert exact.all() and np.array_equal(out, x.astype(np.float64)) and not bound.any()
    out, exact, bound = X.ra_ref(x, one((6, 0.5)))
    assert out[0, :, 0, 0].tolist() == [0.75, 0.375, 1.0] and not exact.any() and (bound > 0).all()
    # TranslateX by one pixel: the output column x shows the input column x - 1, column 0 the fill
    out, exact, _ = X.ra_ref(x, one((3, 1)))
    assert exact.all() and out[0, :, 1, 2].tolist() == [0.75, 0.5, 0.0] and np.allclose(out[0, :, 1, 0], [0.1, 0.2, 0.3], atol=1e-7)
    # a rotation by 90 degrees about the centre of a square frame moves the corners onto each other and keeps the centre
    x2 = np.arange(27, dtype=f32).reshape(1, 3, 3, 3) / f32(32)
    out, _, _ = X.ra_ref(x2, one((5, 90.0)))
    assert out[0, 0, 1, 1] == x2[0, 0, 1, 1] and sorted(out[0, 0].ravel().tolist()) == sorted(x2[0, 0].ravel().tolist())
    assert not np.array_equal(out[0], x2[0])
    # Sharpness: only the centre of a 3 x 3 frame is interior; factor 0 gives the blur (5 x + the neighbours) / 13
    out, exact, _ = X.ra_ref(x, one((9, -1.0)))
    assert exact[0, :, 0, :].all() and exact[0, :, :, 0].all() and not exact[0, :, 1, 1].any()
    np.testing.assert_allclose(out[0, 0, 1, 1], (5 * 0.75 + 8 * 0.5) * X.C13, rtol=1e-15)
    # Solarize, Posterize, AutoContrast on numbers one can do by hand
    out, _, _ = X.ra_ref(x, one((11, 0.5)))
    assert out[0, :, 0, 0].tolist() == [0.5, 0.25, 0.0] and out[0, :, 1, 1].tolist() == [0.25, 0.5, 0.0]
    u = np.array([[[200]], [[77]], [[255]]], np.uint8)
    out, _, _ = X.ra_ref((u.astype(f32) / f32(255))[None], np.array([RA.make_job([(10, 3)], 1, 1)]))
    assert (out[0, :, 0, 0] * 255).round().tolist() == [192, 64, 224]
    out, exact, _ = X.ra_ref(x, one((12, None)))
    assert out[0, 0].tolist() == [[0, 0, 0], [0, 1, 0], [0, 0, 0]] and out[0, 1, 1, 1] == 1 and out[0, 2, 1, 1] == 0 and out[0, 2, 0, 0] == 1
    # Equalize by hand: 510 pixels of two values, counts 300 and 210 -> step (510 - 210) // 255 = 1, lut[a] = 0, lut[b] = 255 capped
    img = np.concatenate([np.full(300, 10), np.full(210, 20)]).astype(np.uint8).reshape(1, 1, 30, 17).repeat(3, axis=1)
    out, _, _ = X.ra_ref(img.astype(f32) / f32(255), np.array([RA.make_job([(13, None)], 30, 17)]))
    assert sorted(set((out * 255).round().ravel().tolist())) == [0.0, 255.0]


def test_restatement_holds_against_the_reference_over_the_grid():
    worst, seen, ops_seen = 0.0, 0, set()
    for tag, x, jobs in _grid():
        ref = X.ra_ref(x, jobs)
        got = RA.apply_host(x, jobs)
        assert got.dtype == f32
        assert X.holds(got, ref), tag + (jobs['op'][:, :3].tolist(), X.worst(got, ref))
        worst = max(worst, X.worst(got, ref))
        ops_seen |= {(int(j['op'][0]), float(j['f'][0][0]), tuple(int(v) for v in j['a'][0])) for j in jobs if j['layers'] == 1}
        seen += 1
    assert {o[0] for o in ops_seen} == set(range(14)) and len(ops_seen) > 100
    print('%d tables, worst error / bound %.3f' % (seen, worst))
    assert worst > 0.01         # the bound is not vacuous


@pytest.mark.parametrize('mutant', X.MUTANTS)
def test_the_checks_tell_a_wrong_implementation_from_the_right_one(mutant):
    assert len(X.MUTANTS) >= 6
    outside = 0
    for tag, x, jobs in _grid():
        if tag[:2] == (1, 1):
            continue
        wrong = X.ra_ref(x, jobs, mutant=mutant)[0].astype(f32)
        outside += int(not X.holds(wrong, X.ra_ref(x, jobs)))
    assert outside > 0, mutant
    print('%s: rejected on %d tables' % (mutant, outside))


def test_apply_host_leaves_its_input_alone_and_refuses_other_shapes():
    x = X.frames(2, 7, 5)
    keep = x.copy()
    jobs = X.case_jobs(2, 7, 5)[3]
    RA.apply_host(x, jobs)
    assert np.array_equal(x, keep)
    with pytest.raises(ValueError):
        RA.apply_host(x.astype(np.float64), jobs)
    with pytest.raises(ValueError):
        RA.apply_host(x, jobs[:1])
    with pytest.raises(ValueError):
        RA.make_job([], 7, 5)
    with pytest.raises(ValueError):
        RA.make_job([(0, None)] * 5, 7, 5)
    assert len(RA.OPS) == 14 and RA.OPS[5] == 'Rotate' and RA.OPS[13] == 'Equalize'


def test_identity_layers_leave_the_image_bit_for_bit():
    from loans_amd import ops
    x = X.frames(1, 7, 5)
    for layers in ([(0, None)], [(1, 0.0), (2, 0.0)], [(3, 0), (4, 0), (5, 0.0)], [(6, 0.0), (7, 0.0), (8, 0.0), (9, 0.0)], [(10, 8)]):
        jobs = np.array([RA.make_job(layers, 7, 5)])
        assert ops.ra_identity(jobs, 7, 5).all() and np.array_equal(RA.apply_host(x, jobs).view(np.uint32), x.view(np.uint32))
    assert not ops.ra_identity(np.array([RA.make_job([(11, 1.0)], 7, 5)]), 7, 5).all()
    sharp = np.array([RA.make_job([(9, 0.5)], 2, 5)])
    assert ops.ra_identity(sharp, 2, 5).all() and not ops.ra_identity(sharp, 3, 5).all()
    assert np.array_equal(RA.apply_host(x[:, :, :2], sharp), x[:, :, :2])


# ---- Pillow ---------------------------------------------------------------------------------------------------------------------
PIL_SHAPES = X.SHAPES + ((224, 224),)


def _bytes(seed, H, W):
    return np.random.RandomState(seed).randint(0, 256, (H, W, 3)).astype(np.uint8)


def _stage(u, layers, fill=(0.0, 0.0, 0.0)):
    """``apply_host`` of one uint8 HWC image under one job -> uint8 HWC (every output is an exact byte over 255, or the fill)"""
    H, W = u.shape[:2]
    x = (u.astype(f32) / f32(255)).transpose(2, 0, 1)[None]
    got = RA.apply_host(np.ascontiguousarray(x), np.array([RA.make_job(layers, H, W, fill)]))[0]
    back = RA._bin(got)
    assert np.array_equal((back.astype(f32) / f32(255)).view(np.uint32), got.view(np.uint32))       # nothing but byte-grid values
    return back.transpose(1, 2, 0).astype(np.uint8)


@pytest.mark.parametrize('H, W', PIL_SHAPES)
def test_the_gathers_equal_pillows_affine_transform_byte_for_byte(H, W):
    u = _bytes(H + W, H, W)
    for b in range(256):
        assert RA._bin(np.array([f32(b) / f32(255)]))[0] == b
    image = Image.fromarray(u)
    fill = (10, 20, 30)
    shears = np.linspace(-0.99, 0.99, 23)
    angles = sorted(set(np.linspace(-135, 135, 56).tolist() + [0.0, 90.0, -90.0, 180.0]))
    cases = [(1, v) for v in shears] + [(2, v) for v in shears] + [(3, t) for t in range(-W, W + 1, max(1, W // 16))] + \
        [(4, t) for t in range(-H, H + 1, max(1, H // 16))] + [(5, a) for a in angles]
    assert len(angles) == 60
    for op, v in cases:
        coef = tuple(float(c) for c in RA.coefficients(op, v, H, W))
        want = np.asarray(image.transform((W, H), Image.AFFINE, coef, Image.NEAREST, fillcolor=fill))
        got = _stage(u, [(op, v)], tuple(f32(c) / f32(255) for c in fill))
        assert np.array_equal(got, want), (op, v)


def _kinds(H, W, seed):
    rng = np.random.RandomState(seed)
    yield rng.randint(0, 256, (H, W, 3)).astype(np.uint8)                               # uniform noise
    yield rng.randint(100, 132, (H, W, 3)).astype(np.uint8)                             # a narrow band
    yield np.round(255 * rng.beta(0.3, 0.3, (H, W, 3))).astype(np.uint8)                # a U shape
    one = np.full((H, W, 3), 77, np.uint8)                                              # one value and one odd pixel
    one[H // 2, W // 2] = (3, 200, 78)
    yield one


@pytest.mark.parametrize('H, W', PIL_SHAPES)
def test_equalize_and_posterize_equal_pillows(H, W):
    real = 0
    for seed in range(3):
        for u in _kinds(H, W, seed):
            image = Image.fromarray(u)
            got = _stage(u, [(13, None)])
            assert np.array_equal(got, np.asarray(ImageOps.equalize(image))), seed
            real += int(not np.array_equal(got, u))
            for bits in range(2, 9):
                assert np.array_equal(_stage(u, [(10, bits)]), np.asarray(ImageOps.posterize(image, bits))), bits
    assert (real > 0) == (H * W >= 510)


# ---- the policy -------------------------------------------------------------------------------------------------------------
def _by_hand(rng, kind, N, M, H, W):
    """the layers of one example, listed from the documented order of the draws and the table of the module docstring"""
    layers = []
    for _ in range(1 if kind == 'trivial' else N):
        op = rng.randrange(14)
        k = M
        if kind == 'trivial':
            k = rng.randrange(31) if 1 <= op <= 11 else 0
        neg = rng.randrange(2) if 1 <= op <= 9 else 0
        wide = kind == 'trivial'
        hi = {1: 0.99 if wide else 0.3, 2: 0.99 if wide else 0.3, 3: 32.0 if wide else 150.0 / 331.0 * W,
              4: 32.0 if wide else 150.0 / 331.0 * H, 5: 135.0 if wide else 30.0}.get(op, 0.99 if wide else 0.9)
        v = hi * k / 30
        v = -v if neg else v
        if op in (3, 4):
            v = int(v)
        if op == 10:
            v = 8 - round(k / (5 if wide else 7.5))
        if op == 11:
            v = float(f32(1 - k / 30))
        layers.append((op, None if op in (0, 12, 13) else v))
    return layers


@pytest.mark.parametrize('kind, N, M', [('rand', 2, 9), ('rand', 4, 30), ('rand', 1, 0), ('trivial', 1, None)])
def test_draw_known_answers_and_the_documented_order(kind, N, M):
    policy, rng = RA.RandAugmentPolicy(kind, N or 1, M if M is not None else 0, seed=11), random.Random(11)
    seen = set()
    for _ in range(40):
        want = RA.make_job(_by_hand(rng, kind, N, M, 33, 65), 33, 65)
        got = policy.draw(33, 65)
        assert got.tobytes() == want.tobytes(), (got, want)
        seen |= set(got['op'][:int(got['layers'])].tolist())
    assert policy.getstate() == rng.getstate()                                  # nothing else is drawn
    assert len(seen) >= 10
    jobs = RA.RandAugmentPolicy(kind, N or 1, M if M is not None else 0, seed=11).draw_batch(3, 33, 65)
    again = RA.RandAugmentPolicy(kind, N or 1, M if M is not None else 0, seed=11)
    assert jobs.tobytes() == b''.join(again.draw(33, 65).tobytes() for _ in range(3))       # the table is the single draws, in order
    assert jobs.dtype == RA_JOB and (jobs['layers'] == (1 if kind == 'trivial' else N)).all()
    np.testing.assert_array_equal(jobs['fill'], np.tile(np.array(P.IMAGENET_MEAN, f32), (3, 1)))


def test_first_jobs_as_numbers():
    """numbers, not code: RandAugmentPolicy('rand', 2, 9, seed=1) on 224 x 224 starts with ShearY then TranslateY"""
    first = RA.RandAugmentPolicy('rand', 2, 9, seed=1).draw(224, 224)
    assert first['op'].tolist() == [2, 4, 0, 0] and int(first['layers']) == 2
    assert first['a'][0].tolist() == [65536, 0, 32768, 5898, 65536, -624886]    # v = +0.09: FIX(0.09) = 5898, FIX(-0.09 * 112 + 0.045 + 0.5)
    assert first['a'][1, :5].tolist() == [65536, 0, 32768, 0, 65536] and abs(int(first['a'][1, 5]) - 32768) == 30 * 65536
    trivial = RA.RandAugmentPolicy('trivial', seed=1).draw(224, 224)
    assert trivial['op'].tolist() == [2, 0, 0, 0] and trivial['a'][0].tolist() == [65536, 0, 32768, 38928, 65536, -4307747]
    for bad in (dict(kind='auto'), dict(layers=0), dict(layers=5), dict(magnitude=31), dict(magnitude=-1), dict(fill=(0.0, float('nan'), 0.0)),
                dict(fill=(0.0, 0.0))):
        with pytest.raises(ValueError):
            RA.RandAugmentPolicy(**bad)


def test_magnitude_zero_still_draws_the_sign_and_gives_identities():
    from loans_amd import ops
    policy, rng = RA.RandAugmentPolicy('rand', 3, 0, seed=5), random.Random(5)
    jobs = policy.draw_batch(50, 16, 12)
    for _ in range(150):
        if 1 <= rng.randrange(14) <= 9:
            rng.randrange(2)
    assert policy.getstate() == rng.getstate()
    same = ops.ra_identity(jobs, 16, 12)
    assert same[:, 3].all() and (same[:, :3] == (jobs['op'][:, :3] <= 10)).all()        # at bin 0 only 11, 12, 13 act


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


PHOTO_ON = dict(brightness=0.4, contrast=0.4, saturation=0.4, lighting_std=0.1, erase_prob=0.5)


def _stack(crop_seed, ra_seed, photo_seed, mix_seed, ra=True):
    from loans_amd.common.datasets.shard import ShardedDataset
    inner = ShardedDataset(_Crops(crop_seed), 0, 1, pad=True)
    if ra:
        inner = RA.RandAugmentBatches(inner, RA.RandAugmentPolicy('rand', 2, 9, seed=ra_seed))
    photo = P.PhotometricBatches(inner, P.PhotoPolicy(seed=photo_seed, **PHOTO_ON))
    return BM.MixedBatches(photo, BM.MixPolicy(0.4, 1.0, seed=mix_seed))


def test_the_other_streams_do_not_depend_on_the_wrapper_and_the_state_round_trips():
    from loans_amd.runtime.training import _as_draw_state
    without, wrapped = _stack(4, None, 9, 8, ra=False), _stack(4, 6, 9, 8)
    assert len(wrapped) == 6 and wrapped.image_size == (16, 12) and wrapped.dataset.dataset.image_size == (16, 12)
    assert not hasattr(wrapped.dataset.dataset, 'cache')
    batches = [[0, 1, 2], [3, 4, 5], [0, 1, 2], [3, 4, 5]]
    alone = RA.RandAugmentPolicy('rand', 2, 9, seed=6)
    seen = []
    for n, idx in enumerate(batches):
        if n == 2:
            state = wrapped.draw_state()
        ((inner, jobs), photo), mix = wrapped.decode_batch(idx)
        (plain_inner, plain_photo), plain_mix = without.decode_batch(idx)
        # the same crops, the same photometric jobs and the same mix, with the stage or without
        assert inner == plain_inner and photo.tobytes() == plain_photo.tobytes() and mix == plain_mix
        assert jobs.dtype == RA_JOB and jobs.shape == (3,) and jobs.tobytes() == alone.draw_batch(3, 16, 12).tobytes()
        seen.append((inner, jobs.tobytes(), photo.tobytes(), mix))
    ((crop_state, ra_state), photo_state), mix_state = state
    assert isinstance(ra_state, tuple) and len(state) == 2
    fresh = _stack(None, None, None, None)
    arrays = {}
    packed = json.loads(json.dumps(checkpoint.pack(state, 'draw', arrays)))
    fresh.set_draw_state(_as_draw_state(checkpoint.unpack(packed, arrays)))
    for n in (2, 3):
        ((inner, jobs), photo), mix = fresh.decode_batch(batches[n])
        assert (inner, jobs.tobytes(), photo.tobytes(), mix) == seen[n]
    stage = wrapped.dataset.dataset
    stage.reseed(4)
    first = stage.decode_batch(batches[0])
    stage.reseed(4)
    again = stage.decode_batch(batches[0])
    assert first[0] == again[0] and first[1].tobytes() == again[1].tobytes()


def test_the_wrapper_hands_the_inner_batch_on_with_its_cache_counts_and_forwards_the_cache():
    import torch
    from loans_amd.common.datasets.classification_dataset import FeedBatch

    class Cached(_Crops):
        cache = 'the cache'

        def finish_batch(self, decoded, device, map_fn=map):
            batch = FeedBatch((torch.zeros(len(decoded[0]), 3, 16, 12), torch.zeros(len(decoded[0]), dtype=torch.int32)))
            batch.cache_hits, batch.cache_misses = 2, 1
            return batch

    wrapper = RA.RandAugmentBatches(Cached(1), RA.RandAugmentPolicy('rand', 1, 0, seed=3))
    assert wrapper.cache == 'the cache' and len(wrapper) == 6
    # seed 3 at bin 0 starts with ops that are identities there: no launch, the inner batch itself
    for _ in range(20):
        decoded = wrapper.decode_batch([0, 1, 2])
        if (decoded[1]['op'][:, 0] <= 10).all():
            break
    batch = wrapper.finish_batch(decoded, None)
    assert isinstance(batch, FeedBatch) and (batch.cache_hits, batch.cache_misses) == (2, 1) and not batch[0].any()
    with pytest.raises(ValueError):
        RA.RandAugmentBatches(Cached(1), RA.RandAugmentPolicy(seed=1), image_size=(8, 8)).finish_batch(wrapper.decode_batch([0]), None)
    with pytest.raises(AttributeError):
        wrapper.nothing


# ---- the trainer's options ----------------------------------------------------------------------------------------------------
NEW = ('rand_augment', 'trivial_augment', 'ra_fill', 'ra_seed')
DEFAULTS = (None, False, (0.485, 0.456, 0.406), None)
BARE_KEYS = {'train_file', 'val_file', 'use_resnet_18', 'batch_size', 'gpu', 'learning_rate', 'weight_decay', 'optimizer', 'momentum',
             'lr_drop_epochs', 'lr_drop_factor', 'label_smoothing', 'topk', 'num_epoch', 'iterations', 'image_size', 'log_dir', 'ln',
             'log_interval', 'snapshot_interval', 'dtype', 'seed', 'no_shuffle', 'validation', 'dataset_size', 'validation_size',
             'synthetic_classes', 'data_seed', 'flat_log_dir', 'loader_threads'}


def test_the_options_parse_and_leave_the_default_namespace_alone():
    import train_imagenet as T
    bare = T.parse_args([])
    assert not set(NEW) & set(vars(bare)) and set(vars(bare)) == BARE_KEYS
    assert tuple(getattr(bare, n) for n in NEW) == DEFAULTS
    args = T.parse_args(['--augment', 'rrc', '--rand-augment', '2', '9', '--ra-fill', '0', '0.5', '1', '--ra-seed', '3'])
    assert (tuple(args.rand_augment), tuple(args.ra_fill), args.ra_seed, args.trivial_augment) == ((2, 9), (0.0, 0.5, 1.0), 3, False)
    assert set(vars(args)) == set(vars(bare)) | {'rand_augment', 'ra_fill', 'ra_seed', 'augment'}
    trivial = T.parse_args(['--augment', 'rrc', '--trivial-augment'])
    assert trivial.trivial_augment is True and trivial.rand_augment is None
    assert set(T.Arguments._RA) == set(NEW) and set(NEW) <= set(T.RESUME_FIXED)
    for a in (bare, args, trivial):
        T.check_ra_arguments(a)
    assert not T.ra_enabled(bare) and T.ra_enabled(args) and T.ra_enabled(trivial)
    for edge in (['1', '0'], ['4', '30']):
        T.parse_args(['--augment', 'rrc', '--rand-augment'] + edge)


@pytest.mark.parametrize('argv', [
    ['--augment', 'rrc', '--rand-augment', '0', '9'],
    ['--augment', 'rrc', '--rand-augment', '5', '9'],
    ['--augment', 'rrc', '--rand-augment', '2', '31'],
    ['--augment', 'rrc', '--rand-augment', '2', '-1'],
    ['--augment', 'rrc', '--rand-augment', '2', '9', '--trivial-augment'],
    ['--rand-augment', '2', '9'],                                           # the stage needs the device feed
    ['--trivial-augment', '--augment', 'none'],
    ['--augment', 'rrc', '--trivial-augment', '--ra-fill', '0', 'inf', '0'],
    ['--augment', 'rrc', '--rand-augment', '2', '9', '--ra-fill', 'nan', '0', '0'],
])
def test_the_options_are_refused_by_the_parser_and_by_the_check(argv, capsys):
    import train_imagenet as T
    with pytest.raises(SystemExit):
        T.parse_args(argv)
    capsys.readouterr()
    args = T.Arguments()                # the same values on a namespace that never went through the parser
    i = 0
    while i < len(argv):
        name = argv[i][2:].replace('-', '_')
        i += 1
        values = []
        while i < len(argv) and not (argv[i].startswith('--') and not argv[i][2:3].isdigit()):
            values.append(argv[i])
            i += 1
        if name == 'augment':
            args.augment = values[0]
        elif name == 'trivial_augment':
            args.trivial_augment = True
        elif name == 'rand_augment':
            args.rand_augment = tuple(int(v) for v in values)
        else:
            args.ra_fill = tuple(float(v) for v in values)
    with pytest.raises(ValueError):
        T.check_ra_arguments(args)


def test_a_checkpoint_from_before_the_options_resumes_at_their_defaults_only():
    import train_imagenet as T
    args = T.parse_args(['--augment', 'rrc'])
    saved = {k: v for k, v in checkpoint.plain_arguments(args).items() if k not in NEW}
    fixed = [k for k in T.RESUME_FIXED if k != 'gpus']
    assert checkpoint.check_arguments(saved, args, fixed, checkpoint.SILENT, T.RESUME_DEFAULTS_WITH_RA) == []
    for extra, name in ((['--rand-augment', '2', '9'], 'rand_augment'), (['--trivial-augment'], 'trivial_augment'),
                        (['--ra-seed', '1'], 'ra_seed'), (['--ra-fill', '0', '0', '0'], 'ra_fill')):
        given = T.parse_args(['--augment', 'rrc'] + extra)
        with pytest.raises(ValueError, match=name):
            checkpoint.check_arguments(saved, given, fixed, checkpoint.SILENT, T.RESUME_DEFAULTS_WITH_RA)
    given = T.parse_args(['--augment', 'rrc', '--rand-augment', '2', '9', '--ra-seed', '2'])
    now = checkpoint.plain_arguments(given)
    assert checkpoint.check_arguments(now, given, fixed, checkpoint.SILENT, T.RESUME_DEFAULTS_WITH_RA) == []
    for other in (['--rand-augment', '2', '9', '--ra-seed', '3'], ['--rand-augment', '2', '10', '--ra-seed', '2'], ['--trivial-augment', '--ra-seed', '2']):
        with pytest.raises(ValueError):
            checkpoint.check_arguments(now, T.parse_args(['--augment', 'rrc'] + other), fixed, checkpoint.SILENT, T.RESUME_DEFAULTS_WITH_RA)
    spelled = T.parse_args(['--augment', 'rrc', '--ra-fill', '0.485', '0.456', '0.406'])
    assert checkpoint.check_arguments(saved, spelled, fixed, checkpoint.SILENT, T.RESUME_DEFAULTS_WITH_RA) == []
    assert T.RESUME_DEFAULTS_RA == dict(zip(NEW, DEFAULTS))
    assert T.RESUME_DEFAULTS_WITH_RA == dict(T.RESUME_DEFAULTS_WITH_LOSS, **T.RESUME_DEFAULTS_RA)
    assert not set(NEW) & set(T.RESUME_DEFAULTS_WITH_LOSS)                     # the older tables are what they were


# ---- the struct and the entries without a GPU -----------------------------------------------------------------------------------
def test_ra_job_has_the_headers_layout(tmp_path):
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "loans_hip.h"', 'int main(void) {',
           '  printf("size %zu\\n", sizeof(loans_ra_job));']
    for f in RA_JOB.names:
        src.append('  printf("%s %%zu\\n", offsetof(loans_ra_job, %s));' % (f, f))
    src += ['  return 0;', '}']
    c_file, exe = tmp_path / 'layout.c', tmp_path / 'layout'
    c_file.write_text('\n'.join(src))
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), '-o', str(exe), str(c_file)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(got['size']) == RA_JOB.itemsize == 256
    for f in RA_JOB.names:
        assert int(got[f]) == RA_JOB.fields[f][1], f
    assert RA_JOB.fields['a'][0].shape == (4, 6) and RA_JOB.fields['f'][0].shape == (4, 2) and RA_JOB.fields['op'][0].shape == (4,)


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from loans_amd import _lib
    return _lib.load()


def test_ra_entries_check_their_arguments_before_any_hip_call(lib):
    from loans_amd import _lib
    assert 'loans_ra_workspace_bytes' in _lib.RESTYPES
    ws_bytes = lib.loans_ra_workspace_bytes
    # per image one 3072-byte record per 4096 pixels (2048 at most) and one folded record of 3136 bytes, then the scratch batch
    assert ws_bytes(2, 16, 12) == 2 * 3072 + 2 * 3136 + 2 * 3 * 16 * 12 * 4
    assert ws_bytes(256, 224, 224) == 256 * 13 * 3072 + 256 * 3136 + 256 * 3 * 224 * 224 * 4
    assert ws_bytes(1, 4097, 1) == 2 * 3072 + 3136 + 3 * 4097 * 4
    assert ws_bytes(0, 4, 4) == -1 and ws_bytes(4, 0, 4) == -1 and ws_bytes(4, 4, -1) == -1
    need = ws_bytes(2, 4, 4)
    buf = ctypes.create_string_buffer(need + 4096)
    base = (ctypes.addressof(buf) + 63) & ~63
    x, out, jd, ws = base, base + 512, base + 1024, base + 2048
    jobs = np.zeros(2, RA_JOB)
    jobs[0] = RA.make_job([(5, 30.0), (8, 0.5), (10, 4), (11, 0.5)], 4, 4)
    jobs[1] = RA.make_job([(13, None)], 4, 4)
    good = dict(x=x, out=out, B=2, C=3, H=4, W=4, jobs_dev=jd, jobs_host=jobs.ctypes.data, layer=1, ws=ws, ws_bytes=need)
    stats_order = ('x', 'B', 'C', 'H', 'W', 'jobs_dev', 'jobs_host', 'layer', 'ws', 'ws_bytes')
    apply_order = ('x', 'out', 'B', 'C', 'H', 'W', 'jobs_dev', 'jobs_host', 'ws', 'ws_bytes')

    def both(change, table=None):
        args = dict(good, **change)
        if table is not None:
            args['jobs_host'] = table.ctypes.data
        return (lib.loans_ra_stats_f32(*[args[n] for n in stats_order], 0), lib.loans_ra_apply_f32(*[args[n] for n in apply_order], 0))

    for change in (dict(x=0), dict(jobs_dev=0), dict(jobs_host=0), dict(ws=0), dict(B=0), dict(C=1), dict(C=4), dict(H=0), dict(W=-2),
                   dict(x=x + 2), dict(jobs_dev=jd + 4), dict(ws=ws + 8), dict(ws_bytes=need - 1)):
        assert both(change) == (-1, -1), change
    for change in (dict(out=0), dict(out=out + 2)):
        assert lib.loans_ra_apply_f32(*[dict(good, **change)[n] for n in apply_order], 0) == -1
    for layer in (-1, 4):
        assert lib.loans_ra_stats_f32(*[dict(good, layer=layer)[n] for n in stats_order], 0) == -1
    nan, inf = float('nan'), float('inf')
    for field, index, value in (('layers', (0,), 0), ('layers', (0,), 5), ('layers', (1,), -1), ('op', (0, 0), 14), ('op', (1, 0), -1),
                                ('f', (0, 1, 0), nan), ('f', (0, 1, 1), inf), ('f', (0, 3, 0), -inf), ('a', (0, 2, 0), 1), ('a', (0, 2, 0), 9),
                                ('a', (0, 0, 0), (1 << 20) + 1), ('a', (0, 0, 4), -(1 << 20) - 1), ('a', (0, 0, 2), (1 << 50) + 1),
                                ('a', (0, 0, 5), -(1 << 50) - 1), ('fill', (1, 2), nan), ('fill', (0, 0), inf)):
        table = jobs.copy()
        table[field][index] = value
        assert both({}, table) == (-1, -1), (field, index, value)
    # what lies beyond a job's layer count is not read
    table = jobs.copy()
    table['op'][1, 1:], table['f'][1, 1:] = 99, nan
    assert lib.loans_ra_stats_f32(*[dict(good, jobs_host=table.ctypes.data, layer=3)[n] for n in stats_order], 0) == 0
    assert both(dict(H=1 << 10, W=1 << 20, ws_bytes=1 << 62)) == (-2, -2)              # an image past 32-bit indexing
    # no image whose layer needs a statistic: the entry has nothing to launch and says so without touching a device; nor has
    # the stage in place where every layer is the identity
    assert lib.loans_ra_stats_f32(*[dict(good, layer=2)[n] for n in stats_order], 0) == 0
    same = np.array([RA.make_job([(0, None), (6, 0.0)], 4, 4)] * 2)
    assert lib.loans_ra_apply_f32(x, x, 2, 3, 4, 4, jd, same.ctypes.data, ws, need, 0) == 0
    assert bytes(buf) == bytes(need + 4096)
