"""No GPU, no launch: the photometric draws (loans_amd/common/datasets/photometric.py), the fp32 restatement held to the derived
bound over the case grid, the bound's power to tell four wrong implementations from the right one, the trainer's options and
their resume rules, the job struct's layout and the two entries' argument checks."""
import ctypes
import json
import math
import os
import random
import subprocess

import numpy as np
import pytest

from loans_amd.common.datasets import batch_mix as BM
from loans_amd.common.datasets import photometric as P
from loans_amd.ops import PHOTO_JOB
from loans_amd.runtime import checkpoint
from tests.imagenet_photo import reference as X

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


# ---- reference, restatement and bound -----------------------------------------------------------------------------------------
def test_float64_reference_known_answers():
    x = np.zeros((1, 3, 2, 2), np.float32)
    x[0, 0], x[0, 1], x[0, 2] = 0.5, 0.25, 1.0
    w = X.W32
    grey = w[0] * 0.5 + w[1] * 0.25 + w[2] * 1.0
    # brightness alone
    out, copies, bound = X.photo_ref(x, np.array([P.make_job(b=1.5)]))
    assert out[0, :, 0, 0].tolist() == [0.75, 0.375, 1.0] and not copies.any() and (bound > 0).all()
    # saturation 0: every channel the grey; contrast 0 on a flat image: the mean grey, the same number
    out, _, _ = X.photo_ref(x, np.array([P.make_job(s=0.0)]))
    np.testing.assert_allclose(out, grey, rtol=1e-15)
    out, _, _ = X.photo_ref(x, np.array([P.make_job(c=0.0)]))
    np.testing.assert_allclose(out, grey, rtol=1e-15)
    # the mean is the intermediate image's: brightness 0.5 first halves it, contrast first does not
    first = X.photo_ref(x, np.array([P.make_job(b=0.5, c=0.0, order=0)]))[0]
    np.testing.assert_allclose(first, grey / 2, rtol=1e-15)
    last = X.photo_ref(x, np.array([P.make_job(b=0.5, c=0.0, order=2)]))[0]
    np.testing.assert_allclose(last, grey / 2, rtol=1e-15)                  # (C then B: 0.5 * grey -- the same number here)
    x[0, :, 0, 0] = 0.0                                                       # no longer flat
    a = X.photo_ref(x, np.array([P.make_job(b=2.0, c=0.5, order=0)]))[0]      # B, C: the mean of the clamped doubled image
    doubled = np.clip(2.0 * x.astype(np.float64), 0, 1)
    m = (w[0] * doubled[0, 0] + w[1] * doubled[0, 1] + w[2] * doubled[0, 2]).mean()
    np.testing.assert_allclose(a, np.clip(0.5 * doubled + 0.5 * m, 0, 1), rtol=1e-15)
    # the identity, the addend without a clamp, the box with its fill
    job = P.make_job(add=(0.5, 0.0, -2.0), box=(0, 1, 2, 2), fill=(7.0, 8.0, 9.0))
    out, copies, bound = X.photo_ref(x, np.array([job]))
    assert out[0, :, 1, 0].tolist() == [1.0, 0.25, -1.0] and out[0, :, 1, 1].tolist() == [7.0, 8.0, 9.0]
    assert copies[0, :, :, 1].all() and not copies[0, :, :, 0].any() and not bound[copies].any()
    out, copies, bound = X.photo_ref(x, np.array([P.make_job()]))
    assert copies.all() and np.array_equal(out, x.astype(np.float64)) and not bound.any()


def _grid():
    for H, W in X.SHAPES:
        for B in X.BATCHES:
            x = X.frames(B, H, W)
            for jobs in X.case_jobs(B, H, W):
                yield (H, W, B), x, jobs


def test_restatement_is_inside_the_bound_over_the_grid_and_copies_are_exact():
    worst, seen, orders, triples = 0.0, 0, set(), set()
    for tag, x, jobs in _grid():
        out64, copies, bound = X.photo_ref(x, jobs)
        got = P.apply_host(x, jobs)
        assert got.dtype == np.float32
        err = np.abs(got.astype(np.float64) - out64)
        assert np.all(err <= bound), tag + (jobs, float((err - bound).max()))
        assert np.array_equal(got.view(np.uint32)[copies], out64.astype(np.float32).view(np.uint32)[copies]), tag
        live = ~copies
        if live.any():
            worst = max(worst, float((err[live] / bound[live]).max()))
        orders |= set(int(o) for o in jobs['order'])
        triples |= set(zip(jobs['b'].tolist(), jobs['c'].tolist(), jobs['s'].tolist()))
        seen += 1
    assert orders == set(range(6)) and len(triples) == len(X.FACTORS) ** 3 and (1.0, 1.0, 1.0) in triples
    print('%d tables, worst error / bound %.3f' % (seen, worst))
    assert worst > 0.01         # the bound is not vacuous: the restatement comes within two orders of magnitude of it


@pytest.mark.parametrize('mutant', X.MUTANTS)
def test_the_bound_tells_a_wrong_implementation_from_the_right_one(mutant):
    outside = 0
    for tag, x, jobs in _grid():
        if tag[:2] == (1, 1):
            continue
        out64, copies, bound = X.photo_ref(x, jobs)
        wrong = X.photo_ref(x, jobs, mutant=mutant)[0]
        outside += int(np.any(np.abs(wrong - out64) > bound))
    assert outside > 0, mutant
    print('%s: outside the bound on %d tables' % (mutant, outside))


def test_apply_host_leaves_its_input_alone_and_refuses_other_shapes():
    x = X.frames(2, 7, 5)
    keep = x.copy()
    jobs = X.case_jobs(2, 7, 5)[3]
    P.apply_host(x, jobs)
    assert np.array_equal(x, keep)
    with pytest.raises(ValueError):
        P.apply_host(x.astype(np.float64), jobs)
    with pytest.raises(ValueError):
        P.apply_host(x, jobs[:1])


# ---- the policy -------------------------------------------------------------------------------------------------------------
ALL_ON = dict(brightness=0.4, contrast=0.4, saturation=0.4, lighting_std=0.1, erase_prob=0.5)


def test_draw_known_answers():
    """seed 11, every stage on, 16 x 12 frames: the first three jobs, listed by hand from the documented order of the draws"""
    policy = P.PhotoPolicy(seed=11, **ALL_ON)
    rng = random.Random(11)
    for _ in range(3):
        perm = [0, 1, 2]
        rng.shuffle(perm)
        f = [rng.uniform(0.6, 1.4) for _ in range(3)]
        alpha = [rng.gauss(0.0, 0.1) for _ in range(3)]
        box = (0, 0, 0, 0)
        if rng.random() < 0.5:
            for _ in range(10):
                area = 16 * 12 * rng.uniform(0.02, 0.33)
                ar = math.exp(rng.uniform(math.log(0.3), math.log(3.3)))
                h, w = int(round(math.sqrt(area * ar))), int(round(math.sqrt(area / ar)))
                if h < 16 and w < 12:
                    y = rng.randint(0, 16 - h)
                    x = rng.randint(0, 12 - w)
                    box = (y, x, y + h, x + w)
                    break
        j = policy.draw(16, 12)
        assert P.ORDERS[int(j['order'])] == tuple(perm)
        assert (j['b'], j['c'], j['s']) == tuple(np.float32(v) for v in f)
        assert j['omc'] == np.float32(1) - np.float32(f[1]) and j['oms'] == np.float32(1) - np.float32(f[2])
        V, lam = np.array(P.LIGHTING_EIGVEC), np.array(P.LIGHTING_EIGVAL)
        want = np.array([sum(V[r][k] * alpha[k] * lam[k] for k in range(3)) for r in range(3)])
        np.testing.assert_allclose(j['add'], want.astype(np.float32), rtol=1e-6, atol=0)
        assert (int(j['y0']), int(j['x0']), int(j['y1']), int(j['x1'])) == box
        np.testing.assert_array_equal(j['fill'], np.array(P.IMAGENET_MEAN, np.float32))
    assert policy.getstate() == rng.getstate()
    # numbers, not code: the first job of this stream
    first = P.PhotoPolicy(seed=11, **ALL_ON).draw(16, 12)
    assert (int(first['order']), int(first['y0']), int(first['x0']), int(first['y1']), int(first['x1'])) == FIRST_JOB_INTS
    np.testing.assert_allclose([first['b'], first['c'], first['s']], FIRST_JOB_FACTORS, rtol=1e-6)
    np.testing.assert_allclose(first['add'], FIRST_JOB_ADD, rtol=1e-5)


# the first job of PhotoPolicy(seed=11, **ALL_ON).draw(16, 12), written down from a run of the documented draws
FIRST_JOB_INTS = (1, 11, 0, 15, 3)                   # brightness, saturation, contrast; rows 11 .. 14, columns 0 .. 2
FIRST_JOB_FACTORS = (0.96146584, 1.2840365, 0.75192165)
FIRST_JOB_ADD = (-0.0061972076, -0.004583251, -0.0034840887)


def test_lighting_addend_known_answers():
    # alpha = (1, 0, 0): the first eigenvector's column times the first eigenvalue
    np.testing.assert_allclose(P.lighting_addend((1, 0, 0)), [-0.5675 * 0.2175, -0.5808 * 0.2175, -0.5836 * 0.2175], rtol=1e-15)
    np.testing.assert_allclose(P.lighting_addend((0, 2, 0)), [0.7192 * 0.0376, -0.0045 * 0.0376, -0.6948 * 0.0376], rtol=1e-15)
    np.testing.assert_allclose(P.lighting_addend((0, 0, -1)), [-0.4009 * 0.0045, 0.8140 * 0.0045, -0.4203 * 0.0045], rtol=1e-15)
    assert not P.lighting_addend((0, 0, 0)).any()


def test_the_stream_is_consumed_in_the_documented_order_and_only_by_what_is_on():
    off = P.PhotoPolicy(seed=1)
    state = off.getstate()
    job = off.draw(16, 12)
    assert off.getstate() == state and not off.active and job.tobytes() == P.make_job().tobytes()       # nothing on: no draw is taken
    # one strength: the shuffle, then one uniform
    policy, rng = P.PhotoPolicy(contrast=0.3, seed=2), random.Random(2)
    for _ in range(20):
        perm = [0, 1, 2]
        rng.shuffle(perm)
        c = rng.uniform(0.7, 1.3)
        j = policy.draw(16, 12)
        assert P.ORDERS[int(j['order'])] == tuple(perm) and j['c'] == np.float32(c) and j['b'] == 1 and j['s'] == 1
        assert j['omc'] == np.float32(1) - np.float32(c) and j['oms'] == 0 and not j['add'].any()
    assert policy.getstate() == rng.getstate()
    # a strength above one: the lower end is 0, not negative
    policy, rng = P.PhotoPolicy(brightness=1.5, seed=3), random.Random(3)
    for _ in range(20):
        rng.shuffle([0, 1, 2])
        assert policy.draw(4, 4)['b'] == np.float32(rng.uniform(0.0, 2.5))
    # lighting alone: three gauss, no shuffle; erasing alone: random() first
    policy, rng = P.PhotoPolicy(lighting_std=0.1, seed=4), random.Random(4)
    j = policy.draw(16, 12)
    np.testing.assert_array_equal(j['add'], P.lighting_addend([rng.gauss(0.0, 0.1) for _ in range(3)]).astype(np.float32))
    assert j['order'] == 0 and policy.getstate() == rng.getstate()
    policy, rng = P.PhotoPolicy(erase_prob=0.3, seed=5), random.Random(5)
    erased = 0
    for _ in range(100):
        j = policy.draw(16, 12)
        if rng.random() < 0.3:
            twin = P.PhotoPolicy(erase_prob=0.3)
            twin.setstate(rng.getstate())
            box = twin.erase_box(16, 12)
            rng.setstate(twin.getstate())
            erased += 1
        else:
            box = (0, 0, 0, 0)
        assert (int(j['y0']), int(j['x0']), int(j['y1']), int(j['x1'])) == box
        y0, x0, y1, x1 = box
        assert 0 <= y0 <= y1 <= 16 and 0 <= x0 <= x1 <= 12 and y1 - y0 < 16 and x1 - x0 < 12
    assert 10 < erased < 60 and policy.getstate() == rng.getstate()
    for bad in (dict(brightness=-0.1), dict(lighting_std=-1), dict(erase_prob=1.5), dict(erase_scale=(0.5, 0.1)),
                dict(erase_ratio=(0.0, 1.0)), dict(erase_value=(0.0, float('nan'), 0.0))):
        with pytest.raises(ValueError):
            P.PhotoPolicy(**bad)


def test_the_erase_draw_gives_up_after_ten_attempts():
    """a 2 x 2 frame with scale (0.9, 1): h < 2 and w < 2 would need an area below 2.25 / max(ar, 1 / ar) <= 2.25, the area is >= 3.6"""
    policy, rng = P.PhotoPolicy(erase_prob=1.0, erase_scale=(0.9, 1.0), seed=6), random.Random(6)
    for _ in range(5):
        j = policy.draw(2, 2)
        assert (int(j['y0']), int(j['x0']), int(j['y1']), int(j['x1'])) == (0, 0, 0, 0)
        rng.random()
        for _ in range(10):             # exactly ten attempts of two draws each, no randint
            rng.uniform(0.9, 1.0)
            rng.uniform(math.log(0.3), math.log(3.3))
        assert policy.getstate() == rng.getstate()


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


def _stack(crop_seed, photo_seed, mix_seed):
    from loans_amd.common.datasets.shard import ShardedDataset
    photo = P.PhotometricBatches(ShardedDataset(_Crops(crop_seed), 0, 1, pad=True), P.PhotoPolicy(seed=photo_seed, **ALL_ON))
    return BM.MixedBatches(photo, BM.MixPolicy(0.4, 1.0, seed=mix_seed))


def test_the_crop_and_mix_streams_do_not_depend_on_the_wrapper_and_the_state_round_trips():
    from loans_amd.common.datasets.shard import ShardedDataset
    from loans_amd.runtime.training import _as_draw_state
    bare = _Crops(4)
    unwrapped = BM.MixedBatches(ShardedDataset(_Crops(4), 0, 1, pad=True), BM.MixPolicy(0.4, 1.0, seed=8))
    wrapped = _stack(4, 9, 8)
    assert len(wrapped) == 6 and wrapped.image_size == (16, 12) and wrapped.dataset.image_size == (16, 12)
    assert not hasattr(wrapped, 'cache') and not hasattr(wrapped.dataset, 'cache')
    batches = [[0, 1, 2], [3, 4, 5], [0, 1, 2], [3, 4, 5]]
    alone, one = P.PhotoPolicy(seed=9, **ALL_ON), P.PhotoPolicy(seed=9, **ALL_ON)
    seen = []
    for n, idx in enumerate(batches):
        if n == 2:
            state = wrapped.draw_state()
        (inner, jobs), mix = wrapped.decode_batch(idx)
        plain_inner, plain_mix = unwrapped.decode_batch(idx)
        assert inner == bare.decode_batch(idx) == plain_inner and mix == plain_mix      # the same crops and the same mix, with the stage or without
        assert jobs.dtype == PHOTO_JOB and jobs.shape == (3,)
        assert jobs.tobytes() == alone.draw_batch(3, 16, 12).tobytes()                  # one job per example, from a stream of its own
        assert jobs.tobytes() == b''.join(one.draw(16, 12).tobytes() for _ in range(3))   # the table is the single draws, in order
        seen.append((inner, jobs.tobytes(), mix))
    (crop_state, photo_state), mix_state = state
    assert isinstance(photo_state, tuple) and len(state) == 2
    # through a checkpoint's JSON and back: batches 3 and 4 again, from fresh streams
    fresh = _stack(None, None, None)
    arrays = {}
    packed = json.loads(json.dumps(checkpoint.pack(state, 'draw', arrays)))
    fresh.set_draw_state(_as_draw_state(checkpoint.unpack(packed, arrays)))
    for n in (2, 3):
        (inner, jobs), mix = fresh.decode_batch(batches[n])
        assert (inner, jobs.tobytes(), mix) == seen[n]
    # reseed reaches every stream's owner below the wrapper it is called on
    photo = wrapped.dataset
    photo.reseed(4)
    first = photo.decode_batch(batches[0])
    photo.reseed(4)
    again = photo.decode_batch(batches[0])
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

    wrapper = P.PhotometricBatches(Cached(1), P.PhotoPolicy(seed=1))            # nothing on: every job is the identity, no launch
    assert wrapper.cache == 'the cache' and len(wrapper) == 6
    batch = wrapper.finish_batch(wrapper.decode_batch([0, 1, 2]), None)
    assert isinstance(batch, FeedBatch) and (batch.cache_hits, batch.cache_misses) == (2, 1) and not batch[0].any()
    with pytest.raises(ValueError):
        P.PhotometricBatches(Cached(1), P.PhotoPolicy(seed=1), image_size=(8, 8)).finish_batch(wrapper.decode_batch([0]), None)
    with pytest.raises(AttributeError):
        wrapper.nothing


# ---- the trainer's options ----------------------------------------------------------------------------------------------------
NEW = ('color_jitter', 'lighting_std', 'random_erase_prob', 'random_erase_scale', 'random_erase_ratio', 'random_erase_value', 'photo_seed')
DEFAULTS = ((0.0, 0.0, 0.0), 0.0, 0.0, (0.02, 0.33), (0.3, 3.3), (0.485, 0.456, 0.406), None)


def test_the_photo_options_parse_and_leave_the_default_namespace_alone():
    import train_imagenet as T
    bare = T.parse_args([])
    assert not set(NEW) & set(vars(bare))                                     # class-level defaults, not parsed values
    assert set(vars(bare)) == BARE_KEYS
    assert tuple(getattr(bare, n) for n in NEW) == DEFAULTS
    args = T.parse_args(['--augment', 'rrc', '--color-jitter', '0.4', '0.3', '0.2', '--lighting-std', '0.1', '--random-erase-prob', '0.25',
                         '--random-erase-scale', '0.05', '0.2', '--random-erase-ratio', '0.5', '2', '--random-erase-value', '0', '0.5', '1',
                         '--photo-seed', '3'])
    assert tuple(tuple(v) if isinstance(v, list) else v for v in (getattr(args, n) for n in NEW)) == \
        ((0.4, 0.3, 0.2), 0.1, 0.25, (0.05, 0.2), (0.5, 2.0), (0.0, 0.5, 1.0), 3)
    assert set(vars(args)) == set(vars(bare)) | set(NEW) | {'augment'}
    assert set(T.Arguments._PHOTO) == set(NEW) and set(NEW) <= set(T.RESUME_FIXED)
    T.check_photo_arguments(bare)
    T.check_photo_arguments(args)
    assert not T.photo_enabled(bare) and T.photo_enabled(args)
    # one stage is enough, and hue is named as not built
    assert T.photo_enabled(T.parse_args(['--augment', 'rrc', '--random-erase-prob', '0.1']))
    import contextlib
    import io
    text = io.StringIO()
    with contextlib.redirect_stdout(text), pytest.raises(SystemExit):
        T.parse_args(['--help'])
    assert 'hue is not built' in ' '.join(text.getvalue().split())


# what a bare parse holds today, before and after this stage: the options of a run that gives none of them
BARE_KEYS = {'train_file', 'val_file', 'use_resnet_18', 'batch_size', 'gpu', 'learning_rate', 'weight_decay', 'optimizer', 'momentum',
             'lr_drop_epochs', 'lr_drop_factor', 'label_smoothing', 'topk', 'num_epoch', 'iterations', 'image_size', 'log_dir', 'ln',
             'log_interval', 'snapshot_interval', 'dtype', 'seed', 'no_shuffle', 'validation', 'dataset_size', 'validation_size',
             'synthetic_classes', 'data_seed', 'flat_log_dir', 'loader_threads'}


@pytest.mark.parametrize('argv', [
    ['--color-jitter', '0.4', '0.4', '0.4'],                                 # the stage needs the device feed
    ['--lighting-std', '0.1', '--augment', 'none'],
    ['--random-erase-prob', '0.25'],
    ['--augment', 'rrc', '--color-jitter', '0.4', '-0.1', '0.4'],
    ['--augment', 'rrc', '--lighting-std', '-0.1'],
    ['--augment', 'rrc', '--random-erase-prob', '1.5'],
    ['--augment', 'rrc', '--random-erase-prob', '-0.1'],
    ['--augment', 'rrc', '--random-erase-prob', 'nan'],
    ['--augment', 'rrc', '--random-erase-scale', '0.3', '0.1'],
    ['--augment', 'rrc', '--random-erase-scale', '0', '0.1'],
    ['--augment', 'rrc', '--random-erase-ratio', '2', '0.5'],
    ['--augment', 'rrc', '--random-erase-ratio', '-1', '0.5'],
    ['--augment', 'rrc', '--random-erase-value', '0', 'inf', '0'],
    ['--augment', 'rrc', '--color-jitter', 'nan', '0', '0'],
])
def test_the_photo_options_are_refused_by_the_parser_and_by_the_check(argv, capsys):
    import train_imagenet as T
    with pytest.raises(SystemExit):
        T.parse_args(argv)
    capsys.readouterr()
    # the same values on a namespace that never went through the parser (``run`` calls the check too)
    args = T.Arguments()
    i = 0
    while i < len(argv):
        name = argv[i][2:].replace('-', '_')
        i += 1
        values = []
        while i < len(argv) and not argv[i].startswith('--'):
            values.append(argv[i])
            i += 1
        if name == 'augment':
            args.augment = values[0]
        else:
            values = [float(v) for v in values]
            setattr(args, name, values[0] if len(values) == 1 else tuple(values))
    with pytest.raises(ValueError):
        T.check_photo_arguments(args)


def test_a_checkpoint_from_before_the_options_resumes_at_their_defaults_only():
    import train_imagenet as T
    args = T.parse_args(['--augment', 'rrc'])
    saved = {k: v for k, v in checkpoint.plain_arguments(args).items() if k not in NEW}
    fixed = [k for k in T.RESUME_FIXED if k != 'gpus']
    assert checkpoint.check_arguments(saved, args, fixed, checkpoint.SILENT, T.RESUME_DEFAULTS_WITH_PHOTO) == []
    for extra, name in ((['--color-jitter', '0.4', '0.4', '0.4'], 'color_jitter'), (['--random-erase-prob', '0.25'], 'random_erase_prob'),
                        (['--lighting-std', '0.1'], 'lighting_std'), (['--photo-seed', '1'], 'photo_seed'),
                        (['--random-erase-value', '0', '0', '0'], 'random_erase_value')):
        given = T.parse_args(['--augment', 'rrc'] + extra)
        with pytest.raises(ValueError, match=name):
            checkpoint.check_arguments(saved, given, fixed, checkpoint.SILENT, T.RESUME_DEFAULTS_WITH_PHOTO)
    # a checkpoint that holds the keys is compared as it is; the defaults written out in full change nothing
    given = T.parse_args(['--augment', 'rrc', '--color-jitter', '0.4', '0.4', '0.4', '--photo-seed', '2'])
    now = checkpoint.plain_arguments(given)
    assert checkpoint.check_arguments(now, given, fixed, checkpoint.SILENT, T.RESUME_DEFAULTS_WITH_PHOTO) == []
    with pytest.raises(ValueError, match='photo_seed'):
        checkpoint.check_arguments(now, T.parse_args(['--augment', 'rrc', '--color-jitter', '0.4', '0.4', '0.4', '--photo-seed', '3']), fixed,
                                   checkpoint.SILENT, T.RESUME_DEFAULTS_WITH_PHOTO)
    spelled = T.parse_args(['--augment', 'rrc', '--color-jitter', '0', '0', '0', '--random-erase-scale', '0.02', '0.33'])
    assert checkpoint.check_arguments(saved, spelled, fixed, checkpoint.SILENT, T.RESUME_DEFAULTS_WITH_PHOTO) == []
    assert T.RESUME_DEFAULTS_PHOTO == dict(zip(NEW, DEFAULTS))
    assert T.RESUME_DEFAULTS_WITH_PHOTO == dict(T.RESUME_DEFAULTS_WITH_LARS, **T.RESUME_DEFAULTS_PHOTO)
    assert not set(NEW) & set(T.RESUME_DEFAULTS_WITH_LARS)                     # the older tables are what they were


# ---- the struct and the entries without a GPU -----------------------------------------------------------------------------------
def test_photo_job_has_the_headers_layout(tmp_path):
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "loans_hip.h"', 'int main(void) {',
           '  printf("size %zu\\n", sizeof(loans_photo_job));']
    for f in PHOTO_JOB.names:
        src.append('  printf("%s %%zu\\n", offsetof(loans_photo_job, %s));' % (f, f))
    src += ['  return 0;', '}']
    c_file, exe = tmp_path / 'layout.c', tmp_path / 'layout'
    c_file.write_text('\n'.join(src))
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), '-o', str(exe), str(c_file)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(got['size']) == PHOTO_JOB.itemsize == 64
    for f in PHOTO_JOB.names:
        assert int(got[f]) == PHOTO_JOB.fields[f][1], f
    assert PHOTO_JOB.fields['add'][0].shape == (3,) and PHOTO_JOB.fields['fill'][0].shape == (3,)


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from loans_amd import _lib
    return _lib.load()


def test_photo_entries_check_their_arguments_before_any_hip_call(lib):
    from loans_amd import _lib
    assert 'loans_photo_workspace_bytes' in _lib.RESTYPES
    ws_bytes = lib.loans_photo_workspace_bytes
    # one fp64 partial per 1024 pixels, 2048 at most, then one fp32 mean per image, padded to 8 bytes
    assert ws_bytes(2, 16, 12) == 2 * 8 + 8 and ws_bytes(256, 224, 224) == 256 * 49 * 8 + 256 * 4 and ws_bytes(1, 1, 1) == 8 + 8
    assert ws_bytes(3, 1025, 1) == 3 * 2 * 8 + 16 and ws_bytes(1, 4096, 4096) == 2048 * 8 + 8
    assert ws_bytes(0, 4, 4) == -1 and ws_bytes(4, 0, 4) == -1 and ws_bytes(4, 4, -1) == -1
    buf = ctypes.create_string_buffer(4096)
    base = (ctypes.addressof(buf) + 63) & ~63
    x, out, jd, ws = base, base + 1024, base + 2048, base + 3072
    jobs = np.zeros(2, PHOTO_JOB)
    jobs[0] = P.make_job(0.6, 1.4, 0.6, 3, (0.1, 0, 0), (0, 0, 2, 2))
    jobs[1] = P.make_job()
    good = dict(x=x, out=out, B=2, C=3, H=4, W=4, jobs_dev=jd, jobs_host=jobs.ctypes.data, ws=ws, ws_bytes=24)
    grey_order = ('x', 'B', 'C', 'H', 'W', 'jobs_dev', 'jobs_host', 'ws', 'ws_bytes')
    apply_order = ('x', 'out', 'B', 'C', 'H', 'W', 'jobs_dev', 'jobs_host', 'ws', 'ws_bytes')

    def both(change, table=None):
        args = dict(good, **change)
        if table is not None:
            args['jobs_host'] = table.ctypes.data
        return (lib.loans_photo_grey_means_f32(*[args[n] for n in grey_order], 0),
                lib.loans_photo_apply_f32(*[args[n] for n in apply_order], 0))

    for change in (dict(x=0), dict(jobs_dev=0), dict(jobs_host=0), dict(ws=0), dict(B=0), dict(C=1), dict(C=4), dict(H=0), dict(W=-2),
                   dict(x=x + 2), dict(jobs_dev=jd + 1), dict(ws=ws + 4), dict(ws_bytes=16)):
        assert both(change) == (-1, -1), change
    assert lib.loans_photo_apply_f32(x, 0, 2, 3, 4, 4, jd, jobs.ctypes.data, ws, 24, 0) == -1
    assert lib.loans_photo_apply_f32(x, out + 2, 2, 3, 4, 4, jd, jobs.ctypes.data, ws, 24, 0) == -1
    nan, inf = float('nan'), float('inf')
    for field, value in (('b', nan), ('c', inf), ('s', -inf), ('omc', nan), ('oms', inf), ('order', 6), ('order', -1), ('y0', -1), ('y1', 5),
                         ('x1', 5), ('x0', 3)):
        table = jobs.copy()
        table[field][0] = value
        assert both({}, table) == (-1, -1), field
    for field in ('add', 'fill'):
        table = jobs.copy()
        table[field][1, 2] = nan
        assert both({}, table) == (-1, -1), field
    table = jobs.copy()
    table['y0'][0], table['y1'][0] = 3, 2
    assert both({}, table) == (-1, -1)
    assert both(dict(H=1 << 10, W=1 << 20)) == (-2, -2)                       # an image past 32-bit indexing
    # no image with a contrast factor: the grey entry has nothing to launch and says so without touching a device
    table = jobs.copy()
    table[0] = P.make_job(0.6, 1.0, 0.6)
    assert lib.loans_photo_grey_means_f32(x, 2, 3, 4, 4, jd, table.ctypes.data, ws, 24, 0) == 0
    assert bytes(buf) == bytes(4096)
