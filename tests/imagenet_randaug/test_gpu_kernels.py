"""-m gpu: the RandAugment kernels (loans_amd/csrc/randaug.hip) through ``ops.rand_augment``: the gathers, Posterize, Solarize,
Equalize and every copy bit for bit against the exact NumPy form, Brightness, Color, Contrast, Sharpness and AutoContrast inside
the bound tests/imagenet_randaug/reference.py derives against float64, and chains of layers against single-layer calls fed with
each other's output."""
import numpy as np
import pytest
import torch

import loans_amd
from loans_amd import _lib, ops
from loans_amd.common.datasets import rand_augment as RA
from loans_amd.ops import RA_JOB
from tests.gpu_util import dev
from tests.imagenet_randaug import reference as X

pytestmark = pytest.mark.gpu


def bits(t):
    return t.view(torch.int32)


def check(x, xd, jobs, tag=()):
    """out of place twice, then in place on a copy, all against the reference: the worst error / bound of the elements that are
    not exact"""
    before = xd.clone()
    got_d = ops.rand_augment(xd, jobs)
    again = ops.rand_augment(xd, jobs)
    tag = tag + (tuple(x.shape), jobs['op'][:, :2].tolist())
    assert got_d.data_ptr() != xd.data_ptr() and torch.equal(bits(xd), bits(before)), tag         # x is read only
    assert torch.equal(bits(got_d), bits(again)), tag                                             # two runs, the same bits
    place = xd.clone()
    assert ops.rand_augment(place, jobs, out=place) is place
    assert torch.equal(bits(place), bits(got_d)), tag                                             # in place, the same bits
    got = got_d.cpu().numpy()
    ref = X.ra_ref(x, jobs)
    assert X.holds(got, ref), tag + (X.worst(got, ref),)
    return X.worst(got, ref)


@pytest.mark.parametrize('H, W', X.SHAPES)
def test_every_op_over_shapes_batches_signs_and_magnitudes(H, W):
    worst, seen = 0.0, set()
    for B in X.BATCHES:
        for x in (X.frames(B, H, W), X.band_frames(B, H, W)):
            xd = dev(x)
            assert xd.data_ptr() % 16 == 0
            for jobs in X.case_jobs(B, H, W) + X.chain_jobs(B, H, W):
                worst = max(worst, check(x, xd, jobs, (B,)))
                seen |= {(int(j['op'][0]), int(j['layers'])) for j in jobs}
    assert {op for op, layers in seen if layers == 1} == set(range(14))
    # AutoContrast is reproducible in NumPy fp32: it is held bit for bit as well
    x = X.frames(2, H, W, seed=3)
    jobs = np.array([RA.make_job([(12, None)], H, W)] * 2)
    assert np.array_equal(ops.rand_augment(dev(x), jobs).cpu().numpy().view(np.uint32), RA.apply_host(x, jobs).view(np.uint32))
    print('%d x %d worst error / bound %.3f' % (H, W, worst))


def test_equalize_builds_real_tables_and_copies_where_the_step_is_zero():
    for (H, W), real in (((16, 12), False), ((33, 65), True), ((40, 64), True)):
        x = X.frames(2, H, W)
        jobs = np.array([RA.make_job([(13, None)], H, W)] * 2)
        got = ops.rand_augment(dev(x), jobs).cpu().numpy()
        assert np.array_equal(got.view(np.uint32), x.view(np.uint32)) != real, (H, W)


def _identities(B, H, W):
    layers = [[(0, None)], [(1, 0.0), (10, 8)], [(5, 0.0), (6, 0.0), (3, 0)], [(7, 0.0), (8, 0.0), (4, 0), (2, 0.0)], [(0, None), (0, None)]]
    return np.array([RA.make_job(layers[n % len(layers)], H, W) for n in range(B)])


def test_identity_jobs_leave_the_batch_bit_for_bit_and_launch_nothing_in_place():
    x = X.frames(5, 16, 12)
    xd = dev(x)
    jobs = _identities(5, 16, 12)
    assert ops.ra_identity(jobs, 16, 12).all()
    small = dev(X.frames(1, 2, 7))
    sharp = np.array([RA.make_job([(9, 0.9)], 2, 7)])
    assert ops.ra_identity(sharp, 2, 7).all() and not ops.ra_identity(sharp, 3, 7).all()       # no interior: a copy altogether
    calls = []
    lib = _lib.load()
    real = lib.loans_ra_apply_f32
    try:
        lib.loans_ra_apply_f32 = lambda *a: calls.append(a) or real(*a)
        assert ops.rand_augment(xd, jobs, out=xd) is xd and calls == []
        assert ops.rand_augment(small, sharp, out=small) is small and calls == []
        fresh = ops.rand_augment(xd, jobs)                                  # out of place: one call, a copy
        assert len(calls) == 1
    finally:
        lib.loans_ra_apply_f32 = real
    assert torch.equal(bits(fresh), bits(xd)) and np.array_equal(xd.cpu().numpy().view(np.uint32), x.view(np.uint32))
    # one image of the batch changes, the others still leave bit for bit
    jobs[2] = RA.make_job([(0, None), (11, 0.5)], 16, 12)
    got = ops.rand_augment(xd, jobs, out=xd).cpu().numpy()
    keep = np.array([0, 1, 3, 4])
    assert np.array_equal(got[keep].view(np.uint32), x[keep].view(np.uint32)) and not np.array_equal(got[2], x[2])


def test_a_batch_without_a_statistics_op_makes_no_statistics_launch():
    B, H, W = 5, 16, 12
    x = X.frames(B, H, W)
    xd = dev(x)
    nbytes = int(_lib.load().loans_ra_workspace_bytes(B, H, W))
    stat_bytes = nbytes - x.nbytes
    assert stat_bytes == B * 3072 + B * 3136                    # one block record and one folded record per image
    ws = ops.ra_workspace(xd.device, nbytes)
    assert ops.ra_workspace(xd.device, nbytes) is ws and ws.dtype == torch.uint8 and ws.numel() >= nbytes
    ws.fill_(0xA5)
    jobs = np.array([RA.make_job(layers, H, W) for layers in
                     ([(5, 30.0), (9, 0.9)], [(11, 0.5), (7, -0.5)], [(10, 3), (11, 0.5)], [(0, None)], [(1, 0.3), (8, 0.0)])])
    check(x, xd, jobs)                                                      # (a Contrast of factor 1 is the identity)
    torch.cuda.synchronize()
    assert bool((ws[:stat_bytes] == 0xA5).all())                            # no record was written
    # Contrast in image 1's second layer, Equalize in image 3: their records are written, the others' are not
    jobs[1] = RA.make_job([(6, 0.5), (8, -0.5)], H, W)
    jobs[3] = RA.make_job([(13, None)], H, W)
    ops.rand_augment(xd, jobs)
    torch.cuda.synchronize()
    records = ws[:B * 3072].view(B, 3072)
    assert (records != 0xA5).any(dim=1).cpu().tolist() == [False, True, False, True, False]
    folded = ws[B * 3072:stat_bytes].view(B, 3136)
    assert (folded != 0xA5).any(dim=1).cpu().tolist() == [False, True, False, True, False]


def test_a_source_off_the_16_byte_boundary_takes_the_one_pixel_form_and_stays_inside_its_tensor():
    B, H, W = 5, 16, 12
    x = X.frames(B, H, W, seed=1)
    buf = torch.full((x.size + 8,), 7.0, device='cuda')
    xd = buf[1:1 + x.size].view(B, 3, H, W)
    xd.copy_(dev(x))
    assert xd.data_ptr() % 16 == 4 and xd.is_contiguous()
    aligned = dev(x)
    for jobs in (X.case_jobs(B, H, W) + X.chain_jobs(B, H, W))[::3]:
        want = ops.rand_augment(aligned, jobs)
        check(x, xd, jobs)
        assert torch.equal(bits(ops.rand_augment(xd, jobs)), bits(want))                # both forms: the same bits
        xd2buf = buf.clone()
        xd2 = xd2buf[1:1 + x.size].view(B, 3, H, W)
        ops.rand_augment(xd2, jobs, out=xd2)
        assert torch.equal(bits(xd2), bits(want))
        assert float(xd2buf[0]) == 7.0 and bool((xd2buf[1 + x.size:] == 7.0).all())
        obuf = torch.full((x.size + 8,), 7.0, device='cuda')
        out = obuf[1:1 + x.size].view(B, 3, H, W)
        assert ops.rand_augment(aligned, jobs, out=out) is out and torch.equal(bits(out), bits(want))
        assert float(obuf[0]) == 7.0 and bool((obuf[1 + x.size:] == 7.0).all())
    assert float(buf[0]) == 7.0 and bool((buf[1 + x.size:] == 7.0).all())
    with pytest.raises(ValueError):
        ops.rand_augment(aligned[:, :, :, ::2], X.case_jobs(B, H, W)[0])
    with pytest.raises(ValueError):
        ops.rand_augment(aligned, X.case_jobs(B, H, W)[0][:3])                          # one job per image
    with pytest.raises(ValueError):
        ops.rand_augment(aligned, np.zeros(B, np.float32))
    for field, index, value in (('op', (0, 0), 14), ('layers', (0,), 5), ('layers', (1,), 0)):
        bad = X.case_jobs(B, H, W)[1].copy()
        bad[field][index] = value
        with pytest.raises(loans_amd._lib.HipKernelError):
            ops.rand_augment(aligned, bad)


def test_beyond_one_trip_of_both_grids():
    """725 x 725 single pixels per image (the width is odd: the one-pixel form) are more than the 2048 x 256 threads of the capped
    apply grid, which leaves one block row for four images: both loops of the apply kernel make a second trip.  The statistics
    pass cuts an image into 129 records of 4096 pixels, sixteen trips of a block each."""
    B, H, W = 4, 725, 725
    assert H * W > 2048 * 256 and -(-H * W // 4096) == 129
    x = X.frames(B, H, W)
    xd = dev(x)
    jobs = np.array([RA.make_job(layers, H, W) for layers in
                     ([(5, 30.0), (8, 0.9)], [(13, None)], [(3, 7), (12, None)], [(11, 0.5), (9, 0.9)])])
    got_d = ops.rand_augment(xd, jobs)
    place = xd.clone()
    ops.rand_augment(place, jobs, out=place)
    assert torch.equal(bits(place), bits(got_d)) and torch.equal(bits(ops.rand_augment(xd, jobs)), bits(got_d))
    got, ref = got_d.cpu().numpy(), X.ra_ref(x, jobs)
    assert X.holds(got, ref), X.worst(got, ref)
    assert not np.array_equal(got[1], x[1])                                             # a real table
    print('worst error / bound %.3f' % X.worst(got, ref))


def test_more_images_than_block_rows_in_the_16_byte_form():
    """2049 images of 4 x 4: one block per image in x, 2048 block rows -- the image loops of all kernels make a second trip in the
    16-byte form"""
    B, H, W = 2049, 4, 4
    x = X.frames(B, H, W)
    every = X.combos(H, W)
    jobs = np.array([RA.make_job([every[n % len(every)]], H, W, X.FILLS[n % 2]) for n in range(B)])
    print('worst error / bound %.3f' % check(x, dev(x), jobs))


# ---- chains: one N-layer call against N single-layer calls, GPU against GPU ------------------------------------------------------
def _layer_of(jobs, l):
    """the single-layer table that performs layer l of ``jobs`` (the identity where a job has no such layer)"""
    one = np.zeros(len(jobs), RA_JOB)
    one['layers'], one['fill'] = 1, jobs['fill']
    has = jobs['layers'] > l
    one['op'][:, 0] = np.where(has, jobs['op'][:, l], 0)
    one['a'][:, 0], one['f'][:, 0] = jobs['a'][:, l], jobs['f'][:, l]
    return one


def _chain_check(x, jobs):
    xd = dev(x)
    step = xd
    for l in range(int(jobs['layers'].max())):
        step = ops.rand_augment(step, _layer_of(jobs, l))
    whole = ops.rand_augment(xd, jobs)
    assert torch.equal(bits(whole), bits(step)), jobs['op'].tolist()
    place = xd.clone()
    ops.rand_augment(place, jobs, out=place)
    assert torch.equal(bits(place), bits(step)), jobs['op'].tolist()
    assert torch.equal(bits(xd), bits(dev(x)))
    return whole


PAIR_OPS = ((5, 30.0), (9, 0.9), (8, 0.9), (12, None), (13, None), (11, 0.5))       # a gather, Sharpness, the statistics, Solarize


@pytest.mark.parametrize('H, W', [(33, 65), (40, 64)])
def test_chains_equal_single_layer_calls_fed_with_each_others_output(H, W):
    # every ordered pair, one image each
    pairs = [[a, b] for a in PAIR_OPS for b in PAIR_OPS]
    x = X.frames(len(pairs), H, W)
    jobs = np.array([RA.make_job(p, H, W) for p in pairs])
    out = _chain_check(x, jobs).cpu().numpy()
    assert not np.array_equal(out, x)
    # every pair alone in its batch: the plans of the buffers differ with what the other images do
    for p in pairs[::5]:
        _chain_check(x[:2], np.array([RA.make_job(p, H, W), RA.make_job([(0, None)], H, W)]))
    # three and four layers, moving layers in every position and number (the buffers' parities)
    g, s, c, e, q = (5, -30.0), (9, -0.9), (8, 0.5), (13, None), (10, 3)
    for chain in ([g, c, s], [c, g, e], [q, c, e], [g, s, g], [c, e, g], [g, s, g, s], [c, g, q, s], [q, c, e, q], [g, q, c, e], [q, q, q, g]):
        rotations = [chain[k:] + chain[:k] for k in range(len(chain))]
        _chain_check(x[:len(rotations)], np.array([RA.make_job(r, H, W) for r in rotations]))
        _chain_check(x[:1], np.array([RA.make_job(chain, H, W)]))
    # drawn tables
    for N in (2, 3, 4):
        policy = RA.RandAugmentPolicy('rand', N, 9 + 7 * (N - 2), seed=N)
        for B in (1, 5, 36):
            _chain_check(x[:B], policy.draw_batch(B, H, W))
    _chain_check(x, RA.RandAugmentPolicy('trivial', seed=1).draw_batch(len(x), H, W))
