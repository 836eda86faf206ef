"""-m gpu: the photometric kernels (loans_amd/csrc/photo.hip) through ``ops.photometric`` against float64 NumPy, held to the bound
tests/imagenet_photo/reference.py derives and the CPU test establishes on the fp32 restatement."""
import numpy as np
import pytest
import torch

import loans_amd
from loans_amd import _lib, ops
from loans_amd.common.datasets import photometric as P
from loans_amd.ops import PHOTO_JOB
from tests.gpu_util import dev
from tests.imagenet_photo import reference as X

pytestmark = pytest.mark.gpu


def bits(t):
    return t.view(torch.int32)


def check(x, xd, jobs, tag=()):
    """out of place twice, then in place on a copy: the worst error / bound of the elements that are not copies"""
    before = xd.clone()
    got_d = ops.photometric(xd, jobs)
    again = ops.photometric(xd, jobs)
    tag = tag + (tuple(x.shape),)
    assert got_d.data_ptr() != xd.data_ptr() and torch.equal(bits(xd), bits(before)), tag         # x is read only
    assert torch.equal(bits(got_d), bits(again)), tag                                             # two launches, the same bits
    place = xd.clone()
    assert ops.photometric(place, jobs, out=place) is place
    assert torch.equal(bits(place), bits(got_d)), tag                                             # in place, the same bits
    got = got_d.cpu().numpy()
    out64, copies, bound = X.photo_ref(x, jobs)
    assert np.array_equal(got.view(np.uint32)[copies], out64.astype(np.float32).view(np.uint32)[copies]), tag + (jobs,)
    err = np.abs(got.astype(np.float64) - out64)
    live = ~copies
    assert np.all(err[live] <= bound[live]), tag + (jobs, float((err[live] / bound[live]).max()))
    return float((err[live] / bound[live]).max()) if live.any() else 0.0


@pytest.mark.parametrize('H, W', X.SHAPES)
def test_photometric_over_shapes_orders_factors_addends_and_boxes(H, W):
    worst, orders, triples, kinds = 0.0, set(), set(), set()
    for B in X.BATCHES:
        x = X.frames(B, H, W)
        xd = dev(x)
        assert xd.data_ptr() % 16 == 0
        for jobs in X.case_jobs(B, H, W):
            worst = max(worst, check(x, xd, jobs, (B,)))
            orders |= set(int(o) for o in jobs['order'])
            triples |= set(zip(jobs['b'].tolist(), jobs['c'].tolist(), jobs['s'].tolist()))
            kinds |= {(bool(j['add'].any()), (int(j['y0']), int(j['x0']), int(j['y1']), int(j['x1']))) for j in jobs}
    assert orders == set(range(6)) and len(triples) == len(X.FACTORS) ** 3 and (1.0, 1.0, 1.0) in triples
    assert {k[1] for k in kinds} == set(X.boxes(H, W)) and {k[0] for k in kinds} == {False, True}
    print('%d x %d worst error / bound %.3f' % (H, W, worst))


def test_identity_jobs_leave_the_batch_bit_for_bit_and_launch_nothing_in_place():
    x = X.frames(5, 16, 12)
    xd = dev(x)
    jobs = np.zeros(5, PHOTO_JOB)
    for n in range(5):
        jobs[n] = P.make_job(order=n, box=((0, 3, 7, 3), (4, 0, 4, 12), (0, 0, 0, 0), (2, 2, 2, 2), (5, 1, 5, 1))[n])
    assert ops.photo_identity(jobs).all()
    calls = []
    lib = _lib.load()
    real = lib.loans_photo_apply_f32
    try:
        lib.loans_photo_apply_f32 = lambda *a: calls.append(a) or real(*a)
        assert ops.photometric(xd, jobs, out=xd) is xd and calls == []
        fresh = ops.photometric(xd, jobs)                                   # out of place: one launch, a copy
        assert len(calls) == 1
    finally:
        lib.loans_photo_apply_f32 = real
    assert torch.equal(bits(fresh), bits(xd)) and np.array_equal(xd.cpu().numpy().view(np.uint32), x.view(np.uint32))
    # one image of the batch changes, the others still leave bit for bit
    jobs[2] = P.make_job(0.6, 1.4, 0.6, 3)
    got = ops.photometric(xd, jobs, out=xd).cpu().numpy()
    keep = np.array([0, 1, 3, 4])
    assert np.array_equal(got[keep].view(np.uint32), x[keep].view(np.uint32)) and not np.array_equal(got[2], x[2])


def test_a_source_off_the_16_byte_boundary_takes_the_one_pixel_form_and_stays_inside_its_tensor():
    B, H, W = 5, 16, 12
    x = X.frames(B, H, W, seed=1)
    buf = torch.full((x.size + 8,), 7.0, device='cuda')
    xd = buf[1:1 + x.size].view(B, 3, H, W)
    xd.copy_(dev(x))
    assert xd.data_ptr() % 16 == 4 and xd.is_contiguous()
    aligned = dev(x)
    for jobs in X.case_jobs(B, H, W)[::7]:
        want = ops.photometric(aligned, jobs)
        check(x, xd, jobs)
        assert torch.equal(bits(ops.photometric(xd, jobs)), bits(want))                 # both forms: the same bits
        # in place there, and into a destination off the boundary
        xd2buf = buf.clone()
        xd2 = xd2buf[1:1 + x.size].view(B, 3, H, W)
        ops.photometric(xd2, jobs, out=xd2)
        assert torch.equal(bits(xd2), bits(want))
        assert float(xd2buf[0]) == 7.0 and bool((xd2buf[1 + x.size:] == 7.0).all())
        obuf = torch.full((x.size + 8,), 7.0, device='cuda')
        out = obuf[1:1 + x.size].view(B, 3, H, W)
        assert ops.photometric(aligned, jobs, out=out) is out and torch.equal(bits(out), bits(want))
        assert float(obuf[0]) == 7.0 and bool((obuf[1 + x.size:] == 7.0).all())
    assert float(buf[0]) == 7.0 and bool((buf[1 + x.size:] == 7.0).all())
    with pytest.raises(ValueError):
        ops.photometric(aligned[:, :, :, ::2], X.case_jobs(B, H, W)[0])
    with pytest.raises(ValueError):
        ops.photometric(aligned, X.case_jobs(B, H, W)[0][:3])                            # one job per image
    with pytest.raises(ValueError):
        ops.photometric(aligned, np.zeros(B, np.float32))
    bad = X.case_jobs(B, H, W)[0].copy()
    bad['y1'][1] = H + 1
    with pytest.raises(loans_amd._lib.HipKernelError):
        ops.photometric(aligned, bad)
    bad = X.case_jobs(B, H, W)[0].copy()
    bad['order'][0] = 6
    with pytest.raises(loans_amd._lib.HipKernelError):
        ops.photometric(aligned, bad)


def test_beyond_one_trip_of_both_grids():
    """725 x 725 single pixels per image (the width is odd: the one-pixel form) are more than the 2048 x 256 threads of the capped
    apply grid, which leaves one block row for four images: both loops of the apply kernel make a second trip.  The grey pass cuts an
    image into 514 partials of 1024 pixels, four trips of a block each, and 2048 // 514 = 3 block rows for four images: both of its
    loops too.  (419 x 419, the mix test's shape, fills only 686 blocks of the apply grid here: a lane owns a pixel in all three
    planes.)  Contrast is on in every image but the last, so the fold sees 514 partials per image."""
    B, H, W = 4, 725, 725
    assert H * W > 2048 * 256 and -(-H * W // 1024) == 514
    x = X.frames(B, H, W)
    xd = dev(x)
    jobs = np.zeros(B, PHOTO_JOB)
    jobs[0] = P.make_job(0.6, 1.4, 0.6, 0, (0.03, -0.02, 0.01), (100, 0, 300, 211))
    jobs[1] = P.make_job(1.4, 0.6, 1.0, 3, box=(0, 7, 725, 725))
    jobs[2] = P.make_job(1.0, 1.4, 1.4, 5)
    jobs[3] = P.make_job(0.6, 1.0, 1.4, 4, (0.0, 0.5, 0.0))
    got_d = ops.photometric(xd, jobs)
    place = xd.clone()
    ops.photometric(place, jobs, out=place)
    assert torch.equal(bits(place), bits(got_d)) and torch.equal(bits(ops.photometric(xd, jobs)), bits(got_d))
    out64, copies, bound = X.photo_ref(x, jobs)
    got = got_d.cpu().numpy()
    assert np.array_equal(got.view(np.uint32)[copies], out64.astype(np.float32).view(np.uint32)[copies])
    err = np.abs(got.astype(np.float64) - out64)
    assert np.all(err <= bound), float((err[~copies] / bound[~copies]).max())
    print('worst error / bound %.3f' % float((err[~copies] / bound[~copies]).max()))


def test_more_images_than_block_rows_in_the_16_byte_form():
    """2049 images of 4 x 4: one block per image in x, 2048 block rows -- the image loops of both kernels make a second trip in the
    16-byte form"""
    B, H, W = 2049, 4, 4
    x = X.frames(B, H, W)
    xd = dev(x)
    jobs = np.zeros(B, PHOTO_JOB)
    picks = [(0.6, 1.4, 0.6), (1.4, 0.6, 1.0), (1.0, 1.4, 1.4), (0.0, 0.6, 1.4), (1.0, 1.0, 1.0)]
    for n in range(B):
        b, c, s = picks[n % 5]
        jobs[n] = P.make_job(b, c, s, n % 6, (0.03, -0.02, 0.01) if n % 4 == 0 else (0, 0, 0), (1, 1, 3, 4) if n % 3 == 0 else (0, 0, 0, 0))
    worst = check(x, xd, jobs)
    print('worst error / bound %.3f' % worst)


def test_a_batch_without_a_contrast_factor_makes_no_reduction_launch():
    B, H, W = 5, 16, 12
    x = X.frames(B, H, W)
    xd = dev(x)
    nbytes = int(_lib.load().loans_photo_workspace_bytes(B, H, W))
    assert nbytes == B * 8 + 24                     # five partials, five fp32 means padded to 8 bytes
    ws = ops.photo_workspace(xd.device, nbytes)
    assert ops.photo_workspace(xd.device, nbytes) is ws and ws.dtype == torch.float64 and ws.numel() * 8 >= nbytes
    ws.fill_(-3.0)
    jobs = np.zeros(B, PHOTO_JOB)
    for n in range(B):
        jobs[n] = P.make_job((0.6, 1.4, 1.0, 0.0, 1.4)[n], 1.0, (1.4, 1.0, 0.6, 0.6, 0.0)[n], n, (0.03, -0.02, 0.01), (0, 1, 9, 6))
    calls = []
    lib = _lib.load()
    real = lib.loans_photo_grey_means_f32
    try:
        lib.loans_photo_grey_means_f32 = lambda *a: calls.append(a) or real(*a)
        check(x, xd, jobs)
        assert calls == [] and bool((ws == -3.0).all())                                 # the workspace is untouched
        # contrast in images 1 and 3: their partials are written, the others' slots are not
        jobs['c'][1], jobs['omc'][1] = P.complement32(1.4)
        jobs['c'][3], jobs['omc'][3] = P.complement32(0.0)
        check(x, xd, jobs)
        assert len(calls) == 3                                                          # (check launches three times)
    finally:
        lib.loans_photo_grey_means_f32 = real
    touched = (ws[:B] != -3.0).cpu().numpy()
    assert touched.tolist() == [False, True, False, True, False]
    sentinel = torch.full((1,), -3.0, dtype=torch.float64).view(torch.float32)            # what an untouched fp32 slot reads as
    means = ws[B:B + 3].view(torch.float32)[:B].cpu()
    assert [bool(torch.equal(means[n:n + 1].view(torch.int32), sentinel[n % 2:n % 2 + 1].view(torch.int32))) for n in range(B)] == \
        [True, False, True, False, True]
    assert bool((ws[B + 3:] == -3.0).all())
