"""-m gpu: ``loans_crop_resize_u8_f32`` against Pillow, byte for byte.  Every frame of this file lies in ONE packed source buffer,
back to back without alignment padding (odd widths: odd byte offsets) between guard bytes; a call resizes a mixed batch of
crops to one output size into a tensor with a sentinel slot either side."""
import numpy as np
import pytest
import torch

from loans_amd import _lib
from loans_amd.common.datasets import crop_resize as CR
from loans_amd.common.datasets.resample import resample_coeffs

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
GUARD = 13
# a crop taller than the LDS holds at this output width, in one band: the block works through it in several fills
FILL_OW = 64
FILL_OH = 8
FILL_H = 2 * CR.lds_row_capacity(FILL_OW) + 50

FRAMES = {'a': (37, 53), 'b': (64, 48), 'c': (300, 401), 'd': (9, 9), 'e': (40, 40), 'f': (50, 70), 'g': (FILL_H + 3, 41)}

# output size -> [(frame, (y0, x0, h, w), flip)]
CALLS = {
    (16, 16): [('a', (5, 7, 20, 31), False), ('f', (10, 10, 16, 16), False),
               ('a', (0, 0, 20, 31), False), ('a', (0, 22, 20, 31), True), ('a', (17, 0, 20, 31), True), ('a', (17, 22, 20, 31), False),
               ('d', (0, 0, 9, 9), True), ('c', (0, 100, 300, 1), False), ('c', (299, 0, 1, 401), True)],
    (24, 40): [('a', (0, 0, 37, 53), True), ('a', (5, 7, 20, 31), False), ('b', (0, 0, 64, 48), False)],
    (32, 32): [('b', (3, 1, 9, 11), True), ('b', (3, 1, 9, 11), False), ('d', (4, 4, 1, 1), True)],
    (16, 24): [('c', (17, 33, 250, 301), False), ('c', (50, 100, 250, 301), True), ('a', (5, 7, 20, 31), True)],
    (8, 8): [('d', (4, 4, 1, 1), False), ('d', (8, 8, 1, 1), False), ('d', (0, 0, 9, 9), False)],
    (40, 24): [('e', (0, 8, 40, 24), True), ('e', (0, 8, 40, 24), False), ('e', (0, 16, 40, 24), True)],
    (16, 17): [('f', (10, 10, 16, 16), False), ('a', (5, 7, 20, 31), True), ('c', (0, 0, 300, 401), False)],
    (33, 129): [('a', (5, 7, 20, 31), True), ('c', (17, 33, 250, 301), False)],                 # two bands, the second a short one
    (FILL_OH, FILL_OW): [('g', (2, 3, FILL_H, 30), True), ('g', (0, 0, FILL_H + 3, 41), False), ('a', (5, 7, 20, 31), False)],
    # the launcher picks a smaller LDS image (more blocks per CU) where twice the largest window fits it, and a vertical pass
    # of four pixels per thread where the output width is a multiple of four: several fills in the small image at such a width
    # (400 rows to 16: a window of 51), and the full image at a width that is not
    (16, 64): [('g', (1, 2, 400, 36), False), ('a', (5, 7, 20, 31), True)],
    (FILL_OH, FILL_OW + 1): [('g', (0, 0, FILL_H + 3, 41), True), ('a', (5, 7, 20, 31), False)],
}


@pytest.fixture(scope='module')
def packed():
    """(host frames by name, byte offset of each, the packed buffer on the device)"""
    rng = np.random.RandomState(7)
    frames = {k: rng.randint(0, 256, (H, W, 3)).astype(np.uint8) for k, (H, W) in FRAMES.items()}
    parts, where, off = [np.full(GUARD, 201, np.uint8)], {}, GUARD
    for k, f in frames.items():
        where[k] = off
        parts.append(f.ravel())
        off += f.size
    parts.append(np.full(GUARD, 201, np.uint8))
    assert any(o % 2 for o in where.values())                       # a frame at an odd byte offset
    return frames, where, torch.from_numpy(np.concatenate(parts)).cuda()


def test_the_fill_case_needs_more_than_one_fill():
    band = _lib.load().loans_crop_band_rows(FILL_OH, FILL_OW)
    bounds, _, vks = resample_coeffs(FILL_H, FILL_OH, 'bilinear')
    cap = CR.lds_row_capacity(FILL_OW)
    assert band == FILL_OH                                          # one block owns every output row ...
    assert bounds[-1, 0] + bounds[-1, 1] - bounds[0, 0] > 2 * cap   # ... and they need more than two fills' worth of rows
    assert vks <= cap                                               # while a single output row fits


@pytest.mark.parametrize('out_hw', list(CALLS), ids=lambda s: '%dx%d' % s)
def test_crop_resize_equals_pillow(packed, out_hw):
    frames, where, dev_all = packed
    oh, ow = out_hw
    cases = CALLS[out_hw]
    jobs = [(where[k], FRAMES[k][1] * 3, FRAMES[k][0], FRAMES[k][1], box, flip) for k, box, flip in cases]
    out = torch.full((len(cases) + 2, 3, oh, ow), SENTINEL, device='cuda', dtype=torch.float32)
    got = CR.crop_resize_device(dev_all, jobs, out_hw, out=out[1:-1])
    torch.cuda.synchronize()
    assert got.data_ptr() == out[1].data_ptr()
    host = out.cpu().numpy()
    assert (host[0] == SENTINEL).all() and (host[-1] == SENTINEL).all()
    for n, (k, box, flip) in enumerate(cases):
        want = CR.crop_resize_host(frames[k], box, out_hw, flip)
        assert want.min() >= 0.0                                    # (so a surviving sentinel cannot pass for a pixel)
        np.testing.assert_array_equal(host[1 + n], want, err_msg='%s %s flip=%s -> %s' % (FRAMES[k], box, flip, out_hw))


def test_a_fresh_output_tensor_and_a_pitch_wider_than_the_frame(packed):
    """the wrapper's own allocation; and the left 20 columns of frame 'e' addressed as a 40 x 20 frame of pitch 120"""
    frames, where, dev_all = packed
    jobs = [(where['e'], 120, 40, 20, (3, 2, 30, 17), True), (where['e'] + 60, 120, 40, 20, (0, 0, 40, 20), False)]
    got = CR.crop_resize_device(dev_all, jobs, (12, 10)).cpu().numpy()
    np.testing.assert_array_equal(got[0], CR.crop_resize_host(frames['e'][:, :20], (3, 2, 30, 17), (12, 10), True))
    np.testing.assert_array_equal(got[1], CR.crop_resize_host(frames['e'][:, 20:], (0, 0, 40, 20), (12, 10), False))
