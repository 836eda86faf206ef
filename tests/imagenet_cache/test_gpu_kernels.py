"""-m gpu: ``loans_crop_resize_srcs_u8_f32`` -- one launch over several source buffers -- against Pillow, byte for byte, and
against the single-source launch."""
import numpy as np
import pytest
import torch

from loans_amd.common.datasets import crop_resize as CR
from loans_amd.common.datasets.resample import resample_coeffs

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
# three sources of different lengths, frames back to back: odd widths put pixels at every byte alignment; 'a' and 'e' start at
# offset 0 of their sources, 'b', 'd' and 'e' end on their sources' last bytes; 'c' lies behind five guard bytes
FRAMES = {'a': (29, 37), 'b': (240, 33), 'c': (40, 41), 'd': (32, 32), 'e': (31, 23)}
LAYOUT = [(0, ['a', 'b']), (5, ['c', 'd']), (0, ['e'])]                 # per source: guard bytes in front, then its frames

# output size -> [(frame, (y0, x0, h, w), flip)], sources interleaved
CALLS = {
    (16, 16): [('a', (0, 0, 29, 37), False), ('c', (3, 5, 30, 31), True), ('e', (0, 0, 31, 23), True), ('b', (100, 1, 77, 31), False),
               ('d', (9, 16, 16, 16), False), ('e', (15, 7, 16, 16), True), ('a', (13, 0, 16, 16), False),       # identity tables
               ('c', (0, 0, 1, 41), True), ('e', (30, 22, 1, 1), False)],
    (13, 18): [('e', (2, 0, 29, 23), False), ('a', (0, 18, 13, 18), True), ('d', (0, 0, 32, 32), True), ('b', (0, 0, 240, 33), True),
               ('c', (27, 23, 13, 18), False), ('e', (0, 0, 31, 23), False)],
    # 240 rows to 4: a window of 121 rows against the small form's 106 at 32 pixels -- the 64 KB form
    (4, 32): [('b', (0, 0, 240, 33), False), ('c', (0, 9, 4, 32), True), ('e', (1, 0, 30, 23), False), ('b', (0, 1, 240, 32), True),
              ('d', (28, 0, 4, 32), False)],
    (32, 32): [('d', (0, 0, 32, 32), False), ('e', (0, 0, 31, 23), True), ('d', (0, 0, 32, 32), True), ('a', (0, 0, 29, 37), True)],
}


@pytest.fixture(scope='module')
def sources():
    """(host frames by name, {name: (source, byte offset)}, the source buffers on the device)"""
    rng = np.random.RandomState(11)
    frames = {k: rng.randint(0, 256, (H, W, 3)).astype(np.uint8) for k, (H, W) in FRAMES.items()}
    where, buffers = {}, []
    for s, (guard, names) in enumerate(LAYOUT):
        parts, off = [np.full(guard, 201, np.uint8)], guard
        for k in names:
            where[k] = (s, off)
            parts.append(frames[k].ravel())
            off += frames[k].size
        buffers.append(torch.from_numpy(np.concatenate(parts)).cuda())
    assert len({b.numel() for b in buffers}) == 3
    assert {o % 4 for _, o in where.values()} > {0} and where['a'] == (0, 0) and where['e'] == (2, 0)
    for k in ('b', 'd', 'e'):
        assert where[k][1] + frames[k].size == buffers[where[k][0]].numel()
    return frames, where, buffers


def _jobs(where, cases):
    return [(where[k][1], FRAMES[k][1] * 3, FRAMES[k][0], FRAMES[k][1], box, flip, where[k][0]) for k, box, flip in cases]


def test_the_long_downscale_needs_the_large_form():
    assert resample_coeffs(240, 4, 'bilinear')[2] == 121 and 2 * 121 > 20480 // (32 * 3) and 121 <= CR.lds_row_capacity(32)


@pytest.mark.parametrize('out_hw', list(CALLS), ids=lambda s: '%dx%d' % s)
def test_one_launch_over_three_sources_equals_pillow(sources, out_hw):
    frames, where, buffers = sources
    oh, ow = out_hw
    cases = CALLS[out_hw]
    jobs = _jobs(where, cases)
    assert {j[6] for j in jobs} == {0, 1, 2} and all(a[6] != b[6] for a, b in zip(jobs, jobs[1:]))
    out = torch.full((len(cases) + 2, 3, oh, ow), SENTINEL, device='cuda', dtype=torch.float32)
    got = CR.crop_resize_device_multi(buffers, jobs, out_hw, out=out[1:-1])
    torch.cuda.synchronize()
    assert got.data_ptr() == out[1].data_ptr()
    host = out.cpu().numpy()
    assert (host[0] == SENTINEL).all() and (host[-1] == SENTINEL).all()
    for n, (k, box, flip) in enumerate(cases):
        want = CR.crop_resize_host(frames[k], box, out_hw, flip)
        assert want.min() >= 0.0
        np.testing.assert_array_equal(host[1 + n], want, err_msg='%s %s flip=%s -> %s' % (k, box, flip, out_hw))


@pytest.mark.parametrize('out_hw', [(16, 16), (13, 18), (4, 32)], ids=lambda s: '%dx%d' % s)
def test_all_jobs_in_source_0_equal_the_single_source_launch(sources, out_hw):
    frames, where, buffers = sources
    cases = [c for c in CALLS[out_hw] if where[c[0]][0] == 0]
    jobs = _jobs(where, cases)
    single = CR.crop_resize_device(buffers[0], [j[:6] for j in jobs], out_hw)
    multi = CR.crop_resize_device_multi(buffers, jobs, out_hw)                  # (two sources that no job names)
    alone = CR.crop_resize_device_multi(buffers[:1], jobs, out_hw)
    assert torch.equal(single, multi) and torch.equal(single, alone)
    np.testing.assert_array_equal(single[0].cpu().numpy(), CR.crop_resize_host(frames[cases[0][0]], cases[0][1], out_hw, cases[0][2]))
