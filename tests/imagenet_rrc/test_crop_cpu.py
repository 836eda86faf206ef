"""CPU side of the random-resized-crop feed: the box samplers, the job table's layout against the header, the host-side
validation of ``crop_resize_device`` and of the launcher (nothing here touches a GPU), the trainer's new options."""
import ctypes
import math
import os
import random
import subprocess

import numpy as np
import pytest
import torch
from PIL import Image

from loans_amd.common.datasets import crop_resize as CR
from loans_amd.common.datasets.resample import resample_coeffs

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SCALE, RATIO = (0.08, 1.0), (3 / 4, 4 / 3)


class CountingRandom(random.Random):
    """``random.Random`` that counts its ``randint`` calls: ``sample_rrc_box`` draws an origin for an accepted box only"""
    randints = 0

    def randint(self, a, b):
        self.randints += 1
        return super().randint(a, b)


@pytest.mark.parametrize('H,W', [(375, 500), (64, 64), (37, 53), (2, 3), (1, 1)])
def test_rrc_boxes_lie_inside_the_frame_and_inside_the_ranges(H, W):
    rng = CountingRandom(1234)
    n, fallbacks = 20000, 0
    for _ in range(n):
        before = rng.randints
        y0, x0, h, w = CR.sample_rrc_box(rng, H, W, SCALE, RATIO)
        assert h >= 1 and w >= 1 and 0 <= y0 and 0 <= x0 and y0 + h <= H and x0 + w <= W
        if rng.randints == before:
            fallbacks += 1
            continue
        # w = round(w'), h = round(h') with w' h' = area in [lo, hi] H W and w' / h' in the ratio range: each side is within
        # half a pixel of its real value
        eps = 1e-9
        assert (w + 0.5) * (h + 0.5) >= SCALE[0] * H * W * (1 - eps)
        assert max(w - 0.5, 0) * max(h - 0.5, 0) <= SCALE[1] * H * W * (1 + eps)
        assert (w - 0.5) / (h + 0.5) <= RATIO[1] * (1 + eps)
        assert (w + 0.5) >= RATIO[0] * max(h - 0.5, 0) * (1 - eps)
    assert fallbacks < 0.01 * n, fallbacks


def test_rrc_known_answers_and_seeding():
    for seed in range(50):
        assert CR.sample_rrc_box(random.Random(seed), 10, 400) == (0, 193, 10, 13)
        assert CR.sample_rrc_box(random.Random(seed), 400, 10) == (193, 0, 13, 10)

    def sequence(seed):
        rng = random.Random(seed)
        return [CR.sample_rrc_box(rng, 375, 500) for _ in range(20)]

    assert sequence(3) == sequence(3)
    assert sequence(3) != sequence(4)
    # a narrowed range is honoured: the whole frame only
    assert CR.sample_rrc_box(random.Random(0), 64, 64, scale=(1.0, 1.0), ratio=(1.0, 1.0)) == (0, 0, 64, 64)


def test_center_crop_known_answers():
    # landscape 375 x 500 -> square: the largest square is 375, * 0.875 = 328.125 -> 328; (375 - 328) // 2 = 23, (500 - 328) // 2 = 86
    assert CR.center_crop_box(375, 500, (224, 224)) == (23, 86, 328, 328)
    # portrait: the same, transposed
    assert CR.center_crop_box(500, 375, (224, 224)) == (86, 23, 328, 328)
    # square 256 -> 224: 256 * 0.875 = 224, (256 - 224) // 2 = 16
    assert CR.center_crop_box(256, 256, (224, 224)) == (16, 16, 224, 224)
    # a 2 : 1 output in a square frame of 100: the box is 50 x 100, * 0.5 = 25 x 50; origin (37, 25)
    assert CR.center_crop_box(100, 100, (32, 64), crop_pct=0.5) == (37, 25, 25, 50)
    # never less than a pixel a side, never more than the frame
    assert CR.center_crop_box(1, 1, (224, 224)) == (0, 0, 1, 1)
    assert CR.center_crop_box(3, 200, (224, 224), crop_pct=0.1) == (1, 99, 1, 1)
    assert CR.center_crop_box(10, 20, (8, 8), crop_pct=1.0) == (0, 5, 10, 10)


def test_crop_job_dtype_has_the_headers_layout(tmp_path):
    fields = list(CR.CROP_JOB.names)
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "loans_hip.h"', 'int main(void) {',
           '  printf("size %zu\\n", sizeof(loans_crop_job));', '  printf("lds %d\\n", LOANS_CROP_LDS_BYTES);']
    src += ['  printf("%s %%zu\\n", offsetof(loans_crop_job, %s));' % (f, f) for f in fields]
    src += ['  return 0;', '}']
    c_file, exe = tmp_path / 'layout.c', tmp_path / 'layout'
    c_file.write_text('\n'.join(src))
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), '-o', str(exe), str(c_file)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(got['size']) == CR.CROP_JOB.itemsize
    assert int(got['lds']) == CR.CROP_LDS_BYTES
    for f in fields:
        assert int(got[f]) == CR.CROP_JOB.fields[f][1], f
    assert len(got) == len(fields) + 2
    assert CR.lds_row_capacity(224) == CR.CROP_LDS_BYTES // 672


def test_crop_resize_device_rejects_bad_jobs_on_the_host():
    buf = torch.zeros(40 * 50 * 3 + 10, dtype=torch.uint8)          # a host tensor: a launch would fail, validation comes first
    ok = (10, 150, 40, 50, (0, 0, 40, 50), False)
    for bad, what in [((10, 150, 40, 50, (0, 21, 40, 30), False), 'box'),          # leaves the frame on the right
                      ((10, 150, 40, 50, (1, 0, 40, 50), False), 'box'),           # ... at the bottom
                      ((10, 150, 40, 50, (-1, 0, 10, 10), True), 'box'),
                      ((10, 150, 40, 50, (0, 0, 0, 10), False), 'box'),
                      ((11, 150, 40, 50, (0, 0, 8, 8), False), 'buffer'),          # the frame ends one byte behind the buffer
                      ((-1, 150, 40, 50, (0, 0, 8, 8), False), 'buffer'),
                      ((0, 149, 40, 50, (0, 0, 8, 8), False), 'pitch')]:
        with pytest.raises(ValueError, match=what):
            CR.crop_resize_device(buf, [ok, bad], (16, 16))
    # a vertical window above the LDS capacity: out_w = 1024 holds 21 rows, 40 rows -> 2 have a window of 41
    assert CR.lds_row_capacity(1024) == 21 and resample_coeffs(40, 2, 'bilinear')[2] == 41
    with pytest.raises(ValueError, match='window'):
        CR.crop_resize_device(buf, [ok], (2, 1024))
    with pytest.raises(ValueError):
        CR.crop_resize_device(buf, [], (16, 16))
    with pytest.raises(ValueError, match='device'):                  # everything in order but the buffer's home
        CR.crop_resize_device(buf, [ok], (16, 16))


def test_launcher_rejects_bad_arguments_before_any_launch():
    import __graft_entry__
    __graft_entry__.build()
    from loans_amd import _lib
    fn = _lib.load().loans_crop_resize_u8_f32
    p = 4096                                                        # a non-null pointer value that nothing dereferences
    assert fn(0, p, p, 1, p, 3, 16, 16, 0) == -1
    assert fn(p, 0, p, 1, p, 3, 16, 16, 0) == -1
    assert fn(p, p, 0, 1, p, 3, 16, 16, 0) == -1
    assert fn(p, p, p, 1, 0, 3, 16, 16, 0) == -1
    assert fn(p, p, p, 0, p, 3, 16, 16, 0) == -1
    assert fn(p, p, p, 65536, p, 3, 16, 16, 0) == -1
    assert fn(p, p, p, 1, p, 0, 16, 16, 0) == -1
    assert fn(p, p, p, 1, p, 3, 0, 16, 0) == -1
    assert fn(p, p, p, 1, p, 3, 16, -2, 0) == -1
    cap = CR.lds_row_capacity(224)
    assert fn(p, p, p, 1, p, cap + 1, 224, 224, 0) == -1            # one output row needs more rows than fit
    assert fn(p, p, p, 1, p, 1, 4, CR.CROP_LDS_BYTES, 0) == -1      # not even one row fits
    band = _lib.load().loans_crop_band_rows
    assert band(224, 224) == 2048 // 224 and band(8, 64) == 8 and band(5, 10000) == 1 and band(0, 5) < 0


def test_trainer_options_default_to_todays_run():
    import train_imagenet as T
    a = T.parse_args([])
    assert a.augment == 'none' and tuple(a.rrc_scale) == (0.08, 1.0) and tuple(a.rrc_ratio) == (3 / 4, 4 / 3)
    assert a.val_crop_pct == 0.875 and a.augment_seed is None
    b = T.parse_args(['--augment', 'rrc', '--rrc-scale', '0.25', '1', '--rrc-ratio', '0.5', '2', '--val-crop-pct', '1.0', '--augment-seed', '7'])
    assert b.augment == 'rrc' and tuple(b.rrc_scale) == (0.25, 1.0) and tuple(b.rrc_ratio) == (0.5, 2.0)
    assert b.val_crop_pct == 1.0 and b.augment_seed == 7
    with pytest.raises(SystemExit):
        T.parse_args(['--augment', 'autoaugment'])


def test_dataset_draws_in_index_order_from_its_own_stream(tmp_path):
    from loans_amd.common.datasets.classification_dataset import ClassificationImageDataset
    rng = np.random.RandomState(0)
    lines = []
    for n, (H, W, mode) in enumerate([(30, 41, 'RGB'), (25, 25, 'L'), (33, 20, 'RGBA')]):
        shape = (H, W) if mode == 'L' else (H, W, len(mode))
        Image.fromarray(rng.randint(0, 256, shape).astype(np.uint8)).save(str(tmp_path / ('%d.png' % n)))
        lines.append('%d.png\t%d' % (n, 10 + n))
    (tmp_path / 'set.tsv').write_text('\n'.join(lines) + '\n')
    ds = ClassificationImageDataset(str(tmp_path / 'set.tsv'), str(tmp_path), image_size=(16, 12), train=True, augment_seed=5)
    assert len(ds) == 3
    first = [ds.get_example(i) for i in range(3)]
    again = [ds.get_example(i) for i in range(3)]
    ds.reseed(5)
    replay = [ds.get_example(i) for i in range(3)]
    for (a, la), (b, lb), (c, lc) in zip(first, again, replay):
        assert a.shape == (3, 16, 12) and a.dtype == np.float32 and la.dtype == np.int32 and la == lc
        np.testing.assert_array_equal(a, c)
        assert not np.array_equal(a, b)
    assert [int(l) for _, l in first] == [10, 11, 12]
    assert np.array_equal(first[1][0][0], first[1][0][1])                       # the grey file: three equal channels
    # the host half of a batch draws what get_example draws, in index order, and decodes by the same convention
    ds.reseed(5)
    frames, draws, labels = ds.decode_batch([0, 1, 2])
    assert labels.dtype == np.int32 and labels.tolist() == [10, 11, 12]
    for f, (box, flip), (want, _) in zip(frames, draws, first):
        assert f.dtype == np.uint8 and f.shape[2] == 3
        np.testing.assert_array_equal(CR.crop_resize_host(f, box, (16, 12), flip), want)
    # validation: the centre crop, no draws
    val = ClassificationImageDataset(str(tmp_path / 'set.tsv'), str(tmp_path), image_size=(16, 12), train=False)
    state = val._aug_rng.getstate()
    a, b = val.get_example(0), val.get_example(0)
    np.testing.assert_array_equal(a[0], b[0])
    assert val._aug_rng.getstate() == state
    assert val.decode_batch([0])[1] == [(CR.center_crop_box(30, 41, (16, 12)), False)]
