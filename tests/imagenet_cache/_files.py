"""tiny PNG sets for the frame-cache tests"""
import os

import numpy as np
from PIL import Image

# (H, W, mode): odd sizes, one grey file, one larger than the small slabs the tests use
SIZES = [(23, 31, 'RGB'), (40, 17, 'RGB'), (64, 64, 'RGB'), (20, 30, 'L'), (33, 29, 'RGB')]


def write_set(folder, sizes=SIZES, name='f', seed=0):
    """``name``.tsv in ``folder`` over one PNG per entry of ``sizes``; returns its path"""
    rng = np.random.RandomState(seed + len(sizes))
    lines = []
    for n, (H, W, mode) in enumerate(sizes):
        shape = (H, W) if mode == 'L' else (H, W, 3)
        Image.fromarray(rng.randint(0, 256, shape).astype(np.uint8)).save(os.path.join(folder, '%s%d.png' % (name, n)))
        lines.append('%s%d.png\t%d' % (name, n, (3 * n + 1) % 4))
    path = os.path.join(folder, name + '.tsv')
    with open(path, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    return path


def nbytes(n, sizes=SIZES):
    return sizes[n][0] * sizes[n][1] * 3
