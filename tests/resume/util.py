"""What the continuation tests share: how two trajectories are compared and how a measured run-to-run spread becomes a bound.

Two uninterrupted runs of one fp32 command are not bit-identical on this GPU (weight gradients and BN statistics close with
atomics), so a resumed run cannot be asked to match a straight one more closely than a second straight run does.
``d0`` is the largest relative difference between two straight runs of the test's own command, measured once on an MI355X and
written next to each assert; the resumed run is allowed ``max(4 * d0, 1e-6)`` -- 4 because a resumed run re-zeroes and refills
its workspaces in another order than a straight one.  A wrong batch, a lost momentum buffer or a lost draw moves these
quantities in the first or second digit."""
import json
import os

import numpy as np


def tolerance(d0):
    return max(4.0 * d0, 1e-6)


def rel(a, b):
    """largest difference of two arrays relative to the largest magnitude of the second"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    scale = np.abs(b).max()
    return float(np.abs(a - b).max() / scale) if scale > 0 else float(np.abs(a).max())


def read_log(log_dir):
    with open(os.path.join(log_dir, 'log')) as f:
        return json.load(f)


def worst(got, want, keys):
    """largest ``rel`` over ``keys`` of paired entries, entry by entry (a scalar is relative to itself)"""
    return max(rel(g[k], w[k]) for g, w in zip(got, want) for k in keys)


def snapshot_spread(path_a, path_b):
    """The largest difference between two snapshots, over all their float arrays, relative to the largest magnitude in the
    second one (integer persistents must be equal).  Relative to the snapshot, not to each array: some parameters have an
    analytically zero gradient (a conv bias in front of a BN) and hold nothing but rounding noise, which two straight runs
    do not share."""
    diff = scale = 0.0
    with np.load(path_a) as a, np.load(path_b) as b:
        assert set(a.files) == set(b.files)
        for k in a.files:
            if a[k].dtype.kind in 'iu':
                assert np.array_equal(a[k], b[k]), k
            else:
                diff = max(diff, float(np.abs(a[k].astype(np.float64) - b[k]).max()))
                scale = max(scale, float(np.abs(b[k]).max()))
    return diff / scale
