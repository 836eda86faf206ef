"""Records tests/golden/conv_f32_tap_loop_bits.npz: the outputs of the deterministic launches of
tests/conv_tap_loop/test_gpu_kernels.py (forward, forward with relu(in), data gradient per class and as a class launch, the
second convolution of the pair launch), from the library that is built in the tree (run it on the commit BEFORE a change
that has to keep these bits).  Every launch runs twice on every tile; the run stops if the kernel does not reproduce
itself.  Every tile shape contracts K in the same order: one array per case and kind is kept, an array per tile only
for a tile that differs from the first, and a class launch's only where it differs from the per-class launches'.

    python -m tests.golden.make_conv_tap_loop_golden [out.npz]
"""
import sys

import numpy as np
import torch

from tests.conv_tap_loop import test_gpu_kernels as T


class _Recorded(dict):
    """what the test's lookup (golden_array) sees of an .npz file"""
    files = property(lambda self: list(self))


def main():
    from loans_amd import ops
    out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
    arrays = _Recorded()
    for name, kind in T.bit_cases():
        for tile in T.TILES:
            a = T.run(name, kind, tile)[0].cpu()
            b = T.run(name, kind, tile)[0].cpu()
            key = T.golden_key(name, kind, tile)
            if not torch.equal(a, b):
                raise SystemExit('%s: two runs differ' % key)
            try:
                found = T.golden_array(arrays, name, kind, tile)
            except KeyError:
                found = None
            if found is not None and np.array_equal(found, a.numpy()):
                print('%-28s %s  repeat run identical, equal to the array already kept' % (key, tuple(a.shape)))
                continue
            if T.golden_key(name, kind) not in arrays:
                key = T.golden_key(name, kind)
            arrays[key] = a.numpy()
            print('%-28s %s  repeat run identical, kept' % (key, tuple(a.shape)))
    c, b = T._case('c64'), T._case('co32')
    ys = [ops.conv_fprop(c['x'], b['w'], b['geo'], tile=t).cpu() for t in T.TILES + T.TILES]
    if not all(torch.equal(ys[0], y) for y in ys):
        raise SystemExit('pair_second: the tiles or two runs differ')
    arrays['pair_second'] = ys[0].numpy()
    np.savez(out, **arrays)
    print('wrote %s (%d arrays)' % (out, len(arrays)))


if __name__ == '__main__':
    main()
