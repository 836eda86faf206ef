"""Records tests/golden/conv_rows_bits.npz: the outputs of the launches of tests/conv_rows/test_gpu_kernels.py (forward,
forward with relu(in), data gradient per class and, in fp32, as a class launch; bf16 and fp32 storage), from the library
that is built in the tree (run it on the commit BEFORE a change that has to keep these bits).  Every launch runs twice on
every tile; the run stops if a kernel does not reproduce itself.  One array per storage, geometry and kind is kept, an
array per tile (as its XOR with that one) only for a tile that differs from the first, and a class launch's only where it
differs from the per-class launches'.

    python -m tests.golden.make_conv_rows_golden [out.npz]
"""
import sys

import numpy as np

from tests.conv_rows import test_gpu_kernels as T


class _Recorded(dict):
    """what the test's lookup (golden_array) sees of an .npz file"""
    files = property(lambda self: list(self))


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
    arrays = _Recorded()
    for storage, name, tile in T.cases():
        for kind in T.kinds(storage, name):
            a = T.bits(T.run(storage, name, kind, tile)[0])
            b = T.bits(T.run(storage, name, kind, tile)[0])
            key = T.golden_key(storage, name, kind, tile)
            if not np.array_equal(a, b):
                raise SystemExit('%s: two runs differ' % key)
            try:
                found = T.golden_array(arrays, storage, name, kind, tile)
            except KeyError:
                found = None
            if found is not None and np.array_equal(found, a):
                print('%-36s %s  repeat run identical, equal to the array already kept' % (key, a.shape))
                continue
            base = T.golden_key(storage, name, kind)
            if base not in arrays:
                key = base
            arrays[key] = a if key == base else a ^ arrays[base]
            print('%-36s %s  repeat run identical, kept' % (key, a.shape))
    np.savez_compressed(out, **arrays)
    print('wrote %s (%d arrays)' % (out, len(arrays)))


if __name__ == '__main__':
    main()
