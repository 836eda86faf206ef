"""Records tests/golden/wgrad_f32_loader_bits.npz: dw of loans_wgrad_f32 at splits = 1 for the cases of
tests/wgrad_loader/test_gpu_kernels.py::test_wgrad_loader_bits, from the library that is built in the tree (run it on the
commit BEFORE a change that has to keep these bits).  Every case runs twice; the run stops if the kernel does not
reproduce itself.

    python -m tests.golden.make_wgrad_loader_golden [out.npz]
"""
import sys

import numpy as np
import torch

from tests.wgrad_loader import test_gpu_kernels as T


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
    arrays = {}
    for name, relu, tile in T.golden_cases():
        a = T.run_wgrad(name, relu, tile, 1).cpu()
        b = T.run_wgrad(name, relu, tile, 1).cpu()
        if not torch.equal(a, b):
            raise SystemExit('%s: two runs differ' % T.golden_key(name, relu, tile))
        arrays[T.golden_key(name, relu, tile)] = a.numpy()
        print('%-24s %s  repeat run identical' % (T.golden_key(name, relu, tile), tuple(a.shape)))
    np.savez(out, **arrays)
    print('wrote %s (%d arrays)' % (out, len(arrays)))


if __name__ == '__main__':
    main()
