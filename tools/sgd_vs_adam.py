#!/usr/bin/env python
"""Development probe: the momentum-SGD update and plain Adam ALONE, operands cold, interleaved in one sitting, at the ResNet-18
localizer's and the ResNet-50 localizer + assessor's parameter counts.  SGD moves 20 bytes per parameter (p, g, v read; p, v
written), plain Adam 28 (p, g, m, v read; p, m, v written)."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                # noqa: E402
from loans_amd import ops   # noqa: E402

scrub = torch.empty(512 << 20, device='cuda', dtype=torch.uint8)


def once(fn):
    scrub.zero_()           # nothing of the operands left in the Infinity Cache
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); e1.synchronize()
    return e0.elapsed_time(e1)


def line(name, ts, n, nbytes):
    med = statistics.median(ts)
    return '%-13s n = %9d: median %.4f ms (%.4f .. %.4f over %d) = %.2f TB/s at %d bytes per parameter' % (
        name, n, med, min(ts), max(ts), len(ts), n * nbytes / med * 1e-9, nbytes)


for n in (12_600_000, 78_000_000):
    p, g, m, v = (torch.rand(n, device='cuda') * 0.01 for _ in range(4))
    sgd = lambda: ops.momentum_sgd(p, g, v, 0.05, 0.9, 5e-4)                                   # noqa: E731
    adam = lambda: ops.adam_amsgrad(p, g, m, v, None, 1e-4, 0.9, 0.999, 1e-8, 1.0, 0.0)         # noqa: E731
    for fn in (sgd, adam, sgd, adam):
        once(fn)
    ts, ta = [], []
    for _ in range(21):
        ts.append(once(sgd))
        ta.append(once(adam))
    print(line('momentum_sgd', ts, n, 20), flush=True)
    print(line('adam (plain)', ta, n, 28), flush=True)
