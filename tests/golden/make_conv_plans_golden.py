"""Records tests/golden/conv_launch_plans.json: what the convolution wrappers of loans_amd/ops.py ask the autotuner and the
library for the cases of tests/test_conv_plans_cpu.py (run it on the commit BEFORE a change that has to keep these plans;
it needs neither a device nor the built library, and two runs write the same bytes).

    python -m tests.golden.make_conv_plans_golden [out.json]
"""
import sys

import pytest

from tests import test_conv_plans_cpu as T


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
    plans = {}
    for name in T.PASSES:
        with pytest.MonkeyPatch.context() as mp:
            plans[name] = T.record_pass(mp, name)
        print('%-18s %3d cases, %4d library calls, %3d tune requests' % (
            name, len(plans[name]), sum(len(c['calls']) for c in plans[name].values()),
            sum(len(c['tune']) for c in plans[name].values())))
    with open(out, 'w') as f:
        f.write(T.dumps(plans))
    print('wrote %s' % out)


if __name__ == '__main__':
    main()
