"""The host-side rule of a segment table (loans_amd/csrc/seg_table.h) on the CPU: the header compiles as plain C++, and
segtable_cpu.cpp -- a stand-alone program built here with AddressSanitizer and UndefinedBehaviorSanitizer -- answers every table
the three GPU argument-check tests (tests/weight_average, tests/imagenet_lars, tests/imagenet_lamb) hand to the entries, the unit
counts of ops.lars_first_units and a table that ends at 2^63 - 1.  The expected answers are a restatement of the rule in Python
integers (units_ref), not read off the program."""
import os
import subprocess

import pytest

from tests.imagenet_lars import cases as A

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
UNIT, LIMIT = A.UNIT, A.MAX_SEGMENTS
ANY = -1
TOO_MANY = list(range(4, 4 * LIMIT + 8, 4))         # LIMIT + 1 segments of four floats


def units_ref(ends, nseg, n, unit=UNIT):
    """exclusive ends, ascending, no empty segment, every end but the last a multiple of 4, the last one n (ANY: whatever it is),
    1 <= nseg <= LIMIT: the sum of ceil(length / unit) over the first nseg segments, or -1"""
    if ends is None or not 1 <= nseg <= LIMIT:
        return -1
    starts = [0] + list(ends[:nseg - 1])
    for s, (lo, hi) in enumerate(zip(starts, ends[:nseg])):
        if hi <= lo or (s < nseg - 1 and hi % 4):
            return -1
    if n != ANY and ends[nseg - 1] != n:
        return -1
    return sum(-(-(hi - lo) // unit) for lo, hi in zip(starts, ends[:nseg]))


# (name, ends, nseg, n, accepted); the argument-check tests' tables are over n = 40 floats
CHECKS = [
    ('as built', [8, 24, 40], 3, 40, True),
    ('not ascending', [24, 8, 40], 3, 40, False),
    ('an empty segment', [8, 8, 40], 3, 40, False),
    ('an empty first segment', [0, 24, 40], 3, 40, False),
    ('an inner end that is no multiple of 4', [8, 22, 40], 3, 40, False),
    ('a ragged last end', [8, 24, 39], 3, 39, True),
    ('the last end is short of n', [8, 24, 36], 3, 40, False),
    ('the last end is behind n', [8, 24, 44], 3, 40, False),
    ('any n', [8, 24, 44], 3, ANY, True),
    ('an inner end that is no multiple of 4, any n', [8, 22, 40], 3, ANY, False),
    ('nseg 0', [8, 24, 40], 0, 40, False),
    ('nseg negative', [8, 24, 40], -1, 40, False),
    ('no table', None, 3, 40, False),
    ('the limit', TOO_MANY[:LIMIT], LIMIT, TOO_MANY[LIMIT - 1], True),
    ('the limit + 1', TOO_MANY, LIMIT + 1, TOO_MANY[-1], False),
    ('the limit + 1, n of the small table', TOO_MANY, LIMIT + 1, 40, False),
    ('the workspace example', [4096, 4096 + 4100, 3 * 4096 + 4100], 3, ANY, True),
]
LENGTHS = (1, UNIT - 1, UNIT, UNIT + 1)
COUNTS = [('n%d' % n, [n], 1, n, True) for n in LENGTHS] + [('resnet', A.TABLES['resnet'][1], len(A.TABLES['resnet'][1]), A.TABLES['resnet'][0], True)]
INT64_MAX = 2 ** 63 - 1
HUGE = [('an end at 2^63 - 1', [8, INT64_MAX], 2, INT64_MAX, True), ('an end at 2^63 - 1, any n', [8, INT64_MAX], 2, ANY, True),
        ('one segment of 2^63 - 1', [INT64_MAX], 1, INT64_MAX, True)]
ALL = CHECKS + COUNTS + HUGE


@pytest.fixture(scope='module')
def answers(tmp_path_factory):
    exe = tmp_path_factory.mktemp('arena_kernels') / 'segtable_cpu'
    subprocess.check_call(['g++', '-O1', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover', '-Wall', '-Werror',
                           '-I', os.path.join(ROOT, 'include'), '-I', os.path.join(ROOT, 'loans_amd', 'csrc'),
                           os.path.join(HERE, 'segtable_cpu.cpp'), '-o', str(exe)])
    lines = []
    for _, ends, nseg, n, _ in ALL:
        lines.append(' '.join(map(str, [n, UNIT, nseg, -1 if ends is None else len(ends)] + list(ends or []))))
    run = subprocess.run([str(exe)], input='\n'.join(lines) + '\n', stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]       # a sanitizer report ends the program
    out = run.stdout.split('\n')
    assert out[len(ALL)] == 'limit %d' % LIMIT
    return dict(zip([c[0] for c in ALL], map(int, out[:len(ALL)])))


@pytest.mark.parametrize('name,ends,nseg,n,ok', CHECKS, ids=[c[0] for c in CHECKS])
def test_accepts_and_rejects(answers, name, ends, nseg, n, ok):
    want = units_ref(ends, nseg, n)
    assert (want >= 0) == ok                # (the restatement itself says what the argument-check tests say)
    assert answers[name] == want


def test_unit_counts_are_lars_first_units(answers):
    from loans_amd import ops
    assert (ops.LARS_UNIT, ops.LARS_MAX_SEGMENTS, ops.SGD_MAX_SEGMENTS) == (UNIT, LIMIT, LIMIT)
    for (name, ends, nseg, n, _), units in zip(COUNTS, (1, 1, 1, 2, None)):
        want = ops.lars_first_units(ends)[1]
        assert want == units_ref(ends, nseg, n) == A.first_units(ends)[1] and units in (None, want)
        assert answers[name] == want, name
    assert answers['the workspace example'] == 1 + 2 + 2


def test_an_end_near_int64_max_does_not_overflow(answers):
    """(len + unit - 1) / unit would wrap for these; the sanitizers end the program on a signed overflow"""
    for name, ends, nseg, n, _ in HUGE:
        want = units_ref(ends, nseg, n)
        last = ends[-1] - (ends[-2] if len(ends) > 1 else 0)
        assert want == len(ends) - 1 + 2 ** 51 and last + UNIT - 1 > INT64_MAX
        assert answers[name] == want, name
