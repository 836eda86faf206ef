"""The host-side launch rules of the convolution entry points (loans_amd/csrc/conv_desc.h) on the CPU: the header compiles as
plain C++, and desc_cpu.cpp -- a stand-alone program built here with AddressSanitizer and UndefinedBehaviorSanitizer -- runs
every per-entry check on the cases of cases.py.  The answers are pinned by tests/golden/conv_desc_codes.json, recorded from
the commit that only MOVED the launchers' statements into the header (make_conv_desc_golden.py): the rules decide what they
decided in the launchers, except where the launchers' `int` arithmetic overflowed -- those (case, check) pairs are listed,
and there the header, which computes in int64_t, must reject."""
import json
import os
import subprocess

import pytest

from . import cases as C

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REJECTED = 'IR0'


@pytest.fixture(scope='module')
def golden():
    with open(os.path.join(ROOT, 'tests', 'golden', 'conv_desc_codes.json')) as f:
        return json.load(f)


@pytest.fixture(scope='module')
def answers(tmp_path_factory):
    exe = tmp_path_factory.mktemp('conv_desc') / 'desc_cpu'
    subprocess.check_call(['g++', '-O1', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover', '-Wall', '-Werror',
                           '-I', os.path.join(ROOT, 'include'), '-I', os.path.join(ROOT, 'loans_amd', 'csrc'),
                           os.path.join(HERE, 'desc_cpu.cpp'), '-o', str(exe)])
    cs = C.cases()
    run = subprocess.run([str(exe)], input=C.stdin_text(cs), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]       # a sanitizer report ends the program
    return cs, run.stdout.split()


def test_checks_answer_as_recorded(golden, answers):
    cs, got = answers
    assert golden['checks'] == C.CHECKS and len(golden['codes']) == len(cs) == len(got)
    bad = [(cs[i][0], got[i], golden['codes'][i]) for i in range(len(cs)) if got[i] != golden['codes'][i]]
    assert not bad, bad[:10]


def test_overflow_cases_are_rejected(golden, answers):
    cs, got = answers
    over = {int(i): ks for i, ks in golden['overflow'].items()}
    assert over
    for i, ks in over.items():
        for k in ks:
            assert got[i][k] in REJECTED, (cs[i][0], C.CHECKS[k], got[i])
    # the issue's example: an output stride whose product with the grid wraps a 32-bit int, on every forward check
    names = {cs[i][0]: i for i in over}
    for k in map(C.CHECKS.index, C.FORWARD):
        hit = [n for n, i in names.items() if n.endswith('gridH=3 osy=0x40000001') and k in over[i]]
        assert hit, C.CHECKS[k]


def test_golden_covers_every_outcome(golden):
    codes, cs = golden['codes'], C.cases()
    for k, name in enumerate(C.CHECKS):
        col = {c[k] for c in codes}
        assert col & set('K1'), name
        assert col & set('I0'), name
        assert ('R' in col) == (name in C.CAN_ERANGE), name
    unmutated = {n for n, _, _ in C.bases()}
    for i, c in enumerate(cs):
        if c[0] in unmutated:
            assert 'K' in codes[i], c[0]
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'conv_desc_codes.json')) < 300 * 1024
