#!/usr/bin/env python
"""Records tests/golden/conv_desc_codes.json: what every check of loans_amd/csrc/conv_desc.h answers on the cases of
tests/conv_desc/cases.py.

    python tests/golden/make_conv_desc_golden.py [--moved <directory with the move-only conv_desc.h>]

The answers are those of the MOVE-ONLY header -- the launchers' own statements cut into per-entry functions as they were,
`int` arithmetic included: the first commit of the change that introduced conv_desc.h, kept verbatim as
tests/golden/conv_desc_moved/conv_desc.h so that this record can be made again from the tree alone (compare it with the
launchers of the commit before).  It is built without a sanitizer (that arithmetic overflows).  A second build of it with
UndefinedBehaviorSanitizer, every check in a process of its own, marks every (case, check) that it stops on a signed
overflow; for those, and only for those, the file holds what THIS tree's header answers, and
tests/conv_desc/test_desc_cpu.py asserts that answer is a rejection."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests.conv_desc import cases as C  # noqa: E402


def build(first, flags, exe):
    """this tree's desc_cpu.cpp, conv_desc.h taken from the directory `first` (the move-only header has the same check functions)"""
    subprocess.check_call(['g++', '-O1', '-std=c++17', '-Wall', '-Werror'] + flags +
                          ['-I', first, '-I', os.path.join(ROOT, 'include'), '-I', os.path.join(ROOT, 'loans_amd', 'csrc'),
                           os.path.join(ROOT, 'tests', 'conv_desc', 'desc_cpu.cpp'), '-o', exe])


def run(exe, text, *args):
    r = subprocess.run([exe] + list(args), input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout.split(), r.stderr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--moved', default=os.path.join(HERE, 'conv_desc_moved'))
    ap.add_argument('--out', default=os.path.join(HERE, 'conv_desc_codes.json'))
    a = ap.parse_args()
    cs = C.cases()
    text = C.stdin_text(cs)
    with tempfile.TemporaryDirectory() as tmp:
        moved = ['-DCONV_DESC_MOVED']
        build(a.moved, moved, os.path.join(tmp, 'plain'))
        build(a.moved, moved + ['-fsanitize=undefined', '-fno-sanitize-recover'], os.path.join(tmp, 'ubsan'))
        recorded, _ = run(os.path.join(tmp, 'plain'), text)
        marks, _ = run(os.path.join(tmp, 'ubsan'), text, 'mark')
        build(os.path.join(ROOT, 'loans_amd', 'csrc'), ['-fsanitize=address,undefined', '-fno-sanitize-recover'], os.path.join(tmp, 'new'))
        new, _ = run(os.path.join(tmp, 'new'), text)
    assert len(recorded) == len(new) == len(cs)
    assert len(marks) == len(cs) and '?' not in ''.join(marks) + ''.join(recorded)
    marked = {}
    for i, (m, r) in enumerate(zip(marks, recorded)):
        ks = [k for k in range(len(C.CHECKS)) if m[k] == '!']
        assert all(m[k] == r[k] for k in range(len(C.CHECKS)) if k not in ks), (cs[i][0], m, r)
        if ks:
            marked[i] = ks
    codes = []
    for i, (r, n) in enumerate(zip(recorded, new)):
        codes.append(''.join(n[k] if k in marked.get(i, ()) else r[k] for k in range(len(C.CHECKS))))
    with open(a.out, 'w') as f:
        f.write('{"what": "one string per case of tests/conv_desc/cases.py, one character per check: K = LOANS_OK, I = LOANS_EINVAL, '
                'R = LOANS_ERANGE, 1 / 0 = covered / not, - = not asked; overflow = the (case, checks) whose int arithmetic '
                'overflowed before conv_desc.h computed it in int64_t",\n')
        f.write(' "checks": %s,\n' % json.dumps(C.CHECKS))
        f.write(' "overflow": {%s},\n' % ', '.join('"%d": %s' % (i, json.dumps(sorted(marked[i]))) for i in sorted(marked)))
        f.write(' "codes": [\n%s\n]}\n' % ',\n'.join('"%s"' % c for c in codes))
    print('%d cases, %d with an overflow, %d bytes' % (len(cs), len(marked), os.path.getsize(a.out)))


if __name__ == '__main__':
    main()
