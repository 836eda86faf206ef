"""No GPU, no launch: ``--num-classes`` and its refusals, and the argument checks of the three split-row entries."""
import contextlib
import ctypes

import pytest

from loans_amd.runtime import checkpoint


def test_num_classes_parses_defaults_to_1000_and_is_fixed_on_resume():
    import train_imagenet as T
    bare, wide = T.parse_args([]), T.parse_args(['--num-classes', '21841'])
    assert 'num_classes' not in vars(bare) and bare.num_classes == 1000        # a class-level default, not a parsed value
    assert wide.num_classes == 21841 and set(vars(wide)) == set(vars(bare)) | {'num_classes'}
    assert T.parse_args(['--num-classes', '9', '--synthetic-classes', '9']).num_classes == 9 and T.parse_args(['--num-classes', '65536'])
    saved, fixed = checkpoint.plain_arguments(wide), [k for k in T.RESUME_FIXED if k != 'gpus']
    older = {k: v for k, v in saved.items() if k != 'num_classes'}              # a checkpoint from before the option: 1000
    for state, args, ok in ((saved, wide, True), (saved, bare, False), (older, bare, True), (older, wide, False)):
        with contextlib.nullcontext() if ok else pytest.raises(ValueError, match='num_classes'):
            assert checkpoint.check_arguments(state, args, fixed, checkpoint.SILENT, T.RESUME_DEFAULTS_WITH_CLASSES) == []


@pytest.mark.parametrize('argv, message', [
    (['--num-classes', '8'], 'error: --num-classes is'),
    (['--num-classes', '65537'], 'error: --num-classes is'),
    (['--num-classes', '9'], 'error: --synthetic-classes 10'),          # the 10 synthetic classes must fit the head
    (['--num-classes', '8193', '--loss', 'bce'], 'error: --loss bce above 8192'),
    (['--num-classes', '8193', '--teacher', 'teacher.npz'], 'error: --teacher above 8192'),
])
def test_num_classes_is_refused(argv, message, capsys):
    import train_imagenet as T
    with pytest.raises(SystemExit):
        T.parse_args(argv)
    assert message in capsys.readouterr().err
    T.parse_args(['--num-classes', '8192', '--loss', 'bce'])            # the one-block kernels' own limit is served


def test_split_entries_check_their_arguments_before_any_hip_call():
    from loans_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(1 << 10)
    p = ctypes.addressof(buf)

    def fwd(ptrs=None, ws_bytes=1 << 10, B=4, N=8, eps=0.1, k=1, lam=0.5):
        z, ta, tb, gz, rl, rh, rhk, out, ws = ptrs or [p] * 9
        return lib.loans_softmax_xent_split_fwd_f32(z, ta, tb, lam, 0.5, gz, rl, rh, rhk, out, ws, ws_bytes, B, N, eps, k, 0)

    def evaluate(ptrs=None, ws_bytes=1 << 10, B=4, N=8, k=1):
        z, t, rows, acc, ws = ptrs or [p] * 5
        return lib.loans_softmax_xent_split_eval_f32(z, t, rows, acc, ws, ws_bytes, B, N, k, 0)

    for f, n in ((fwd, 9), (evaluate, 5)):
        for missing in range(n):
            assert f([p] * missing + [0] + [p] * (n - missing - 1)) == -1, (f.__name__, missing)
        assert f(B=0) == -1 and f(N=0) == -1 and f(k=0) == -1
        assert f(ws_bytes=4 * 32 - 1) == -1                             # one record of 32 bytes per row here
        assert f(N=65537) == -2 and f(B=65537) == -2 and f(B=1 << 15, N=1 << 16) == -2
    assert fwd(eps=1.0) == -1 and fwd(eps=float('nan')) == -1 and fwd(lam=float('inf')) == -1
    assert bytes(buf) == bytes(1 << 10)
    plan = lib.loans_softmax_xent_split_workspace
    assert plan(256, 21841) == 256 * 3 * 32 and plan(1, 65536) == 8 * 32
    assert plan(0, 8) == -1 and plan(4, 65537) == -2 and plan(65537, 8) == -2 and plan(1 << 15, 1 << 16) == -2
