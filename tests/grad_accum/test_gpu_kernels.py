"""-m gpu: loans_grad_accum_f32 on the operand table and the size grid of tests/grad_accum/cases.py: every mode against ``torch.add``
on the same device, bit for bit, and against the NumPy restatement; the operand a mode does not write and the floats behind n
unchanged, bit for bit; repeatability; the K-step chain; the argument checks.  Both buffers start 8 floats into an allocation, the
arena's alignment.  Every case is one or two launches over at most 34 MB."""
import numpy as np
import pytest
import torch

from tests.grad_accum import cases as A

pytestmark = pytest.mark.gpu

_HOST = {}


def _rows(n):
    """the table tiled to n floats (shared, read-only), with GUARD floats of NaN and of 3.0 behind them"""
    if n not in _HOST:
        rows = A.tiled(n)
        _HOST[n] = [np.concatenate([r, np.full(A.GUARD, fill, np.float32)]) for r, fill in zip(rows, (np.nan, 3.0, -5.0))]
        for r in _HOST[n]:
            r.setflags(write=False)
    return _HOST[n]


def _bits(t):
    return (t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)).view(np.int32)


def _device(host):
    """a device copy that starts ARENA_ALIGN floats into its allocation: 32 bytes, what an arena offset guarantees and no more"""
    base = torch.empty(A.ARENA_ALIGN + host.size, device='cuda', dtype=torch.float32)
    view = base[A.ARENA_ALIGN:]
    view.copy_(torch.from_numpy(np.array(host)))
    assert view.data_ptr() % 32 == 0 and view.data_ptr() % 64 != 0
    return view


@pytest.mark.parametrize('mode', ['store', 'add', 'close'])
@pytest.mark.parametrize('n', A.SIZES)
def test_a_mode_is_torch_add_bit_for_bit(n, mode):
    from loans_amd import ops
    acc_h, g_h, _ = _rows(n)
    if mode == 'store':         # a dirty accumulator: STORE does not read it
        acc_h = np.full(n + A.GUARD, A.DIRTY, np.float32)
        acc_h[::3] = np.nan
    acc, g = _device(acc_h), _device(g_h)
    want_dev = g[:n].clone() if mode == 'store' else torch.add(acc[:n], g[:n])
    ops.grad_accum(acc[:n], g[:n], mode)
    written, other, other_h = (g, acc, acc_h) if mode == 'close' else (acc, g, g_h)
    got = written.cpu().numpy()
    assert np.array_equal(_bits(got[:n]), _bits(want_dev)), 'not the bits of torch.add'
    want_acc, want_g = A.apply(A.MODES[mode], acc_h[:n], g_h[:n])
    assert A.same_bits(got[:n], want_g if mode == 'close' else want_acc), 'not the restatement\'s'
    assert np.array_equal(_bits(other), _bits(other_h)), 'the operand the mode does not write changed'
    assert np.array_equal(_bits(got[n:]), _bits((g_h if mode == 'close' else acc_h)[n:])), 'floats behind n were written'
    # the same inputs, the same bits
    acc2, g2 = _device(acc_h), _device(g_h)
    ops.grad_accum(acc2[:n], g2[:n], mode)
    assert np.array_equal(_bits(g2 if mode == 'close' else acc2), _bits(got))


@pytest.mark.parametrize('K', [2, 3, 5])
def test_a_step_of_K_micro_batches_is_the_sequential_sum(K):
    from loans_amd import ops
    n = A.UNIT + 5
    rows = _rows(n)
    gs_h = [rows[k % 3][:n] for k in range(K)]
    acc = _device(np.full(n, np.nan, np.float32))
    g = _device(np.zeros(n, np.float32))
    want_dev = None
    for mode, g_h in zip(A.modes_of(K), gs_h):
        g.copy_(torch.from_numpy(np.array(g_h)))              # the backward of this micro-batch
        want_dev = g.clone() if want_dev is None else torch.add(want_dev, g)
        if mode == A.CLOSE:
            before = acc.clone()
        ops.grad_accum(acc, g, {v: k for k, v in A.MODES.items()}[mode])
    assert np.array_equal(_bits(g), _bits(want_dev))            # ((g1 + g2) + ..) + gK as torch adds it
    closed_h, acc_h = A.chain(gs_h)
    assert A.same_bits(g.cpu().numpy(), closed_h) and A.same_bits(acc.cpu().numpy(), acc_h)
    assert np.array_equal(_bits(acc), _bits(before))            # CLOSE left the accumulator alone
    if K > 2:       # (K = 2 is ONE correctly rounded addition: fp64 rounded once and the reverse order give the same bits)
        assert not A.same_bits(g.cpu().numpy(), A.wrong_fp64_once(gs_h)) and not A.same_bits(g.cpu().numpy(), A.wrong_reversed(gs_h))


def test_argument_checks_launch_nothing():
    from loans_amd import _lib, ops
    lib = _lib.load()
    EINVAL, ERANGE = -1, -2
    n = 40
    acc_h, g_h, _ = _rows(n)
    acc, g = _device(acc_h), _device(g_h)

    def call(acc_=None, g_=None, n_=n, mode=A.ADD):
        return lib.loans_grad_accum_f32(acc.data_ptr() if acc_ is None else acc_, g.data_ptr() if g_ is None else g_, n_, mode, ops._stream())

    assert call(acc_=0) == EINVAL and call(g_=0) == EINVAL                                                          # null pointers
    assert call(acc_=acc.data_ptr() + 4) == EINVAL and call(g_=g.data_ptr() + 8) == EINVAL                          # misaligned
    assert call(n_=0) == EINVAL and call(n_=-4) == EINVAL and call(n_=2 ** 42 + 4) == ERANGE
    assert call(mode=-1) == EINVAL and call(mode=3) == EINVAL and call(mode=2 ** 16) == EINVAL                      # unknown modes
    for mode in (A.STORE, A.ADD, A.CLOSE):
        assert call(acc_=0, mode=mode) == EINVAL and call(n_=0, mode=mode) == EINVAL
    torch.cuda.synchronize()
    assert np.array_equal(_bits(acc), _bits(acc_h)) and np.array_equal(_bits(g), _bits(g_h))
    with pytest.raises(ValueError, match='store'):
        ops.grad_accum(acc[:n], g[:n], 'sum')
    with pytest.raises(ValueError, match='differ in size'):
        ops.grad_accum(acc[:n], g[:n - 4], 'add')
    with pytest.raises(ValueError, match='float32'):
        ops.grad_accum(acc[:n].double(), g[:n], 'add')
    with pytest.raises(_lib.HipKernelError, match='LOANS_EINVAL'):
        ops.grad_accum(acc[1:n + 1], g[1:n + 1], 'add')                 # 4 bytes off the boundary
    torch.cuda.synchronize()
    assert np.array_equal(_bits(acc), _bits(acc_h)) and np.array_equal(_bits(g), _bits(g_h))
    # ... and sane arguments are taken
    assert call(mode=A.CLOSE) == 0
    torch.cuda.synchronize()
    assert A.same_bits(g.cpu().numpy()[:n], A.apply(A.CLOSE, acc_h[:n], g_h[:n])[1])
