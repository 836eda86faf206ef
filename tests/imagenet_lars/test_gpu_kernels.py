"""-m gpu: loans_lars_ratios_f32 against float64 inside the derived bound and loans_lars_update_f32 bit-identical to
loans_momentum_sgd_f32 per segment, on the case grid of tests/imagenet_lars/cases.py; repeatability, the flags, the guards and the
argument checks of the three entries.  Every case is a handful of launches over at most 20 MB."""
import numpy as np
import pytest
import torch

from tests.imagenet_lars import cases as A

pytestmark = pytest.mark.gpu

IDS = ['%s-gs%g-wd%g' % c for c in A.GRID]
_SHARED = {}


def _values(name):
    if name not in _SHARED:
        _SHARED[name] = A.make(name)
    return _SHARED[name]


def _bits(t):
    return (t.cpu().numpy() if torch.is_tensor(t) else t).view(np.int32)


def _table(name):
    from loans_amd import ops
    device = torch.device('cuda', torch.cuda.current_device())
    if name == 'prefix':
        table = ops.LarsTable(A.PREFIX_FULL[1], A.PREFIX_FULL[2], device).prefix(A.PREFIX_N)
        assert isinstance(table, ops.LarsTable) and table.ends_host.tolist() == A.TABLES['prefix'][1]
        assert table.ends.cpu().tolist() == A.TABLES['prefix'][1] and table.flags.cpu().tolist() == A.TABLES['prefix'][2]
        return table
    n, ends, flags = A.TABLES[name]
    return ops.LarsTable(ends, flags, device)


def _device(name):
    return tuple(torch.from_numpy(a).cuda() for a in _values(name))


@pytest.mark.parametrize('name,gs,wd', A.GRID, ids=IDS)
def test_ratios_against_float64(name, gs, wd):
    from loans_amd import ops
    n, ends, flags = A.TABLES[name]
    p_h, g_h, v_h = _values(name)
    p, g, _ = _device(name)
    table = _table(name)
    table.ratios.fill_(float('nan'))
    ops.lars_ratios(p[:n], g[:n], wd, A.ETA, A.EPS, table, gs)
    got = table.ratios.cpu().numpy()
    worst = A.check_ratios(got, p_h, g_h, ends, flags, wd, gs)
    print('%s: ratio error / bound %.3f over %d segments' % (name, worst, len(ends)))
    assert worst <= 1.0, worst
    # the inputs are only read, the NaNs behind n reached nothing
    assert np.array_equal(_bits(p), _bits(p_h)) and np.array_equal(_bits(g), _bits(g_h))
    # the norms, where kept: the same sums before the quotient
    _, W, G = A.ratios_ref(p_h, g_h, ends, flags, wd, gs)
    norms = table.norms.cpu().numpy().reshape(-1, 2)
    rel = A.C * A.additions(ends) * A.U64 * A.SLACK
    assert np.all(np.abs(norms[:, 0] - W) <= rel * W) and np.all(np.abs(norms[:, 1] - G) <= rel * G)


def _per_segment(name, gs, wd, lr_dev):
    """(p, v) after ratios + loans_lars_update_f32, and after loans_momentum_sgd_f32 once per segment at the rate
    float(np.float32(lr) * np.float32(r_s)), on copies of the same buffers"""
    from loans_amd import ops
    n, ends, flags = A.TABLES[name]
    h = A.UPDATE_HYPER
    p_h, g_h, v_h = _values(name)
    p, g, v = _device(name)
    table = _table(name)
    ops.lars_ratios(p[:n], g[:n], wd, A.ETA, A.EPS, table, gs)
    ratios = table.ratios.cpu().numpy()
    lr = torch.full((1,), h['lr'], device='cuda', dtype=torch.float32) if lr_dev else h['lr']
    ops.lars_update(p[:n], g[:n], v[:n], lr, h['momentum'], wd, table, gs)
    q, w = torch.from_numpy(p_h).cuda(), torch.from_numpy(v_h).cuda()
    lo = 0
    for hi, flag, r in zip(ends, flags, ratios):
        rate = float(np.float32(h['lr']) * np.float32(r))
        ops.momentum_sgd(q[lo:hi], g[lo:hi], w[lo:hi], rate, h['momentum'], 0.0 if flag & 1 else wd, gs)
        lo = hi
    assert np.array_equal(_bits(g), _bits(g_h))
    assert np.array_equal(_bits(table.ratios), _bits(ratios))              # the update only reads the ratios
    return (p, v), (q, w), (p_h, v_h, ratios)


@pytest.mark.parametrize('name,gs,wd,lr_dev', [('n5', 1.0, 5e-5, False), ('n%d' % (2 * A.UNIT + 3), 1.0, 5e-5, False), ('prefix', 1.0, 5e-5, True),
                                               ('kinds', 0.5, 5e-5, False), ('kinds', 0.125, 0.0, True), ('resnet', 1.0, 5e-5, False),
                                               ('resnet', 0.125, 0.0, True)])
def test_update_is_the_plain_kernel_per_segment_at_one_fp32_product(name, gs, wd, lr_dev):
    n = A.TABLES[name][0]
    (p, v), (q, w), (p_h, v_h, ratios) = _per_segment(name, gs, wd, lr_dev)
    assert np.array_equal(_bits(p), _bits(q)) and np.array_equal(_bits(v), _bits(w))
    assert not np.array_equal(_bits(p)[:n], _bits(p_h)[:n])                        # something moved
    assert np.array_equal(_bits(p)[n:], _bits(p_h)[n:]) and np.array_equal(_bits(v)[n:], _bits(v_h)[n:])      # the guards did not
    # ... and the whole step sits inside the bound of the float64 rule
    ends, flags = A.TABLES[name][1:]
    h = A.UPDATE_HYPER
    g_h = _values(name)[1]
    worst = A.check_step(p.cpu().numpy(), v.cpu().numpy(), p_h, g_h, v_h, ends, flags, h['lr'], h['momentum'], wd, gs)
    print('%s: step error / bound %.3f' % (name, worst))
    assert worst <= 1.0, worst


@pytest.mark.parametrize('name', ['many', 'resnet'])
def test_two_runs_give_the_same_bits(name):
    from loans_amd import ops
    n = A.TABLES[name][0]
    h = A.UPDATE_HYPER
    out = []
    for _ in range(2):
        p, g, v = _device(name)
        table = _table(name)
        ops.lars_ratios(p[:n], g[:n], 5e-5, A.ETA, A.EPS, table, 0.5)
        ops.lars_update(p[:n], g[:n], v[:n], h['lr'], h['momentum'], 5e-5, table, 0.5)
        out.append((_bits(table.ratios), _bits(table.norms.view(torch.float32)), _bits(p), _bits(v)))
    for a, b in zip(*out):
        assert np.array_equal(a, b)


def test_flags_and_zero_norms():
    """bit 1 and a zero norm give r = 1 exactly; bit 0 takes the decay out of the ratio and out of the update"""
    from loans_amd import ops
    n, ends, flags = A.TABLES['kinds']
    kinds = A.kinds_of(len(ends), 'kinds')
    p, g, v = _device('kinds')
    table = _table('kinds')
    ops.lars_ratios(p[:n], g[:n], 0.5, A.ETA, A.EPS, table, 1.0)
    decayed = table.ratios.cpu().numpy().copy()
    ops.lars_ratios(p[:n], g[:n], 0.0, A.ETA, A.EPS, table, 1.0)
    free = table.ratios.cpu().numpy().copy()
    for s, (flag, kind) in enumerate(zip(flags, kinds)):
        if flag & 2 or kind in ('zero_w', 'zero_g'):
            assert decayed[s] == 1.0 == free[s], (s, flag, kind)
        elif flag & 1:
            assert decayed[s] == free[s] != 1.0, (s, flag, kind)
        elif kind == 'tiny':        # (eps dominates the denominator: the decay term may vanish beside it)
            assert decayed[s] <= free[s] < 1.0, (s, flag, kind)
        else:
            assert decayed[s] < free[s], (s, flag, kind)
    # zero gradient, zero momentum: a float exempt from decay stays; the others shrink by lr * r * wd with r = 1 (G = 0)
    g.zero_()
    p_h = _values('kinds')[0]
    ops.lars_ratios(p[:n], g[:n], 0.25, A.ETA, A.EPS, table, 1.0)
    assert np.array_equal(table.ratios.cpu().numpy(), np.ones(len(ends), np.float32))
    ops.lars_update(p[:n], g[:n], v[:n], 0.5, 0.0, 0.25, table, 1.0)
    got = p.cpu().numpy()
    lo = 0
    for hi, flag in zip(ends, flags):
        if flag & 1:
            assert np.array_equal(_bits(got[lo:hi]), _bits(p_h[lo:hi]))
        else:
            assert np.allclose(got[lo:hi], p_h[lo:hi] * np.float32(0.875), rtol=1e-6, atol=0)
        lo = hi


def test_argument_checks_launch_nothing():
    from loans_amd import _lib, ops
    lib = _lib.load()
    EINVAL = -1
    n, ends, flags = 40, [8, 24, 40], [0, 3, 0]
    rng = np.random.RandomState(7)
    p_h, g_h, v_h = (rng.standard_normal(n).astype(np.float32) for _ in range(3))
    p, g, v = (torch.from_numpy(a).cuda() for a in (p_h, g_h, v_h))
    table = ops.LarsTable(ends, flags, p.device)
    table.ratios.fill_(7.0)
    table.norms.fill_(7.0)
    table.workspace.fill_(7.0)
    ws_bytes = table.workspace.numel() * 8
    host = np.asarray(ends, np.int64)
    assert lib.loans_lars_workspace_bytes(host.ctypes.data, 3) == 3 * 16 == ws_bytes
    assert lib.loans_lars_workspace_bytes(np.asarray([4096, 4096 + 4100, 3 * 4096 + 4100], np.int64).ctypes.data, 3) == (1 + 2 + 2) * 16
    assert lib.loans_lars_workspace_bytes(0, 3) == -1 and lib.loans_lars_workspace_bytes(host.ctypes.data, 0) == -1
    assert lib.loans_lars_workspace_bytes(np.asarray([8, 22, 40], np.int64).ctypes.data, 3) == -1

    def tables(ends_host, nseg):
        if isinstance(ends_host, str):
            return None, 0
        keep = np.ascontiguousarray(ends if ends_host is None else ends_host, dtype=np.int64)
        return keep, keep.ctypes.data

    def ratios(p_=None, g_=None, n_=n, ends_dev=None, flags_dev=None, first_dev=None, ends_host=None, nseg=3, out=None, norms=None, ws=None,
               ws_bytes_=ws_bytes, eta=0.001, eps=1e-8):
        keep, host_ptr = tables(ends_host, nseg)
        return lib.loans_lars_ratios_f32(p.data_ptr() if p_ is None else p_, g.data_ptr() if g_ is None else g_, n_, 0.1, 1.0, eta, eps,
                                         table.ends.data_ptr() if ends_dev is None else ends_dev,
                                         table.flags.data_ptr() if flags_dev is None else flags_dev,
                                         table.first_unit.data_ptr() if first_dev is None else first_dev, host_ptr, nseg,
                                         table.ratios.data_ptr() if out is None else out, table.norms.data_ptr() if norms is None else norms,
                                         table.workspace.data_ptr() if ws is None else ws, ws_bytes_, ops._stream())

    def update(p_=None, g_=None, v_=None, n_=n, ends_dev=None, flags_dev=None, ratios_dev=None, ends_host=None, nseg=3):
        keep, host_ptr = tables(ends_host, nseg)
        return lib.loans_lars_update_f32(p.data_ptr() if p_ is None else p_, g.data_ptr() if g_ is None else g_,
                                         v.data_ptr() if v_ is None else v_, n_, 0.1, 0, 0.9, 0.1, 1.0,
                                         table.ends.data_ptr() if ends_dev is None else ends_dev,
                                         table.flags.data_ptr() if flags_dev is None else flags_dev,
                                         table.ratios.data_ptr() if ratios_dev is None else ratios_dev, host_ptr, nseg, ops._stream())

    too_many = list(range(4, 4 * ops.LARS_MAX_SEGMENTS + 8, 4))
    for call in (ratios, update):
        assert call(p_=0) == EINVAL and call(g_=0) == EINVAL                                # null pointers
        assert call(ends_dev=0) == EINVAL and call(flags_dev=0) == EINVAL and call(ends_host='null') == EINVAL
        assert call(p_=p.data_ptr() + 4) == EINVAL and call(g_=g.data_ptr() + 8) == EINVAL  # misaligned
        assert call(n_=0) == EINVAL and call(n_=-4) == EINVAL
        assert call(nseg=0) == EINVAL and call(nseg=ops.LARS_MAX_SEGMENTS + 1, ends_host=too_many, n_=too_many[-1]) == EINVAL
        assert call(ends_host=[24, 8, 40]) == EINVAL and call(ends_host=[8, 8, 40]) == EINVAL      # not ascending
        assert call(ends_host=[8, 22, 40]) == EINVAL                                        # an inner end that is no multiple of 4
        assert call(ends_host=[8, 24, 36]) == EINVAL and call(ends_host=[8, 24, 44]) == EINVAL     # the last end is not n
    assert update(v_=0) == EINVAL and update(v_=v.data_ptr() + 4) == EINVAL and update(ratios_dev=0) == EINVAL
    assert ratios(first_dev=0) == EINVAL and ratios(out=0) == EINVAL and ratios(ws=0) == EINVAL
    assert ratios(ws=table.workspace.data_ptr() + 8) == EINVAL
    assert ratios(ws_bytes_=ws_bytes - 1) == EINVAL and ratios(ws_bytes_=0) == EINVAL        # a workspace that is too small
    assert ratios(eta=0.0) == EINVAL and ratios(eta=-0.001) == EINVAL and ratios(eps=-1e-8) == EINVAL
    assert ratios(eta=float('nan')) == EINVAL and ratios(eps=float('nan')) == EINVAL
    torch.cuda.synchronize()
    assert np.array_equal(_bits(p), _bits(p_h)) and np.array_equal(_bits(v), _bits(v_h)) and np.array_equal(_bits(g), _bits(g_h))
    assert (table.ratios == 7.0).all() and (table.norms == 7.0).all() and (table.workspace == 7.0).all()
    # ... and the table as it was built is taken; eps = 0 is allowed, the norms are optional
    assert ratios(eps=0.0) == 0 and ratios(norms=0) == 0 and update() == 0
    torch.cuda.synchronize()
    assert not (table.ratios == 7.0).any() and not np.array_equal(_bits(p), _bits(p_h))
    assert table.ratios.cpu().numpy()[1] == 1.0
