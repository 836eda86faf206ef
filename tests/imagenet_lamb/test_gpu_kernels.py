"""-m gpu: loans_lamb_moments_f32, loans_lamb_ratios_f32 and loans_lamb_update_f32 against the float64 rule inside the derived
bounds on the case grid of tests/imagenet_lamb/cases.py; what each pass leaves alone, the guards, repeatability, segmentation that
changes no bit, the identity |p' - p| = lr |p| and the argument checks of the three entries.  Every case is a handful of launches
over at most 20 MB."""
import numpy as np
import pytest
import torch

from tests.imagenet_lamb import cases as A

pytestmark = pytest.mark.gpu

_SHARED = {}


def _values(name, warm):
    if (name, warm) not in _SHARED:
        _SHARED[name, warm] = A.make(name, warm)
    return _SHARED[name, warm]


def _bits(t):
    return (t.cpu().numpy() if torch.is_tensor(t) else t).view(np.int32)


def _table(name):
    from loans_amd import ops
    device = torch.device('cuda', torch.cuda.current_device())
    if name == 'prefix':
        table = ops.LarsTable(A.PREFIX_FULL[1], A.PREFIX_FULL[2], device).prefix(A.PREFIX_N)
        assert isinstance(table, ops.LarsTable) and table.ends_host.tolist() == A.TABLES['prefix'][1]
        return table
    n, ends, flags = A.TABLES[name]
    return ops.LarsTable(ends, flags, device)


def _device(name, warm):
    return tuple(torch.from_numpy(a).cuda() for a in _values(name, warm))


def _step(p, g, m, v, n, table, t, wd, gs, lr=A.LR, between=None):
    """the three entries over the first n floats"""
    from loans_amd import ops
    c1, c2 = A.corrections(t)
    ops.lamb_moments(p[:n], g[:n], m[:n], v[:n], A.BETA1, A.BETA2, c1, c2, A.EPS, wd, table, gs)
    ops.lamb_ratios(table)
    if between is not None:
        between()
    ops.lamb_update(p[:n], m[:n], v[:n], lr, c1, c2, A.EPS, wd, table)


@pytest.mark.parametrize('name,t,gs,wd,warm', A.GRID, ids=A.IDS)
def test_a_whole_step_against_float64(name, t, gs, wd, warm):
    n, ends, flags = A.TABLES[name]
    p_h, g_h, m_h, v_h = _values(name, warm)
    p, g, m, v = _device(name, warm)
    table = _table(name)
    table.ratios.fill_(float('nan'))
    table.norms.fill_(float('nan'))
    seen = {}

    def after_two_passes():         # p and g are only read by passes 1 and 2
        seen['p'], seen['g'], seen['r'] = _bits(p).copy(), _bits(g).copy(), _bits(table.ratios).copy()
    _step(p, g, m, v, n, table, t, wd, gs, between=after_two_passes)
    assert np.array_equal(seen['p'], _bits(p_h)) and np.array_equal(seen['g'], _bits(g_h))
    # pass 3 reads g not at all and the ratios only
    assert np.array_equal(_bits(g), _bits(g_h)) and np.array_equal(_bits(table.ratios), seen['r'])
    got = dict(p=p.cpu().numpy(), m=m.cpu().numpy(), v=v.cpu().numpy(), r=table.ratios.cpu().numpy(), norms=table.norms.cpu().numpy())
    worst = A.check(got, p_h, g_h, m_h, v_h, ends, flags, t, A.LR, wd, gs)
    print('%s: error / bound %s' % (name, ' '.join('%s %.3f' % kv for kv in sorted(worst.items()))))
    assert set(worst) == {'p', 'm', 'v', 'r', 'W', 'U'} and max(worst.values()) <= 1.0, worst
    # the NaNs and the sentinels behind n reached nothing and were not written
    for have, host in zip((p, m, v), (p_h, m_h, v_h)):
        assert np.array_equal(_bits(have)[n:], _bits(host)[n:])
    # every adapting segment moved by lr of its norm: pass 3 stepped along the u whose norm pass 1 summed
    ident, count = A.identity_check(got['p'], p_h, g_h, m_h, v_h, ends, flags, t, A.LR, wd, gs)
    print('%s: | |dp| / (lr |p|) - 1 | / tolerance %.3f over %d segments' % (name, ident, count))
    assert ident <= 1.0, ident
    assert count > 0


@pytest.mark.parametrize('name', ['many', 'resnet'])
def test_two_runs_give_the_same_bits(name):
    n = A.TABLES[name][0]
    out = []
    for _ in range(2):
        p, g, m, v = _device(name, True)
        table = _table(name)
        _step(p, g, m, v, n, table, 2, 5e-5, 0.5)
        out.append((_bits(table.ratios), _bits(table.norms.view(torch.float32)), _bits(p), _bits(m), _bits(v)))
    for a, b in zip(*out):
        assert np.array_equal(a, b)


@pytest.mark.parametrize('name,t,gs,wd', [('kinds', 2, 0.5, 5e-5), ('kinds', 1, 1.0, 0.0), ('prefix', 2, 1.0, 5e-5), ('resnet', 1000, 0.125, 5e-5)])
def test_segmentation_changes_no_bit(name, t, gs, wd):
    """the three entries over the whole table equal the same three entries called once per segment on a one-segment table of that
    slice: p', m', v' and the ratios, bit for bit"""
    from loans_amd import ops
    n, ends, flags = A.TABLES[name]
    p, g, m, v = _device(name, True)
    table = _table(name)
    _step(p, g, m, v, n, table, t, wd, gs)
    q, h, k, w = _device(name, True)
    ratios = []
    lo = 0
    for hi, flag in zip(ends, flags):
        one = ops.LarsTable([hi - lo], [flag], q.device)
        _step(q[lo:hi], h[lo:hi], k[lo:hi], w[lo:hi], hi - lo, one, t, wd, gs)
        ratios.append(one.ratios)
        lo = hi
    for whole, pieces in ((p, q), (m, k), (v, w), (table.ratios, torch.cat(ratios))):
        assert np.array_equal(_bits(whole), _bits(pieces))
    assert not np.array_equal(_bits(p)[:n], _bits(_values(name, True)[0])[:n])


def test_flags_and_zero_norms():
    """bit 1 and a zero norm give r = 1 exactly; bit 0 takes the decay out of u"""
    n, ends, flags = A.TABLES['kinds']
    kinds = A.kinds_of(len(ends), 'kinds')
    p_h = _values('kinds', False)[0]
    ratios = {}
    for wd in (0.5, 0.0):
        p, g, m, v = _device('kinds', False)
        table = _table('kinds')
        _step(p, g, m, v, n, table, 1, wd, 1.0)
        ratios[wd] = table.ratios.cpu().numpy().copy()
        if wd == 0.0:
            got, lo = p.cpu().numpy(), 0
            for hi, kind in zip(ends, kinds):        # zero gradient, zero moments, no decay: nothing moves
                assert kind != 'zero_g' or np.array_equal(_bits(got[lo:hi]), _bits(p_h[lo:hi]))
                lo = hi
    for s, (flag, kind) in enumerate(zip(flags, kinds)):
        if flag & 2 or kind == 'zero_w':
            assert ratios[0.5][s] == 1.0 == ratios[0.0][s], (s, flag, kind)
        elif kind == 'zero_g':
            assert ratios[0.0][s] == 1.0 and (ratios[0.5][s] == 1.0 if flag & 1 else ratios[0.5][s] == pytest.approx(2.0, rel=1e-6)), (s, flag, kind)
        elif flag & 1:
            assert ratios[0.5][s] == ratios[0.0][s] != 1.0, (s, flag, kind)
        else:
            assert ratios[0.5][s] != ratios[0.0][s], (s, flag, kind)


def test_argument_checks_launch_nothing():
    from loans_amd import _lib, ops
    lib = _lib.load()
    EINVAL = -1
    n, ends, flags = 40, [8, 24, 40], [0, 3, 0]
    rng = np.random.RandomState(7)
    p_h, g_h, m_h = (rng.standard_normal(n).astype(np.float32) for _ in range(3))
    v_h = np.square(rng.standard_normal(n)).astype(np.float32)
    p, g, m, v = (torch.from_numpy(a).cuda() for a in (p_h, g_h, m_h, v_h))
    table = ops.LarsTable(ends, flags, p.device)
    table.ratios.fill_(7.0)
    table.norms.fill_(7.0)
    table.workspace.fill_(7.0)
    ws_bytes = table.workspace.numel() * 8
    assert lib.loans_lars_workspace_bytes(np.asarray(ends, np.int64).ctypes.data, 3) == ws_bytes

    def tables(ends_host):
        if isinstance(ends_host, str):
            return None, 0
        keep = np.ascontiguousarray(ends if ends_host is None else ends_host, dtype=np.int64)
        return keep, keep.ctypes.data

    def pick(given, tensor):
        return tensor.data_ptr() if given is None else given

    def moments(p_=None, g_=None, m_=None, v_=None, n_=n, ends_dev=None, flags_dev=None, first_dev=None, ends_host=None, nseg=3, ws=None,
                ws_bytes_=ws_bytes, beta1=0.9, beta2=0.999, c1=10.0, c2=1000.0, eps=1e-6, **unused):
        keep, host_ptr = tables(ends_host)
        return lib.loans_lamb_moments_f32(pick(p_, p), pick(g_, g), pick(m_, m), pick(v_, v), n_, beta1, beta2, c1, c2, eps, 0.1, 1.0,
                                          pick(ends_dev, table.ends), pick(flags_dev, table.flags), pick(first_dev, table.first_unit),
                                          host_ptr, nseg, pick(ws, table.workspace), ws_bytes_, ops._stream())

    def fold(n_=n, ends_dev=None, flags_dev=None, first_dev=None, ends_host=None, nseg=3, out=None, norms=None, ws=None, ws_bytes_=ws_bytes,
             **unused):
        keep, host_ptr = tables(ends_host)
        return lib.loans_lamb_ratios_f32(n_, pick(ends_dev, table.ends), pick(flags_dev, table.flags), pick(first_dev, table.first_unit),
                                         host_ptr, nseg, pick(out, table.ratios), pick(norms, table.norms), pick(ws, table.workspace),
                                         ws_bytes_, ops._stream())

    def update(p_=None, m_=None, v_=None, n_=n, ends_dev=None, flags_dev=None, ratios_dev=None, ends_host=None, nseg=3, c1=10.0, c2=1000.0,
               eps=1e-6, **unused):
        keep, host_ptr = tables(ends_host)
        return lib.loans_lamb_update_f32(pick(p_, p), pick(m_, m), pick(v_, v), n_, 0.1, c1, c2, eps, 0.1, pick(ends_dev, table.ends),
                                         pick(flags_dev, table.flags), pick(ratios_dev, table.ratios), host_ptr, nseg, ops._stream())

    too_many = list(range(4, 4 * ops.LARS_MAX_SEGMENTS + 8, 4))
    nan = float('nan')
    for call in (moments, fold, update):
        assert call(ends_dev=0) == EINVAL and call(flags_dev=0) == EINVAL and call(ends_host='null') == EINVAL        # null pointers
        assert call(ends_dev=table.ends.data_ptr() + 4) == EINVAL                               # an int64 table off its boundary
        assert call(n_=0) == EINVAL and call(n_=-4) == EINVAL
        assert call(nseg=0) == EINVAL and call(nseg=ops.LARS_MAX_SEGMENTS + 1, ends_host=too_many, n_=too_many[-1]) == EINVAL
        assert call(ends_host=[24, 8, 40]) == EINVAL and call(ends_host=[8, 8, 40]) == EINVAL      # not ascending
        assert call(ends_host=[8, 22, 40]) == EINVAL                                        # an inner end that is no multiple of 4
        assert call(ends_host=[8, 24, 36]) == EINVAL and call(ends_host=[8, 24, 44]) == EINVAL     # the last end is not n
    for call in (moments, update):
        assert call(p_=0) == EINVAL and call(m_=0) == EINVAL and call(v_=0) == EINVAL
        assert call(p_=p.data_ptr() + 4) == EINVAL and call(m_=m.data_ptr() + 8) == EINVAL and call(v_=v.data_ptr() + 4) == EINVAL
        assert call(c1=0.5) == EINVAL and call(c2=0.999) == EINVAL and call(c1=nan) == EINVAL and call(c2=nan) == EINVAL
        assert call(eps=-1e-8) == EINVAL and call(eps=nan) == EINVAL
    assert moments(g_=0) == EINVAL and moments(g_=g.data_ptr() + 8) == EINVAL
    assert moments(beta1=1.0) == EINVAL and moments(beta1=-0.1) == EINVAL and moments(beta2=1.0) == EINVAL and moments(beta2=nan) == EINVAL
    for call in (moments, fold):
        assert call(first_dev=0) == EINVAL and call(first_dev=table.first_unit.data_ptr() + 4) == EINVAL
        assert call(ws=0) == EINVAL and call(ws=table.workspace.data_ptr() + 8) == EINVAL
        assert call(ws_bytes_=ws_bytes - 1) == EINVAL and call(ws_bytes_=0) == EINVAL        # a workspace that is too small
    assert fold(out=0) == EINVAL and fold(out=table.ratios.data_ptr() + 2) == EINVAL and fold(norms=table.norms.data_ptr() + 4) == EINVAL
    assert update(ratios_dev=0) == EINVAL and update(ratios_dev=table.ratios.data_ptr() + 2) == EINVAL
    torch.cuda.synchronize()
    for have, host in zip((p, g, m, v), (p_h, g_h, m_h, v_h)):
        assert np.array_equal(_bits(have), _bits(host))
    assert (table.ratios == 7.0).all() and (table.norms == 7.0).all() and (table.workspace == 7.0).all()
    # ... and the table as it was built is taken; eps = 0, beta = 0 and c = 1 are allowed, the norms are optional
    assert moments(eps=0.0, beta1=0.0, beta2=0.0, c1=1.0, c2=1.0) == 0 and fold(norms=0) == 0
    torch.cuda.synchronize()
    assert (table.norms == 7.0).all() and not (table.ratios == 7.0).any() and not (table.workspace == 7.0).any()
    assert np.array_equal(_bits(p), _bits(p_h)) and not np.array_equal(_bits(m), _bits(m_h))
    assert fold() == 0 and update(eps=0.0, c1=1.0, c2=1.0) == 0
    torch.cuda.synchronize()
    assert not (table.norms == 7.0).any() and not np.array_equal(_bits(p), _bits(p_h))
    assert table.ratios.cpu().numpy()[1] == 1.0
