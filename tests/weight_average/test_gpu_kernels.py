"""-m gpu: loans_average_jobs_f32 (UPDATE against float64 inside the derived bound, SWAP bit for bit) and
loans_momentum_sgd_seg_f32 (bit-identical to loans_momentum_sgd_f32 per segment) on the case grid of tests/weight_average/cases.py,
and the argument checks of both entries.  Every case is a handful of launches over at most 34 MB."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.weight_average import cases as A

pytestmark = pytest.mark.gpu

GRID = [(n,) for n in A.SINGLE_N] + [A.TABLE_N, (A.LONG_N,)]
IDS = ['n%d' % ns[0] if len(ns) == 1 else 'table' for ns in GRID]


def _jobs(ns, dst, src):
    from loans_amd import ops
    return ops.AverageJobs([(dst[o:o + n], src[o:o + n]) for n, o in zip(ns, A.layout(ns)[0])])


def _bits(t):
    return t.cpu().numpy().view(np.int32)


@pytest.mark.parametrize('ns', GRID, ids=IDS)
def test_update_against_float64(ns):
    from loans_amd import ops
    for k, omd in enumerate(A.OMDS):
        dst_h, src_h = A.make_update(ns, 10 + k)
        dst, src = torch.from_numpy(dst_h).cuda(), torch.from_numpy(src_h).cuda()
        jobs = _jobs(ns, dst, src)
        assert jobs.njobs == len(ns) and jobs.units == sum(-(-n // A.UNIT) for n in ns)
        ops.average_jobs(jobs, 'update', omd)
        worst = A.check_update(dst.cpu().numpy(), dst_h, src_h, omd, ns)
        print('omd %.6g: error / bound %.3f' % (omd, worst))
        assert worst <= 1.0, (omd, worst)
        assert np.array_equal(_bits(src), src_h.view(np.int32))                    # the live side is only read


@pytest.mark.parametrize('ns', GRID, ids=IDS)
def test_update_is_nothing_where_average_and_live_value_are_equal(ns):
    from loans_amd import ops
    dst_h, src_h = A.make_update(ns, 20, equal=True)
    for omd in A.OMDS_EQUAL:
        dst, src = torch.from_numpy(dst_h).cuda(), torch.from_numpy(src_h).cuda()
        ops.average_jobs(_jobs(ns, dst, src), 'update', omd)
        assert np.array_equal(_bits(dst), dst_h.view(np.int32)), omd
        assert np.array_equal(_bits(src), src_h.view(np.int32)), omd


@pytest.mark.parametrize('ns', GRID, ids=IDS)
def test_swap_is_bit_for_bit_and_twice_the_identity(ns):
    from loans_amd import ops
    dst_h, src_h = A.make_swap(ns, 30)
    dst, src = torch.from_numpy(dst_h).cuda(), torch.from_numpy(src_h).cuda()
    jobs = _jobs(ns, dst, src)
    ops.average_jobs(jobs, 'swap')
    want_dst, want_src = dst_h.copy(), src_h.copy()
    for n, o in zip(ns, A.layout(ns)[0]):
        want_dst[o:o + n], want_src[o:o + n] = src_h[o:o + n], dst_h[o:o + n]
    assert np.array_equal(_bits(dst), want_dst.view(np.int32)) and np.array_equal(_bits(src), want_src.view(np.int32))
    ops.average_jobs(jobs, 'swap')
    assert np.array_equal(_bits(dst), dst_h.view(np.int32)) and np.array_equal(_bits(src), src_h.view(np.int32))


def _segmented(name, lr_dev=False):
    """(p, v) after loans_momentum_sgd_seg_f32 and after loans_momentum_sgd_f32 once per segment, on copies of the same buffers"""
    from loans_amd import ops
    n, ends, flags = A.SGD_CASES[name]
    h = A.SGD_HYPER
    p_h, g_h, v_h = A.make_sgd(n, 40)
    lr = torch.full((1,), h['lr'], device='cuda', dtype=torch.float32) if lr_dev else h['lr']
    p, g, v = (torch.from_numpy(a).cuda() for a in (p_h, g_h, v_h))
    ops.momentum_sgd_seg(p, g, v, lr, h['momentum'], h['weight_decay_rate'], ops.SegmentTable(ends, flags, p.device), h['grad_scale'])
    q, w = torch.from_numpy(p_h).cuda(), torch.from_numpy(v_h).cuda()
    lo = 0
    for hi, flag in zip(ends, flags):
        ops.momentum_sgd(q[lo:hi], g[lo:hi], w[lo:hi], lr, h['momentum'], 0.0 if flag & 1 else h['weight_decay_rate'], h['grad_scale'])
        lo = hi
    assert np.array_equal(_bits(g), g_h.view(np.int32))
    return (p, v), (q, w), (p_h, flags, ends)


@pytest.mark.parametrize('name,lr_dev', [('one', False), ('eights', False), ('eights', True), ('edges', False)])
def test_segmented_sgd_is_the_plain_kernel_per_segment(name, lr_dev):
    (p, v), (q, w), (p_h, flags, ends) = _segmented(name, lr_dev)
    assert np.array_equal(_bits(p), _bits(q)) and np.array_equal(_bits(v), _bits(w))
    assert not np.array_equal(_bits(p), p_h.view(np.int32))                    # something moved
    if name == 'one':       # the plain kernel over the whole buffer
        from loans_amd import ops
        h = A.SGD_HYPER
        a, b, c = (torch.from_numpy(x).cuda() for x in A.make_sgd(A.SGD_CASES[name][0], 40))
        ops.momentum_sgd(a, b, c, h['lr'], h['momentum'], h['weight_decay_rate'], h['grad_scale'])
        assert np.array_equal(_bits(p), _bits(a)) and np.array_equal(_bits(v), _bits(c))


def test_exempt_segments_take_no_decay():
    """the flags reach the arithmetic: with a zero gradient and zero momentum an exempt float stays, the others shrink"""
    from loans_amd import ops
    n, ends, flags = A.SGD_CASES['eights']
    p_h = np.random.RandomState(5).standard_normal(n).astype(np.float32)
    p, g, v = torch.from_numpy(p_h).cuda(), torch.zeros(n, device='cuda'), torch.zeros(n, device='cuda')
    ops.momentum_sgd_seg(p, g, v, 0.5, 0.0, 0.25, ops.SegmentTable(ends, flags, p.device))
    exempt = np.repeat(np.asarray(flags, bool), 8)
    got = p.cpu().numpy()
    assert np.array_equal(got[exempt], p_h[exempt]) and np.allclose(got[~exempt], p_h[~exempt] * 0.875, rtol=1e-6, atol=0)


def test_argument_checks_launch_nothing():
    from loans_amd import _lib, ops
    lib = _lib.load()
    EINVAL = -1
    ns = (64, 5)
    dst_h, src_h = A.make_update(ns, 50)
    dst, src = torch.from_numpy(dst_h).cuda(), torch.from_numpy(src_h).cuda()
    jobs = _jobs(ns, dst, src)
    host, dev = C.addressof(jobs.host), jobs.dev.data_ptr()

    def call(dev=dev, host=host, njobs=2, units=jobs.units, mode=_lib.AVG_UPDATE):
        return lib.loans_average_jobs_f32(dev, host, njobs, units, mode, 0.5, ops._stream())

    assert call(dev=0) == EINVAL and call(host=0) == EINVAL
    assert call(njobs=0) == EINVAL and call(njobs=-1) == EINVAL
    assert call(mode=2) == EINVAL and call(mode=-1) == EINVAL
    assert call(units=jobs.units + 1) == EINVAL
    for field, value in (('dst', 0), ('src', 0), ('dst', jobs.host[1].dst + 4), ('src', jobs.host[1].src + 8), ('n', 0),
                         ('first_unit', 2)):
        bad = (_lib.AvgJob * 2)()
        C.memmove(bad, jobs.host, C.sizeof(bad))
        setattr(bad[1], field, value)
        assert call(host=C.addressof(bad)) == EINVAL, field
    torch.cuda.synchronize()
    assert np.array_equal(_bits(dst), dst_h.view(np.int32)) and np.array_equal(_bits(src), src_h.view(np.int32))
    with pytest.raises(ValueError):
        ops.AverageJobs([(dst[1:65], src[1:65].clone())][:0])
    with pytest.raises(ValueError):
        ops.AverageJobs([(dst[:64], src[:32])])
    assert call() == 0          # and the table as it was built is taken

    n, ends, flags = 40, [8, 24, 40], [0, 1, 0]
    p_h, g_h, v_h = A.make_sgd(n, 51)
    p, g, v = (torch.from_numpy(a).cuda() for a in (p_h, g_h, v_h))
    table = ops.SegmentTable(ends, flags, p.device)

    def sgd(p_=None, g_=None, v_=None, n_=n, ends_dev=None, flags_dev=None, ends_host=None, nseg=3):
        keep = np.ascontiguousarray(ends if ends_host is None else ends_host, dtype=np.int64)
        return lib.loans_momentum_sgd_seg_f32(p.data_ptr() if p_ is None else p_, g.data_ptr() if g_ is None else g_,
                                              v.data_ptr() if v_ is None else v_, n_, 0.1, 0, 0.9, 0.1, 1.0,
                                              table.ends.data_ptr() if ends_dev is None else ends_dev,
                                              table.flags.data_ptr() if flags_dev is None else flags_dev,
                                              keep.ctypes.data if ends_host != 'null' else 0, nseg, ops._stream())

    assert sgd(ends_host=[8, 22, 40]) == EINVAL            # an inner end that is no multiple of 4
    assert sgd(ends_host=[8, 24, 36]) == EINVAL            # the last end is not n
    assert sgd(ends_host=[8, 24, 44]) == EINVAL
    assert sgd(ends_host=[24, 8, 40]) == EINVAL            # not ascending
    assert sgd(ends_host=[8, 8, 40]) == EINVAL             # an empty segment
    assert sgd(nseg=0) == EINVAL and sgd(nseg=ops.SGD_MAX_SEGMENTS + 1, ends_host=list(range(4, 4 * ops.SGD_MAX_SEGMENTS + 8, 4))) == EINVAL
    assert sgd(p_=0) == EINVAL and sgd(g_=0) == EINVAL and sgd(v_=0) == EINVAL and sgd(n_=0) == EINVAL
    assert sgd(ends_dev=0) == EINVAL and sgd(flags_dev=0) == EINVAL
    assert sgd(p_=p.data_ptr() + 4) == EINVAL
    assert lib.loans_momentum_sgd_seg_f32(p.data_ptr(), g.data_ptr(), v.data_ptr(), n, 0.1, 0, 0.9, 0.1, 1.0, table.ends.data_ptr(),
                                          table.flags.data_ptr(), 0, 3, ops._stream()) == EINVAL           # no host copy of the ends
    assert lib.loans_momentum_sgd_max_segments() == ops.SGD_MAX_SEGMENTS == A.SGD_MAX_SEGMENTS
    torch.cuda.synchronize()
    assert np.array_equal(_bits(p), p_h.view(np.int32)) and np.array_equal(_bits(v), v_h.view(np.int32))
    assert sgd() == 0
    torch.cuda.synchronize()
    assert not np.array_equal(_bits(p), p_h.view(np.int32))


def test_prefix_of_a_segment_table():
    """the optimiser steps the arena's active prefix: the table cut at a parameter boundary, inside a merged segment or at its end"""
    from loans_amd import ops
    table = ops.SegmentTable([8, 24, 40], [0, 1, 0], torch.device('cuda', 0))
    assert table.prefix(40) is table
    cut = table.prefix(24)
    assert cut.ends_host.tolist() == [8, 24] and cut.ends.cpu().tolist() == [8, 24] and cut.flags.cpu().tolist() == [0, 1]
    cut = table.prefix(16)
    assert cut.ends_host.tolist() == [8, 16] and cut.ends.cpu().tolist() == [8, 16] and cut.flags.cpu().tolist() == [0, 1]
    assert table.ends.cpu().tolist() == [8, 24, 40]
