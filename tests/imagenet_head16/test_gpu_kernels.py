"""-m gpu: the wide Linear on the bf16 matrix cores (loans_linear_wide16_*, csrc/head_bf16.hip) against float64 on operands rounded
by ``.to(torch.bfloat16)``.  Integer operands in [-4, 4] are exact in bf16 and every partial sum stays below 2^24, so the kernels
must match exactly; standard-normal operands are held to  R 2^-23 sum_r |a_r| |b_r|  (R additions in any order at a unit roundoff
of 2^-23, twice fp32's; the products of two bf16 are exact in fp32) plus 2^-24 |out| for the bias / prior-gradient add."""
import ctypes

import pytest
import torch

from loans_amd import _lib, ops

pytestmark = pytest.mark.gpu
T, C = ops.WIDE16_TILE, ops.WIDE16_CHUNK
# (B, K, N).  B is a tile row (forward, data gradient) and the weight gradient's reduction; K the forward's reduction and a tile
# edge of both gradients; N a tile column (forward, weight gradient) and the data gradient's reduction
SHAPES = ([(1, 4, 9)]
          + [(T + d, C + 4 * d, C + d) for d in (-1, 0, 1)]       # one short of, at, one past: tile in B, chunk in K and N
          + [(C + d, T + 4 * d, T + d) for d in (-1, 0, 1)]       # ... chunk in B, tile in K and N
          + [(6, 8, 9 * C + 12),                                  # data gradient: 10 chunks in 3 slices of 4, 4, 2, the last ragged
             (T + 2, T + 4, T + 3)])                              # two tiles in every dimension, two slices


def r(a):
    return a.to(torch.bfloat16).double()


def operands(shape, kind):
    B, K, N = shape
    g = torch.Generator().manual_seed(B * 1000003 + K * 1009 + N)
    draw = (lambda *s: torch.randint(-4, 5, s, generator=g).float()) if kind == 'int' else (lambda *s: torch.randn(*s, generator=g))
    return [draw(*s) for s in ((B, K), (N, K), (N,), (B, N), (N, K), (N,))]       # x, W, b, gy, prior gW, prior gb


def run(x, W, b, gy, gW0, gb0):
    xd, Wd, bd, gyd = x.cuda(), W.cuda(), b.cuda(), gy.cuda()
    gW, gb = gW0.cuda(), gb0.cuda()
    y = ops.linear_wide_fwd(xd, Wd, bd, compute='bf16')
    gx = ops.linear_wide_bwd(xd, Wd, gyd, gW=gW, gb=gb, compute='bf16')
    return [t.cpu() for t in (y, gx, gW, gb)]


@pytest.mark.parametrize('kind', ['int', 'normal'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_three_directions_against_float64_of_the_rounded_operands(shape, kind):
    x, W, b, gy, gW0, gb0 = operands(shape, kind)
    B, K, N = shape
    got = run(x, W, b, gy, gW0, gb0)
    want = [r(x) @ r(W).T + b.double(), r(gy) @ r(W), gW0.double() + r(gy).T @ r(x), gb0.double() + gy.double().sum(0)]
    mass = [r(x).abs() @ r(W).abs().T, r(gy).abs() @ r(W).abs(), r(gy).abs().T @ r(x).abs(), gy.double().abs().sum(0)]
    for name, out, ref, m, R in zip(('y', 'gx', 'gW', 'gb'), got, want, mass, (K, N, B, B)):
        err = (out.double() - ref).abs()
        bound = R * 2.0 ** -23 * m + 2.0 ** -24 * out.double().abs() if kind == 'normal' else torch.zeros_like(ref)
        print('%s %s %s: max error %.3g, smallest margin %.3g' % (shape, kind, name, err.max(), (bound - err).min()))
        assert out.shape == ref.shape and bool((err <= bound).all()), name
    again = run(x, W, b, gy, gW0, gb0)
    assert all(torch.equal(a, o) for a, o in zip(again, got))               # two runs, the same bits


def test_every_operand_is_rounded_to_nearest_even():
    """a contraction against identity rows returns one rounded operand: ties to even in both directions, both neighbours of a tie,
    negatives.  Truncation or round-half-up gives other bits."""
    one = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 255 + 0.5, 3.0e38], dtype=torch.float32)      # ties: down to 1, up to 1 + 2^-6, ...
    s = torch.cat([one, torch.nextafter(one, torch.zeros(4)), torch.nextafter(one, torch.full((4,), float('inf'))), torch.tensor([0.1, 1e-20])])
    special = torch.cat([s, -s])                                            # 28 values
    vals = torch.cat([special, torch.randn(40 * 32 - 28, generator=torch.Generator().manual_seed(1))])
    eye = torch.eye(32)
    z = lambda *shape: torch.zeros(*shape)
    Wv, xv, gv = vals.reshape(40, 32), vals.reshape(40, 32).flip(0), vals.reshape(32, 40)
    want = lambda a: a.to(torch.bfloat16).float()
    assert torch.equal(run(eye, Wv, z(40), z(32, 40), z(40, 32), z(40))[0], want(Wv).T)             # y[m][c] = r(W[c][m])
    assert torch.equal(run(xv, eye, z(32), z(40, 32), z(32, 32), z(32))[0], want(xv))               # y = r(x)
    y, gx, gW, _ = run(eye, eye, z(32), gv[:, :32].contiguous(), z(32, 32), z(32))
    assert torch.equal(gx, want(gv[:, :32])) and torch.equal(gW, want(gv[:, :32]).T)                # gx = r(gy), gW = r(gy)^T
    assert want(special[:2]).tolist() == [1.0, 1 + 2.0 ** -6]


def test_workspace_contract_and_the_untouched_fp32_arm():
    lib = _lib.load()
    B, K, N = 6, 8, 9 * C + 12
    x, W, b, gy, gW0, gb0 = [t.cuda() for t in operands((B, K, N), 'normal')]
    need = lib.loans_linear_wide16_workspace(B, K, N)
    assert need == 3 * B * K * 4
    ws, gx = torch.empty(need // 4, device='cuda'), torch.full((B, K), 7.0, device='cuda')
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    bwd16 = lambda nbytes: lib.loans_linear_wide16_bwd_f32(p(x), p(W), p(gy), p(gx), None, None, p(ws), nbytes, B, K, N, ops._stream())
    assert bwd16(need - 1) == -1 and bool((gx == 7.0).all())                # refused before any launch
    assert bwd16(need) == 0 and torch.equal(gx, ops.linear_wide_bwd(x, W, gy, compute='bf16'))
    # compute='f32', and no compute at all, are the fp32 entries' bits
    y32, gx32, gW32, gb32 = torch.empty(B, N, device='cuda'), torch.empty(B, K, device='cuda'), gW0.clone(), gb0.clone()
    assert lib.loans_linear_wide_fwd_f32(p(x), p(W), p(b), p(y32), B, K, N, ops._stream()) == 0
    assert lib.loans_linear_wide_bwd_f32(p(x), p(W), p(gy), p(gx32), p(gW32), p(gb32), B, K, N, ops._stream()) == 0
    for kw in ({}, {'compute': 'f32'}):
        gW, gb = gW0.clone(), gb0.clone()
        assert torch.equal(ops.linear_wide_fwd(x, W, b, **kw), y32)
        assert torch.equal(ops.linear_wide_bwd(x, W, gy, gW=gW, gb=gb, **kw), gx32) and torch.equal(gW, gW32) and torch.equal(gb, gb32)
    gb16 = gb0.clone()
    ops.linear_wide_bwd(x, W, gy, gb=gb16, need_gx=False, compute='bf16')
    assert torch.equal(gb16, gb32)                                          # the bias gradient is the fp32 arm's, bit for bit
    with pytest.raises(ValueError):
        ops.linear_wide_fwd(x, W, b, compute='fp16')
