"""-m gpu: the batch-mix kernel (loans_amd/csrc/mix.hip) and the two-label loss (loans_amd/csrc/classify.hip) through ``ops``
against float64 NumPy, held to the bounds tests/imagenet_mix/reference.py derives and the CPU test establishes on the fp32
restatement."""
import numpy as np
import pytest
import torch

import loans_amd
from loans_amd import ops
from loans_amd.functions import ops_small
from loans_amd.mixed_labels import MixedLabels
from tests.gpu_util import dev
from tests.imagenet import reference as R
from tests.imagenet_mix import reference as X

pytestmark = pytest.mark.gpu

WEIGHTS = ((1.0, 0.0), (0.0, 1.0), (0.5, 0.5), X.weights(np.float32(0.3)))


def boxes(H, W):
    """empty (twice: no rows, no columns), the whole frame, a single pixel, and one box on each edge"""
    y, x = H // 2, W // 2
    found = [(0, 0, 0, 0), (0, x, H, x), (0, 0, H, W), (y, x, y + 1, x + 1),
             (0, W // 3, max(1, H // 2), max(W // 3 + 1, 2 * W // 3)),          # top
             (H // 2, W // 3, H, max(W // 3 + 1, 2 * W // 3)),                  # bottom
             (H // 3, 0, max(H // 3 + 1, 2 * H // 3), max(1, W // 2)),          # left
             (H // 3, W // 2, max(H // 3 + 1, 2 * H // 3), W)]                  # right
    return sorted(set(found))


def check_mix(x, xd, shift, wa, wb, box):
    before = xd.clone()
    got_d = ops.batch_mix(xd, shift, wa, wb, box)
    again = ops.batch_mix(xd, shift, wa, wb, box)
    tag = (tuple(x.shape), shift, wa, wb, box)
    assert got_d.data_ptr() != xd.data_ptr() and torch.equal(xd, before), tag                     # x is read only
    assert torch.equal(got_d, again), tag                                                         # two launches, the same bits
    got = got_d.cpu().numpy()
    out64, blended, bound = X.batch_mix_ref(x, shift, wa, wb, box)
    copies = out64.astype(np.float32)               # (exact: every copy is an fp32 number)
    assert np.array_equal(got.view(np.uint32)[~blended], copies.view(np.uint32)[~blended]), tag
    err = np.abs(got.astype(np.float64) - out64)
    assert np.all(err[blended] <= bound[blended]), tag + (float((err[blended] / bound[blended]).max()),)
    return float((err[blended] / bound[blended]).max()) if blended.any() else 0.0


def frames(B, C, H, W, seed=0):
    """[0, 1] pixels like the feed's, with signs, a zero and large and tiny magnitudes mixed in"""
    rng = np.random.RandomState(1000 * B + 10 * H + W + seed)
    x = rng.rand(B, C, H, W).astype(np.float32)
    flat = x.reshape(-1)
    flat[::7] *= -1
    flat[::11] *= 1e4
    flat[::13] *= 1e-30
    flat[0] = 0.0
    return x


@pytest.mark.parametrize('H, W', [(1, 1), (7, 5), (16, 12), (33, 65), (40, 64)])
def test_batch_mix_over_shapes_shifts_boxes_and_weights(H, W):
    """(40, 64) is beyond the issue's shapes: the 16-byte form on more than one block per row of the batch"""
    worst = 0.0
    for B in (1, 2, 5):
        x = frames(B, 3, H, W)
        xd = dev(x)
        assert xd.data_ptr() % 16 == 0
        for shift in sorted({0, 1 % B, B - 1}):
            for box in boxes(H, W):
                for wa, wb in WEIGHTS:
                    worst = max(worst, check_mix(x, xd, shift, wa, wb, box))
    print('%d x %d worst blended error / bound %.3f' % (H, W, worst))


def test_batch_mix_with_a_source_off_the_16_byte_boundary_and_into_a_given_buffer():
    B, C, H, W = 5, 3, 16, 12
    x = frames(B, C, H, W, seed=1)
    buf = torch.zeros(x.size + 4, device='cuda')
    xd = buf[1:1 + x.size].view(B, C, H, W)
    xd.copy_(dev(x))
    assert xd.data_ptr() % 16 == 4 and xd.is_contiguous()
    for box in boxes(H, W):
        for wa, wb in WEIGHTS:
            check_mix(x, xd, 1, wa, wb, box)
    assert float(buf[0]) == 0.0 and not buf[1 + x.size:].any()
    # a destination off the boundary, given by the caller
    aligned = dev(x)
    obuf = torch.zeros(x.size + 4, device='cuda')
    out = obuf[1:1 + x.size].view(B, C, H, W)
    assert ops.batch_mix(aligned, 1, 0.5, 0.5, out=out) is out
    want, _, bound = X.batch_mix_ref(x, 1, 0.5, 0.5, (0, 0, 0, 0))
    assert np.all(np.abs(out.cpu().numpy() - want) <= bound) and float(obuf[0]) == 0.0 and not obuf[1 + x.size:].any()
    with pytest.raises(loans_amd._lib.HipKernelError):
        ops.batch_mix(aligned, 1, 0.5, 0.5, out=aligned)        # not computable in place
    with pytest.raises(loans_amd._lib.HipKernelError):
        ops.batch_mix(aligned, 5, 0.5, 0.5)                     # shift outside [0, B)
    with pytest.raises(ValueError):
        ops.batch_mix(aligned[:, :, :, ::2], 1, 0.5, 0.5)


def test_batch_mix_beyond_one_trip_of_the_grid():
    """3 x 419 x 419 single pixels per row are more than the 2048 x 256 threads of the capped grid, which leaves one block row
    for five rows of the batch: both loops of the kernel make a second trip"""
    B, C, H, W = 5, 3, 419, 419
    assert C * H * W > 2048 * 256
    x = frames(B, C, H, W)
    xd = dev(x)
    wa, wb = X.weights(np.float32(0.3))
    check_mix(x, xd, 1, wa, wb, (100, 0, 300, 211))
    check_mix(x, xd, 4, 1.0, 0.0, (0, 7, 419, 419))


# ---- the two-label loss ---------------------------------------------------------------------------------------------------------
K = 2


def _launch(zd, ta, tb, wa, wb, eps):
    return ops.softmax_xent_mix_fwd(zd, dev(ta), dev(tb), wa, wb, eps, K)


def _inside(got, ref, bounds, tag, worst=None):
    out, gzd, rl, rh, rhk = got
    loss, acc, acck, gz, row_loss, hit, hitk = ref
    lb, gb, bb = bounds
    err = np.abs(rl.cpu().numpy().astype(np.float64) - row_loss)
    gerr = np.abs(gzd.cpu().numpy().astype(np.float64) - gz)
    got_loss = float(out[0])
    assert np.all(err <= lb), tag + (float((err - lb).max()),)
    assert np.all(gerr <= gb), tag + (float((gerr - gb).max()),)
    assert abs(got_loss - loss) <= bb, tag + (got_loss, loss, bb)
    np.testing.assert_array_equal(rh.cpu().numpy(), hit.astype(np.float32), err_msg=str(tag))
    np.testing.assert_array_equal(rhk.cpu().numpy(), hitk.astype(np.float32), err_msg=str(tag))
    assert float(out[1]) == float(np.float32(acc)) and float(out[2]) == float(np.float32(acck)), tag
    valid = lb > 0
    if not valid.any():
        assert got_loss == 0.0 and not gzd.any() and not rh.any() and not rhk.any(), tag          # exact
    elif worst is not None:
        worst['loss'] = max(worst['loss'], float((err[valid] / lb[valid]).max()))
        worst['gz'] = max(worst['gz'], float((gerr[valid] / gb[valid]).max()))
        worst['batch'] = max(worst['batch'], abs(got_loss - loss) / bb)


@pytest.mark.parametrize('eps', X.MIX_EPS)
@pytest.mark.parametrize('B', X.GPU_B)
@pytest.mark.parametrize('N', X.GPU_N)
def test_mixed_loss_over_the_case_grid(N, B, eps):
    worst = {'loss': 0.0, 'gz': 0.0, 'batch': 0.0}
    seen = 0
    for name, z, ta, tb, t, expect in X.mix_cases(N, batches=(B,)):
        assert R.argmax_margin_ok(z), name
        zd = dev(z)
        for lam in X.LAMS:
            wa, wb = X.weights(lam)
            tag = (name, lam, eps)
            ref = X.mixed_ref(z, ta, tb, wa, wb, eps, K)
            bounds = X.mixed_bounds(z, ta, tb, wa, wb, eps)
            got = _launch(zd, ta, tb, wa, wb, eps)
            _inside(got, ref, bounds, tag, worst)
            for a, b in zip(got, _launch(zd, ta, tb, wa, wb, eps)):
                assert torch.equal(a, b), tag                                                   # two launches, the same bits
            # the two labels with their weights the other way round: the same target (equal weights: the dominant label is the
            # first one, so the hits are the other label's)
            ref_swapped = ref if wa != wb else X.mixed_ref(z, tb, ta, wb, wa, eps, K)
            _inside(_launch(zd, tb, ta, wb, wa, eps), ref_swapped, bounds, tag + ('swapped',))
            if wb == 0.0:       # one label: the label-smoothed entry's bits, whatever the second label holds
                for a, b in zip(got, ops.softmax_xent_ls_fwd(zd, dev(ta), eps, K)):
                    assert torch.equal(a, b), tag
            if expect is not None and np.array_equal(ta if wa >= wb else tb, t):
                # the tie profile against the dominant label: the first of two equal maxima is the hit, the second is rank 1
                valid = bounds[0] > 0
                np.testing.assert_array_equal(got[3].cpu().numpy() != 0, expect & valid, err_msg=str(tag))
                np.testing.assert_array_equal(got[4].cpu().numpy() != 0, valid, err_msg=str(tag))
            seen += 1
    assert seen == (len(R.PROFILES) if N >= 2 else len(R.PROFILES) - 1) * len(X.PAIRS) * len(X.LAMS)
    print('N=%d B=%d eps=%g worst error / bound: row loss %.3f, gz %.3f, batch loss %.3f' % (N, B, eps, worst['loss'], worst['gz'], worst['batch']))


def test_plain_bits_at_eps_zero_and_the_function_with_its_backward():
    N, B = 65, 5
    name, z, ta, tb, t, _ = next(c for c in X.mix_cases(N, batches=(B,)) if c[0].startswith('normal') and c[0].endswith('different'))
    zd = dev(z)
    # weights (1, 0), eps 0: through the label-smoothed entry the plain entry's bits
    out, gz, rl, rh, _ = ops.softmax_xent_mix_fwd(zd, dev(ta), dev(tb), 1.0, 0.0, 0.0, 1)
    p_out, p_gz, p_rl, p_rh = ops.softmax_xent_fwd(zd, dev(ta))
    assert torch.equal(out[:2], p_out) and torch.equal(gz, p_gz) and torch.equal(rl, p_rl) and torch.equal(rh, p_rh)
    # the Function on MixedLabels: upstream gradient 1 and a non-unit one
    labels = MixedLabels(dev(ta), dev(tb), 0.3)
    assert (labels.lam32, labels.oml32) == X.weights(0.3)
    ref = X.mixed_ref(z, ta, tb, labels.lam32, labels.oml32, 0.1, K)
    lb, gb, bb = X.mixed_bounds(z, ta, tb, labels.lam32, labels.oml32, 0.1)
    for g in (1.0, 0.625):
        zv = loans_amd.Variable(zd)
        lv, av, akv = ops_small.softmax_cross_entropy_mixed(zv, labels, label_smoothing=0.1, topk=K)
        assert abs(float(lv.data) - ref[0]) <= bb and float(av.data) == float(np.float32(ref[1])) and float(akv.data) == float(np.float32(ref[2]))
        lv.grad = torch.full((), g, device='cuda')
        lv.backward()
        want = ref[3] * g
        assert np.all(np.abs(zv.grad.cpu().numpy().astype(np.float64) - want) <= gb * abs(g) + R.U * np.abs(want) * R.SLACK)
    with pytest.raises(AssertionError):
        ops.softmax_xent_mix_fwd(zd, dev(ta), dev(tb)[:3], 0.5, 0.5, 0.0, 1)
