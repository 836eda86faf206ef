"""CPU: what tests/eval_mode/cases.py writes down holds before any GPU run -- the fp32 restatement of bn_eval_coeffs_kernel sits
inside every derived bound on every case, with ``beta - rm sc`` contracted into an FMA and not; ``RefNet`` is the oracle's and the
existing SE / blur references' model; and the conditions on the model inputs: training-mode and test-mode logits at least 100 bounds
apart (a device path that silently used batch statistics fails), no ReLU input within 1e-6 of zero, gates that are not saturated,
labels whose rank the bound cannot change."""
import json

import numpy as np
import pytest

from oracle import model as M
from tests.eval_mode import cases as K
from tests.imagenet import reference as R


@pytest.mark.parametrize('C_', K.COEFF_C)
def test_the_restatement_sits_inside_the_derived_bounds(C_):
    ratios, seen = {}, set()
    for rot in K.rotations(C_):
        d = K.make_coeffs(C_, rot)
        seen |= set(d['profile'].tolist())
        for fma in (False, True):
            K.check_coeffs(K.coeffs_fp32(d, fma), d, ratios)
    print('EVAL_RATIOS C%d %s' % (C_, json.dumps(ratios, sort_keys=True)))
    assert seen == set(range(K.N_PROFILES))             # every combination of variance, mean and gamma, at every channel count
    assert all(0 < r <= 1 for r in ratios.values())


def test_the_grid_holds_the_edge_values():
    d = K.make_coeffs(2048)
    eps = np.float32(K.C.BN_EPS)
    assert (d['rv'] == 0).any() and (d['rv'] < 2e-12).any() and (np.abs(d['rv'] / eps - 1) <= 0.26).any() and (d['rv'] > 5e5).any()
    assert (d['rm'] == 0).any() and (d['rm'] > 9e3).any() and (d['rm'] < -50).any() and ((d['rm'] > 50) & (d['rm'] < 70)).any()
    assert (d['gamma'] == 0).any() and (d['gamma'] == np.float32(1e-3)).any() and (d['gamma'] < -0.5).any() and (d['gamma'] > 0.5).any()
    worst = (d['rv'] == 0) & (d['rm'] > 9e3) & (d['gamma'] < 0)         # rstd = 1 / sqrt(eps) meets the largest mean
    assert worst.any()
    # the two readings of the shift differ somewhere: the bound is asked to cover both, not one twice
    a, b = K.coeffs_fp32(d, False)['shift'], K.coeffs_fp32(d, True)['shift']
    assert (a != b).any()
    # a wrong kernel is outside: no eps, and gamma in the place of scale
    ref, bounds = K.coeffs_ref(d), K.coeffs_bounds(K.coeffs_ref(d))
    with np.errstate(divide='ignore', invalid='ignore'):
        no_eps = 1 / np.sqrt(d['rv'].astype(np.float64))
    live = (d['rv'] > 0.1) & (d['rv'] < 10)         # (at 1e6 eps is below the rounding, at 0 its absence is infinite)
    assert (np.abs(no_eps - ref['rstd']) > bounds['rstd'])[live].all()
    wrong = d['beta'].astype(np.float64) - ref['mean'] * d['gamma']
    assert (np.abs(wrong - ref['shift']) > bounds['shift'])[(d['rm'] != 0) & (d['gamma'] != 0) & ~live].all() and live.any()


@pytest.mark.parametrize('variant', list(K.VARIANTS))
def test_conditions_on_the_model_inputs(variant):
    test, train = K.reference(variant, 'f64'), K.reference(variant, 'f64', train=True)
    z, bound = K.model_tol(variant, False)
    gap = float(np.abs(train.logits - test.logits[:2]).max())
    print('%s: train / test logits %.4g apart, largest bound %.4g (%.0f bounds); closest ReLU input %.3g (test) %.3g (train); '
          'label margin %.3g bounds' % (variant, gap, bound.max(), gap / bound.max(), test.closest_to_zero(), train.closest_to_zero(),
                                        K.label_margin(variant, False)))
    assert gap >= 100 * bound.max()
    assert test.closest_to_zero() >= 1e-6 and train.closest_to_zero() >= 1e-6
    assert K.label_margin(variant, False) > 2 and K.label_margin(variant, False, rows=3) > 2
    if 'se' in variant:         # every unit's gates spread, none saturated (cases.SE_DOWN_SCALE)
        assert len(test.gates) == 8
        for g in test.gates + train.gates:
            assert 1e-3 < g.min() < 0.3 and 0.7 < g.max() < 1 - 1e-3
    # a sample's test-mode logits do not depend on the batch it is in: the references of B = 1, 2 come from the one of B = 3
    alone = K.run(K.start_params(variant), variant, K.frames3()[1:2], False, np.float64).logits
    assert np.abs(alone[0] - test.logits[1]).max() <= 1e-9 * np.abs(test.logits[1]).max()
    t = K.labels(variant)
    assert K.metrics(test.logits[:2], t[:2])[1:] == (0.5, 1.0)
    acc3 = K.metrics(test.logits, t)[1:]
    assert abs(acc3[0] - 1 / 3) < 1e-12 and abs(acc3[1] - 2 / 3) < 1e-12


@pytest.mark.parametrize('variant', K.BF16_ARMS)
def test_the_bf16_bound_is_measured_against_the_oracle(variant):
    z, bound = K.model_tol(variant, True, slice(0, 2))
    d = float(np.abs(K.reference(variant, 'bf16').logits[:2] - z).max())
    sep64, sep16 = K.separation(variant, 'f64'), K.separation(variant, 'bf16')
    print('%s bf16: emulated fp32 oracle %.4g from the float64 oracle (largest logit %.4g, largest bound %.4g); train / test logits '
          '%.4g apart in float64 (%.1f bounds), %.4g in the emulation (%.1f bounds); label margin %.3g bounds'
          % (variant, d, np.abs(z).max(), bound.max(), sep64, sep64 / bound.max(), sep16, sep16 / bound.max(),
             K.label_margin(variant, True)))
    assert 0 < d < 0.1 * np.abs(z).max() and np.all(bound >= 5 * d)
    # a device path that used batch statistics is far outside the bf16 bound too (cases.BF16_SEPARATION: why not 100)
    assert sep64 >= K.BF16_SEPARATION * bound.max() and sep16 >= K.BF16_SEPARATION * bound.max()
    # accuracy and top-5 accuracy of the reference are decided within the bf16 bound
    assert K.label_margin(variant, True) > 2
    assert K.metrics(z, K.labels(variant)[:2])[1:] == (0.5, 1.0)


def test_the_frames_are_the_generators():
    from loans_amd.datasets import synthetic
    assert np.array_equal(K.frames3()[:2], synthetic.make_frames(K.FRAME_SEED, 2, K.H, K.W))
    assert K.frames3().shape == (3, 3, K.H, K.W) and K.frames3().dtype == np.float32


def test_refnet_is_the_existing_references_model():
    """the same bits as R.ResNet18Classifier (also inside the bf16 emulation), tests/imagenet_se's and tests/imagenet_blurpool's
    classifiers, in test and in training mode.  SE and blur together have no reference to be held to (cases.py)."""
    from tests.imagenet_blurpool.test_gpu_model import BlurResNet18Classifier, BlurResUnit
    from tests.imagenet_se.reference import SEResNet18Classifier
    fr, t = K.frames3()[:2], np.array([3, 7], np.int32)
    for variant, cls in (('plain', R.ResNet18Classifier), ('se', SEResNet18Classifier), ('blur', BlurResNet18Classifier)):
        for train in (False, True):
            other = cls(M.cast_params(dict(K.start_params(variant)), np.float64), K.FE, train)
            other.forward(fr.astype(np.float64), t)
            mine = K.run(K.start_params(variant), variant, fr, train, np.float64, t=t)
            assert np.array_equal(mine.logits, other.logits) and mine.loss == other.loss, (variant, train)
            for key in K.STATE_KEYS:
                assert np.array_equal(mine.p[key + '/avg_var'], other.p[key + '/avg_var']), key
    other = R.ResNet18Classifier(M.cast_params(dict(K.start_params('plain')), np.float32), K.FE, False)
    with M.emulate_bf16_storage():
        other.forward(fr, t)
    assert np.array_equal(K.run(K.start_params('plain'), 'plain', fr, False, np.float32, bf16=True).logits, other.logits)
    for blur_pool in (False, True):
        blk, x = K.build_bottleneck(blur_pool)
        p = M.cast_params(blk.state_dict_chainer(), np.float64)
        mine = K.RefUnit(p, K.BOTTLENECK_STAGES, K.BOTTLENECK_SHORTCUT, False, blur_pool).fwd(x.astype(np.float64))
        unit = (BlurResUnit if blur_pool else M._ResUnit)(p, K.BOTTLENECK_STAGES, K.BOTTLENECK_SHORTCUT, False)
        assert np.array_equal(mine, unit.fwd(x.astype(np.float64)))
        probe = K.RefUnit(p, K.BOTTLENECK_STAGES, K.BOTTLENECK_SHORTCUT, False, blur_pool)
        probe.fwd(x.astype(np.float64))
        assert min(float(np.abs(a).min()) for a in probe.pre) >= 1e-6           # the same condition on the bottleneck's inputs
