"""CPU: ``blur_pool`` through the constructors and the three command lines, the refusals that need no device (the launch checks of
csrc/blur.hip, VisualBackprop, a strided last stage, ``--resume`` with a changed value) and the ceil(H / 2) size rule."""
import ctypes

import pytest

import evaluate as E
import loans_amd
import train_imagenet as T
import train_sheep_localizer as S
from loans_amd import _lib, links as L, ops
from loans_amd.functions import blocks
from loans_amd.runtime import checkpoint


@pytest.mark.parametrize('cls', [loans_amd.SheepLocalizer, loans_amd.Resnet50SheepLocalizer])
def test_the_option_reaches_every_strided_unit_and_adds_no_parameter(cls):
    plain, blur = cls((75, 75)), cls((75, 75), blur_pool=True)
    assert blur.blur_pool and blur.feature_extractor.blur_pool and not plain.blur_pool
    assert [(k, p.logical_shape) for k, p in blur.namedparams()] == [(k, p.logical_shape) for k, p in plain.namedparams()]
    units = lambda m: [u for u in m.links() if getattr(u, 'blur_pool', False) and u is not m and u is not m.feature_extractor]   # noqa: E731
    assert len(units(blur)) == 5 and not units(plain)           # res3 .. res7: the first unit of each strided stage


def test_unit_refusals():
    conv = lambda s: L.Convolution2D(64, 64, 3, s, 1, nobias=True)      # noqa: E731
    bn = L.BatchNormalization(64)
    with pytest.raises(ValueError, match='last stage'):
        blocks.ResidualUnitFunction([(conv(1), bn), (conv(2), bn)], blur=True)
    f = blocks.ResidualUnitFunction([(conv(2), bn), (conv(1), bn)], (conv(2), bn), blur=True)
    assert f.blurred == [True, False] and f.blur_shortcut
    assert not any(blocks.ResidualUnitFunction([(conv(2), bn), (conv(1), bn)], (conv(2), bn)).blurred)
    old, ops.VBP_TAPS = ops.VBP_TAPS, []
    try:
        with pytest.raises(RuntimeError, match='VisualBackprop'):
            f.forward([None] * 10)
    finally:
        ops.VBP_TAPS = old


def test_size_rule():
    conv = L.Convolution2D(64, 64, 3, 2, 1, nobias=True)
    for size in (2, 3, 7, 56, 57):
        assert ops.blur_outsize(size) == -(-size // 2) == ops.conv_outsize(size, 3, 2, 1) == ops.conv_outsize(size, 1, 2, 0)
        assert conv.geometry(2, size, size, 1).out_shape == (2, size, size, 64)
        assert conv.geometry(2, size, size).out_shape == (2, ops.blur_outsize(size), ops.blur_outsize(size), 64)


def test_command_lines_forward_the_flag(monkeypatch):
    assert T.parse_args([]).blur_pool is False and T.parse_args(['--blur-pool']).blur_pool is True
    with pytest.raises(SystemExit):
        T.parse_args(['--teacher-blur-pool'])
    assert T.build_model(T.parse_args(['--use-resnet-18', '--blur-pool', '--se-ratio', '16'])).predictor.blur_pool
    assert not T.build_model(T.parse_args(['--use-resnet-18'])).predictor.blur_pool
    assert S.build_models(S.parse_args(['--use-resnet-18', '--blur-pool']))[0].blur_pool
    assert not S.build_models(S.parse_args(['--use-resnet-18']))[0].blur_pool
    seen = []

    class Stop(Exception):
        pass

    def evaluator(args):
        seen.append(args.blur_pool)
        raise Stop

    monkeypatch.setattr(E, 'Evaluator', evaluator)
    monkeypatch.setattr(E.torch.cuda, 'set_device', lambda i: None)
    for argv in (['d', 'p', '--synthetic', '2'], ['d', 'p', '--synthetic', '2', '--blur-pool']):
        with pytest.raises(Stop):
            E.main(argv)
    assert seen == [False, True]


def test_resume_with_a_changed_value_is_refused():
    assert 'blur_pool' in T.RESUME_FIXED and 'blur_pool' in S.RESUME_FIXED
    saved = {k: v for k, v in checkpoint._plain({k: getattr(T.parse_args([]), k) for k in T.RESUME_FIXED}).items() if k != 'blur_pool'}
    fixed = [k for k in T.RESUME_FIXED if k != 'gpus']
    assert checkpoint.check_arguments(saved, T.parse_args([]), fixed, checkpoint.SILENT, T.RESUME_DEFAULTS_WITH_BLUR) == []
    with pytest.raises(ValueError, match='blur_pool: False in the checkpoint, True now'):
        checkpoint.check_arguments(saved, T.parse_args(['--blur-pool']), fixed, checkpoint.SILENT, T.RESUME_DEFAULTS_WITH_BLUR)


@pytest.mark.parametrize('bad', ['channels', 'height', 'dtypes'])
def test_launch_refusals_need_no_device(bad):
    """C = 96, H = 1 and a wrong dtype pair are LOANS_EINVAL before the first launch, never a fall-back"""
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    B, H, C_, b, x, want = 2, 4, 64, 4, p, -1
    if bad == 'channels': C_ = 96
    if bad == 'height': H = 1
    if bad == 'dtypes': b = 2
    assert lib.loans_blur_fwd(x, p, p, p, B, H, 4, C_, 4, b, 0) == lib.loans_blur_fwd(x, 0, 0, p, B, H, 4, C_, 4, b, 0) == want
    assert lib.loans_blur_bwd_reduce(x, p, p, p, p, p, p, B, H, 4, C_, 4, b, 0) == want
    assert lib.loans_blur_bwd_apply(x, p, p, p, p, p, B, H, 4, C_, 4, b, 0) == want
    assert lib.loans_blur_bwd_plain(x, 0, p, B, H, 4, C_, 4, b, 0) == want
