"""CPU: ``--se-ratio`` on the command line and on ``--resume``, the launch refusals of csrc/se.hip that need no device, and the
new parameters in the optimisers' segment table."""
import ctypes

import pytest
import torch

import loans_amd
import train_imagenet as T
from loans_amd import _lib
from loans_amd.runtime import checkpoint


def test_se_ratio_parsing_and_resume():
    assert T.parse_args([]).se_ratio == 0 and T.parse_args(['--se-ratio', '16']).se_ratio == 16
    for bad in (['--se-ratio', '-1'], ['--se-ratio', '16', '--drop-path', '0.1'], ['--teacher-se-ratio', '16']):
        with pytest.raises(SystemExit):
            T.parse_args(bad)
    assert 'se_ratio' in T.RESUME_FIXED and T.RESUME_DEFAULTS_WITH_SE == dict(T.RESUME_DEFAULTS_WITH_ACCUM, se_ratio=0)
    # a checkpoint from before the option ran the model without: it resumes without, and with --se-ratio it is refused
    saved = {k: v for k, v in checkpoint._plain({k: getattr(T.parse_args([]), k) for k in T.RESUME_FIXED}).items() if k != 'se_ratio'}
    fixed = [k for k in T.RESUME_FIXED if k != 'gpus']
    assert checkpoint.check_arguments(saved, T.parse_args([]), fixed, checkpoint.SILENT, T.RESUME_DEFAULTS_WITH_SE) == []
    with pytest.raises(ValueError, match='se_ratio: 0 in the checkpoint, 16 now'):
        checkpoint.check_arguments(saved, T.parse_args(['--se-ratio', '16']), fixed, checkpoint.SILENT, T.RESUME_DEFAULTS_WITH_SE)
    with pytest.raises(ValueError, match='hidden width'):
        loans_amd.SheepLocalizer((75, 75), train_imagenet=True, se_ratio=32)        # 64 / 32 = 2 hidden units


@pytest.mark.parametrize('bad', ['null', 'misaligned', 'batch', 'channels', 'hidden', 'range'])
def test_launch_refusals_need_no_device(bad):
    """every refusal comes before the first launch: LOANS_EINVAL / LOANS_ERANGE on a machine without a GPU"""
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    B, P, C_, hid, x, want = 2, 9, 64, 4, p, -1
    if bad == 'null': x = 0
    if bad == 'misaligned': x = p + 4
    if bad == 'batch': B = 0
    if bad == 'channels': C_ = 96           # 24 units per row: no divisor, no multiple of 256
    if bad == 'hidden': hid = 6
    if bad == 'range': P, want = 1 << 28, -2
    if bad == 'hidden':
        assert lib.loans_se_excite_fwd_f32(*([p] * 10), B, P, C_, hid, 0) == want
        assert lib.loans_se_excite_bwd_f32(*([p] * 24), B, P, C_, hid, 0) == want
        return
    assert lib.loans_se_squeeze_f32(x, p, p, B, P, C_, 0) == want
    assert lib.loans_bn_apply_gate_f32(x, *([p] * 8), B, P, C_, 1, 0) == want
    assert lib.loans_se_bwd_reduce_f32(x, *([p] * 7), B, P, C_, 0) == want
    assert lib.loans_bn_bwd_apply_gate_f32(x, *([p] * 13), B, P, C_, 0) == want
    if bad not in ('null', 'misaligned'):
        assert lib.loans_se_slabs(B, P, C_, 4) == want


def test_the_segment_table_takes_the_two_biases_as_one_dimensional():
    """what --no-decay-1d steps by: the excitation's biases are exempt segments of their own, its weights decay, and the table
    of the ResNet-50 model still fits the kernels"""
    from loans_amd import ops
    from loans_amd.runtime.optimizers import decay_segments
    for cls, units in ((loans_amd.SheepLocalizer, 8), (loans_amd.Resnet50SheepLocalizer, 16)):
        model = loans_amd.Classifier(cls((75, 75), train_imagenet=True, se_ratio=16))
        model.materialize()
        model.finalize(torch.device('cpu'))
        a = model.arena
        exempt = [len(p.logical_shape) <= 1 for p in a.params]
        keys = [k for k, _ in model.namedparams()]
        assert [k.endswith('/b') for k, e in zip(keys, exempt) if '/se/' in k] == [e for k, e in zip(keys, exempt) if '/se/' in k]
        assert sum('/se/' in k for k in keys) == 4 * units
        ends, flags = decay_segments([p.size for p in a.params], a.offsets, exempt, a.numel)
        starts = [0] + [int(e) for e in ends[:-1]]
        for k, i in ((k, i) for i, k in enumerate(keys) if k.endswith('/se/down/b')):      # W | b | W | b: a segment each
            assert int(a.offsets[i]) in starts and flags[starts.index(int(a.offsets[i]))] == 1, k
        assert len(ends) <= ops.SGD_MAX_SEGMENTS
