"""No GPU, no launch: ``--head-dtype``, the ``compute`` argument of the Linear link, and the slab planner of the bf16 head."""
import pytest


def test_head_dtype_parses_defaults_to_fp32_and_is_free_on_resume(capsys):
    import train_imagenet as T
    bare, given = T.parse_args([]), T.parse_args(['--head-dtype', 'bf16', '--dtype', 'bf16', '--num-classes', '21841'])
    assert 'head_dtype' not in vars(bare) and bare.head_dtype == 'fp32'         # a class-level default, not a parsed value
    assert given.head_dtype == 'bf16' and T.parse_args(['--head-dtype', 'fp32']).head_dtype == 'fp32'
    assert set(vars(T.parse_args(['--head-dtype', 'bf16']))) == set(vars(bare)) | {'head_dtype'}
    assert 'head_dtype' not in T.RESUME_FIXED
    with pytest.raises(SystemExit):
        T.parse_args(['--head-dtype', 'fp16'])
    assert "--head-dtype: invalid choice: 'fp16'" in capsys.readouterr().err


def test_compute_is_refused_where_it_has_no_kernel():
    from loans_amd import links as L
    assert L.Linear(512, 24).compute == 'f32' and L.Linear(512, 9, compute='bf16').compute == 'bf16'
    for kwargs in (dict(out_size=8, compute='bf16'), dict(out_size=24, compute='fp16')):
        with pytest.raises(ValueError):
            L.Linear(512, **kwargs)
    assert L.head_compute('fp32', False) == 'f32' and L.head_compute('bf16') == 'bf16'
    for bad in (('bf16', False), ('f32', True)):
        with pytest.raises(ValueError):
            L.head_compute(*bad)


def test_slab_planner_follows_the_rule_in_the_header():
    from loans_amd import _lib
    plan = _lib.load().loans_linear_wide16_workspace
    # ResNet-50 at batch 256, 21841 classes: 683 chunks, 2 x 16 tiles -> want min(8, 171) = 8, 86 chunks each, 8 slices
    assert plan(256, 2048, 21841) == 8 * 256 * 2048 * 4
    # 10 chunks, 1 x 4 tiles -> want min(64, 3) = 3, 4 chunks each, 3 slices (4, 4, 2)
    assert plan(6, 512, 300) == 3 * 6 * 512 * 4
    assert plan(6, 512, 128) == 0                                               # 4 chunks: one slice, gx written directly
    assert plan(4, 6, 16) == -1 and plan(4, 8, 8) == -1 and plan(4, 8, 1 << 20) == -2
