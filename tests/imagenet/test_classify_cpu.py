"""CPU side of the ImageNet pre-training arm: link trees, snapshot transfer into a LoANs localizer, the trainer's command line
and dataset wiring, and the error bound of the loss kernel's arithmetic (tests/imagenet/reference.py), established on an fp32
NumPy restatement over the case grid the GPU test then runs the kernel on."""
import os

import numpy as np
import pytest

import loans_amd
from tests.imagenet import reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _logical(link):
    return {k: p.logical_shape for k, p in link.namedparams()}


def test_link_trees_of_the_classification_models():
    np.random.seed(0)
    loc = loans_amd.SheepLocalizer((75, 75), train_imagenet=True)
    keys = _logical(loc)
    assert not any(k.startswith(('/res6', '/res7', '/param_predictor')) for k in keys)
    assert not hasattr(loc, 'res6') and not hasattr(loc, 'param_predictor')
    assert loc.feature_extractor.fc.W is None and '/feature_extractor/fc/W' not in keys       # unsized until first use
    loc.feature_extractor.materialize_head()
    keys = _logical(loc)
    assert keys['/feature_extractor/fc/W'] == (1000, 512) and keys['/feature_extractor/fc/b'] == (1000,)
    assert not loc.feature_extractor.fc.b.host.any()
    w = loc.feature_extractor.fc.W.host
    assert abs(w.std() - 1 / np.sqrt(512)) < 0.02 / np.sqrt(512) * 5                          # LeCunNormal
    st = loc.state_dict_chainer()
    assert st['feature_extractor/fc/W'].shape == (1000, 512) and st['feature_extractor/conv1/W'].shape == (64, 3, 7, 7)

    r50 = loans_amd.Resnet50SheepLocalizer((75, 75), train_imagenet=True)
    keys = _logical(r50)
    assert keys['/feature_extractor/fc6/W'] == (1000, 2048) and keys['/feature_extractor/fc6/b'] == (1000,)
    assert not any(k.startswith(('/res6', '/res7', '/param_predictor')) for k in keys)
    assert r50.feature_extractor.keys_to_remove == ['prob'] and 'fc6' in r50.feature_extractor.functions
    assert r50.cold_links == ()

    from loans_amd.sheep.resnet import ResNet
    net = ResNet(18, class_labels=10)
    assert net.fc.W is None and net.fc.out_size == 10
    net.materialize_head()
    assert _logical(net)['/fc/W'] == (10, 512) and _logical(net)['/fc/b'] == (10,)
    assert [k for k, _ in ResNet(18).namedparams()] == [k for k in _logical(net) if not k.startswith('/fc/')]


def test_plain_localizers_keep_their_tree_and_count():
    np.random.seed(0)
    loc = loans_amd.SheepLocalizer((75, 75))
    logical = _logical(loc)
    assert sum(int(np.prod(s)) for k, s in logical.items() if not k.startswith(('/res6', '/res7'))) == 12592902
    assert not any('/fc/' in k for k in logical) and loc.cold_links == ('res6', 'res7')
    assert not hasattr(loc.feature_extractor, 'fc')
    r50 = loans_amd.Resnet50SheepLocalizer((75, 75))
    assert r50.cold_links == ('res6', 'res7', 'feature_extractor/fc6')
    assert r50.feature_extractor.keys_to_remove == ['fc6', 'prob']


def test_classifier_snapshot_transfers_into_a_loans_localizer(tmp_path):
    np.random.seed(1)
    pre = loans_amd.SheepLocalizer((75, 75), train_imagenet=True)
    pre.feature_extractor.materialize_head()
    rng = np.random.RandomState(2)
    for k, p in pre.namedparams():                   # away from the initial values, BN included
        p.set_logical((p.get_logical() + 0.1 * rng.standard_normal(p.logical_shape)).astype(np.float32))
    pre.feature_extractor.bn1.avg_mean[...] = rng.standard_normal(64)
    path = str(tmp_path / 'SheepLocalizer_20.npz')
    loans_amd.save_npz(path, pre)
    with np.load(path) as h:
        assert h['feature_extractor/fc/W'].shape == (1000, 512) and h['feature_extractor/fc/b'].shape == (1000,)
    np.random.seed(3)
    loc = loans_amd.SheepLocalizer((75, 75))
    before = loc.state_dict_chainer()
    import train_sheep_localizer
    train_sheep_localizer.load_pretrained_model(path, loc)
    after, src = loc.state_dict_chainer(), pre.state_dict_chainer()
    for k, v in after.items():
        if k.startswith('feature_extractor/'):
            np.testing.assert_array_equal(v, src[k], err_msg=k)
        else:                                        # res6 / res7 / param_predictor: their initial values
            np.testing.assert_array_equal(v, before[k], err_msg=k)
    assert not any(k.startswith('feature_extractor/fc') for k in after)
    np.testing.assert_array_equal(after['param_predictor/b'], np.array([0.8, 0, 0, 0, 0.8, 0], np.float32))
    assert not after['param_predictor/W'].any()


def test_trainer_command_line_and_dataset_wiring(tmp_path):
    import train_imagenet as T
    a = T.parse_args([])
    assert (a.train_file, a.val_file) == ('synthetic', 'synthetic') and a.validation and not a.use_resnet_18
    assert a.dtype == 'f32' and a.weight_decay == 0.0 and tuple(a.image_size) == (224, 224)
    a = T.parse_args(['tr.tsv', 'va.tsv', '--use-resnet-18', '-b', '8', '--lr', '0.01', '--weight-decay', '1e-4', '--num-epoch', '3',
                      '--iterations', '7', '--image-size', '64', '48', '-l', 'logs', '--ln', 'run', '--snapshot-interval', '5',
                      '--dtype', 'bf16', '--seed', '4', '--no-shuffle', '--no-validation'])
    assert (a.train_file, a.val_file, a.batch_size, a.learning_rate, a.weight_decay) == ('tr.tsv', 'va.tsv', 8, 0.01, 1e-4)
    assert (a.num_epoch, a.iterations, tuple(a.image_size), a.log_dir, a.ln) == (3, 7, (64, 48), 'logs', 'run')
    assert (a.snapshot_interval, a.dtype, a.seed, a.no_shuffle, a.validation) == (5, 'bf16', 4, True, False)

    # the synthetic set: seeded, int32 labels, frames exactly k / 255, classes shared between the splits
    a = T.parse_args(['--use-resnet-18', '--image-size', '32', '32', '--dataset-size', '12', '--validation-size', '6',
                      '--synthetic-classes', '3'])
    train, val = T.build_datasets(a)
    x, t = train[4]
    assert x.shape == (3, 32, 32) and x.dtype == np.float32 and t.dtype == np.int32 and int(t) == 1
    np.testing.assert_array_equal(np.round(x * 255) / np.float32(255), x)
    assert len(train) == 12 and len(val) == 6
    np.testing.assert_array_equal(T.build_datasets(a)[0].x, train.x)
    same_class = np.abs(train.x[0] - val.x[0]).mean()
    other_class = np.abs(train.x[0] - val.x[1]).mean()
    assert same_class < other_class

    # files: tab-separated `path<TAB>class`, read through LabeledImageDataset(label_dtype=int32)
    from PIL import Image
    for i in range(2):
        Image.fromarray((np.random.RandomState(i).rand(20, 24, 3) * 255).astype(np.uint8)).save(str(tmp_path / ('im%d.png' % i)))
    (tmp_path / 'train.tsv').write_text('im0.png\t7\nim1.png\t999\n')
    a = T.parse_args([str(tmp_path / 'train.tsv'), '--no-validation', '--image-size', '16', '16'])
    train, val = T.build_datasets(a)
    assert val is None and len(train) == 2
    x, t = train[1]
    assert x.shape == (3, 16, 16) and x.dtype == np.float32 and t.dtype == np.int32 and t.reshape(-1).tolist() == [999]

    # the model the loop trains: Classifier over the train_imagenet localizer, head materialised before the arena exists
    np.random.seed(0)
    model = T.build_model(T.parse_args(['--use-resnet-18']))
    assert isinstance(model, loans_amd.Classifier) and model.predictor.train_imagenet
    assert '/predictor/feature_extractor/fc/W' in dict(model.namedparams())
    # ... by Classifier itself, whatever the depth of the lazily sized head in the predictor's tree
    fresh = loans_amd.Classifier(loans_amd.SheepLocalizer((75, 75), train_imagenet=True))
    assert '/predictor/feature_extractor/fc/W' not in dict(fresh.namedparams())
    fresh.materialize()
    assert dict(fresh.namedparams())['/predictor/feature_extractor/fc/W'].logical_shape == (1000, 512)
    assert 'oracle' not in open(os.path.join(ROOT, 'train_imagenet.py')).read()


@pytest.mark.parametrize("N", R.XENT_N)
def test_loss_restatement_is_inside_the_derived_bound(N):
    """the fp32 restatement of the loss kernel against the float64 reference over the case grid: every row loss, every gz
    element and the batch loss inside the first-order bound; accuracy exact; the known answers; and the bound itself no looser
    than the project's fp32 contract (1e-4 relative on the batch loss, 1e-5 absolute where lse and z_t cancel)"""
    worst = {'loss': 0.0, 'gz': 0.0, 'batch': 0.0}
    for name, z, t, expect in R.xent_cases(N):
        assert R.argmax_margin_ok(z), name
        loss, acc, gz, row_loss, am = R.softmax_xent_ref(z, t)
        lb, gb, bb = R.row_bounds(z, t)
        l32, a32, g32, r32 = R.softmax_xent_fp32(z, t)
        valid = (t >= 0) & (t < N)
        err = np.abs(r32.astype(np.float64) - row_loss)
        assert np.all(err <= lb), (name, float((err - lb).max()))
        gerr = np.abs(g32.astype(np.float64) - gz)
        assert np.all(gerr <= gb), (name, float((gerr - gb).max()))
        assert abs(l32 - loss) <= bb, (name, l32, loss, bb)
        assert a32 == np.float32(acc), name
        assert bb <= max(1e-4 * abs(loss), 1e-5), (name, bb, loss)
        if valid.any():
            worst['loss'] = max(worst['loss'], float((err[valid] / lb[valid]).max()))
            worst['gz'] = max(worst['gz'], float((gerr[valid] / gb[valid]).max()))
            worst['batch'] = max(worst['batch'], abs(l32 - loss) / bb)
        else:                                       # every row ignored: loss 0 and a zero gradient, both exact
            assert l32 == 0.0 and loss == 0.0 and not g32.any() and not gz.any(), name
        if name.startswith('equal') and valid.any():
            count = valid.sum()
            np.testing.assert_allclose(row_loss[valid], np.log(N), rtol=1e-12, atol=1e-15)
            onehot = np.zeros_like(gz)
            onehot[np.arange(len(t)), np.where(valid, t, 0)] = 1
            np.testing.assert_allclose(gz[valid], ((1.0 / N - onehot) / count)[valid], rtol=1e-12, atol=1e-18)
        if expect is not None:
            np.testing.assert_array_equal(am == t, expect, err_msg=name)
            assert acc == expect.mean()
    print('N=%d worst error / bound: row loss %.3f, gz %.3f, batch loss %.3f' % (N, worst['loss'], worst['gz'], worst['batch']))
    assert max(worst.values()) <= 1.0
