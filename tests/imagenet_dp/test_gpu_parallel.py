"""-m gpu: data-parallel ImageNet pre-training.  Two ranks on GPU 0 with gradients and metric sums exchanged through gloo (RCCL
wants one device per rank; everything else is what ``train_imagenet.py --gpus 2`` runs): one momentum-SGD step of the smoothed
classifier against the float64 oracle's mean over the shards, summed validation metrics over shards of different lengths,
``train_imagenet.run`` end to end, and the RCCL (nccl) path at world size 1."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
WORLD, B, H, W = 2, 2, 64, 64
LR, MOMENTUM, DECAY, SMOOTH, TOPK = 0.05, 0.9, 5e-4, 0.1, 3
LABELS = (np.array([3, 7], np.int32), np.array([0, 9], np.int32))
EVAL = {0: ((50, [1, 4]), (51, [6])), 1: ((52, [2, 8]),)}            # rank -> (frame seed, labels) of its evaluation batches


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _env(rank, world, port):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), LOANS_DIST_BACKEND='gloo')


def _tiles(calls, n):
    """the [lo, hi) ranges cover [0, n) exactly once"""
    at = 0
    for lo, hi in sorted(calls):
        if lo != at or hi <= lo:
            return False
        at = hi
    return at == n


# ---- one step and the summed metrics ------------------------------------------------------------------------------------------
def _worker_step(rank, world, port, outdir):
    _env(rank, world, port)
    import torch
    import loans_amd
    from loans_amd import parallel
    from loans_amd.datasets import synthetic
    from tests.gpu_util import dev
    from tests.imagenet import test_gpu_model as G
    from tests.imagenet_sgd.test_gpu_model import _classifier
    comm = parallel.init_from_env()
    assert comm.active and comm.size == world
    model, net = _classifier(20 + rank, label_smoothing=SMOOTH, topk=TOPK)        # different weights per rank
    model.to_gpu(0)
    comm.bcast_data(model)
    if rank == 0:
        np.savez(os.path.join(outdir, 'init.npz'), **net.state_dict_chainer())
    opt = parallel.create_multi_node_optimizer(
        loans_amd.MomentumSGD(lr=LR, momentum=MOMENTUM, weight_decay_rate=DECAY).setup(model), comm)
    calls, plain = [], comm.allreduce_range
    comm.allreduce_range = lambda arena, lo, hi, async_op=False: (calls.append((lo, hi)), plain(arena, lo, hi, async_op))[1]
    seen = {}

    def keep(o):
        torch.cuda.synchronize()
        seen.update({k[len('/predictor/'):]: p.grad_logical() * o.grad_scale for k, p in o.target.namedparams()})
    opt.add_hook(keep, name='keep')
    frames = synthetic.make_frames(40 + rank, B, H, W)
    opt.update(model, G._prepared(net, frames), dev(LABELS[rank]))
    torch.cuda.synchronize()
    comm.allreduce_range = plain
    assert opt.grad_scale == 1.0 / world and opt.t == 1
    n = model.arena.active_numel
    assert n == model.arena.numel and _tiles(calls, n), (calls, n)            # every float once, the head included
    head = min(o for p, o in zip(model.arena.params, model.arena.offsets) if p is net.fc.W or p is net.fc.b)
    assert any(lo <= head < hi for lo, hi in calls)
    np.savez(os.path.join(outdir, 'grads_%d.npz' % rank), **seen)
    np.savez(os.path.join(outdir, 'after_%d.npz' % rank), **net.state_dict_chainer())

    # validation sums over shards of different lengths: rank 0 adds batches of 2 and 1 rows, rank 1 one batch of 2
    metrics = loans_amd.ClassificationMetrics(topk=TOPK)
    logits, labels = [], []
    for seed, t in EVAL[rank]:
        t = np.array(t, np.int32)
        model.evaluate(G._prepared(net, synthetic.make_frames(seed, len(t), H, W)), dev(t), metrics)
        logits.append(model.y.data.cpu().numpy())
        labels.append(t)
    local = metrics.result()
    assert local['rows'] == sum(len(t) for _, t in EVAL[rank])
    total = metrics.result(comm)
    assert metrics.result() == local                                           # the exchange works on a copy of the sums
    np.savez(os.path.join(outdir, 'eval_%d.npz' % rank), z=np.concatenate(logits), t=np.concatenate(labels))
    with open(os.path.join(outdir, 'result_%d.json' % rank), 'w') as f:
        json.dump(total, f)
    comm.barrier()
    parallel.shutdown()


def test_two_rank_sgd_step_and_summed_metrics_against_the_oracle(tmp_path):
    from loans_amd.datasets import synthetic
    from oracle import model as M
    from tests.gpu_util import rel_err
    from tests.imagenet_sgd import reference as S
    out = str(tmp_path)
    mp.spawn(_worker_step, args=(WORLD, _free_port(), out), nprocs=WORLD, join=True)
    load = lambda n: dict(np.load(os.path.join(out, n)))       # noqa: E731

    after = [load('after_%d.npz' % r) for r in range(WORLD)]
    for k in after[0]:                                          # replicas stay in sync (BN running statistics are local)
        if 'avg_' not in k and not k.endswith('/N'):
            np.testing.assert_array_equal(after[0][k], after[1][k], err_msg=k)
    init = load('init.npz')
    assert np.abs(after[0]['res5/1/conv2/W'] - init['res5/1/conv2/W']).max() > 0

    mean = {}
    for dtype in (np.float32, np.float64):
        total = None
        for r in range(WORLD):
            params = M.cast_params({k: v.copy() for k, v in init.items()}, dtype)
            oracle = S.SmoothedClassifier(params, SMOOTH, TOPK)
            oracle.forward(synthetic.make_frames(40 + r, B, H, W).astype(dtype), LABELS[r])
            grads = oracle.backward({})
            total = grads if total is None else {k: total[k] + v for k, v in grads.items()}
        mean[dtype] = {k: v / WORLD for k, v in total.items()}
    worst = 0.0
    for r in range(WORLD):
        got = load('grads_%d.npz' % r)
        assert set(got) == {k for k in init if M.is_trainable(k)}
        for key, ref in mean[np.float64].items():
            if key == 'conv1/b':            # analytically zero gradient (BN follows): rounding noise on both sides
                continue
            e = rel_err(got[key], ref)
            worst = max(worst, e)
            assert e <= max(5 * rel_err(mean[np.float32][key], ref), 5e-4), (r, key, e, rel_err(mean[np.float32][key], ref))
    print('worst relative error of the averaged gradients %.3g' % worst)

    results = [json.load(open(os.path.join(out, 'result_%d.json' % r))) for r in range(WORLD)]
    assert results[0] == results[1]
    ev = [load('eval_%d.npz' % r) for r in range(WORLD)]
    z, t = np.concatenate([e['z'] for e in ev]), np.concatenate([e['t'] for e in ev])
    assert z.shape == (5, 10)
    _, _, _, _, row_loss, hit, hitk = S.softmax_xent_ls_ref(z, t, 0.0, TOPK)
    got = results[0]
    assert (got['rows'], got['valid']) == (5, 5)
    assert got['accuracy'] == hit.sum() / 5 and got['accuracy_top%d' % TOPK] == hitk.sum() / 5
    bound = S.ls_bounds(z, t, 0.0)[0].sum() * (1 + 1e-6)
    assert abs(got['loss'] * 5 - row_loss.sum()) <= bound, (got['loss'] * 5, row_loss.sum(), bound)


# ---- the trainer ------------------------------------------------------------------------------------------------------------------
RUN = ['--use-resnet-18', '-b', '2', '--image-size', '64', '64', '--dataset-size', '8', '--validation-size', '5', '--iterations', '4',
       '--optimizer', 'sgd', '--augment', 'rrc', '--augment-seed', '3', '--warmup-epochs', '1', '--seed', '0', '--flat-log-dir']


def _worker_run(rank, world, port, outdir):
    _env(rank, world, port)
    import train_imagenet
    from loans_amd import parallel
    args = train_imagenet.parse_args(RUN + ['-l', os.path.join(outdir, 'log_%d' % rank)])
    entries, model = train_imagenet.run(args, log=lambda *a: None)
    np.savez(os.path.join(outdir, 'params_%d.npz' % rank), **model.predictor.state_dict_chainer())
    with open(os.path.join(outdir, 'entries_%d.json' % rank), 'w') as f:
        json.dump(entries, f, default=str)
    parallel.shutdown()


def _decided(z, t, k):
    """rows whose hit at rank k is settled by a logit gap above 1e-4 of the row's largest magnitude: the label's logit against
    the k-th largest of the others"""
    out = []
    for row, label in zip(np.asarray(z, np.float64), t):
        others = np.sort(np.delete(row, label))[::-1]
        out.append(abs(row[label] - others[k - 1]) > 1e-4 * np.abs(row).max())
    return np.array(out)


def test_trainer_on_two_ranks_end_to_end(tmp_path):
    import torch
    import loans_amd
    import train_imagenet as T
    out = str(tmp_path)
    mp.spawn(_worker_run, args=(WORLD, _free_port(), out), nprocs=WORLD, join=True)
    # rank 0 alone wrote the log and the snapshot
    assert sorted(os.listdir(os.path.join(out, 'log_0'))) == ['SheepLocalizer_4.npz', 'log']
    assert not os.path.exists(os.path.join(out, 'log_1'))
    a, b = (dict(np.load(os.path.join(out, 'params_%d.npz' % r))) for r in range(WORLD))
    for k in a:
        if 'avg_' not in k and not k.endswith('/N'):
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    with open(os.path.join(out, 'log_0', 'log')) as f:
        log = json.load(f)
    # 8 examples over 2 ranks: shares of 4, batches of 2, two iterations an epoch; entries at the end of each epoch
    assert [(e['iteration'], e['epoch']) for e in log] == [(2, 1), (4, 2)]
    for e, detail in zip(log, (0.5, 1.5)):                      # epoch_detail in front of the logged step
        want = T.scheduled_lr(0.001, int(detail), (), 0.1) * T.warmup_factor(detail, 1.0, 0.1)
        assert e['lr'] == pytest.approx(want, rel=1e-12), e
    assert log[0]['lr'] == pytest.approx(0.00055, rel=1e-12) and log[1]['lr'] == 0.001
    assert log[0]['gpus'] == 2 and log[0]['warmup_epochs'] == 1.0 and log[0]['validation_sums'] is False
    other = json.load(open(os.path.join(out, 'entries_1.json')))
    for mine, theirs in zip(log, other):                        # the same numbers on both ranks: means and sums over ranks
        for k in ('loss', 'accuracy', 'accuracy_top5', 'validation/loss', 'validation/accuracy', 'validation/accuracy_top5'):
            assert mine[k] == theirs[k], k
    last = log[-1]
    assert last['validation/rows'] == last['validation/valid'] == 5          # every example once: 5 = 3 + 2, batches of 2

    # the snapshot in a fresh single-process model over all 5 validation examples in one batch
    args = T.parse_args(RUN)
    device = torch.device('cuda', 0)
    _, validation = T.build_crop_datasets(args, device)
    model = T.build_model(args)
    model.to_gpu(0)
    loans_amd.load_npz(os.path.join(out, 'log_0', 'SheepLocalizer_4.npz'), model.predictor)
    x, t = validation.device_batch(range(5), device)
    metrics = loans_amd.ClassificationMetrics(topk=5)
    model.evaluate(x, t, metrics)
    whole = metrics.result()
    assert (whole['rows'], whole['valid']) == (5, 5)
    assert abs(whole['loss'] - last['validation/loss']) <= 1e-4 * abs(whole['loss']), (whole['loss'], last['validation/loss'])
    z, labels = model.y.data.cpu().numpy(), t.cpu().numpy()
    for k, key in ((1, 'accuracy'), (5, 'accuracy_top5')):
        decided = _decided(z, labels, k)
        assert decided.sum() >= 4, (k, decided)
        # the rows a gap decides count the same in both runs; an undecided row may fall either way
        assert abs(round(last['validation/' + key] * 5) - round(whole[key] * 5)) <= 5 - decided.sum(), (k, last, whole)


def test_validation_sums_in_one_process_logs_the_same_keys(tmp_path):
    import train_imagenet as T
    logs = {}
    for flag in ((), ('--validation-sums',)):
        path = os.path.join(str(tmp_path), 'sums' if flag else 'means')
        entries, _ = T.run(T.parse_args(RUN + ['-l', path] + list(flag)), log=lambda *a: None)
        with open(os.path.join(path, 'log')) as f:
            logs[bool(flag)] = json.load(f)
        assert entries[0]['validation_sums'] is bool(flag) and entries[0]['gpus'] == 1
    assert [set(e) for e in logs[True]] == [set(e) for e in logs[False]]
    assert [(e['iteration'], e['lr']) for e in logs[True]] == [(e['iteration'], e['lr']) for e in logs[False]]
    assert 'validation/rows' not in logs[True][-1] and 'validation/loss' in logs[True][-1]
    # 5 examples in batches of 2, 2 and 1: the sums weigh rows -- the accuracy is a count of hits over 5
    for e in logs[True]:
        assert np.isfinite(e['validation/loss']) and e['validation/loss'] > 0
        assert abs(round(e['validation/accuracy'] * 5) - e['validation/accuracy'] * 5) < 1e-9


# ---- RCCL at world size 1 -----------------------------------------------------------------------------------------------------------
def _selftest(outdir):
    """runs in a process of its own with LOANS_DIST_SELFTEST=1: backend nccl, every collective issued at world size 1"""
    import torch
    import loans_amd
    from loans_amd import parallel
    from loans_amd.datasets import synthetic
    from tests.gpu_util import dev
    from tests.imagenet import test_gpu_model as G
    from tests.imagenet_sgd.test_gpu_model import _classifier
    comm = parallel.init_from_env()
    assert comm.active and comm.size == 1 and comm.backend == 'nccl', (comm.active, comm.size, comm.backend)
    sums = torch.tensor([1.25, 3.0, 2.0, 5.0, 2.0 ** 53], dtype=torch.float64, device='cuda')
    want = sums.clone()
    assert comm.allreduce_sum(sums) is sums
    torch.cuda.synchronize()
    assert torch.equal(sums, want)
    metrics = loans_amd.ClassificationMetrics(topk=2)
    z = np.random.RandomState(0).standard_normal((5, 10)).astype(np.float32)
    metrics.add(dev(z), np.arange(5, dtype=np.int32))
    assert metrics.result(comm) == metrics.result()

    frames = synthetic.make_frames(1, B, H, W)
    t = np.array([3, 7], np.int32)
    states, pre, kept = {}, {}, {}
    for mode in ('plain', 'parallel'):
        model, net = _classifier(0, label_smoothing=SMOOTH, topk=TOPK)
        model.to_gpu(0)
        opt = loans_amd.MomentumSGD(lr=LR, momentum=MOMENTUM, weight_decay_rate=DECAY).setup(model)
        if mode == 'parallel':
            comm.bcast_data(model)
            parallel.create_multi_node_optimizer(opt, comm)
            plain = comm.allreduce_range

            def recording(arena, lo, hi, async_op=False):
                pre[(lo, hi)] = arena.grad[lo:hi].clone()        # on the stream the exchange is issued from: what goes in
                return plain(arena, lo, hi, async_op)
            comm.allreduce_range = recording
            opt.add_hook(lambda o: kept.update(grad=o.target.arena.grad.clone(), data=o.target.arena.data.clone()), name='keep')
        opt.update(model, G._prepared(net, frames), dev(t))
        torch.cuda.synchronize()
        if mode == 'parallel':
            comm.allreduce_range = plain
            assert _tiles(list(pre), model.arena.active_numel), list(pre)
            # a sum over one rank gives back what went in, bit for bit
            summed_is_identity = all(torch.equal(kept['grad'][lo:hi], g) for (lo, hi), g in pre.items())
            stepped = model.arena.data.clone()
        assert opt.grad_scale == 1.0
        states[mode] = net.state_dict_chainer()
    different = [k for k in states['plain'] if not np.array_equal(states['plain'][k], states['parallel'][k])]

    # the plain optimiser on the gradients the data-parallel step consumed, from the parameters it started from
    model, net = _classifier(0, label_smoothing=SMOOTH, topk=TOPK)
    model.to_gpu(0)
    same_start = torch.equal(model.arena.data, kept['data'])
    model.arena.grad.copy_(kept['grad'])
    opt = loans_amd.MomentumSGD(lr=LR, momentum=MOMENTUM, weight_decay_rate=DECAY).setup(model)
    opt.update()
    torch.cuda.synchronize()
    with open(os.path.join(outdir, 'selftest.json'), 'w') as f:
        json.dump({'backend': comm.backend, 'different': different, 'keys': len(states['plain']), 'same_start': same_start,
                   'summed_is_identity': summed_is_identity, 'same_step': torch.equal(model.arena.data, stepped),
                   'moved': not torch.equal(stepped, kept['data'])}, f)
    parallel.shutdown()


def test_rccl_at_world_size_one_equals_the_plain_step(tmp_path):
    e = dict(os.environ, LOANS_DIST_SELFTEST='1', RANK='0', WORLD_SIZE='1', LOCAL_RANK='0', MASTER_ADDR='127.0.0.1',
             MASTER_PORT=str(_free_port()))
    e.pop('LOANS_DIST_BACKEND', None)
    code = 'from tests.imagenet_dp.test_gpu_parallel import _selftest; _selftest(%r)' % str(tmp_path)
    r = subprocess.run([sys.executable, '-c', code], cwd=ROOT, env=e, timeout=600, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.load(open(os.path.join(str(tmp_path), 'selftest.json')))
    assert out['backend'] == 'nccl' and out['keys'] > 60
    # Bit for bit.  The gradient of the stem's weights is summed with float atomics, one per element and block (csrc/stem.hip):
    # its last bits differ between any two backward passes, with or without a communicator.  So the two independent steps are
    # compared on every other array, and the data-parallel arithmetic on all of them, conv1/W included, on ONE backward pass:
    # the all-reduce returns the bits it was given, and the plain optimiser on those gradients lands on the same parameters.
    assert set(out['different']) <= {'conv1/W'}, out['different']
    assert out['same_start'] and out['moved']
    assert out['summed_is_identity'] and out['same_step']
