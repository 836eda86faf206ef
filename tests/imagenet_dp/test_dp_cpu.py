"""Data-parallel ImageNet pre-training, the parts that need no GPU: the shard views, the warm-up and the new options, the two new
collectives over gloo, and the argument checks of the evaluation entry."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from loans_amd.common.datasets.shard import ShardedDataset
from loans_amd.runtime import training

SIZES, WORLDS, BATCHES = range(1, 18), range(1, 5), (1, 2, 3, 5)


# ---- shards ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", WORLDS)
def test_shards_cover_the_set_and_keep_the_ranks_in_lock_step(world):
    for n in SIZES:
        base = list(range(100, 100 + n))
        padded = [ShardedDataset(base, r, world, pad=True) for r in range(world)]
        plain = [ShardedDataset(base, r, world, pad=False) for r in range(world)]
        per = -(-n // world)
        assert [len(s) for s in padded] == [per] * world
        seen = [s[i] for s in padded for i in range(len(s))]
        assert set(seen) == set(base)
        assert len(seen) - n == per * world - n < world                     # fewer than `world` entries are repeated
        for r, s in enumerate(padded):
            assert [s.base_index(j) for j in range(per)] == [(r + j * world) % n for j in range(per)]
            assert [s[j] for j in range(per)] == [base[(r + j * world) % n] for j in range(per)]
        once = [s[i] for s in plain for i in range(len(s))]
        assert sorted(once) == base                                         # disjoint, every index exactly once
        lengths = [len(s) for s in plain]
        assert max(lengths) - min(lengths) <= 1 and sum(lengths) == n
        assert (min(lengths) == 0) == (n < world)
        if world == 1:
            assert [padded[0][i] for i in range(n)] == base == [plain[0][i] for i in range(n)]
        for batch in BATCHES:
            sequences = []
            for s in padded:
                it = training.SerialIterator(s, batch, repeat=True, shuffle=True)
                seq = []
                while it.epoch < 3:
                    next(it)
                    seq.append((it.epoch, it.is_new_epoch))
                sequences.append(seq)
            assert all(seq == sequences[0] for seq in sequences), (n, world, batch)
            assert sequences[0][-1] == (3, True)


def test_shard_refuses_an_empty_set_and_a_rank_outside_the_world():
    with pytest.raises(ValueError):
        ShardedDataset([], 0, 2, pad=True)
    with pytest.raises(ValueError):
        ShardedDataset([1, 2], 2, 2, pad=False)


class _Stub:
    """a dataset with the device-feed methods that records the base indices it is asked for"""

    def __init__(self, n):
        self.n, self.asked, self.seeds = n, [], []

    def __len__(self):
        return self.n

    def get_example(self, i):
        self.asked.append(('get_example', i))
        return i

    __getitem__ = get_example

    def decode_batch(self, indices, map_fn=map, farm=None):
        self.asked.append(('decode_batch', list(indices), farm))
        return list(indices)

    def finish_batch(self, decoded, device, map_fn=map):
        self.asked.append(('finish_batch', decoded, device))
        return decoded

    def reseed(self, seed):
        self.seeds.append(seed)


def test_shard_forwards_the_device_feed_with_base_indices_and_nothing_the_base_lacks():
    base = _Stub(7)
    shard = ShardedDataset(base, 1, 3, pad=True)             # base indices 1, 4, 0 (wrapped)
    assert len(shard) == 3
    assert shard.decode_batch([0, 2, 1], map, 'farm') == [1, 0, 4]
    assert base.asked[-1] == ('decode_batch', [1, 0, 4], 'farm')
    assert shard.decode_batch([1]) == [4] and base.asked[-1] == ('decode_batch', [4], None)
    assert shard.finish_batch([1, 0, 4], 'dev') == [1, 0, 4] and base.asked[-1] == ('finish_batch', [1, 0, 4], 'dev')
    assert shard[2] == 0 and shard.get_example(1) == 4
    shard.reseed(11)
    assert base.seeds == [11]
    assert hasattr(shard, 'decode_batch') and hasattr(shard, 'finish_batch') and hasattr(shard, 'reseed')
    assert not hasattr(shard, 'get_examples') and not hasattr(shard, 'device_batch')        # the stub has neither
    plain = ShardedDataset(list(range(5)), 0, 2, pad=False)
    for name in ('decode_batch', 'finish_batch', 'get_examples', 'device_batch', 'reseed'):
        assert not hasattr(plain, name), name                # MultithreadIterator takes the host path, as for the base

    class WithExamples(_Stub):
        def get_examples(self, indices, map_fn=map):
            return [10 * i for i in indices]

        def device_batch(self, indices, device, map_fn=map):
            return [(i, device) for i in indices]

    s2 = ShardedDataset(WithExamples(5), 1, 2, pad=False)    # base indices 1, 3
    assert s2.get_examples([1, 0]) == [30, 10] and s2.device_batch([0], 'd') == [(1, 'd')]


# ---- warm-up and options --------------------------------------------------------------------------------------------------------
def test_warmup_factor_and_its_product_with_the_schedule():
    import train_imagenet as T
    f = T.warmup_factor
    assert f(0.0, 5, 0.1) == 0.1
    assert f(2.5, 5, 0.1) == pytest.approx(0.55, rel=1e-12)
    assert f(5.0, 5, 0.1) == 1.0 and f(7.25, 5, 0.1) == 1.0
    assert f(0.0, 0, 0.1) == 1.0 and f(3.0, 0, 0.1) == 1.0
    assert f(1.0, 4, 0.0) == pytest.approx(0.25, rel=1e-12)
    values = [f(e, 2, 0.25) for e in np.linspace(0, 2, 9)]
    assert all(b > a for a, b in zip(values, values[1:]))                     # a ramp
    # on top of the steps: epoch 31.5 of a run that drops at 30 and 60 and warms up over 5 epochs, and epoch 1.25 of it
    lr = T.scheduled_lr(0.8, 31, (30, 60), 0.1) * f(31.5, 5, 0.1)
    assert lr == pytest.approx(0.08, rel=1e-12)
    lr = T.scheduled_lr(0.8, 1, (30, 60), 0.1) * f(1.25, 5, 0.1)
    assert lr == pytest.approx(0.8 * (0.1 + 0.9 * 0.25), rel=1e-12)


def test_the_new_options_parse_and_leave_the_default_namespace_alone():
    import train_imagenet as T
    new = ('gpus', 'warmup_epochs', 'warmup_start_factor', 'validation_sums')
    bare = T.parse_args([])
    assert not set(new) & set(vars(bare))                                     # class-level defaults, not parsed values
    assert (bare.gpus, bare.warmup_epochs, bare.warmup_start_factor, bare.validation_sums) == (1, 0, 0.1, False)
    args = T.parse_args(['--gpus', '4', '--warmup-epochs', '2.5', '--warmup-start-factor', '0.2', '--validation-sums'])
    assert (args.gpus, args.warmup_epochs, args.warmup_start_factor, args.validation_sums) == (4, 2.5, 0.2, True)
    assert set(vars(args)) == set(vars(bare)) | set(new)
    assert set(T.Arguments._PARALLEL) == set(new)
    from loans_amd import launch
    assert launch.requested_gpus(['--use-resnet-18', '--gpus', '4']) == 4


# ---- collectives ----------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    import torch.distributed as dist
    import loans_amd
    from loans_amd import links as L
    from loans_amd import parallel
    comm = parallel.init_from_env(backend='gloo')
    assert comm.active and (comm.size, comm.rank) == (world, rank)
    sums = torch.tensor([0.1 + rank, 3.0, 2.0 * rank, 5.0, 2.0 ** 53 - 1 if rank == 0 else 1.0], dtype=torch.float64)
    back = comm.allreduce_sum(sums)
    assert back is sums and sums.dtype == torch.float64
    assert sums.tolist() == [0.1 + (0.1 + 1), 6.0, 2.0, 10.0, 2.0 ** 53]                   # doubles all the way: 2^53 is exact

    class Net(loans_amd.Chain):
        def __init__(self):
            super().__init__()
            with self.init_scope():
                self.fc = L.Linear(3, 2)
                self.bn = L.BatchNormalization(2)

    np.random.seed(rank)
    net = Net()
    net.finalize(torch.device('cpu'))
    net.bn.avg_mean.fill_(float(rank + 1))
    net.bn.avg_var.fill_(float(10 * (rank + 1)))
    net.fc.b.set_logical(np.full(2, rank + 1, np.float32))
    comm.bcast_persistents(net)
    assert net.bn.avg_mean.tolist() == [1.0, 1.0] and net.bn.avg_var.tolist() == [10.0, 10.0]
    np.testing.assert_array_equal(net.fc.b.get_logical(), np.full(2, rank + 1, np.float32))      # persistents only
    net.bn.avg_mean.fill_(float(rank + 5))
    comm.bcast_data(net)                                                                        # parameters and persistents
    assert net.bn.avg_mean.tolist() == [5.0, 5.0]
    np.testing.assert_array_equal(net.fc.b.get_logical(), np.full(2, 1, np.float32))
    comm.barrier()
    if rank == 0:
        out.put('ok')
    dist.destroy_process_group()


def test_allreduce_sum_and_bcast_persistents_over_two_gloo_ranks():
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=240)
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    assert q.get(timeout=5) == 'ok'


def test_inactive_communicator_leaves_the_tensor_alone():
    from loans_amd import parallel
    comm = parallel.Communicator()
    assert not comm.active
    t = torch.tensor([1.5, 2.5], dtype=torch.float64)
    assert comm.allreduce_sum(t) is t and t.tolist() == [1.5, 2.5]
    comm.bcast_persistents(None)                                              # returns before it looks at the link


# ---- the evaluation entry without a GPU -----------------------------------------------------------------------------------------
def test_eval_entry_checks_its_arguments_before_any_hip_call():
    import ctypes
    from loans_amd import _lib
    f = _lib.load().loans_softmax_xent_eval_f32
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    assert f(p, p, p, p, 4, 8, 0, 0) == -1                  # k = 0
    assert f(p, p, p, p, 4, 8193, 1, 0) == -2               # beyond one row of LDS
    assert f(p, p, p, p, 65537, 8, 1, 0) == -2
    assert f(p, p, p, p, 0, 8, 1, 0) == -1 and f(p, p, p, p, 4, 0, 1, 0) == -1
    for missing in range(4):
        args = [p, p, p, p]
        args[missing] = 0
        assert f(*args, 4, 8, 1, 0) == -1, missing
    assert bytes(buf) == bytes(64)
