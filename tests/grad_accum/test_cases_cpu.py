"""CPU: the NumPy restatement of gradient accumulation (cases.py) against the sequential fp32 sum and against five implementations
that are not the rule, on the operand table the GPU tests use; the size grid's regimes; and the host logic on fakes -- the
``StandardUpdater(accum_steps=K)`` bookkeeping, the mean of the observations, the command line and the resume tables."""
import numpy as np
import pytest

from loans_amd.runtime import checkpoint, training
from tests.grad_accum import cases as A

F32 = np.float32


# ---- the rule ------------------------------------------------------------------------------------------------------------------------
def test_the_three_modes_write_what_they_say_and_nothing_else():
    g1, g2, _ = A.tiled(64)
    acc0 = np.full(64, 7.0, F32)
    acc, g = A.apply(A.STORE, acc0, g1)
    assert A.same_bits(acc, g1) and np.array_equal(A.bits(g), A.bits(g1))
    acc2, g = A.apply(A.ADD, acc, g2)
    with np.errstate(all='ignore'):
        assert A.same_bits(acc2, (g1 + g2).astype(F32)) and np.array_equal(A.bits(g), A.bits(g2))
    acc3, g = A.apply(A.CLOSE, acc, g2)
    assert np.array_equal(A.bits(acc3), A.bits(acc)) and A.same_bits(g, acc2)
    with pytest.raises(ValueError):
        A.apply(3, acc, g1)
    assert A.modes_of(2) == [A.STORE, A.CLOSE] and A.modes_of(4) == [A.STORE, A.ADD, A.ADD, A.CLOSE]


@pytest.mark.parametrize('K', [2, 3, 5])
def test_the_chain_is_the_sequential_sum_bit_for_bit(K):
    rows = A.tiled(100)
    gs = [rows[k % 3] for k in range(K)]
    closed, acc = A.chain(gs, acc0=np.full(100, np.nan, F32))
    assert A.same_bits(closed, A.sequential_sum(gs))
    assert A.same_bits(acc, A.sequential_sum(gs[:-1]))                 # the accumulator holds the first K - 1, CLOSE left it alone
    # whatever the accumulator held before: STORE does not read it
    other, _ = A.chain(gs, acc0=np.full(100, A.DIRTY, F32))
    assert np.array_equal(A.bits(other), A.bits(closed))


def test_the_table_holds_what_the_issue_asks_for():
    t = A.TABLE.astype(np.float64)
    with np.errstate(all='ignore'):
        left = ((A.TABLE[0] + A.TABLE[1]).astype(F32) + A.TABLE[2]).astype(F32)
        right = (A.TABLE[0] + (A.TABLE[1] + A.TABLE[2]).astype(F32)).astype(F32)
    numbers = ~(np.isnan(left) | np.isnan(right))
    assert (A.bits(left)[numbers] != A.bits(right)[numbers]).any()                                  # (a + b) + c != a + (b + c)
    closed = A.sequential_sum(A.TABLE)
    zeros = closed == 0
    assert (np.signbit(closed[zeros])).any() and (~np.signbit(closed[zeros])).any()                 # cancellation to -0 and to +0
    tiny = float(np.finfo(F32).tiny)
    assert ((np.abs(t) > 0) & (np.abs(t) < tiny)).any() and ((np.abs(closed) > 0) & (np.abs(closed) < tiny)).any()      # subnormals in, out
    assert np.isposinf(t).any() and np.isneginf(t).any() and np.isnan(t).any()
    assert np.isnan(closed).any() and np.isinf(closed).any()
    assert (A.TABLE == F32(1e30)).any() and (A.TABLE == F32(1e-30)).any()


def _differs(a, b):
    return not A.same_bits(a, b)


def test_five_wrong_implementations_each_differ_on_the_table():
    gs = list(A.TABLE)
    want, acc = A.chain(gs)
    assert _differs(A.wrong_fp64_once(gs), want)
    assert _differs(A.wrong_reversed(gs), want)
    assert _differs(A.wrong_scaled_per_micro_batch(gs), A.scaled_once(gs))
    wrong_acc, wrong_g = A.wrong_close_writes_acc(acc, gs[-1])
    assert A.same_bits(wrong_g, want) and _differs(wrong_acc, acc)           # the gradient is right: only the untouched operand tells
    assert _differs(A.wrong_add_for_store(gs, np.full(len(want), A.DIRTY, F32)), want)
    # ... and on the tiled form the kernel tests use, at the smallest size that holds the whole table
    n = A.TABLE.shape[1]
    tiled = A.tiled(n)
    assert all(np.array_equal(A.bits(a), A.bits(b)) for a, b in zip(tiled, gs))


def test_the_size_grid_reaches_every_path_of_the_kernel():
    got = {n: A.regime(n) for n in A.SIZES}
    assert got[1] == (0, 0, 1, 1) and got[3] == (0, 0, 3, 1) and got[4] == (0, 1, 0, 1) and got[5] == (0, 1, 1, 1)
    assert got[A.THREAD_TRIP - 1] == (0, 3, 3, 1) and got[A.THREAD_TRIP] == (0, 4, 0, 1) and got[A.THREAD_TRIP + 1] == (0, 4, 1, 1)
    assert got[A.UNIT - 1] == (0, 1023, 3, 1) and got[A.UNIT] == (1, 0, 0, 1) and got[A.UNIT + 1] == (1, 0, 1, 1)
    assert got[A.GRID_CAP * A.UNIT + 1] == (A.GRID_CAP, 0, 1, 2)
    big = got[3 * 1000 * 1000 + 7]
    assert big[0] > 700 and big[1] > 256 and big[2] == 3 and big[3] == 1 and (3 * 1000 * 1000 + 7) % 2 == 1
    assert A.GUARD % 4 == 0 and A.ARENA_ALIGN == 8


# ---- StandardUpdater(accum_steps=K) on fakes --------------------------------------------------------------------------------------------
class _FakeOptimizer:
    """records which method took which batch, and reports a loss per micro-batch the way a Classifier does"""

    def __init__(self, losses):
        self.target, self.calls, self.losses = None, [], list(losses)

    def _take(self, kind, lossfun, batch):
        from loans_amd.runtime.core import report
        self.calls.append((kind, list(batch)))
        value = self.losses[len(self.calls) - 1]
        report({'loss': value, 'accuracy': value * 0 + 0.5})

    def accumulate(self, lossfun, batch):
        self._take('accumulate', lossfun, batch)

    def update(self, lossfun, batch):
        self._take('update', lossfun, batch)


class _HostUpdater(training.StandardUpdater):
    """the updater with the device half of a micro-step taken out: a batch goes to the optimiser as it is"""

    def _micro_step(self, call):
        call(None, next(self._iterators['main']))


@pytest.mark.parametrize('n_examples,K', [(6, 2), (6, 3), (8, 2), (10, 3)])
def test_iteration_epoch_and_new_epoch_bookkeeping(n_examples, K):
    import torch
    steps = 5
    losses = [torch.tensor(float(i + 1), dtype=torch.float32) for i in range(steps * K)]
    opt = _FakeOptimizer(losses)
    it = training.SerialIterator(list(range(n_examples)), 2, shuffle=False)
    upd = _HostUpdater(it, opt, device=0, accum_steps=K)
    assert upd.accum_steps == K and upd.is_new_epoch is False
    want = A.updater_schedule(n_examples, 2, K, steps)
    seen_non_final = False
    for step, (epoch, crossed) in enumerate(want, 1):
        upd.update()
        assert upd.iteration == step and upd.epoch == epoch == it.epoch and upd.is_new_epoch is crossed
        assert upd.epoch_detail == it.epoch_detail
        seen_non_final = seen_non_final or (crossed and not it.is_new_epoch)
        # the mean of the K micro-batches' observations, as a device scalar
        from loans_amd.runtime.core import reporter
        mean = reporter.observation['loss']
        assert torch.is_tensor(mean) and float(mean) == np.mean([float(l) for l in losses[(step - 1) * K:step * K]])
        assert float(reporter.observation['accuracy']) == 0.5
    if (n_examples, K) in ((6, 2), (10, 3)):
        assert seen_non_final              # a boundary on a non-final micro-batch: the iterator alone would have said False
    kinds = [k for k, _ in opt.calls]
    assert kinds == (['accumulate'] * (K - 1) + ['update']) * steps
    flat = [i for _, batch in opt.calls for i in batch]
    assert flat == [i % n_examples for i in range(2 * K * steps)]         # every batch once, in order


def test_accum_steps_one_is_the_plain_updater_and_bad_values_are_refused():
    opt = _FakeOptimizer([1.0])
    it = training.SerialIterator(list(range(4)), 2, shuffle=False)
    plain = training.StandardUpdater(it, opt, device=0)
    assert plain.accum_steps == 1 and '_crossed' not in plain.__dict__ and plain.is_new_epoch is it.is_new_epoch
    for bad in (0, -1, 1.5, '2', True, None):
        with pytest.raises(ValueError, match='accum_steps'):
            training.StandardUpdater(it, opt, device=0, accum_steps=bad)


# ---- the command line and the resume tables ---------------------------------------------------------------------------------------------
def test_the_option_parses_and_leaves_the_default_namespace_alone():
    import train_imagenet as T
    bare = T.parse_args([])
    assert 'accum_steps' not in vars(bare) and bare.accum_steps == 1
    args = T.parse_args(['--accum-steps', '8'])
    assert args.accum_steps == 8 and set(vars(args)) == set(vars(bare)) | {'accum_steps'}
    assert T.parse_args(['--accum-steps', '1']).accum_steps == 1
    T.parse_args(['--accum-steps', '2', '--optimizer', 'lamb', '--dtype', 'bf16', '--loss', 'bce', '--gpus', '2', '--drop-path', '0.1',
                  '--ema-decay', '0.9', '--clip-grad-norm', '1'])


@pytest.mark.parametrize('value', ['0', '-2', '1.5', 'two', 'nan'])
def test_zero_and_non_integers_are_refused(value, capsys):
    import train_imagenet as T
    with pytest.raises(SystemExit):
        T.parse_args(['--accum-steps=' + value])
    assert '--accum-steps' in capsys.readouterr().err
    args = T.Arguments()
    args.accum_steps = 0 if value == 'two' else (float(value) if '.' in value or value == 'nan' else int(value))
    with pytest.raises(ValueError, match='--accum-steps'):
        T.check_accum_arguments(args)


def test_the_option_is_in_the_help_text_and_the_docstring(capsys):
    import train_imagenet as T
    with pytest.raises(SystemExit):
        T.parse_args(['--help'])
    assert '--accum-steps K' in capsys.readouterr().out
    assert '--accum-steps' in T.__doc__ and 'per micro-batch' in T.__doc__


def test_resume_tables_and_the_argument_record():
    import train_imagenet as T
    assert 'accum_steps' in T.RESUME_FIXED and T.Arguments._ACCUM == ('accum_steps',)
    assert T.RESUME_DEFAULTS_ACCUM == {'accum_steps': 1}
    assert T.RESUME_DEFAULTS_WITH_ACCUM == dict(T.RESUME_DEFAULTS_WITH_DROP, accum_steps=1)
    assert 'accum_steps' not in T.RESUME_DEFAULTS_WITH_DROP                    # the older tables are what they were
    fixed = [k for k in T.RESUME_FIXED if k != 'gpus']
    # a checkpoint from before the option ran at 1
    args = T.parse_args([])
    saved = {k: v for k, v in checkpoint.plain_arguments(args).items() if k != 'accum_steps'}
    assert checkpoint.check_arguments(saved, args, fixed, checkpoint.SILENT, T.RESUME_DEFAULTS_WITH_ACCUM) == []
    assert checkpoint.check_arguments(saved, T.parse_args(['--accum-steps', '1']), fixed, checkpoint.SILENT, T.RESUME_DEFAULTS_WITH_ACCUM) == []
    with pytest.raises(ValueError, match='accum_steps: 1 in the checkpoint, 2 now'):
        checkpoint.check_arguments(saved, T.parse_args(['--accum-steps', '2']), fixed, checkpoint.SILENT, T.RESUME_DEFAULTS_WITH_ACCUM)
    # the record round-trips it, and a resume with another K is refused in the message that lists the fixed arguments
    given = T.parse_args(['--accum-steps', '2'])
    record = checkpoint._plain(checkpoint.plain_arguments(given))
    assert record['accum_steps'] == 2
    assert checkpoint.check_arguments(record, given, fixed, checkpoint.SILENT, T.RESUME_DEFAULTS_WITH_ACCUM) == []
    for other in (['--accum-steps', '4'], []):
        with pytest.raises(ValueError, match='these arguments must equal the checkpointed run\'s.*accum_steps: 2 in the checkpoint'):
            checkpoint.check_arguments(record, T.parse_args(other), fixed, checkpoint.SILENT, T.RESUME_DEFAULTS_WITH_ACCUM)
