"""The optimisers, each ONE fused kernel launch over the model's flat parameter arena: ``chainer.optimizers.Adam(alpha,
amsgrad=True)`` (train_sheep_localizer.py:130-134) and ``chainer.optimizers.MomentumSGD`` with the ``WeightDecay`` hook folded
in (the ImageNet pre-training recipe, train_imagenet.py).  ``GradientMethod`` holds what is not an update rule's arithmetic:
hooks, the ``lossfun`` path, the data-parallel gradient exchange, the stepped prefix and the capture hooks; an optimiser
supplies its state buffers (``_new_state``), its rate (``lr``) and its kernel call (``_step``).

Adam, Chainer 4.1.0 semantics (oracle/chainer_ops.py:adam_amsgrad_update): eps sits outside
the bias correction, ``lr_t = alpha * sqrt(1 - beta2^t) / (1 - beta1^t)``, parameters
without a gradient are updated with zeros (``reallocate_cleared_grads``): for a parameter
that never had one (m = v = 0) that is a no-op, so the arena's never-used tail -- res6 / res7
below 225 / 301 px -- is skipped; once a parameter HAS been stepped with a gradient its moments
keep decaying and it keeps moving on zero gradients, so the step covers the largest prefix any
update of this optimiser has seen, with the gradients beyond the current graph zeroed.  With a communicator attached
(``parallel.create_multi_node_optimizer``) gradients are all-reduced over RCCL first."""
import math
from types import SimpleNamespace

import numpy as np
import torch

from .. import ops


class GradientMethod:
    """``chainer.GradientMethod`` over one arena.  A subclass sets ``self.hyperparam`` and provides ``_new_state(zeros)`` (its
    state buffers, each the size of the arena), the property ``lr`` (the rate of step ``self.t``) and
    ``_step(arena, n, state, lr, grad_scale)`` (one kernel launch over the first ``n`` floats; ``lr`` is a float, or the device
    scalar of a captured step)."""

    def __init__(self):
        self.t = 0
        self.target = None
        self.comm = None
        self._state = None
        self._hooks = {}
        self._pending, self._exchanged_from, self._plan = [], None, None      # staged gradient exchange (data parallel)
        # gradient accumulation: (arena, accumulator) once accumulate() has run, the micro-batches summed since the last step, the
        # active prefix they covered, and whether accumulate() is inside its backward
        self._accum, self._accum_count, self._accum_numel, self._accumulating = None, 0, None, False

    def setup(self, link):
        self.target = link
        return self

    # chainer.Optimizer.add_hook / remove_hook / call_hooks: a hook is called with the optimiser once per update(), after
    # the gradients are complete (data parallel: after the all-reduce) and before the parameters move -- where Chainer's
    # GradientMethod.update calls them.  The parity tests read every step's gradients through one.
    def add_hook(self, hook, name=None):
        if not callable(hook):
            raise TypeError('hook function is not callable')
        name = name or getattr(hook, 'name', None) or getattr(hook, '__name__', None) or 'hook%d' % len(self._hooks)
        if name in self._hooks:
            raise KeyError('hook %s already exists' % name)
        self._hooks[name] = hook

    def remove_hook(self, name):
        del self._hooks[name]

    def call_hooks(self):
        for hook in list(self._hooks.values()):
            hook(self)

    def _ensure_state(self):
        arena = self.target.arena
        if arena is None:
            arena = self.target.finalize()
        if self._state is None or self._state[0].numel() != arena.numel:
            self._state = tuple(self._new_state(lambda: torch.zeros(arena.numel, device=arena.device, dtype=torch.float32)))
        return arena

    # ---- gradient accumulation (train_imagenet.py --accum-steps K) ------------------------------------------------------------
    def _accum_buffer(self, arena):
        """the accumulator's first ``arena.active_numel`` floats: one buffer the size of the arena, allocated on first use -- an
        optimiser that never accumulates holds none -- and the prefix held to the one the step's first micro-batch covered"""
        n = arena.active_numel
        if self._accum_count == 0:
            self._accum_numel = n
        elif n != self._accum_numel:
            raise RuntimeError('the active parameter prefix changed from %d to %d floats between the micro-batches of one accumulated '
                               'step' % (self._accum_numel, n))
        if self._accum is None or self._accum[0] is not arena:
            self._accum = (arena, torch.empty(arena.numel, device=arena.device, dtype=torch.float32))
        return self._accum[1][:n]

    def _refuse_mid_step(self, what):
        if self._accum_count:
            raise RuntimeError('%s in the middle of an accumulated step (%d micro-batches since the last update()): a checkpoint lies '
                               'between steps' % (what, self._accum_count))

    def accumulate(self, lossfun, *args, **kwds):
        """The first half of ``update(lossfun, ...)`` for all micro-batches of a step but the last: evaluate, clear, differentiate,
        wait for the weight gradients -- then add the gradient arena's active prefix into the accumulator (``ops.grad_accum``: it is
        stored by the first call since the last step and added by the later ones, one fp32 addition per element) and count the call.
        Nothing is exchanged, no hook runs, no parameter moves and ``t`` stands still.  The ``update(lossfun, ...)`` of the last
        micro-batch closes the step: the sum ``((g1 + g2) + ..) + gK`` lands in the gradient arena, is exchanged once, and the
        step is taken with ``grad_scale = 1 / (K * world size)``.  BN statistics are those of each micro-batch."""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('accumulate() launches once per micro-batch from the host: not inside a captured step')
        self._accumulating = True       # the backward's stage boundaries start no exchange: the arena holds one micro-gradient
        try:
            loss = lossfun(*args, **kwds)
            self.target.cleargrads()
            loss.backward()
            del loss
        finally:
            self._accumulating = False
        if not any(p.update_rule.enabled for p in self.target.params()):
            return
        arena = self._ensure_state()
        ops.join_side_stream(arena.device)      # all weight gradients of this micro-batch have landed
        acc = self._accum_buffer(arena)
        ops.grad_accum(acc, arena.grad[:acc.numel()], 'add' if self._accum_count else 'store')
        self._accum_count += 1

    def _close_accumulated(self, arena):
        """the closing ``update()``: the accumulated sum into the gradient arena, ONE exchange of the whole active prefix behind it
        (the staged overlap is given up under accumulation: during the closing backward the arena held only the last
        micro-gradient), and the scale that makes the step the mean over micro-batches and ranks, formed in double"""
        ops.join_side_stream(arena.device)
        acc = self._accum_buffer(arena)
        ops.grad_accum(acc, arena.grad[:acc.numel()], 'close')
        world = 1
        if self.comm is not None and getattr(self.comm, 'active', self.comm.size > 1):
            self.comm.allreduce_grad(arena)
            world = self.comm.size
        grad_scale = 1.0 / ((self._accum_count + 1) * world)
        self._accum_count = 0
        return grad_scale

    def update(self, lossfun=None, *args, **kwds):
        if self._accum_count and torch.cuda.is_current_stream_capturing():
            raise RuntimeError('an accumulated step is closed from the host: not inside a captured step')
        if lossfun is not None:
            # chainer.GradientMethod.update(lossfun, *args): evaluate, clear, differentiate, then the step below
            # (the LoANs updater calls update() bare, sheep_updater.py:52,66)
            loss = lossfun(*args, **kwds)
            self.target.cleargrads()
            loss.backward()
            del loss
        if not any(p.update_rule.enabled for p in self.target.params()):
            return
        arena = self._ensure_state()
        grad_scale = 1.0
        if self._accum_count:                   # accumulate() ran since the last step: this backward's was the last micro-batch
            grad_scale = self._close_accumulated(arena)
        elif self._exchanged_from is not None:  # stage_done() / update_begin() already started the exchange of this step
            if self._exchanged_from > 0:
                self._exchange(arena, 0)        # what the stage boundaries left (stem .. res3, or everything below the last one)
            for work in self._pending:
                work.wait()                     # the current stream waits for RCCL's
            self._pending, self._exchanged_from = [], None
            ops.join_side_stream(arena.device)
            grad_scale = 1.0 / self.comm.size
        else:
            ops.join_side_stream(arena.device)  # all weight gradients of this step have landed
            if self.comm is not None and getattr(self.comm, 'active', self.comm.size > 1):
                self.comm.allreduce_grad(arena)
                grad_scale = 1.0 / self.comm.size
        self.grad_scale = grad_scale        # data parallel: the arena holds the SUM over ranks, the kernel applies 1 / world size
        if self._hooks:
            if arena.grad.is_cuda and torch.cuda.is_current_stream_capturing():
                # hooks run on the host.  A data-parallel step is captured in two segments with the exchange between their
                # replays (sheep_updater._capture_segments): there the replay loop calls the hooks at that point of every step
                if not getattr(self, 'hooks_by_replay', False):
                    raise RuntimeError('optimizer hooks run on the host: not inside a captured step')
            else:
                self.call_hooks()
        # parameters beyond the prefix the current graph touches have no gradient.  Those that never had one are skipped
        # (m = v = 0: Chainer's zero-gradient step is a no-op); those that were trained before -- the frame height crossed
        # 224 / 300 px between steps -- are stepped with a zero gradient like Chainer does (their m decays, they keep moving)
        n = arena.active_numel
        seen = max(getattr(self, '_stepped_numel', 0), n)
        if seen > n:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError('the active parameter prefix shrank inside a captured step')
            arena.grad[n:seen].zero_()
            n = seen
        self._stepped_numel = seen
        if torch.cuda.is_current_stream_capturing():
            # being recorded into a hipGraph (SheepAssessor(use_graph=True)): nothing executes now, and the replays
            # must not bake in this step's rate -- the kernel reads it from device memory, `begin_replay()` advances it
            if getattr(self, '_lr_dev', None) is None:
                raise RuntimeError('call prepare_capture() before recording %s.update() into a graph' % type(self).__name__)
            lr = self._lr_dev
            self._captured = True
        else:
            self.t += 1
            lr = self.lr
        self._step(arena, n, self._state, lr, grad_scale)

    def _exchange_active(self):
        if self._accumulating or self._accum_count:
            return False        # under accumulation stage_done() / update_begin() start nothing: the closing update() exchanges the sum once
        return self.comm is not None and getattr(self.comm, 'active', self.comm.size > 1) and \
            any(p.update_rule.enabled for p in self.target.params())

    def _exchange(self, arena, lo):
        """Start the all-reduce of the gradient floats [lo, what has been started already) and return.  It is issued from the
        weight-gradient stream after that stream has caught up with the current one: RCCL's stream then waits for every
        gradient kernel enqueued so far -- weight gradients (side stream) and the BN gamma / beta sums (current stream) --
        and for nothing that is enqueued afterwards; neither stream waits for the collective."""
        hi = arena.active_numel if self._exchanged_from is None else self._exchanged_from
        if lo < hi:
            if arena.grad.is_cuda:
                main = torch.cuda.current_stream(arena.device)
                side = ops._side_stream(arena.device)
                side.wait_stream(main)
                with torch.cuda.stream(side):
                    self._pending += self.comm.allreduce_range(arena, lo, hi, async_op=True)
            else:
                self._pending += self.comm.allreduce_range(arena, lo, hi, async_op=True)
        self._exchanged_from = min(lo, hi)

    def stage_done(self, name):
        """A backbone's StageBoundary reports that the backward has left stage ``name``: every gradient from that stage's
        first float to the end of the arena's active prefix is complete (parallel.exchange_plan) and its exchange starts now,
        beside the backward of the stages in front of it (attached by parallel.create_multi_node_optimizer)."""
        if not self._exchange_active():
            return
        arena = self._ensure_state()
        if arena.grad.is_cuda and torch.cuda.is_current_stream_capturing():
            return
        if self._plan is None:
            from .. import parallel
            self._plan = parallel.exchange_plan(self.target)
        lo = self._plan.get(name)
        if lo is not None and lo < arena.active_numel:
            self._exchange(arena, lo)

    def update_begin(self):
        """Data parallel only: start the all-reduce of whatever part of the gradient arena the stage boundaries have not
        started yet and return, so that it runs beside whatever the caller issues next; the following ``update()`` waits for
        all parts and applies the step.  The gradients must not be touched (no ``cleargrads``) in between.  Without an active
        communicator this is a no-op."""
        if not self._exchange_active():
            return
        self._exchange(self._ensure_state(), 0)

    def exchange_wait(self):
        """Make the current stream wait for every exchange started so far and forget them -- for a caller that applies the
        step itself (the captured update of a data-parallel hipGraph, sheep_updater._capture_segments: the graph recorded
        "already exchanged", so nothing inside it waits)."""
        for work in self._pending:
            work.wait()
        self._pending, self._exchanged_from = [], None

    def prepare_capture(self):
        """Allocate what a captured update reads at replay time -- outside the capture, so that neither the buffer nor
        its initialisation belongs to the graph."""
        arena = self._ensure_state()
        if getattr(self, '_lr_dev', None) is None:
            self._lr_dev = torch.zeros(1, device=arena.device, dtype=torch.float32)

    def begin_replay(self):
        """Before replaying a captured step: count it and publish its rate (Adam: bias-corrected) to the kernel."""
        if getattr(self, '_captured', False):
            self.t += 1
            self._lr_dev.fill_(self.lr)

    # ---- checkpoints (runtime/checkpoint.py) --------------------------------------------------------------------------
    def _state_names(self):
        """names of the state buffers a step reads, in ``_new_state`` order"""
        raise NotImplementedError

    def state_dict(self):
        """Everything a later ``update()`` depends on, independent of the arena's layout: ``class``, ``t``, ``hyperparam`` (a
        dict), ``stepped_cold`` (None before the first step, else the cold links -- res6 / res7, fc6 -- the stepped prefix has
        reached) and ``state``: every state buffer cut per parameter, in the parameter's Chainer layout, under
        ``<param path>/<buffer name>`` with the paths ``state_dict_chainer()`` uses.  Full length: parameters behind the active
        prefix are included.  Nothing of a gradient accumulator: a checkpoint lies between steps, where it holds nothing that has to
        survive -- in the middle of an accumulated step this is a RuntimeError."""
        self._refuse_mid_step('state_dict()')
        arena = self._ensure_state()
        named = {id(p): k[1:] for k, p in self.target.namedparams()}
        state = {}
        for name, buf in zip(self._state_names(), self._state):
            host = buf.detach().cpu().numpy()
            for p, o in zip(arena.params, arena.offsets):
                state['%s/%s' % (named[id(p)], name)] = np.ascontiguousarray(p._to_logical(host[o:o + p.size].reshape(p.physical_shape)))
        stepped = getattr(self, '_stepped_numel', 0)
        return {'class': type(self).__name__, 't': int(self.t), 'hyperparam': dict(vars(self.hyperparam)),
                'stepped_cold': None if stepped == 0 else [n for n, o in arena.cold_offsets.items() if o < stepped],
                'state': state}

    def load_state_dict(self, sd):
        """Restore ``state_dict()``'s record into this optimiser (set up on a model of the same architecture).  ValueError
        naming the first offending field or key where the class, ``amsgrad``, the parameter paths or a shape differ; nothing is
        changed then.  The buffers are written in place, so a captured step keeps reading them, and the device copy of the rate
        a captured step reads is republished for the restored ``t``."""
        self._refuse_mid_step('load_state_dict()')
        if sd['class'] != type(self).__name__:
            raise ValueError('class: the checkpoint holds %s, this optimiser is %s' % (sd['class'], type(self).__name__))
        hp = dict(sd['hyperparam'])
        if bool(hp.get('amsgrad', False)) != bool(getattr(self.hyperparam, 'amsgrad', False)):
            raise ValueError('amsgrad: the checkpoint has %r, this optimiser %r' % (hp.get('amsgrad'), self.hyperparam.amsgrad))
        arena = self._ensure_state()
        named = {id(p): k[1:] for k, p in self.target.namedparams()}
        names = self._state_names()
        want = {'%s/%s' % (named[id(p)], n): p for p in arena.params for n in names}
        state = sd['state']
        odd = sorted(set(want) ^ set(state))
        if odd:
            raise ValueError('%s: %s' % (odd[0], 'not in the checkpoint' if odd[0] in want else 'no such parameter state in this model'))
        for key, p in want.items():
            if tuple(np.shape(state[key])) != p.logical_shape:
                raise ValueError('%s: shape %s in the checkpoint, %s in this model' % (key, tuple(np.shape(state[key])), p.logical_shape))
        for name, buf in zip(names, self._state):
            host = np.zeros(arena.numel, np.float32)
            for p, o in zip(arena.params, arena.offsets):
                host[o:o + p.size] = p._from_logical(np.asarray(state['%s/%s' % (named[id(p)], name)], dtype=np.float32)).ravel()
            buf.copy_(torch.from_numpy(host))
        for k, v in hp.items():
            setattr(self.hyperparam, k, v)
        self.t = int(sd['t'])
        stepped = sd['stepped_cold']
        if stepped is None:
            self._stepped_numel = 0
        else:       # the cold links lie behind the hot parameters in `cold_links` order: the prefix ends at the first one not stepped
            self._stepped_numel = min([o for n, o in arena.cold_offsets.items() if n not in stepped] + [arena.numel])
        if getattr(self, '_lr_dev', None) is not None and self.t > 0:
            self._lr_dev.fill_(self.lr)


class Adam(GradientMethod):

    def __init__(self, alpha=0.001, beta1=0.9, beta2=0.999, eps=1e-8, eta=1.0, weight_decay_rate=0, amsgrad=False):
        super().__init__()
        self.hyperparam = SimpleNamespace(alpha=alpha, beta1=beta1, beta2=beta2, eps=eps, eta=eta,
                                          weight_decay_rate=weight_decay_rate, amsgrad=amsgrad)

    @property
    def alpha(self):
        return self.hyperparam.alpha

    @alpha.setter
    def alpha(self, v):
        self.hyperparam.alpha = v

    @property
    def lr(self):
        hp = self.hyperparam
        if self.t == 0:
            raise RuntimeError("Can't determine the learning rate of Adam optimizer because the update steps have not been started.")
        fix1 = 1. - math.pow(hp.beta1, self.t)
        fix2 = 1. - math.pow(hp.beta2, self.t)
        return hp.alpha * math.sqrt(fix2) / fix1

    def _new_state(self, zeros):
        return zeros(), zeros(), zeros()        # m, v, vhat

    def _state_names(self):
        return ('m', 'v', 'vhat') if self.hyperparam.amsgrad else ('m', 'v')

    def _step(self, arena, n, state, lr, grad_scale):
        hp = self.hyperparam
        m, v, vhat = state
        ops.adam_amsgrad(arena.data[:n], arena.grad[:n], m[:n], v[:n], vhat[:n] if hp.amsgrad else None, lr, hp.beta1, hp.beta2,
                         hp.eps, hp.eta, hp.weight_decay_rate, grad_scale)


def decay_segments(sizes, offsets, exempt, numel):
    """The segment table of ``ops.momentum_sgd_seg`` for parameters of ``sizes`` floats at ``offsets`` of a flat buffer of
    ``numel`` floats (ascending, every offset a multiple of 4, the first one 0; ``ParamArena`` pads to 8), ``exempt[i]`` true where
    parameter i takes no weight decay: ``(ends, flags)`` -- exclusive ends as int64 and one flag byte per segment, bit 0 = exempt.
    A parameter's segment runs to the next parameter's offset (the padding behind it is zero and has a zero gradient: it does not
    move either way), the last one to ``numel``; neighbours with equal flags are one segment.  A pure function of its arguments."""
    sizes, offsets = [int(s) for s in sizes], [int(o) for o in offsets]
    if not sizes or len(sizes) != len(offsets) or len(sizes) != len(exempt):
        raise ValueError('one size, one offset and one flag per parameter, and at least one parameter')
    if offsets[0] != 0:
        raise ValueError('the first parameter starts at offset %d, not 0' % offsets[0])
    stops = offsets[1:] + [int(numel)]
    ends, flags = [], []
    for size, start, stop, flag in zip(sizes, offsets, stops, exempt):
        if start % 4 or size <= 0 or start + size > stop:
            raise ValueError('a parameter of %d floats at offset %d does not fit in front of %d on a float4 boundary' % (size, start, stop))
        if flags and flags[-1] == int(bool(flag)):
            ends[-1] = stop
        else:
            ends.append(stop)
            flags.append(int(bool(flag)))
    return np.asarray(ends, np.int64), np.asarray(flags, np.uint8)


class MomentumSGD(GradientMethod):
    """``chainer.optimizers.MomentumSGD(lr, momentum)`` with ``chainer.optimizer.WeightDecay(weight_decay_rate)`` applied to the
    gradient first: ``g' = g + rate * p; v = momentum * v - lr * g'; p += v``.  State: one ``v`` the size of the arena.  The
    prefix rule of the module docstring holds as it stands: v = 0 and g = 0 make the step of a never-used parameter a no-op,
    and a parameter that was stepped before keeps moving by its decaying ``v``.

    ``decay_exempt_1d=True``: parameters whose Chainer shape has at most one dimension -- BN ``gamma`` / ``beta``, biases -- take
    no weight decay (``decay_segments`` over the arena, ``ops.momentum_sgd_seg``: still one launch)."""

    def __init__(self, lr=0.01, momentum=0.9, weight_decay_rate=0.0, decay_exempt_1d=False):
        super().__init__()
        self.hyperparam = SimpleNamespace(lr=lr, momentum=momentum, weight_decay_rate=weight_decay_rate,
                                          decay_exempt_1d=bool(decay_exempt_1d))
        self._segments, self._segment_cuts = None, {}

    def _segment_table(self, arena, n):
        """the decay segments of the first ``n`` floats of ``arena``: the arena's table is built and uploaded once, and cut once
        per stepped prefix -- that ends at a cold link's offset, so there are at most a few"""
        if self._segments is None or self._segments[0] is not arena:
            if arena.data.is_cuda and torch.cuda.is_current_stream_capturing():
                raise RuntimeError('the decay segment table is uploaded once, outside a captured step: step once before capturing')
            ends, flags = decay_segments([p.size for p in arena.params], arena.offsets,
                                         [len(p.logical_shape) <= 1 for p in arena.params], arena.numel)
            if len(ends) > ops.SGD_MAX_SEGMENTS:
                raise ValueError('%d decay segments: the kernel takes %d' % (len(ends), ops.SGD_MAX_SEGMENTS))
            self._segments, self._segment_cuts = (arena, ops.SegmentTable(ends, flags, arena.device)), {}
        table = self._segment_cuts.get(n)
        if table is None:
            table = self._segment_cuts[n] = self._segments[1].prefix(n)
        return table

    @property
    def lr(self):
        return self.hyperparam.lr

    @lr.setter
    def lr(self, v):
        self.hyperparam.lr = v

    def _new_state(self, zeros):
        return (zeros(),)

    def _state_names(self):
        return ('v',)

    def _step(self, arena, n, state, lr, grad_scale):
        hp = self.hyperparam
        if getattr(hp, 'decay_exempt_1d', False):
            ops.momentum_sgd_seg(arena.data[:n], arena.grad[:n], state[0][:n], lr, hp.momentum, hp.weight_decay_rate,
                                 self._segment_table(arena, n), grad_scale)
            return
        ops.momentum_sgd(arena.data[:n], arena.grad[:n], state[0][:n], lr, hp.momentum, hp.weight_decay_rate, grad_scale)


def lars_segments(sizes, offsets, exempt_decay, exempt_adapt, numel):
    """The segment table of ``ops.lars_ratios`` / ``ops.lars_update`` for the parameters ``decay_segments`` describes: ``(ends,
    flags)`` with bit 0 of a flag byte = no weight decay (``exempt_decay[i]``) and bit 1 = no adaptation (``exempt_adapt[i]``).  A
    trust ratio belongs to ONE tensor, so a parameter that adapts is a segment of its own; neighbours are one segment only where
    both have bit 1 set and their flags are equal.  A parameter's segment runs to the next parameter's offset: the padding behind
    it is zero and has a zero gradient, it adds nothing to either norm.  A pure function of its arguments."""
    sizes, offsets = [int(s) for s in sizes], [int(o) for o in offsets]
    if not sizes or len(sizes) != len(offsets) or len(sizes) != len(exempt_decay) or len(sizes) != len(exempt_adapt):
        raise ValueError('one size, one offset and two flags per parameter, and at least one parameter')
    if offsets[0] != 0:
        raise ValueError('the first parameter starts at offset %d, not 0' % offsets[0])
    stops = offsets[1:] + [int(numel)]
    ends, flags = [], []
    for size, start, stop, nodecay, noadapt in zip(sizes, offsets, stops, exempt_decay, exempt_adapt):
        if start % 4 or size <= 0 or start + size > stop:
            raise ValueError('a parameter of %d floats at offset %d does not fit in front of %d on a float4 boundary' % (size, start, stop))
        flag = int(bool(nodecay)) | int(bool(noadapt)) << 1
        if flags and flag & 2 and flags[-1] == flag:
            ends[-1] = stop
        else:
            ends.append(stop)
            flags.append(flag)
    return np.asarray(ends, np.int64), np.asarray(flags, np.uint8)


class LARS(GradientMethod):
    """Layer-wise adaptive rate scaling (You et al. 2017, the MLPerf ResNet-50 recipe) on ``MomentumSGD``'s rule: per parameter
    ``r = eta * |p| / (|g| + wd * |p| + eps)`` (1 where either norm is zero), then ``g' = g + wd * p; v = momentum * v - lr * r * g';
    p += v``.  Parameters whose Chainer shape has at most one dimension -- BN ``gamma`` / ``beta``, biases -- never adapt (r = 1) and,
    with ``decay_exempt_1d=True``, take no weight decay.  Two passes over the arena: ``ops.lars_ratios`` (norms in float64, ratios
    left on the device), ``ops.lars_update``.  State: one ``v`` the size of the arena; the prefix rule of the module docstring
    holds as for ``MomentumSGD`` (a never-used parameter has zero norms: r = 1, and v = g = 0 make its step a no-op)."""

    def __init__(self, lr=0.01, momentum=0.9, weight_decay_rate=0.0, eta=0.001, eps=1e-8, decay_exempt_1d=False):
        super().__init__()
        self.hyperparam = SimpleNamespace(lr=lr, momentum=momentum, weight_decay_rate=weight_decay_rate, eta=eta, eps=eps,
                                          decay_exempt_1d=bool(decay_exempt_1d))
        self._segments, self._segment_cuts, self._last_table = None, {}, None

    def _segment_table(self, arena, n):
        """the segments of the first ``n`` floats of ``arena``, with the ratio buffer and the workspace: built and allocated once
        per arena and cut once per stepped prefix, as ``MomentumSGD._segment_table`` -- no device allocation in a step"""
        exempt = bool(getattr(self.hyperparam, 'decay_exempt_1d', False))
        if self._segments is None or self._segments[0] is not arena or self._segments[2] != exempt:
            if arena.data.is_cuda and torch.cuda.is_current_stream_capturing():
                raise RuntimeError('the decay segment table is uploaded once, outside a captured step: step once before capturing')
            one_d = [len(p.logical_shape) <= 1 for p in arena.params]
            ends, flags = lars_segments([p.size for p in arena.params], arena.offsets, [exempt and d for d in one_d], one_d, arena.numel)
            if len(ends) > ops.LARS_MAX_SEGMENTS:
                raise ValueError('%d LARS segments: the kernel takes %d' % (len(ends), ops.LARS_MAX_SEGMENTS))
            self._segments, self._segment_cuts = (arena, ops.LarsTable(ends, flags, arena.device), exempt), {}
        table = self._segment_cuts.get(n)
        if table is None:
            table = self._segment_cuts[n] = self._segments[1].prefix(n)
        return table

    @property
    def lr(self):
        return self.hyperparam.lr

    @lr.setter
    def lr(self, v):
        self.hyperparam.lr = v

    def _new_state(self, zeros):
        return (zeros(),)

    def _state_names(self):
        return ('v',)

    def _step(self, arena, n, state, lr, grad_scale):
        hp = self.hyperparam
        table = self._last_table = self._segment_table(arena, n)
        ops.lars_ratios(arena.data[:n], arena.grad[:n], hp.weight_decay_rate, hp.eta, hp.eps, table, grad_scale)
        ops.lars_update(arena.data[:n], arena.grad[:n], state[0][:n], lr, hp.momentum, hp.weight_decay_rate, table, grad_scale)

    def trust_ratios(self):
        """``{parameter path: ratio}`` of the last step, for the parameters it covered (1.0 for those that never adapt).
        Synchronises with the device: for diagnostics and tests, not for a training loop."""
        table = self._last_table
        if table is None:
            raise RuntimeError('no step has been taken yet')
        arena = self._segments[0]
        ratios = table.ratios.detach().cpu().numpy()
        named = {id(p): k[1:] for k, p in self.target.namedparams()}
        n = int(table.ends_host[-1])
        out = {}
        for p, o in zip(arena.params, arena.offsets):
            if o < n:
                out[named[id(p)]] = float(ratios[int(np.searchsorted(table.ends_host, o, side='right'))])
        return out


class LAMB(GradientMethod):
    """LAMB (You et al. 2019, "Large Batch Optimization for Deep Learning", algorithm 2 with the identity for phi): Adam's direction
    with decoupled weight decay, its length set per parameter tensor by the trust ratio.  Step ``t`` (1-based), ``gs`` the gradient
    scale of a data-parallel step; segment ``s`` of the arena has flag byte ``f``: bit 0 = no weight decay, bit 1 = no adaptation
    (``lars_segments``' table)::

        g^  = g * gs
        m'  = m + (1 - beta1) (g^ - m)
        v'  = v + (1 - beta2) (g^ g^ - v)
        c1  = 1 / (1 - beta1^t)      c2 = 1 / (1 - beta2^t)
        a   = (m' c1) / (sqrt(v' c2) + eps)
        wd_s = (f & 1) ? 0 : wd
        u   = a + wd_s p                 (decoupled decay, inside the trust ratio as in the paper)
        W   = |p|_2 over the segment     U = |u|_2 over the segment
        r   = (f & 2) or W == 0 or U == 0 ?  1  :  W / U
        p'  = p - (lr r) u

    ``c1`` and ``c2`` are formed in double here and rounded to fp32 once; ``W``, ``U`` and ``r`` are formed in double from fp64 sums
    of the squares of the fp32 values, and ``r`` is rounded to fp32 once.  Parameters whose Chainer shape has at most one dimension
    -- BN ``gamma`` / ``beta``, biases -- never adapt (r = 1) and, with ``decay_exempt_1d=True``, take no decay, as for ``LARS``.
    There is no clamp on ``W``; clipping by the global norm is the ``GradientClipping`` hook.  Wherever a segment adapts, ``|p' - p|_2 = lr |p|_2`` at every step,
    whatever the gradient.  ``v = g^2`` overflows fp32 beyond ``|g gs|`` ~ 1e19: Adam's own limit.

    Three launches per step (``ops.lamb_moments``, ``ops.lamb_ratios``, ``ops.lamb_update``; ``csrc/lamb.hip``); the bias correction
    travels as ``c1``, ``c2``, not inside the rate, so ``lr`` is the plain hyperparameter.  State: ``m`` and ``v``, each the size of
    the arena.  The prefix rule of the module docstring holds: beyond the stepped prefix nothing is touched (inside it a
    parameter with zero gradient and zero moments has u = wd_s p: with decay it shrinks by lr of its norm, without it stays)."""

    def __init__(self, lr=0.001, beta1=0.9, beta2=0.999, eps=1e-6, weight_decay_rate=0.0, decay_exempt_1d=False):
        super().__init__()
        self.hyperparam = SimpleNamespace(lr=lr, beta1=beta1, beta2=beta2, eps=eps, weight_decay_rate=weight_decay_rate,
                                          decay_exempt_1d=bool(decay_exempt_1d))
        self._segments, self._segment_cuts, self._last_table = None, {}, None

    _segment_table = LARS._segment_table        # built once per arena, cut once per stepped prefix: no device allocation in a step
    trust_ratios = LARS.trust_ratios

    @property
    def lr(self):
        return self.hyperparam.lr

    @lr.setter
    def lr(self, v):
        self.hyperparam.lr = v

    def _new_state(self, zeros):
        return zeros(), zeros()

    def _state_names(self):
        return ('m', 'v')

    def _step(self, arena, n, state, lr, grad_scale):
        if torch.is_tensor(lr) or (arena.data.is_cuda and torch.cuda.is_current_stream_capturing()):
            raise RuntimeError('LAMB is not built for a captured step: its bias corrections c1, c2 change with every step and '
                               'travel as launch arguments')
        hp = self.hyperparam
        c1, c2 = 1.0 / (1.0 - math.pow(hp.beta1, self.t)), 1.0 / (1.0 - math.pow(hp.beta2, self.t))
        table = self._last_table = self._segment_table(arena, n)
        m, v = state
        ops.lamb_moments(arena.data[:n], arena.grad[:n], m[:n], v[:n], hp.beta1, hp.beta2, c1, c2, hp.eps, hp.weight_decay_rate,
                         table, grad_scale)
        ops.lamb_ratios(table)
        ops.lamb_update(arena.data[:n], m[:n], v[:n], lr, c1, c2, hp.eps, hp.weight_decay_rate, table)


class GradientClipping:
    """``chainer.optimizer_hooks.GradientClipping(threshold)``: clip the gradient by its global L2 norm, on the device.  Used as
    ``optimizer.add_hook(loans_amd.GradientClipping(1.0))`` with any ``GradientMethod`` (``Adam``, ``MomentumSGD`` in both forms,
    ``LARS``, ``LAMB``): ``update()`` calls it once per step, after the data-parallel all-reduce and before the parameters move.
    For the first ``n = arena.active_numel`` floats ``g`` of the gradient arena, ``gs = optimizer.grad_scale`` (1 / world size where
    the arena holds the sum over ranks) and the threshold ``c > 0``::

        S    = sum g_i^2                      every g_i converted to double and squared (exact), summed in fp64 in a FIXED order
        N    = |gs| * sqrt(S)                 in double: the norm of the gradient the optimiser will actually apply
        k    = (N is finite and N > c) ? c / N : 1          in double, rounded to fp32 ONCE
        g_i' = fl32(g_i * k)                  one fp32 product per element, in place -- skipped entirely when k == 1

    ``N == c`` does not clip (Chainer's ``rate < 1``); an all-zero gradient gives ``N = 0``, ``k = 1`` and no division.  A non-finite
    ``N`` -- a NaN or inf anywhere in ``g``, or a sum that overflows -- gives ``k = 1``: the gradient is left bit for bit as it was and
    the record holds the non-finite ``N``, so that a log shows it.  This is a deliberate departure from Chainer, which would write
    ``0 * inf`` over the whole gradient.  ``threshold=inf`` is legal and means "measure only": the norm is recorded, nothing is scaled.

    Two launches for the norm (``ops.grad_norm``), a third for the product (``ops.grad_clip_apply``; not issued for ``inf``, and
    returning before it touches ``g`` where ``k == 1``); ``N`` (rounded to fp32 once) and ``k`` stay in a two-float device record,
    nothing returns to the host.  The gradients ``update()`` zeroes behind ``n`` afterwards are zero either way.  The hook holds no
    training state -- its workspace is allocated once per arena, nothing goes into a checkpoint.  Hooks run on the host, so
    ``update()`` refuses them inside a captured step: clipping in a hipGraph step is not built.

    ``last_norm()`` and ``last_coefficient()`` read the record.  They synchronise with the device: for diagnostics, tests and a log
    entry's synchronisation point, not for every step of a training loop."""
    name = 'GradientClipping'

    def __init__(self, threshold):
        threshold = float(threshold)
        if not threshold > 0.0:
            raise ValueError('the threshold of GradientClipping must be positive (inf: measure only), got %r' % threshold)
        self.threshold = threshold
        self._clip = None       # (arena, ops.GradClipState)

    def __call__(self, opt):
        arena = opt.target.arena
        n = arena.active_numel
        if n <= 0:
            return
        if self._clip is None or self._clip[0] is not arena:
            self._clip = (arena, ops.GradClipState(arena.numel, arena.device))
        state = self._clip[1]
        g = arena.grad[:n]
        ops.grad_norm(g, self.threshold, state, getattr(opt, 'grad_scale', 1.0))
        if self.threshold != math.inf:
            ops.grad_clip_apply(g, state)

    def _record(self):
        if self._clip is None:
            raise RuntimeError('no step has been taken yet')
        return self._clip[1].record.detach().cpu().numpy()

    def last_norm(self):
        """``N`` of the last step, before clipping, as the device record holds it (fp32).  Synchronises with the device."""
        return float(self._record()[0])

    def last_coefficient(self):
        """``k`` of the last step (1.0: nothing was scaled).  Synchronises with the device."""
        return float(self._record()[1])
