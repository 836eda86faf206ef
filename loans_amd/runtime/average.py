"""An exponential moving average (EMA) of a model's weights, kept beside the live model.

``WeightAverage(link, decay)`` holds one buffer the size of the link's parameter arena and one tensor per float persistent
(BN ``avg_mean`` / ``avg_var``), all starting as copies of the live values.  ``update()`` -- once after every optimiser step --
moves every one of them towards the live value in ONE kernel launch over a job table built at construction
(``ops.average_jobs``, csrc/misc.hip: ``avg += (1 - d) * (live - avg)``).  The update is exactly nothing where average and live
value are equal, so the arena's never-trained cold tail (res6 / res7) needs no prefix rule: it costs its bytes and stays put.

``applied()`` exchanges averages and live values in place -- one launch on entry, one on exit -- so that inside the block the
model IS the averaged model, for validation and for snapshots, without a second model; afterwards the live model is back bit for
bit.  It is for use between steps: inside a step ``ops`` trusts buffers derived from the weights (bf16 shadow, fragment-order
packs, data-gradient re-packs; all rebuilt from the masters by the next ``begin_step``), outside it derives them per call.

Data parallel: every rank keeps its own average.  The parameters are identical on all ranks, so their averages are too; the
averaged BN statistics are local, like the live ones, and ``Communicator.bcast_persistents`` called inside ``applied()`` sends
rank 0's to every rank exactly as it does for the live ones."""
import contextlib
from types import SimpleNamespace

import numpy as np
import torch

from .. import ops


def ema_decay_at(decay, t):
    """the decay of update ``t`` (1-based): ``min(decay, (1 + t) / (10 + t))`` -- the warm-up of the averaged model, so that a
    short run does not average its initial weights for ever.  A pure function."""
    return min(float(decay), (1.0 + t) / (10.0 + t))


class WeightAverage:
    """See the module docstring.  ``link``: a finalized ``Link`` (``to_gpu`` / ``finalize`` called); 0 < ``decay`` < 1."""

    def __init__(self, link, decay):
        if not 0.0 < float(decay) < 1.0:
            raise ValueError('the decay of a weight average lies in (0, 1), got %r' % (decay,))
        arena = link.arena
        if arena is None:
            raise ValueError('WeightAverage needs a finalized link: call to_gpu() / finalize() first')
        self.target = link
        self.hyperparam = SimpleNamespace(decay=float(decay))
        self.t = 0
        self._applied = False
        self._arena = arena
        self.avg = arena.data.clone()
        # float persistents only: BN's N is a Python int and is not averaged
        self._persistents = [(key[1:], getattr(l, n)) for key, l, n in link.namedpersistents()
                             if torch.is_tensor(getattr(l, n)) and getattr(l, n).dtype == torch.float32]
        self.avg_persistents = [v.clone() for _, v in self._persistents]
        self._jobs = ops.AverageJobs([(self.avg, arena.data)] + [(a, v) for a, (_, v) in zip(self.avg_persistents, self._persistents)])

    def update(self):
        """One launch: every averaged tensor moves towards its live value by ``1 - ema_decay_at(decay, t)``."""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('WeightAverage.update() counts its steps on the host: not inside a captured step')
        if self._applied:
            raise RuntimeError('WeightAverage.update() inside applied(): the model holds the average')
        self.t += 1
        ops.average_jobs(self._jobs, 'update', 1.0 - ema_decay_at(self.hyperparam.decay, self.t))      # 1 - d in double

    def _swap(self):
        if ops.in_step(self._arena.device):
            raise RuntimeError('WeightAverage.applied() between steps only: a step is live and trusts buffers derived from the weights')
        ops.join_side_stream(self._arena.device)
        ops.average_jobs(self._jobs, 'swap')

    @contextlib.contextmanager
    def applied(self):
        """Inside the block the model holds the averaged parameters and BN statistics (and this object the live ones)."""
        if self._applied:
            raise RuntimeError('WeightAverage.applied() is already active')
        self._swap()
        self._applied = True
        try:
            yield self
        finally:
            self._swap()
            self._applied = False

    # ---- checkpoints: the shape of GradientMethod's record, so runtime/checkpoint.py takes it as an optimiser ----------------
    def _keys(self):
        named = {id(p): k[1:] for k, p in self.target.namedparams()}
        return [named[id(p)] + '/avg' for p in self._arena.params], [k + '/avg' for k, _ in self._persistents]

    def state_dict(self):
        """``class``, ``t``, ``hyperparam`` and ``state``: the average of every parameter in its Chainer layout under
        ``<param path>/avg`` and of every averaged persistent under ``<persistent path>/avg``."""
        if self._applied:
            raise RuntimeError('WeightAverage.state_dict() inside applied()')
        arena = self._arena
        host = self.avg.detach().cpu().numpy()
        pkeys, skeys = self._keys()
        state = {}
        for key, p, o in zip(pkeys, arena.params, arena.offsets):
            state[key] = np.ascontiguousarray(p._to_logical(host[o:o + p.size].reshape(p.physical_shape)))
        for key, a in zip(skeys, self.avg_persistents):
            state[key] = a.detach().cpu().numpy()
        return {'class': type(self).__name__, 't': int(self.t), 'hyperparam': dict(vars(self.hyperparam)), 'state': state}

    def load_state_dict(self, sd):
        """Restore ``state_dict()``'s record; the buffers are written in place.  ValueError naming the first offending field or
        key where the class, the keys or a shape differ; nothing is changed then."""
        if self._applied:
            raise RuntimeError('WeightAverage.load_state_dict() inside applied()')
        if sd['class'] != type(self).__name__:
            raise ValueError('class: the checkpoint holds %s, this is a %s' % (sd['class'], type(self).__name__))
        arena = self._arena
        pkeys, skeys = self._keys()
        want = dict(zip(pkeys, [p.logical_shape for p in arena.params]))
        want.update(zip(skeys, [tuple(a.shape) for a in self.avg_persistents]))
        state = sd['state']
        odd = sorted(set(want) ^ set(state))
        if odd:
            raise ValueError('%s: %s' % (odd[0], 'not in the checkpoint' if odd[0] in want else 'no such averaged tensor in this model'))
        for key, shape in want.items():
            if tuple(np.shape(state[key])) != tuple(shape):
                raise ValueError('%s: shape %s in the checkpoint, %s in this model' % (key, tuple(np.shape(state[key])), tuple(shape)))
        host = np.zeros(arena.numel, np.float32)
        for key, p, o in zip(pkeys, arena.params, arena.offsets):
            host[o:o + p.size] = p._from_logical(np.asarray(state[key], dtype=np.float32)).ravel()
        self.avg.copy_(torch.from_numpy(host))
        for key, a in zip(skeys, self.avg_persistents):
            a.copy_(torch.from_numpy(np.ascontiguousarray(state[key], dtype=np.float32)))
        for k, v in dict(sd['hyperparam']).items():
            setattr(self.hyperparam, k, v)
        self.t = int(sd['t'])
