"""Stochastic depth (Huang et al. 2016) in the residual units: torchvision's ``StochasticDepth(mode='row')`` = timm's ``drop_path``.

Unit l of the L residual units of a backbone, in forward order, drops its main branch for a sample with probability
p_l = P l / (L - 1) (timm's linear rule: 0 for the first unit, P for the last; P for L == 1).  Per training forward and unit every
sample b draws keep_b ~ Bernoulli(1 - p_l); with r_b = keep_b / (1 - p_l) the unit's junction is relu(r_b * bn_n(c_n) + shortcut)
(functions/blocks.py: ResidualUnitFunction(..., drop=r), csrc/bn_pool.hip: loans_bn_*_rows_*).  The batch and running statistics
of bn_n are taken over all samples, as without it; in test mode nothing is drawn and nothing is scaled; a unit with p_l == 0 runs
the launches it always ran.

The draws are taken on the host from a stream of the object's own and go up as ONE table [units with p > 0][B] of r per training
forward, through the pinned staging ring, asynchronously on the step's stream: the step does not wait for the host."""
import weakref

import numpy as np
import torch

from ..runtime.core import config

CAPTURE_MESSAGE = ('stochastic depth is not built for a captured step: its keep table is drawn on the host and uploaded in every '
                   'step (use set_drop_path(0), or train without use_graph)')


def linear_rates(rate, n_units):
    """[p_0 .. p_{L-1}] of timm's linear rule"""
    if not 0.0 <= rate < 1.0:
        raise ValueError('the drop-path rate is a probability below 1: it must lie in [0, 1), got %r' % (rate,))
    if n_units < 1:
        raise ValueError('a backbone without residual units has no stochastic depth')
    if n_units == 1:
        return [float(rate)]
    return [float(rate) * l / (n_units - 1) for l in range(n_units)]


class DropPath:
    """The rates, the draw stream and the current keep table of one backbone."""

    def __init__(self, rate, n_units, seed=None):
        self.rate = float(rate)
        self.rates = linear_rates(rate, n_units)
        self.active = [l for l, p in enumerate(self.rates) if p > 0]           # the units that have a row of the table
        self.rows = {l: i for i, l in enumerate(self.active)}
        self.keep_prob = np.array([1.0 - self.rates[l] for l in self.active], np.float64)
        self.scale = np.array([1.0 / (1.0 - self.rates[l]) for l in self.active], np.float64).astype(np.float32)
        self.rng = np.random.RandomState(seed)
        self.table = None               # device [len(active)][B] float32: r of the forward that drew last
        self.owner = None               # weak reference to the link whose set_drop_path made this object (it draws)

    def sample(self, B, out=None):
        """one forward's table on the host: float32 [len(active)][B], 0 or fl(1 / (1 - p_l)); ONE call of the stream"""
        keep = self.rng.random_sample((len(self.active), int(B))) < self.keep_prob[:, None]
        if out is None:
            out = np.empty(keep.shape, np.float32)
        np.multiply(keep, self.scale[:, None], out=out)
        return out

    def draw(self, B, device):
        """draw the table of one training forward of B samples and upload it with one asynchronous copy on the current stream;
        sets and returns ``self.table`` (None where every rate is 0)"""
        if not self.active:
            return None
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(CAPTURE_MESSAGE)
        from ..common.datasets import resample
        n, B = len(self.active), int(B)
        # (a ring of its own: it waits for the copy of two forwards ago, never for the step)
        raw = resample.upload_staged(lambda host: self.sample(B, out=host.view(np.float32).reshape(n, B)), 4 * n * B, device, 'drop_path')
        self.table = raw.view(torch.float32).view(n, B)
        return self.table

    def vector(self, unit_index):
        """r of unit ``unit_index`` as the last ``draw`` left it (a row of the table), or None for a unit with p == 0"""
        row = self.rows.get(unit_index)
        if row is None:
            return None
        if self.table is None:
            raise RuntimeError('DropPath.draw has not run: the model that owns it draws once per training forward')
        return self.table[row]

    def state_dict(self):
        return {'rng': self.rng.get_state(), 'rate': self.rate, 'units': len(self.rates)}

    def load_state_dict(self, state):
        if int(state['units']) != len(self.rates) or float(state['rate']) != self.rate:
            raise ValueError('drop path: the checkpoint holds rate %r over %d units, this run %r over %d'
                             % (state['rate'], int(state['units']), self.rate, len(self.rates)))
        rng = state['rng']
        self.rng.set_state((rng[0], np.asarray(rng[1], dtype=np.uint32)) + tuple(rng[2:]))


def stage_units(stage):
    """the residual units of one stage (BasicBlock, BuildingBlock, chainercv ResBlock) in forward order"""
    names = stage.__dict__.get('_forward')
    return [getattr(stage, n) for n in names] if names is not None else list(stage.children())


def unit_vector(unit):
    """what a unit's ``__call__`` hands ``blocks.residual_unit`` as ``drop``: its r in training, None otherwise"""
    dp = unit.__dict__.get('drop_path')
    if dp is None or not config.train:
        return None
    return dp.vector(unit.__dict__['drop_slot'])


class DropPathOwner:
    """What ``sheep.resnet.ResNet``, ``ResNet50Layers`` and the localizers share: ``set_drop_path`` over the stages
    ``drop_path_stages()`` lists, and the draw their ``__call__`` makes."""
    drop_path = None

    def drop_path_stages(self):
        raise NotImplementedError

    def set_drop_path(self, rate, seed=None):
        """Stochastic depth at ``rate`` (P of the linear rule) over this model's residual units in forward order, drawn from a
        stream of its own seeded with ``seed``.  Returns the ``DropPath``; rate 0 removes it again and returns None."""
        units = [u for stage in self.drop_path_stages() for u in stage_units(stage)]
        dp = DropPath(rate, len(units), seed) if rate != 0 else None
        # one owner per unit: whoever held any of these units before -- this link, a backbone inside it, or a localizer AROUND it --
        # gives up its whole table (its other units too: their slots were counted with these), and stops drawing
        for link in self.links():
            if isinstance(link, DropPathOwner):
                link.clear_drop_path()
        for unit in units:
            previous = unit.__dict__.get('drop_path')
            owner = previous.owner() if previous is not None and previous.owner is not None else None
            if owner is not None:
                owner.clear_drop_path()
        if dp is not None:
            dp.owner = weakref.ref(self)
            for l, unit in enumerate(units):
                unit.__dict__['drop_path'], unit.__dict__['drop_slot'] = dp, l
            self.__dict__['drop_path'], self.__dict__['drop_units'] = dp, units
        return dp

    def clear_drop_path(self):
        """take this link's ``DropPath`` off it and off every unit that points to it"""
        dp = self.__dict__.get('drop_path')
        for unit in self.__dict__.get('drop_units', ()):
            if unit.__dict__.get('drop_path') is dp:
                unit.__dict__['drop_path'] = None
        self.__dict__['drop_path'], self.__dict__['drop_units'] = None, ()

    def draw_drop_path(self, B, device):
        dp = self.__dict__.get('drop_path')
        if dp is not None and config.train:
            dp.draw(B, device)


def refuse_captured_step(link):
    """RuntimeError, a sentence, where a step that is to be captured into a graph runs a model with a non-zero drop-path rate"""
    for l in link.links():
        dp = l.__dict__.get('drop_path')
        if isinstance(dp, DropPath) and dp.active:
            raise RuntimeError(CAPTURE_MESSAGE)
