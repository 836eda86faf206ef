"""Launch plans of the convolution wrappers, pinned on the CPU (no device, no built library).

The public wrappers of loans_amd/ops.py -- conv_fprop, conv_fprop_pair, conv_fprop_affine, conv_dgrad, _conv_wgrad and the
bf16-storage bodies behind them -- run on CPU tensors of zeros against a recording stand-in for the library.  What they ask the
autotuner (mode string, candidate tuple in order, cold timing), every library call (entry point, integer arguments, descriptor
flags and tile, every pointer as the NAME of its tensor), the keys they leave in geo.tuned and what they add to EVENT_LOG /
FLOP_COUNT / CLASS_COUNT is compared with tests/golden/conv_launch_plans.json, recorded by tests/golden/make_conv_plans_golden.py.

Under the test session's TUNE_POLICY = 'fixed' the mode string and the candidate tuple decide which kernel every GPU parity
test launches and whether a committed tile table still applies: a reordered tuple or a renamed suffix passes every other CPU test.
"""
import ctypes as C
import json
import os

import pytest
import torch

from loans_amd import _lib, ops

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'conv_launch_plans.json')
BF16 = torch.bfloat16
STREAM = 7
ARMS = {'f32': ('f32', 'f32'), 'bf16c': ('bf16', 'f32'), 'bf16s': ('bf16', 'bf16')}
_DT = {torch.float32: 'f32', BF16: 'bf16', torch.float64: 'f64'}

# problem shapes (B, H, W, Cin, Cout, k, stride, pad): the smallest that reach each branch
S33 = (2, 16, 16, 64, 64, 3, 1, 1)           # halo and weight-stationary offers
S33S2 = (2, 16, 16, 64, 128, 3, 2, 1)        # four stride-parity classes, the class-launch offer
S11S2 = (2, 16, 16, 64, 128, 1, 2, 0)        # an empty stride-parity class
S11 = (2, 16, 16, 64, 256, 1, 1, 0)          # the LOANS_TILE_PW offer, cold timing
DEEP = (2, 8, 8, 512, 512, 3, 1, 1)          # the split-K offer
TAIL = (6, 40, 40, 64, 128, 3, 1, 1)         # the fine-tail offer: 300 tiles of 64 x 64 on 256 CUs, 44 left over, 18 K chunks in 4 slices
STEM = (2, 64, 64, 3, 64, 7, 2, 3)           # dense=True
CROP = (2, 16, 16, 4, 128, 4, 2, 1)          # the gradient w.r.t. 4-channel crops


class Recorder:
    """stands in for the ctypes library: every attribute is a callable that returns 0 and records its name and arguments, read by
    the prototypes of _lib.SIGNATURES (pointer -> label of the tensor, POINTER(IgemmDesc) -> flags and tile, integers as they are)"""

    def __init__(self):
        self.reset({}, [])

    def reset(self, named, descs):
        self.calls, self.named, self.descs = [], named, descs
        self.scratch, self.other = [], []

    def label(self, ptr):
        if not ptr:
            return None
        for name, t in list(self.named.items()) + [('s%d' % i, t) for i, t in enumerate(self.scratch)]:
            off = ptr - t.data_ptr()
            if 0 <= off < max(1, t.numel() * t.element_size()):
                return name if off == 0 else '%s+%d' % (name, off)
        if ptr not in self.other:           # (a tensor the wrappers keep themselves: the slab workspace, the stem's weight mask)
            self.other.append(ptr)
        return 'other%d' % self.other.index(ptr)

    def desc(self, d):
        for name, known in self.descs:
            if d is known:
                return [name, d.flags, d.tile]
        return [[d.oy0, d.ox0, d.ntaps], d.flags, d.tile]

    def arg(self, kind, a, last):
        if kind is C.c_void_p:
            return 'st%d' % a if last else self.label(a)
        if kind is C.POINTER(_lib.IgemmDesc):
            return self.desc(a._obj) if hasattr(a, '_obj') else [self.desc(d) for d in a]
        if kind is C.POINTER(C.c_void_p):
            return [self.label(p) for p in a]
        if kind is C.POINTER(C.c_int32):
            return list(a)
        return a

    def __getattr__(self, name):
        kinds = _lib.SIGNATURES[name]

        def call(*args):
            assert len(args) == len(kinds), name
            self.calls.append([name] + [self.arg(k, a, i == len(kinds) - 1 and k is C.c_void_p)
                                        for i, (k, a) in enumerate(zip(kinds, args))])
            return 4096 if name == 'loans_wgrad_bf16s_ws_floats' else 0      # (a workspace need: the slab launches are reached)
        return call


class _Event:
    def __init__(self, enable_timing=False):
        pass

    def record(self):
        pass


class _Props:
    multi_processor_count = 256


def install(mp):
    """the stand-ins, all through `mp` (a pytest MonkeyPatch): undone on exit, with the tile picks the cases made"""
    rec = Recorder()
    mp.setattr(_lib, 'load', lambda: rec)
    mp.setattr(ops, '_stream', lambda: STREAM)
    mp.setattr(torch.cuda, 'get_device_properties', lambda device=None: _Props)
    mp.setattr(torch.cuda, 'current_device', lambda: 0)
    mp.setattr(torch.cuda, 'is_current_stream_capturing', lambda: False)
    mp.setattr(torch.cuda, 'Event', _Event)
    for name, value in (('ASYNC_WGRAD', False), ('TUNE_POLICY', 'fixed'), ('TUNE_SALT', '0'), ('TUNE_VERBOSE', False),
                        ('AUTOTUNE', True), ('TIMED_PICKS', ops.TIMED_PICKS), ('PW_PACK_CALLS', ops.PW_PACK_CALLS),
                        ('_TUNE_CACHE', {}), ('_TUNE_LOADED', {}), ('_weight_preps', {}), ('_step_arenas', {}), ('_zero_pools', {}),
                        ('_wgrad_ws', {}), ('_cold', {}), ('EVENT_LOG', None), ('FLOP_COUNT', None), ('CLASS_COUNT', None),
                        ('COMPUTE', 'f32'), ('STORAGE', 'f32')):
        mp.setattr(ops, name, value)
    tune = rec.tune = []
    real_tuned_tile, real_empty, real_zeros = ops._tuned_tile, ops._empty, ops._zeros_f64

    def tuned_tile(geo, mode, run, candidates, cold=False):
        miss = geo.tuned.get(mode) is None
        tile = real_tuned_tile(geo, mode, run, candidates, cold)
        tune.append([mode, list(candidates), bool(cold), miss, tile])
        return tile

    def empty(shape, device, dtype):
        t = real_empty(shape, device, dtype).fill_(1)       # (1: an output the wrapper cleared itself reads 0 afterwards)
        rec.scratch.append(t)           # (kept alive for the case: no address comes back under another name)
        return t

    def zeros_f64(shape, device):
        t = real_zeros(shape, device)
        rec.scratch.append(t)
        return t

    times = iter(range(1 << 30))

    def time_call(fn, reps=5, cold=False):
        """TUNE_POLICY = 'time' on the CPU: every candidate's closure runs once, the 'time' is a fixed shuffle of the call number"""
        fn()
        i = next(times)
        return float((i * 7 + 3) % 11) + i * 1e-3

    mp.setattr(ops, '_tuned_tile', tuned_tile)
    mp.setattr(ops, '_empty', empty)
    mp.setattr(ops, '_zeros_f64', zeros_f64)
    mp.setattr(ops, '_time_call', time_call)
    return rec


# --------------------------------------------------------------------------------------------------------------------------- #
# cases: (name, arm, function of a Case) -- the function makes its tensors through the Case (which names them) and calls a wrapper
# --------------------------------------------------------------------------------------------------------------------------- #
class Case:
    """the tensors and descriptors of one call; the recorder knows their names from the moment they are made"""

    def __init__(self, arm, rec):
        self.s16 = arm == 'bf16s'
        rec.reset({}, [])
        self.named, self.descs = rec.named, rec.descs

    def geo(self, shape, tag=''):
        g = ops.ConvGeometry(*shape[:8], dense=len(shape) > 8)
        self.descs += [('fwd' + tag, g.fwd)] + [('cls%d%s' % (i, tag), d) for i, (d, _, _) in enumerate(g.dgrad)]
        return g

    def t(self, name, numel_or_shape, dtype=None):
        if dtype is None:
            dtype = BF16 if self.s16 else torch.float32
        # zeros, but for the two tensors a wrapper may clear or copy itself (the empty stride class, split-K): told apart afterwards
        t = self.named[name] = torch.full(numel_or_shape if isinstance(numel_or_shape, tuple) else (numel_or_shape,),
                                          {'out': 1.0, 'addend': 2.0}.get(name, 0.0), dtype=dtype)
        return t

    def x(self, g, name='x', dtype=None):
        return self.t(name, (g.B, g.Hp, g.Wp, 3) if g.dense else (g.B, g.H, g.W, g.Cin), dtype)

    def w(self, g, name='w'):
        return self.t(name, (g.Cout, g.k, g.kwp, 3) if g.dense else (g.Cout, g.k, g.k, g.Cin), torch.float32)

    def y(self, g, name='gy', dtype=None):
        return self.t(name, (g.B, g.Ho, g.Wo, g.Cout), dtype)

    def stats(self, g, name='stats'):
        return self.t(name, (ops.STATS_REPLICAS, 2, g.Cout), torch.float64)

    def bn(self, channels, name='bn'):
        st = ops.BNState.__new__(ops.BNState)
        buf = self.t(name, (4, channels), torch.float32)
        st.mean, st.rstd, st.scale, st.shift, st.count = buf[0], buf[1], buf[2], buf[3], 1
        return st


def fprop(shape, stats=False, relu_in=False, bias=False, addend=None, out=False, tile=0, out_bf16=False, xdtype=None):
    """addend: None, 'own' (a tensor of its own) or 'out' (the addend IS the output tensor)"""
    def run(c):
        g = c.geo(shape)
        o = c.y(g, 'out') if (out or addend == 'out') else None
        return ops.conv_fprop(c.x(g, dtype=xdtype), c.w(g), g, out=o, bias=c.t('bias', g.Cout, torch.float32) if bias else None,
                              stats=c.stats(g) if stats else None, relu_in=relu_in,
                              addend=o if addend == 'out' else (c.y(g, 'addend') if addend else None), tile=tile, out_bf16=out_bf16)
    return run


def pair(shape_a, shape_b, stats=False, tile=0):
    def run(c):
        ga, gb = c.geo(shape_a), c.geo(shape_b, '_b')
        return ops.conv_fprop_pair(c.x(ga), c.w(ga, 'w_a'), c.w(gb, 'w_b'), ga, gb,
                                   c.stats(ga, 'stats_a') if stats else None, c.stats(gb, 'stats_b') if stats else None, tile)
    return run


def affine(shape, stats=False):
    def run(c):
        g = c.geo(shape)
        return ops.conv_fprop_affine(c.x(g), c.bn(g.Cin), c.w(g), g, stats=c.stats(g) if stats else None)
    return run


def dgrad(shape, out=False, mask_ref=False, addend=None, addend_mask_ref=False, tile=0, bn_sums=False, gydtype=None):
    def run(c):
        g = c.geo(shape)
        gx = lambda name: c.t(name, (g.B, g.H, g.W, g.Cin), torch.float32 if g.Cin == 4 else None)      # noqa: E731
        o = gx('out') if (out or addend == 'out') else None
        return ops.conv_dgrad(c.y(g, dtype=gydtype), c.w(g), g, out=o, mask_ref=gx('mask_ref') if mask_ref else None,
                              addend=o if addend == 'out' else (gx('addend') if addend else None),
                              addend_mask_ref=gx('addend_mask_ref') if addend_mask_ref else None, tile=tile,
                              bn_sums=(gx('y'), c.bn(g.Cin)) if bn_sums else None)
    return run


def wgrad(shape, relu_in=False, splits=0, tile=0, stream=None, in_affine=False, xdtype=None, gydtype=None):
    def run(c):
        g = c.geo(shape)
        return ops._conv_wgrad(c.x(g, dtype=xdtype), c.y(g, dtype=gydtype), c.w(g, 'dw'), g, relu_in, splits, tile, stream=stream,
                               in_affine=c.bn(g.Cin) if in_affine else None)
    return run


def _cases():
    out = []
    add = lambda name, arm, fn, **sw: out.append((name, arm, fn, sw))      # noqa: E731
    dense = STEM + (True,)
    for arm in ('f32', 'bf16s'):
        for tag, shape in (('s33', S33), ('s33s2', S33S2), ('s11s2', S11S2), ('s11', S11), ('deep', DEEP)):
            add('fprop_stats_%s_%s' % (tag, arm), arm, fprop(shape, stats=True))
            add('dgrad_%s_%s' % (tag, arm), arm, dgrad(shape))
            add('wgrad_%s_%s' % (tag, arm), arm, wgrad(shape))
        add('fprop_plain_s33_%s' % arm, arm, fprop(S33))
        add('fprop_relu_s33_%s' % arm, arm, fprop(S33, relu_in=True, stats=True))
        add('fprop_bias_s33_%s' % arm, arm, fprop(S33, bias=True))
        add('fprop_addend_out_s33_%s' % arm, arm, fprop(S33, addend='own', out=True))
        add('fprop_all_s33_%s' % arm, arm, fprop(S33, stats=True, relu_in=True, bias=True, addend='own'))
        add('fprop_plain_s11_%s' % arm, arm, fprop(S11))
        add('fprop_relu_s11_%s' % arm, arm, fprop(S11, relu_in=True))
        add('fprop_plain_deep_%s' % arm, arm, fprop(DEEP))
        add('fprop_addend_deep_%s' % arm, arm, fprop(DEEP, addend='own', stats=True))
        add('fprop_tile2_s33_%s' % arm, arm, fprop(S33, stats=True, tile=2))
        add('fprop_tile_splitk_deep_%s' % arm, arm, fprop(DEEP, stats=True, bias=True, addend='own', tile=3 | (4 << 8)))
        add('fprop_tile_splitk_addend_is_out_deep_%s' % arm, arm, fprop(DEEP, addend='out', tile=3 | (2 << 8)))
        add('dgrad_out_s33_%s' % arm, arm, dgrad(S33, out=True))
        add('dgrad_mask_s33_%s' % arm, arm, dgrad(S33, mask_ref=True))
        add('dgrad_mask_addend_s33_%s' % arm, arm, dgrad(S33, mask_ref=True, addend='own'))
        add('dgrad_mask_addend_is_out_s33_%s' % arm, arm, dgrad(S33, mask_ref=True, addend='out'))
        add('dgrad_addend_mask_s33_%s' % arm, arm, dgrad(S33, addend='own', addend_mask_ref=True))
        add('dgrad_bn_sums_s33_%s' % arm, arm, dgrad(S33, bn_sums=True))
        add('dgrad_bn_sums_deep_%s' % arm, arm, dgrad(DEEP, bn_sums=True))
        add('dgrad_addend_s33s2_%s' % arm, arm, dgrad(S33S2, addend='own'))
        add('dgrad_addend_is_out_s33s2_%s' % arm, arm, dgrad(S33S2, addend='out'))
        add('dgrad_mask_s33s2_%s' % arm, arm, dgrad(S33S2, mask_ref=True))
        add('dgrad_addend_s11s2_%s' % arm, arm, dgrad(S11S2, addend='own'))
        add('dgrad_addend_out_s11s2_%s' % arm, arm, dgrad(S11S2, addend='own', out=True))
        add('dgrad_addend_is_out_s11s2_%s' % arm, arm, dgrad(S11S2, addend='out'))
        add('dgrad_addend_is_out_deep_%s' % arm, arm, dgrad(DEEP, addend='out'))
        add('dgrad_tile3_s33s2_%s' % arm, arm, dgrad(S33S2, addend='own', tile=3))
        add('dgrad_tile_splitk_deep_%s' % arm, arm, dgrad(DEEP, mask_ref=True, addend='own', tile=3 | (4 << 8)))
        add('dgrad_tile_splitk_s33s2_%s' % arm, arm, dgrad(S33S2, addend_mask_ref=True, addend='own', tile=3 | (2 << 8)))
        add('wgrad_relu_s33_%s' % arm, arm, wgrad(S33, relu_in=True))
        add('wgrad_splits_s33_%s' % arm, arm, wgrad(S33, splits=4))
        add('wgrad_splits_relu_deep_%s' % arm, arm, wgrad(DEEP, relu_in=True, splits=3))
        add('wgrad_tile_s33_%s' % arm, arm, wgrad(S33, tile=3 | (6 << 8)))
        add('wgrad_tile1_splits_s33_%s' % arm, arm, wgrad(S33, splits=3, tile=1))
        add('crop_dgrad_%s' % arm, arm, dgrad(CROP, gydtype=torch.float32))
    add('wgrad_side_stream_s33_f32', 'f32', wgrad(S33, stream=9))         # (the launch goes to a stream given by handle)
    # the dense stem on the three arms
    add('fprop_stats_stem_f32', 'f32', fprop(dense, stats=True))
    add('fprop_plain_stem_f32', 'f32', fprop(dense))
    add('fprop_stats_stem_bf16c', 'bf16c', fprop(dense, stats=True, out_bf16=True))
    add('fprop_stats_stem_bf16c_f32out', 'bf16c', fprop(dense, stats=True))
    add('fprop_tile_stem_bf16c', 'bf16c', fprop(dense, stats=True, out_bf16=True, tile=ops.TILE_STEM))
    add('fprop_stats_stem_bf16s', 'bf16s', fprop(dense, stats=True))
    add('fprop_stats_stem_bf16s_f32frames', 'bf16s', fprop(dense, stats=True, out_bf16=True, xdtype=torch.float32))
    add('wgrad_stem_f32', 'f32', wgrad(dense))
    add('wgrad_tile3_stem_f32', 'f32', wgrad(dense, tile=3))
    add('wgrad_tile_stem_f32', 'f32', wgrad(dense, tile=ops.TILE_STEM))
    add('wgrad_stem_bf16c', 'bf16c', wgrad(dense))
    add('wgrad_stem_g16_bf16c', 'bf16c', wgrad(dense, gydtype=BF16))
    add('wgrad_stem_g16_bf16s', 'bf16s', wgrad(dense, xdtype=torch.float32))
    add('wgrad_stem_bf16s', 'bf16s', wgrad(dense))
    add('wgrad_tile_stem_bf16s', 'bf16s', wgrad(dense, tile=ops.TILE_STEM))
    # the bf16 compute arm on fp32 tensors
    add('fprop_stats_s33_bf16c', 'bf16c', fprop(S33, stats=True))
    add('fprop_stats_deep_bf16c', 'bf16c', fprop(DEEP, stats=True))
    add('dgrad_s33s2_bf16c', 'bf16c', dgrad(S33S2))
    add('dgrad_deep_bf16c', 'bf16c', dgrad(DEEP))
    add('wgrad_s33_bf16c', 'bf16c', wgrad(S33))
    add('wgrad_g16_s33_bf16c', 'bf16c', wgrad(S33, gydtype=BF16))
    # two convolutions of one input; BN + ReLU on load
    wide = S11S2[:4] + (256,) + S11S2[5:]
    add('pair_f32', 'f32', pair(S11S2, wide))
    add('pair_stats_f32', 'f32', pair(S11S2, wide, stats=True))
    add('pair_stats_s33s2_f32', 'f32', pair(S33S2, S33S2, stats=True))
    add('pair_tile_f32', 'f32', pair(S11S2, wide, stats=True, tile=18))
    add('pair_bf16s', 'bf16s', pair(S11S2, S11S2))
    add('pair_stats_bf16s', 'bf16s', pair(S11S2, S11S2, stats=True))
    add('pair_stats_s33s2_bf16s', 'bf16s', pair(S33S2, S33S2, stats=True))
    add('pair_tile_bf16s', 'bf16s', pair(S11S2, S11S2, stats=True, tile=7))
    add('affine_bf16s', 'bf16s', affine(S11))
    add('affine_stats_bf16s', 'bf16s', affine(S11, stats=True))
    add('fprop_tile_pw_s11_bf16s', 'bf16s', fprop(S11, stats=True, tile=ops.TILE_PW))
    add('wgrad_affine_s11_bf16s', 'bf16s', wgrad(S11, in_affine=True))
    add('wgrad_affine_tile_s11_bf16s', 'bf16s', wgrad(S11, in_affine=True, tile=1 | (5 << 8)))
    add('crop_dgrad_g16_bf16s', 'bf16s', dgrad(CROP, gydtype=BF16))
    add('crop_dgrad_mask_addend_g16_bf16s', 'bf16s', dgrad(CROP, gydtype=BF16, mask_ref=True, addend='own'))
    add('crop_dgrad_addend_mask_f32', 'f32', dgrad(CROP, addend='own', addend_mask_ref=True))     # (not the dedicated kernel's)
    add('dgrad_tile_classes_s33s2_f32', 'f32', dgrad(S33S2, mask_ref=True, addend='own', tile=1 | ops.TILE_CLASSES))
    add('wgrad_no_slabs_s33_bf16s', 'bf16s', wgrad(S33), WGRAD_SLABS=False)
    add('wgrad_no_slabs_tile_s33_bf16s', 'bf16s', wgrad(S33, tile=5 | (3 << 8)), WGRAD_SLABS=False)
    # LOANS_TILE_FINETAIL: offered (mode suffix _ft) with SPLITK and FINETAIL on, two launches in the event log when it slices
    add('fprop_stats_tail_f32', 'f32', fprop(TAIL, stats=True))
    add('fprop_plain_tail_f32', 'f32', fprop(TAIL))
    add('fprop_addend_tail_f32', 'f32', fprop(TAIL, addend='own'))                # (no offer: the sliced rows are summed into zeros)
    add('fprop_tile_finetail_tail_f32', 'f32', fprop(TAIL, stats=True, tile=ops.TILE_FINETAIL))
    add('fprop_tile_finetail_dma_tail_f32', 'f32', fprop(TAIL, tile=ops.TILE_FINETAIL | 16))
    add('fprop_tile_finetail_s33_f32', 'f32', fprop(S33, tile=ops.TILE_FINETAIL))    # (8 tiles on 256 CUs: nothing to slice, one launch)
    add('fprop_tile_split_tail_f32', 'f32', fprop(TAIL, tile=6))                   # (LOANS_TILE_SPLIT: its launch count)
    add('fprop_stats_tail_bf16c', 'bf16c', fprop(TAIL, stats=True))               # (fp32 arithmetic only)
    return out


CASES = _cases()

# passes over the cases: name -> (module switches, which cases).  Both SPLITK states run everything; a pass with one A/B switch
# off, and the pass on the TIMING autotuner (every candidate's tuning closure runs), take the cases that the switch reaches.
_OFF = {
    'HALO': ('fprop_stats_s33_bf16s', 'fprop_relu_s33_bf16s', 'dgrad_s33_bf16s', 'dgrad_bn_sums_s33_bf16s'),
    'PW': ('fprop_stats_s11_bf16s', 'fprop_plain_s11_bf16s'),
    'CLASS_LAUNCH': ('dgrad_s33s2_f32', 'dgrad_addend_s33s2_f32'),
    'FINETAIL': ('fprop_stats_deep_f32', 'fprop_plain_deep_f32', 'fprop_stats_tail_f32', 'fprop_plain_tail_f32'),
    'STEM_DIRECT': ('fprop_stats_stem_f32', 'fprop_stats_stem_bf16c', 'fprop_stats_stem_bf16s', 'wgrad_stem_f32', 'wgrad_stem_bf16s',
                    'wgrad_stem_g16_bf16c'),
}
_TIMED = ('fprop_stats_s33_f32', 'fprop_stats_deep_f32', 'fprop_stats_tail_f32', 'fprop_stats_s33_bf16s', 'fprop_stats_s11_bf16s', 'fprop_stats_deep_bf16s',
          'fprop_stats_stem_f32', 'fprop_stats_stem_bf16c', 'fprop_stats_stem_bf16s', 'pair_stats_f32', 'pair_stats_bf16s',
          'dgrad_s33s2_f32', 'dgrad_deep_f32', 'dgrad_bn_sums_s33_f32', 'dgrad_s33s2_bf16s', 'dgrad_deep_bf16s', 'dgrad_bn_sums_s33_bf16s',
          'dgrad_s33s2_bf16c', 'wgrad_s33_f32', 'wgrad_splits_s33_f32', 'wgrad_s33_bf16s', 'wgrad_stem_f32', 'wgrad_stem_bf16s',
          'wgrad_stem_g16_bf16c', 'wgrad_no_slabs_s33_bf16s')
PASSES = {'splitk_off': ({'SPLITK': False}, None), 'splitk_on': ({'SPLITK': True}, None)}
PASSES.update({k.lower() + '_off': ({'SPLITK': True, k: False}, names) for k, names in _OFF.items()})
PASSES['timed'] = ({'SPLITK': True, 'TUNE_POLICY': 'time'}, _TIMED)


def _call(mp, rec, arm, fn, switches, accounting):
    """one call of a wrapper on fresh tensors of zeros: what it asked the autotuner, what it launched, allocated and returned"""
    case = Case(arm, rec)
    del rec.tune[:]
    with mp.context() as m:
        for k, v in switches.items():
            m.setattr(ops, k, v)
        if accounting:
            log, flops, classes = [], {}, {}
            m.setattr(ops, 'EVENT_LOG', log)
            m.setattr(ops, 'FLOP_COUNT', flops)
            m.setattr(ops, 'CLASS_COUNT', classes)
        with ops.precision(*ARMS[arm]):
            r = fn(case)
    got = {'tune': list(rec.tune), 'calls': rec.calls, 'allocs': [[_DT[t.dtype]] + list(t.shape) for t in rec.scratch],
           'returns': [[rec.label(t.data_ptr()), float(t.flatten()[0])] for t in (r if isinstance(r, tuple) else (r,)) if t is not None]}
    if accounting:      # bench.py reads (tag, flops, ev0, ev1, launches, convolutions, (read, written)): here without the events
        got['acct'] = {'events': [list(e[:2]) + [e[4], e[5], list(e[6])] for e in log], 'flops': flops, 'classes': classes}
    return got, (case, rec.scratch)


def record_case(mp, rec, arm, fn, switches):
    """Three calls on one problem shape: the first resolves the tile, the second is the tuned fast path (no tune request; the same
    launches unless the first one timed candidates), the third runs with EVENT_LOG / FLOP_COUNT / CLASS_COUNT switched on."""
    ops._TUNE_CACHE.clear()
    ops._wgrad_ws.clear()
    first, keep1 = _call(mp, rec, arm, fn, switches, False)          # (keep*: alive until the case is over, so no address repeats)
    out = dict(first, tuned=sorted([ops._tune_key_str(k), m, t] for k, v in ops._TUNE_CACHE.items() for m, t in v.items()))
    again, keep2 = _call(mp, rec, arm, fn, switches, False)
    assert again.pop('tune') == [], 'the tuned call asked the autotuner again'
    if again != {k: first[k] for k in again}:
        out['again'] = again
    logged, keep3 = _call(mp, rec, arm, fn, switches, True)
    out['acct'] = logged.pop('acct')
    assert logged.pop('tune') == [] and logged == again, 'accounting changed what the tuned call does'
    return out


def record_pass(mp, name):
    switches, names = PASSES[name]
    rec = install(mp)
    return {case: record_case(mp, rec, arm, fn, dict(switches, **sw)) for case, arm, fn, sw in CASES if names is None or case in names}


def dumps(plans):
    """the fixture's text: one line per case"""
    lines = []
    for p, cases in plans.items():
        body = ',\n'.join('  %s: %s' % (json.dumps(c), json.dumps(r, separators=(',', ':'))) for c, r in cases.items())
        lines.append(' %s: {\n%s\n }' % (json.dumps(p), body))
    return '{\n%s\n}\n' % ',\n'.join(lines)


@pytest.fixture(scope='module')
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_every_pass_and_wrapper_has_cases(golden):
    assert list(golden) == list(PASSES)
    for name, (_, names) in PASSES.items():
        assert list(golden[name]) == [c[0] for c in CASES if names is None or c[0] in names], name
    assert {n for v in _OFF.values() for n in v} | set(_TIMED) <= {c[0] for c in CASES}
    entry = {call[0] for case in golden['splitk_on'].values() for call in case['calls']}
    # one entry point that only each wrapper reaches: conv_fprop / conv_dgrad (fp32), their bf16-storage bodies, the two pairs,
    # the class launch, the 4-channel gradient, the weight gradients of the three arms and of the slab workspace
    assert entry >= {'loans_igemm_f32', 'loans_igemm_bf16_f32', 'loans_igemm_bf16s', 'loans_igemm_pair_f32', 'loans_igemm_pair_bf16s',
                     'loans_igemm_finalize_f32', 'loans_igemm_bf16s_splitk', 'loans_igemm_finalize_bf16', 'loans_igemm_classes_f32',
                     'loans_dgrad_c4_f32', 'loans_dgrad_c4_bf16_f32', 'loans_repack_dgrad_f32', 'loans_repack_dgrad_bf16',
                     'loans_wgrad_f32', 'loans_wgrad_bf16_f32', 'loans_wgrad_bf16s', 'loans_wgrad_bf16s_ws',
                     'loans_wgrad_bf16s_affine_ws', 'loans_pw_pack_bf16', 'loans_cast_bf16', 'loans_mul_f32'}
    modes = lambda p, c: [t[0] for t in golden[p][c]['tune']]      # noqa: E731
    for case in ('fprop_stats_tail_f32', 'fprop_plain_tail_f32'):     # the fine-tail offer: there with SPLITK and FINETAIL on only
        assert all('_ft' in m for m in modes('splitk_on', case)) and ops.TILE_FINETAIL in golden['splitk_on'][case]['tune'][0][1]
        assert not any('_ft' in m for m in modes('splitk_off', case) + modes('finetail_off', case))
    assert golden['splitk_on']['fprop_tile_finetail_tail_f32']['acct']['events'][0][2] == 2       # launches: it slices
    assert golden['splitk_on']['fprop_tile_finetail_s33_f32']['acct']['events'][0][2] == 1
    flags = {call[-2][1] & ops.F_AFFINE_IN for case in golden['splitk_on'].values() for call in case['calls'] if call[0] == 'loans_igemm_bf16s'}
    assert flags == {0, ops.F_AFFINE_IN}          # conv_fprop_affine


@pytest.mark.parametrize('name', list(PASSES))
def test_conv_launch_plans(name, golden, monkeypatch):
    got = json.loads(json.dumps(record_pass(monkeypatch, name)))
    want = golden[name]
    for case in want:
        for part in want[case]:
            assert got[case].get(part) == want[case][part], '%s / %s / %s' % (name, case, part)
        assert got[case] == want[case], '%s / %s' % (name, case)
