"""The cases of tests/conv_desc/test_desc_cpu.py and tests/golden/make_conv_desc_golden.py: base descriptors from
ops.ConvGeometry (no library, no device) and single mutations of each -- every int32 field to a list of values, every flag
bit and pair of bits, every tile id in its OR-ed forms, every pointer absent or misaligned in turn, the tap list bent -- plus
a few named ones.  A case is (name, descs, focus, splits, Cout_b, have, misaligned, w_have): the single-descriptor checks
get descs[focus], loans_igemm_classes_f32's gets them all."""
import copy
import itertools

from loans_amd import ops

FIELDS = ['B', 'inH', 'inW', 'Cin', 'outH', 'outW', 'Cout', 'gridH', 'gridW', 'osy', 'osx', 'oy0', 'ox0', 'isy', 'isx',
          'ntaps', 'flags', 'tile']
INT_MAX = 2 ** 31 - 1
MAX_TAPS = 64
# one column per check, in the order desc_cpu.cpp prints them
CHECKS = ['igemm_f32', 'igemm_bf16_f32', 'igemm_pair_f32', 'igemm_classes_f32', 'igemm_bf16s', 'igemm_pair_bf16s',
          'igemm_bf16s_splitk', 'igemm_finalize_f32', 'igemm_finalize_bf16', 'wgrad_f32', 'wgrad_bf16_f32', 'wgrad_bf16s',
          'wgrad_bf16s_ws', 'wgrad_bf16s_affine_ws', 'wgrad_bf16s_ws_floats', 'halo16_covers', 'pw16_covers',
          'stem7_wgrad_bf16_covers']
CAN_ERANGE = [c for c in CHECKS if c not in ('igemm_finalize_f32', 'halo16_covers', 'pw16_covers', 'stem7_wgrad_bf16_covers')]
# the forward checks that must reject the descriptor whose output stride overflowed the parent's `int` arithmetic
FORWARD = ['igemm_f32', 'igemm_bf16_f32', 'igemm_bf16s']

# pointer bits: CONV_P_* of conv_desc.h, and desc_cpu.cpp's bit for the array of class weights
P_NAMES = ['in', 'w', 'out', 'bias', 'stats', 'ref', 'addend', 'w2', 'out2', 'stats2', 'partial', 'ws', 'affine', 'w_list']
ALL_PTRS = (1 << len(P_NAMES)) - 1
ALIGNED = {'in': 1, 'w': 2, 'out': 4, 'ws': 2048}       # the pointers the stem launchers want 16-byte aligned

GEOMETRIES = [(2, 16, 16, 64, 64, 3, 1, 1), (2, 16, 16, 64, 128, 3, 2, 1), (2, 16, 16, 64, 256, 1, 1, 0),
              (2, 11, 11, 64, 64, 4, 2, 1), (2, 16, 16, 64, 64, 7, 1, 3), (2, 11, 11, 8, 16, 3, 1, 1),
              (2, 16, 16, 4, 128, 4, 2, 1)]
DENSE_STEM = (2, 64, 64, 3, 64, 7, 2, 3)
CLASSES_OF = GEOMETRIES[1]


def fields(d):
    return [int(getattr(d, f)) for f in FIELDS]


def taps(d):
    return [int(v) for v in d.dy], [int(v) for v in d.dx]


class Desc:
    """a loans_igemm_desc as plain Python values (mutable, copyable)"""

    def __init__(self, d):
        self.f = dict(zip(FIELDS, fields(d)))
        self.dy, self.dx = taps(d)

    def ints(self):
        return [self.f[k] for k in FIELDS] + self.dy + self.dx


def bases():
    """(name, [Desc], focus)"""
    out = []
    for g in GEOMETRIES:
        geo = ops.ConvGeometry(*g)
        out.append(('fwd%s' % (g,), [Desc(geo.fwd)], 0))
        if g == CLASSES_OF:
            cls = [Desc(d) for d, _, _ in geo.dgrad]
            assert len(cls) == 4
            for c in range(4):
                out.append(('dgrad%s.class%d' % (g, c), cls, c))
    geo = ops.ConvGeometry(*DENSE_STEM, dense=True)
    d = Desc(geo.fwd)
    d.f['flags'] = geo.base_flags
    out.append(('dense_stem%s' % (DENSE_STEM,), [d], 0))
    return out


def _case(name, descs, focus, have=ALL_PTRS, mis=0, w_have=None, splits=2):
    d = descs[focus]
    return (name, descs, focus, splits, d.f['Cout'], have, mis, (1 << len(descs)) - 1 if w_have is None else w_have)


def _mutated(descs, focus, **kw):
    descs = list(descs)
    d = descs[focus] = copy.deepcopy(descs[focus])
    for k, v in kw.items():
        if k in ('dy', 'dx'):
            setattr(d, k, v)
        else:
            d.f[k] = v
    return descs


def cases():
    out = []
    for bname, descs, focus in bases():
        b = descs[focus]
        dense = bool(b.f['flags'] & 64)
        out.append(_case(bname, descs, focus))
        for f in FIELDS:
            v0 = b.f[f]
            for v in (0, -1, v0 - 1, v0 + 1, 0x40000001, INT_MAX - 7, INT_MAX):
                if v != v0:
                    out.append(_case('%s %s=%d' % (bname, f, v), _mutated(descs, focus, **{f: v}), focus))
        bits = [1 << i for i in range(11)]
        for fl in bits + [x | y for x, y in itertools.combinations(bits, 2)]:
            out.append(_case('%s flags|=%d' % (bname, fl), _mutated(descs, focus, flags=b.f['flags'] | fl), focus))
        for t in range(64):
            for tile in [t, t + 16, t + 32] + [t | s << 8 for s in (1, 2, 64, 255)]:
                out.append(_case('%s tile=%d' % (bname, tile), _mutated(descs, focus, tile=tile), focus))
        for i, p in enumerate(P_NAMES):
            out.append(_case('%s no %s' % (bname, p), descs, focus, have=ALL_PTRS & ~(1 << i)))
        for c in range(len(descs)):
            out.append(_case('%s no w[%d]' % (bname, c), descs, focus, w_have=((1 << len(descs)) - 1) & ~(1 << c)))
        # the stem launchers' alignment rules, on the tile that has them
        for p, bit in ALIGNED.items():
            out.append(_case('%s misaligned %s' % (bname, p), descs, focus, mis=bit))
            out.append(_case('%s tile=10 misaligned %s' % (bname, p), _mutated(descs, focus, tile=10), focus, mis=bit))
        n = b.f['ntaps']
        t = n // 2
        out.append(_case('%s tap %d moved' % (bname, t), _mutated(descs, focus, dx=b.dx[:t] + [b.dx[t] + 1] + b.dx[t + 1:]), focus))
        out.append(_case('%s taps reversed' % bname,
                         _mutated(descs, focus, dy=b.dy[:n][::-1] + b.dy[n:], dx=b.dx[:n][::-1] + b.dx[n:]), focus))
        if dense:
            out.append(_case('%s negative tap' % bname, _mutated(descs, focus, dy=[-1] + b.dy[1:]), focus))
            # the flags and tiles the stem launchers take, together
            for fl in (64, 64 | 2, 64 | 4, 64 | 128, 64 | 128 | 2 | 4, 64 | 1, 64 | 256):
                out.append(_case('%s tile=10 flags=%d' % (bname, fl), _mutated(descs, focus, tile=10, flags=fl), focus))
        # the frame of test_host_cpu.py::test_argument_validation_without_gpu, beyond 32-bit indexing
        big = dict(B=1 << 20, inH=1 << 10, inW=1 << 10, outH=1 << 10, outW=1 << 10, gridH=1 << 10, gridW=1 << 10)
        out.append(_case('%s oversized frame' % bname, _mutated(descs, focus, **big), focus))
        out.append(_case('%s oversized frame flags|=1024' % bname, _mutated(descs, focus, flags=b.f['flags'] | 1024, **big), focus))
        out.append(_case('%s oversized frame, input only' % bname, _mutated(descs, focus, B=1 << 20, inH=1 << 10, inW=1 << 10), focus))
        # an output stride whose product with the grid wraps a 32-bit int: (3 - 1) * 0x40000001 < 0
        out.append(_case('%s gridH=3 osy=0x40000001' % bname, _mutated(descs, focus, gridH=3, osy=0x40000001), focus))
        out.append(_case('%s gridW=3 osx=0x40000001' % bname, _mutated(descs, focus, gridW=3, osx=0x40000001), focus))
    return out


def stdin_text(cs):
    lines = []
    for _, descs, focus, splits, cout_b, have, mis, w_have in cs:
        ints = [len(descs), focus, splits, cout_b, have, mis, w_have]
        for d in descs:
            ints += d.ints()
        lines.append(' '.join(map(str, ints)))
    return '\n'.join(lines) + '\n'
