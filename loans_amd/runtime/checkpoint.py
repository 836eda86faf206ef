"""Full-state checkpoints: everything a training run needs to continue as if it had not been interrupted.

A checkpoint of iteration ``i`` is ``checkpoint_<i>.npz`` in the log directory -- the COMMON file: a JSON ``meta`` record,
every model's parameters and persistents (``model/<name>/<Chainer key path>``, from ``state_dict_chainer()``), every
optimiser's record (``opt/<name>`` JSON: class, ``t``, hyper-parameters, stepped cold links; ``opt/<name>/<param path>/<m|v|vhat>``
one array per parameter and buffer) and rank 0's RANK RECORD -- plus, under data parallel, ``checkpoint_<i>.rank<r>.npz`` with
the rank record of every rank r > 0.  A rank record (``rank`` JSON + the arrays it points to) is what differs between ranks:
the state of every training iterator as of the last batch it handed out (shuffle stream, order, position, epoch values, the
dataset's draw stream) and NumPy's global stream.

Every file is written under a temporary name in the same directory and moved into place with ``os.replace``, and the common file
is written LAST, after a barrier behind the rank files: a checkpoint is complete when its common file and the
``world_size - 1`` rank files its ``meta`` asks for can all be opened.  Anything else -- a temporary file a killed process left, a
truncated file, a missing rank record -- is passed over by ``resolve``, which falls back to the newest complete checkpoint.  Older
checkpoints are deleted only after the new one is complete.  Nothing here touches the GPU but the copies ``state_dict()`` /
``load_state_dict()`` make; nothing here runs on an iteration that writes no checkpoint."""
import json
import os
import re
import zipfile

import numpy as np

FORMAT = 1
_COMMON = re.compile(r'^checkpoint_(\d+)\.npz$')
_ANY = re.compile(r'^checkpoint_(\d+)\.(?:rank\d+\.)?npz(?:\.tmp\d+)?$')
_UNREADABLE = (OSError, ValueError, KeyError, EOFError, zipfile.BadZipFile)


def common_path(log_dir, iteration):
    return os.path.join(log_dir, 'checkpoint_%d.npz' % iteration)


def rank_path(log_dir, iteration, rank):
    return os.path.join(log_dir, 'checkpoint_%d.rank%d.npz' % (iteration, rank))


# ---- nested Python state <-> one JSON string + arrays ---------------------------------------------------------------------
def pack(obj, prefix, arrays):
    """``obj`` (dicts, lists, tuples, numbers, strings, None, arrays) as something ``json`` takes; arrays go to
    ``arrays[prefix/...]`` and leave a pointer behind, tuples are marked so that ``unpack`` gives tuples back"""
    if isinstance(obj, np.ndarray):
        arrays[prefix] = obj
        return {'__array__': prefix}
    if isinstance(obj, dict):
        return {str(k): pack(v, '%s/%s' % (prefix, k), arrays) for k, v in obj.items()}
    if isinstance(obj, tuple):
        return {'__tuple__': [pack(v, '%s/%d' % (prefix, i), arrays) for i, v in enumerate(obj)]}
    if isinstance(obj, list):
        return [pack(v, '%s/%d' % (prefix, i), arrays) for i, v in enumerate(obj)]
    if isinstance(obj, np.generic):
        return obj.item()
    return obj


def unpack(obj, arrays):
    if isinstance(obj, dict):
        if '__array__' in obj:
            return np.asarray(arrays[obj['__array__']])
        if '__tuple__' in obj:
            return tuple(unpack(v, arrays) for v in obj['__tuple__'])
        return {k: unpack(v, arrays) for k, v in obj.items()}
    if isinstance(obj, list):
        return [unpack(v, arrays) for v in obj]
    return obj


def _json(record):
    return np.array(json.dumps(record, default=str))


# ---- files ----------------------------------------------------------------------------------------------------------------
def write_atomic(path, arrays):
    """``np.savez(path, **arrays)`` that is either there in full or not at all: a process killed while it writes leaves a
    ``<path>.tmp<pid>`` behind, which nothing reads, and whatever was at ``path`` before"""
    tmp = '%s.tmp%d' % (path, os.getpid())
    with open(tmp, 'wb') as f:
        np.savez(f, **arrays)
        f.flush()
        os.fsync(f.fileno())
    os.replace(tmp, path)


def read_meta(path):
    """the ``meta`` record of a common file (the archive's directory and that one member are read, nothing else)"""
    with np.load(path) as handle:
        return json.loads(str(handle['meta'][()]))


def is_complete(path):
    """(True, meta) if ``path`` is a common file that opens and every rank file its meta asks for opens too, else
    (False, the reason)"""
    try:
        meta = read_meta(path)
        if meta.get('format') != FORMAT:
            return False, 'format %r, this code reads format %d' % (meta.get('format'), FORMAT)
        found = _COMMON.match(os.path.basename(path))
        for rank in range(1, int(meta['world_size'])):
            record = rank_path(os.path.dirname(path), int(found.group(1)) if found else meta['iteration'], rank)
            if not os.path.exists(record):
                return False, 'the record of rank %d (%s) is missing' % (rank, os.path.basename(record))
            with np.load(record) as handle:
                json.loads(str(handle['rank'][()]))
    except _UNREADABLE as e:
        return False, '%s: %s' % (type(e).__name__, e)
    return True, meta


def list_checkpoints(log_dir):
    """[(iteration, common file)] of ``log_dir``, newest first; temporary and rank files are not checkpoints"""
    found = [(int(m.group(1)), os.path.join(log_dir, m.group(0))) for m in map(_COMMON.match, os.listdir(log_dir)) if m]
    return sorted(found, reverse=True)


def resolve(path, log=print):
    """The checkpoint ``--resume PATH`` means: the file itself, or for a directory the newest complete checkpoint in it -- an
    incomplete or unreadable one is named through ``log`` and the one before it taken.  ValueError if there is none."""
    if os.path.isdir(path):
        for _, candidate in list_checkpoints(path):
            ok, why = is_complete(candidate)
            if ok:
                return candidate
            log('resume: %s is not a complete checkpoint (%s): falling back to the one before it' % (candidate, why))
        raise ValueError('no complete checkpoint in %s' % path)
    if not os.path.isfile(path):
        raise ValueError('%s: no such checkpoint file or log directory' % path)
    ok, why = is_complete(path)
    if not ok:
        raise ValueError('%s is not a complete checkpoint (%s)' % (path, why))
    return path


def prune(log_dir, keep):
    """delete all but the newest ``keep`` complete checkpoints -- their common file first, so that what is left of one is never
    taken for a checkpoint -- and with them the rank and temporary files of iterations older than the oldest one kept"""
    kept = []
    for iteration, path in list_checkpoints(log_dir):
        if len(kept) < max(int(keep), 1) and is_complete(path)[0]:
            kept.append(iteration)
    if not kept:
        return
    stale = sorted((name for name in os.listdir(log_dir) if _ANY.match(name) and int(_ANY.match(name).group(1)) < min(kept)),
                   key=lambda name: not _COMMON.match(name))
    for name in stale:
        try:
            os.remove(os.path.join(log_dir, name))
        except OSError:
            pass


def write_checkpoint(log_dir, iteration, common, record, meta, rank=0, world=1, keep=2, barrier=None):
    """The file protocol, for any payload.  ``common``: the arrays every rank shares (a callable is evaluated on rank 0 only),
    ``record``: this rank's state (``pack``-able).  Ranks > 0 write their rank file, ``barrier()`` -- every rank calls it --,
    then rank 0 writes the common file with its own record inside and prunes, and a second ``barrier()`` holds the others until
    it has.  Returns the common file's path."""
    arrays = {}
    packed = pack(record, 'rank', arrays)
    arrays['rank'] = _json(packed)
    if rank > 0:
        os.makedirs(log_dir, exist_ok=True)
        write_atomic(rank_path(log_dir, iteration, rank), arrays)
    if barrier is not None:
        barrier()
    path = common_path(log_dir, iteration)
    if rank == 0:
        meta = dict(meta, format=FORMAT, iteration=int(iteration), world_size=int(world))
        arrays.update(common() if callable(common) else common)
        arrays['meta'] = _json(meta)
        write_atomic(path, arrays)
        prune(log_dir, keep)
    if barrier is not None:
        barrier()           # no rank goes on (or ends, and is resumed) before the checkpoint is complete
    return path


def read_record(path, rank=0):
    """the rank record of ``rank`` of the checkpoint whose common file is ``path``"""
    if rank > 0:
        iteration = int(_COMMON.match(os.path.basename(path)).group(1))
        path = rank_path(os.path.dirname(path), iteration, rank)
    with np.load(path) as handle:
        packed = json.loads(str(handle['rank'][()]))
        return unpack(packed, handle)


# ---- the training state ---------------------------------------------------------------------------------------------------
def _common_arrays(models, optimizers):
    arrays = {}
    for name, model in models.items():
        for k, v in model.state_dict_chainer().items():
            arrays['model/%s/%s' % (name, k)] = v
    for name, optimizer in optimizers.items():
        sd = optimizer.state_dict()
        for k, v in sd.pop('state').items():
            arrays['opt/%s/%s' % (name, k)] = v
        arrays['opt/%s' % name] = _json(sd)
    return arrays


def save_checkpoint(log_dir, iteration, models, optimizers, iterators, meta, comm=None, keep=2):
    """Write the checkpoint of ``iteration``: ``models`` / ``optimizers`` / ``iterators`` are ``{name: object}``; ``meta`` holds
    what the caller wants back (epoch, elapsed time, arguments).  Under data parallel every rank calls this at the same
    iteration: model and optimiser state are rank 0's (identical on all ranks but for the BN running statistics, which are
    local and of which rank 0's are kept), the rank records are everyone's own."""
    rank, world = (comm.rank, comm.size) if comm is not None else (0, 1)
    record = {'iterators': {name: it.state_dict() for name, it in iterators.items()}, 'numpy': np.random.get_state()}
    return write_checkpoint(log_dir, iteration, lambda: _common_arrays(models, optimizers), record, meta, rank, world, keep,
                            comm.barrier if comm is not None and world > 1 else None)


def load_checkpoint(path, models, optimizers, iterators, comm=None):
    """Restore what ``save_checkpoint`` wrote into live objects of the same construction and return ``meta``.  Every rank
    reads the common file and its own record.  Models are loaded strictly -- a checkpoint is not a pretrained model --;
    a run of another world size is refused.  Call it between steps: everything the bf16 arm derives from the fp32 masters
    (shadows, fragment-order packs, data-gradient re-packs) is rebuilt from them by the next step's ``begin_step``."""
    rank, world = (comm.rank, comm.size) if comm is not None else (0, 1)
    with np.load(path) as handle:
        meta = json.loads(str(handle['meta'][()]))
        if int(meta['world_size']) != world:
            raise ValueError(world_size_message(meta['world_size'], world))
        for name, model in models.items():
            prefix = 'model/%s/' % name
            model.load_state_dict_chainer({k[len(prefix):]: handle[k] for k in handle.files if k.startswith(prefix)}, strict=True)
        for name, optimizer in optimizers.items():
            prefix = 'opt/%s/' % name
            sd = json.loads(str(handle['opt/%s' % name][()]))
            sd['state'] = {k[len(prefix):]: handle[k] for k in handle.files if k.startswith(prefix)}
            optimizer.load_state_dict(sd)
    record = read_record(path, rank)
    if set(record['iterators']) != set(iterators):
        raise ValueError('iterators: the checkpoint holds %s, the run has %s' % (sorted(record['iterators']), sorted(iterators)))
    for name, it in iterators.items():
        it.load_state_dict(record['iterators'][name])
    state = record['numpy']
    np.random.set_state((state[0], np.asarray(state[1], dtype=np.uint32)) + tuple(state[2:]))
    return meta


def world_size_message(saved, now):
    return 'the checkpoint was written by a run on %d GPU(s): resume it with --gpus %d, not %d (resuming at another world ' \
           'size is not built)' % (int(saved), int(saved), int(now))


# ---- the trainers' side of --resume ----------------------------------------------------------------------------------------
def _plain(value):
    return json.loads(json.dumps(value, default=str))


def check_arguments(saved, args, fixed, silent=(), defaults=None):
    """``saved``: the arguments in a checkpoint's meta; ``args``: this run's namespace.  ValueError listing EVERY argument of
    ``fixed`` that differs, with both values; returns one line per other argument that differs (``silent`` ones left out):
    those are taken from the new command line.  ``defaults``: values for arguments ``saved`` does not hold -- options that did
    not exist when the checkpoint was written, which ran at their defaults."""
    if defaults:
        saved = dict(_plain(dict(defaults)), **saved)
    now = {k: _plain(getattr(args, k)) for k in dir(args) if not k.startswith('_')}
    wrong = ['%s: %r in the checkpoint, %r now' % (k, saved.get(k), now.get(k)) for k in fixed if saved.get(k) != now.get(k)]
    if wrong:
        raise ValueError('--resume: these arguments must equal the checkpointed run\'s -- ' + '; '.join(wrong))
    return ['resume: %s was %r, is now %r' % (k, saved.get(k), now[k]) for k in sorted(now)
            if k not in fixed and k not in silent and k in saved and saved[k] != now[k]]


FLAGS = {'checkpoint_interval': 0, 'checkpoint_keep': 2, 'resume': None}     # the three options and their defaults
SILENT = ('resume', 'log_dir', 'ln', 'flat_log_dir', 'gpu')         # differ on every resume: never reported


def add_arguments(parser, defaults=FLAGS):
    """the three options; ``defaults``: a mapping of their defaults, or ``argparse.SUPPRESS`` for a parser whose namespace
    class holds them"""
    default = defaults.get if isinstance(defaults, dict) else (lambda name: defaults)
    parser.add_argument("--checkpoint-interval", type=int, default=default('checkpoint_interval'),
                        help="write a full-state checkpoint (models, optimisers, iterators, random streams) after every N-th iteration and after the last one (default 0: off)")
    parser.add_argument("--checkpoint-keep", type=int, default=default('checkpoint_keep'), help="keep the newest K checkpoints (default 2)")
    parser.add_argument("--resume", default=default('resume'), metavar='PATH',
                        help="continue the run of this checkpoint file, or of the newest complete checkpoint in this log directory, in its log directory")


def resolve_resume(args, fixed, log=print, world=None, defaults=None):
    """``args.resume`` -> the common file it means (``resolve``), its arguments checked against ``args`` (``check_arguments``;
    ``world``: the world size to hold against the checkpoint's where it is not ``args.gpus``; ``defaults``: see there).  Returns (meta, the lines of
    the arguments that changed); ValueError for a path that is no checkpoint and for arguments that must not change."""
    args.resume = resolve(args.resume, log)
    meta = read_meta(args.resume)
    if world is not None and int(meta['world_size']) != int(world):
        raise ValueError(world_size_message(meta['world_size'], world))
    if 'gpus' in fixed and world is None and int(meta['world_size']) != int(getattr(args, 'gpus', 1)):
        raise ValueError(world_size_message(meta['world_size'], getattr(args, 'gpus', 1)))
    return meta, check_arguments(meta['args'], args, [k for k in fixed if k != 'gpus'], SILENT + ('gpus',), defaults)


def due(iteration, interval, last):
    """whether ``iteration`` writes a checkpoint: a function of the iteration alone (and of whether it is the run's last), so
    that all ranks of a data parallel run agree"""
    return interval > 0 and (iteration % interval == 0 or last)


def plain_arguments(args):
    """the namespace as ``meta`` keeps it"""
    return {k: _plain(getattr(args, k)) for k in dir(args) if not k.startswith('_')}


def read_log(log_dir, iteration):
    """the entries of ``log_dir``'s ``log`` file up to ``iteration``: a resumed run keeps them and appends"""
    path = os.path.join(log_dir, 'log')
    if not os.path.exists(path):
        return []
    with open(path) as f:
        return [entry for entry in json.load(f) if entry.get('iteration', 0) <= iteration]
