"""One rank's share of a dataset under data parallel: ``ShardedDataset(dataset, rank, world, pad)`` is a view over the base
indices ``rank, rank + world, rank + 2 world, ...``.

``pad=True`` (training): every shard has ``ceil(n / world)`` entries, the missing ones taken by wrapping round --
entry ``j`` is base index ``(rank + j * world) % n`` --, so for a given batch size every rank's iterator makes the same
``(epoch, is_new_epoch)`` sequence and no rank reaches a collective its peers do not.  Fewer than ``world`` examples are
seen twice per epoch.  ``pad=False`` (validation): no example is repeated; shards may differ in length by one and may be empty,
so what is computed over them must be summed, not averaged per shard.

Whatever the base offers of ``get_examples`` / ``decode_batch`` / ``finish_batch`` / ``device_batch`` / ``reseed`` / ``draw_state`` / ``set_draw_state`` the view offers
too, with mapped indices -- and nothing the base does not have --, and the base's frame ``cache``, which is keyed by base
indices like everything a mapped call hands the base, so ``MultithreadIterator(device=...)`` treats a shard exactly
like its base."""


class ShardedDataset:

    _INDEXED = ('get_examples', 'decode_batch', 'device_batch')       # first argument: a list of indices
    _PLAIN = ('finish_batch', 'reseed', 'draw_state', 'set_draw_state')
    _ATTRIBUTES = ('cache',)

    def __init__(self, dataset, rank, world, pad):
        n = len(dataset)
        if n == 0:
            raise ValueError('cannot shard an empty dataset')
        if world < 1 or not 0 <= rank < world:
            raise ValueError('rank %d of %d' % (rank, world))
        self.dataset, self.rank, self.world, self.pad = dataset, int(rank), int(world), bool(pad)
        if pad:
            self._indices = [(self.rank + j * self.world) % n for j in range(-(-n // self.world))]
        else:
            self._indices = list(range(self.rank, n, self.world))

    def base_index(self, i):
        return self._indices[i]

    def __len__(self):
        return len(self._indices)

    def __getitem__(self, i):
        return self.dataset[self._indices[i]]

    def get_example(self, i):
        return self.dataset.get_example(self._indices[i])

    def __getattr__(self, name):
        # only reached for names the view itself does not define
        if name in ShardedDataset._INDEXED or name in ShardedDataset._PLAIN or name in ShardedDataset._ATTRIBUTES:
            method = getattr(self.__dict__['dataset'], name)        # AttributeError where the base has none: hasattr() is False
            if name not in ShardedDataset._INDEXED:
                return method
            indices = self.__dict__['_indices']
            return lambda idx, *args, **kwargs: method([indices[int(i)] for i in idx], *args, **kwargs)
        raise AttributeError(name)
