"""TEST INFRASTRUCTURE: the dict-backed group of tests/memh5.py with the rest of the h5py interface that the
statistics containers (tombo_stats.ModelStats / LevelStats / PerReadStats) and the REFERENCE's use: `items()`,
`close`, `flush`, `attrs.get`, a dataset created from a shape and filled through `ds[...] = values`.  The build
image has no HDF5 library, so the containers are exercised against this and their tree is compared with the tree the
reference's containers leave on the same stand-in (tests/golden/gen_golden_stat_store.py)."""
import numpy as np

import memh5


class _Items(dict):
    """MemGroup keeps its children in the attribute `items`; h5py groups have the method: both"""
    def __call__(self):
        return dict.items(self)


class StoreDataset(memh5.MemDataset):
    def __setitem__(self, key, value):
        assert key is Ellipsis
        self.data = np.array(value, dtype=self.data.dtype)


class StoreGroup(memh5.MemGroup):
    def __init__(self):
        memh5.MemGroup.__init__(self)
        self.items = _Items()
        self.closed = False

    def create_group(self, name):
        if name in self.items:
            raise ValueError('Unable to create group (name already exists)')
        self.items[name] = StoreGroup()
        return self.items[name]

    def create_dataset(self, name, shape=None, dtype=None, data=None, **kw):
        d = StoreDataset(np.empty(shape, dtype=dtype) if data is None else data, **kw)
        self.items[name] = d
        return d

    def close(self):
        self.closed = True

    def flush(self):
        pass


def flat_tree(node):
    """memh5.tree with every value an array (what an .npz keeps); object arrays (read ids) as str arrays"""
    out = {}
    for k, v in memh5.tree(node).items():
        v = np.asarray(v)
        out[k] = v.astype(str) if v.dtype == object else v
    return out


def same_array(a, b):
    """equal dtype, shape and values (NaN equal to NaN), record arrays field by field"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.names:
        return all(same_array(a[n], b[n]) for n in a.dtype.names)
    return np.array_equal(a, b, equal_nan=a.dtype.kind == 'f')
