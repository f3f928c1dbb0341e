"""CPU: the facts of a plane that infer_volume and VolumePipeline share (inference/driver.py): slices per model call, the
model's extra arguments, the output datasets, the tables and attributes that the stages store and the result dictionary.
Nothing here touches the GPU."""
import types

import numpy as np


def _dv(hp, wp, scale=1):
    return types.SimpleNamespace(padded_shape=lambda axis: (hp, wp), scale=scale)


def test_slices_per_call():
    from empanada_amd.inference.driver import slices_per_call
    assert slices_per_call(_dv(96, 96), 'xy', 96 * 96 - 1) == 1                 # a plane larger than batch_pixels
    assert slices_per_call(_dv(2048, 2048), 'xy', 1 << 20) == 1
    assert slices_per_call(_dv(96, 64), 'xy', 7 * 96 * 64) == 7                 # an exact multiple
    assert slices_per_call(_dv(96, 64), 'xy', 7 * 96 * 64 - 1) == 6
    assert slices_per_call(_dv(96, 64), 'xy', 7 * 96 * 64 + 1) == 7
    assert slices_per_call(_dv(96, 64, scale=2), 'xy', 8 * 96 * 64) == 2        # the output is 2 x 2 the input
    assert slices_per_call(_dv(96, 64, scale=4), 'xy', 8 * 96 * 64) == 1


def test_model_args():
    from empanada_amd.inference.driver import model_args
    assert model_args(types.SimpleNamespace(), 2) == ()
    assert model_args(types.SimpleNamespace(coarse_boundaries=True), 3) == (3, False)
    assert model_args(types.SimpleNamespace(coarse_boundaries=False), 2) == (2, True)


class _Dataset:
    def __init__(self, written, name):
        self.written, self.name = written, name

    def __setitem__(self, key, value):
        assert key is Ellipsis
        self.written[self.name] = value


class _Group:
    """a store that records what is created and written; refuse_empty: one that cannot hold a zero-row array"""

    def __init__(self, attrs=None, refuse_empty=False):
        self.created, self.written, self.refuse_empty = [], {}, refuse_empty
        if attrs is not None:
            self.attrs = attrs

    def create_dataset(self, name, **kw):
        if self.refuse_empty and kw['shape'][0] == 0:
            raise ValueError(f"{name}: zero-length dimension")
        self.created.append((name, kw))
        return _Dataset(self.written, name)

    def __getitem__(self, name):
        return ('array', name)


def test_open_datasets(monkeypatch):
    import torch
    from empanada_amd.inference.driver import open_datasets
    barriers = []
    monkeypatch.setattr(torch.distributed, 'barrier', lambda group=None: barriers.append(group))
    labels, thing, shape = [1, 2, 5], [1, 5], (4, 6, 8)
    g = _Group()
    ds = open_datasets(g, labels, thing, {1: 'mito', 2: 'er'}, shape, 0, 1, None)
    assert ds == {1: ('array', 'mito_pred'), 2: ('array', 'er_pred'), 5: ('array', '5_pred')}     # no name: the id
    assert [n for n, _ in g.created] == ['mito_pred', 'er_pred', '5_pred']
    assert [kw['dtype'] for _, kw in g.created] == [np.uint32, np.uint8, np.uint32]
    assert all(kw == dict(shape=shape, dtype=kw['dtype'], overwrite=True, chunks=(1, None, None)) for _, kw in g.created)
    assert barriers == []
    g0, g1 = _Group(), _Group()
    open_datasets(g0, labels, thing, None, shape, 0, 2, 'grp')
    ds = open_datasets(g1, labels, thing, None, shape, 1, 2, 'grp')
    assert len(g0.created) == 3 and g1.created == []                             # rank 0 creates, every rank opens
    assert ds == {c: ('array', f'{c}_pred') for c in labels}
    assert barriers == ['grp', 'grp']
    assert open_datasets(None, labels, thing, None, shape, 0, 1, None) == {1: None, 2: None, 5: None}


def test_result_keys():
    from empanada_amd.inference.driver import result
    res = result({1: 'v'}, (0, 4), {1: 2}, {1: None})
    assert res == {'volumes': {1: 'v'}, 'z_range': (0, 4), 'instances': {1: 2}, 'datasets': {1: None}}
    res = result({1: 'v'}, (0, 4), {1: 2}, {1: None}, pipeline={'overlap': True, 'head_bytes': 64})
    assert 'windows' not in res and 'head_bytes' not in res and res['pipeline']['head_bytes'] == 64
    res = result({1: 'v'}, (0, 4), {1: 2}, {1: None}, windows={'xy': 3}, head_bytes=np.int64(96))
    assert res['windows'] == {'xy': 3} and res['head_bytes'] == 96 and type(res['head_bytes']) is int
    assert 'pipeline' not in res
    res = result({1: 'v'}, (0, 4), {1: 2}, {1: None}, windows={}, head_bytes=0, pipeline={})
    assert res['windows'] == {} and res['head_bytes'] == 0 and res['pipeline'] == {}


def _tables():
    """two keys with two datasets each, the second key without rows"""
    full = {'a_vertices': np.arange(12, dtype=np.int32).reshape(4, 3), 'a_objects': np.arange(10, dtype=np.int64).reshape(2, 5)}
    none = {'b_vertices': np.zeros((0, 3), np.int32), 'b_objects': np.zeros((0, 5), np.int64)}
    return {'a': full, 'b': none}, {'a': 2, 'b': 0}


def test_write_tables_rank0_writes_every_array():
    from empanada_amd.inference.driver import _write_tables
    arrays, rows = _tables()
    g = _Group(attrs={'kept': 1, 'meshes': 'old'})
    assert _write_tables(g, None, arrays, rows, {'meshes': {'axes': 'zyx'}}) == set()
    assert [n for n, _ in g.created] == ['a_vertices', 'a_objects', 'b_vertices', 'b_objects']
    flat = {n: a for named in arrays.values() for n, a in named.items()}
    for n, kw in g.created:
        a = flat[n]
        assert kw == dict(shape=a.shape, dtype=a.dtype, overwrite=True, chunks=(max(a.shape[0], 1),) + a.shape[1:])
    assert dict(g.created)['a_vertices']['chunks'] == (4, 3) and dict(g.created)['b_objects']['chunks'] == (1, 5)
    assert sorted(g.written) == ['a_objects', 'a_vertices']                      # an array without rows is created only
    assert all(g.written[n] is flat[n] for n in g.written)
    assert g.attrs == {'kept': 1, 'meshes': {'axes': 'zyx'}}                     # what was there stays, a same key is replaced
    one = {'t': {'t_objects': np.zeros((3,), np.int64)}}                         # one-dimensional: the chunk is the rows alone
    g = _Group()
    assert _write_tables(g, None, one, {'t': 3}, {'x': 1}) == set()
    assert g.created[0][1]['chunks'] == (3,) and not hasattr(g, 'attrs')         # an `out` without attributes gets none


def test_write_tables_store_without_zero_row_arrays():
    import pytest
    from empanada_amd.inference.driver import _write_tables
    arrays, rows = _tables()
    g = _Group(attrs={}, refuse_empty=True)
    assert _write_tables(g, None, arrays, rows, {'meshes': 1}) == {'b'}         # that key only
    assert [n for n, _ in g.created] == ['a_vertices', 'a_objects'] and sorted(g.written) == ['a_objects', 'a_vertices']
    assert g.attrs == {'meshes': 1}
    # rows decide, not the array that failed: a key that has rows re-raises
    g = _Group(attrs={}, refuse_empty=True)
    with pytest.raises(ValueError, match='b_vertices: zero-length'):
        _write_tables(g, None, arrays, {'a': 2, 'b': 1}, {'meshes': 1})
    assert 'meshes' not in g.attrs


def test_write_tables_other_ranks_take_rank0s_answer(monkeypatch):
    import torch
    from empanada_amd.inference import driver, sharded
    arrays, rows = _tables()
    sent = {}

    def broadcast(flag, src=0, group=None):
        assert src == 0 and group is None
        if me[0] == 0:
            sent['flag'] = list(flag)
        else:
            flag[:] = sent['flag']

    me = [0]
    monkeypatch.setattr(sharded, '_world', lambda group=None: (me[0], 2))
    monkeypatch.setattr(torch.distributed, 'broadcast_object_list', broadcast)
    g0, g1 = _Group(attrs={}, refuse_empty=True), _Group(attrs={}, refuse_empty=True)
    assert driver._write_tables(g0, None, arrays, rows, {'meshes': 1}) == {'b'}
    assert sent['flag'] == [['b']]
    me[0] = 1
    assert driver._write_tables(g1, None, arrays, rows, {'meshes': 1}) == {'b'}
    assert g1.created == [] and g1.written == {} and g1.attrs == {}              # rank 0 creates and writes, the others open


def test_update_attrs(tmp_path):
    from empanada_amd.inference.driver import _update_attrs
    from empanada_amd.zarr_utils import ZarrV2Group
    g = _Group(attrs={'multiscales': [1], 'objects': 'old'})
    _update_attrs(g, {'objects': {'columns': ['label']}})
    assert g.attrs == {'multiscales': [1], 'objects': {'columns': ['label']}}
    bare = _Group()
    _update_attrs(bare, {'objects': 1})
    assert not hasattr(bare, 'attrs')
    z = ZarrV2Group(str(tmp_path / 'store.zarr'))
    _update_attrs(z, {'multiscales': [1]})
    _update_attrs(z, {'objects': 2})
    assert ZarrV2Group(str(tmp_path / 'store.zarr'), mode='r').attrs == {'multiscales': [1], 'objects': 2}   # on disk
