"""CPU: the facts of a plane that infer_volume and VolumePipeline share (inference/driver.py): slices per model call, the
model's extra arguments, the output datasets and the result dictionary.  Nothing here touches the GPU."""
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


class _Group:
    def __init__(self):
        self.created = []

    def create_dataset(self, name, **kw):
        self.created.append((name, kw))

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
