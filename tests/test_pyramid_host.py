"""CPU: what the label pyramid decides without a device -- the argument checks of emp_label_pool_mode
(csrc/emp_pool.hip; every refusal is EMP_EINVAL before any launch, the pointers handed over are host buffers that are
never read), pyramid.normalize / plan / multiscales, the group attributes of the zarr store, and the refusals of
_hip.pool_labels and infer_volume(pyramid=)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

EINVAL = -1


@pytest.fixture(scope='module')
def lib():
    from empanada_amd import _hip
    return _hip.load()


@pytest.fixture(scope='module')
def buf():
    b = ctypes.create_string_buffer(1 << 12)
    return ctypes.addressof(b), b


def test_abi_refuses_bad_arguments(lib, buf):
    a, _ = buf
    good = dict(src=a, item=4, D=3, H=4, W=5, fz=2, fy=2, fx=2, dst=a + 2048)

    def call(**kw):
        v = {**good, **kw}
        return lib.emp_label_pool_mode(v['src'], v['item'], v['D'], v['H'], v['W'], v['fz'], v['fy'], v['fx'], v['dst'], None)

    for kw, word in ((dict(item=2), b'item'), (dict(item=0), b'item'), (dict(item=8), b'item'),
                     (dict(fz=0), b'factor'), (dict(fy=3), b'factor'), (dict(fx=-2), b'factor'), (dict(fx=4), b'factor'),
                     (dict(fz=1, fy=1, fx=1), b'(1, 1, 1)'),
                     (dict(D=-1), b'negative'), (dict(H=-4), b'negative'), (dict(W=-5), b'negative'),
                     (dict(src=None), b'null'), (dict(dst=None), b'null'), (dict(src=None, dst=None), b'null'),
                     (dict(src=a + 2), b'misaligned'), (dict(dst=a + 2049), b'misaligned'),
                     (dict(D=1 << 30, H=1 << 30, W=1 << 30), b'64-bit')):
        assert call(**kw) == EINVAL, kw
        assert word in lib.emp_last_error(), (kw, lib.emp_last_error())
    # bad arguments are refused whatever the sizes; an empty volume is a successful no-op, with or without pointers
    assert call(D=0, item=2) == EINVAL and call(W=0, fx=3) == EINVAL
    for kw in (dict(D=0), dict(H=0), dict(W=0), dict(D=0, H=0, W=0), dict(D=0, src=None, dst=None),
               dict(W=0, item=1, fz=1, fy=1)):
        assert call(**kw) == 0, kw


def test_wrapper_refusals_need_no_device():
    from empanada_amd import _hip
    host = torch.zeros((2, 4, 6), dtype=torch.uint8)
    with pytest.raises(ValueError, match='on the GPU'):
        _hip.pool_labels(host)
    with pytest.raises(ValueError, match='on the GPU'):
        _hip.pool_labels(host.numpy())
    with pytest.raises(ValueError, match='on the GPU'):
        _hip.pool_labels(host.to(torch.int32), (1, 2, 2))
    assert _hip.pooled_shape((5, 7, 9), (2, 2, 2)) == (3, 4, 5)
    assert _hip.pooled_shape((5, 7, 9), (1, 2, 1)) == (5, 4, 9)
    if torch.cuda.is_available():
        for bad in (torch.float32, torch.int64, torch.int16, torch.int8):
            with pytest.raises(ValueError, match='dtype'):
                _hip.pool_labels(torch.zeros((2, 4, 6), dtype=bad, device='cuda'))


def test_normalize():
    from empanada_amd.inference import pyramid as P
    assert P.normalize(None) == []
    assert P.normalize(1) == [(2, 2, 2)]
    assert P.normalize(8) == [(2, 2, 2)] * 8
    assert P.normalize(np.int64(3)) == [(2, 2, 2)] * 3
    assert P.normalize([(1, 2, 2), (2, 2, 2)]) == [(1, 2, 2), (2, 2, 2)]
    assert P.normalize(((2, 1, 1),)) == [(2, 1, 1)]
    assert P.normalize([[1, 2, 2], np.array([2, 2, 1])]) == [(1, 2, 2), (2, 2, 1)]
    for bad in (0, 9, -1, True, False, 2.0, 'auto', '2', b'2', [], [(1, 1, 1)], [(2, 3, 2)], [(2, 2)], [(2, 2, 2, 2)],
                [(2, 2, 0)], [(2, 2, 2.0)], [(2, 2, True)], [2, 2, 2], (2, 2, 2), [(2, 2, 2)] * 9, [None], {'levels': 2},
                object()):
        with pytest.raises(ValueError, match='pyramid'):
            P.normalize(bad)


def test_plan_shapes_are_ceilings_of_the_level_below():
    from empanada_amd.inference import pyramid as P
    lv = P.plan((5, 7, 9), P.normalize(2), 0, 5)
    assert [v['shape'] for v in lv] == [(3, 4, 5), (2, 2, 3)]
    assert [v['factor'] for v in lv] == [(2, 2, 2), (4, 4, 4)]
    assert [v['z_range'] for v in lv] == [(0, 3), (0, 2)]
    assert [v['pool'] for v in lv] == [(2, 2, 2), (2, 2, 2)]
    assert [v['shape'] for v in P.plan((1, 1, 11), [(1, 1, 2)] * 3, 0, 1)] == [(1, 1, 6), (1, 1, 3), (1, 1, 2)]
    lv = P.plan((40, 72, 88), [(1, 2, 2), (2, 2, 2)], 0, 40)
    assert [v['shape'] for v in lv] == [(40, 36, 44), (20, 18, 22)]
    assert [v['factor'] for v in lv] == [(1, 2, 2), (2, 4, 4)]
    assert [v['z_range'] for v in lv] == [(0, 40), (0, 20)]


def test_plan_rank_alignment():
    from empanada_amd.inference import pyramid as P
    from empanada_amd.inference.sharded import shard_bounds
    b = shard_bounds(40, 2)
    assert list(b) == [0, 20, 40]
    plans = P.check_ranks((40, 72, 88), P.normalize(2), b)               # 20 % 4 == 0
    assert [v['z_range'] for v in plans[0]] == [(0, 10), (0, 5)]
    assert [v['z_range'] for v in plans[1]] == [(10, 20), (5, 10)]
    assert [v['shape'] for v in plans[0]] == [v['shape'] for v in plans[1]] == [(20, 36, 44), (10, 18, 22)]
    with pytest.raises(ValueError) as e:                                  # 20 % 8 != 0
        P.check_ranks((40, 72, 88), P.normalize(3), b)
    msg = str(e.value)
    assert '[0, 20)' in msg and 'level 3' in msg and 'factor is 8' in msg
    assert 'fewer ranks' in msg and 'fewer levels' in msg and '(1, 2, 2)' in msg
    with pytest.raises(ValueError, match=r'\[20, 40\).*level 3'):        # the second rank's own slab starts misaligned
        P.plan((40, 72, 88), P.normalize(3), 20, 40)
    for n in range(1, 9):                                                 # no pooling along z: any split is aligned
        plans = P.check_ranks((41, 72, 88), [(1, 2, 2)] * n, shard_bounds(41, 3))
        assert [p[-1]['z_range'] for p in plans] == [(0, 14), (14, 28), (28, 41)]
    # an odd last slab is fine when it ends the volume: the last cell is clipped there, as on one rank
    plans = P.check_ranks((39, 8, 8), P.normalize(1), [0, 20, 39])
    assert plans[1][0]['z_range'] == (10, 20) and plans[1][0]['shape'] == (20, 4, 4)
    with pytest.raises(ValueError, match='level 1'):
        P.check_ranks((39, 8, 8), P.normalize(1), [0, 19, 39])
    # the level ranges of the ranks tile the level
    for Z, world, L in ((40, 2, 2), (64, 4, 4), (48, 3, 4)):
        plans = P.check_ranks((Z, 8, 8), P.normalize(L), shard_bounds(Z, world))
        for l in range(L):
            r = [p[l]['z_range'] for p in plans]
            assert r[0][0] == 0 and r[-1][1] == plans[0][l]['shape'][0]
            assert all(a[1] == b[0] for a, b in zip(r[:-1], r[1:]))


def test_multiscales_entry():
    from empanada_amd.inference import pyramid as P
    got = P.multiscales('mito_pred', ['mito_pred', 'mito_pred_s1', 'mito_pred_s2'], [(1, 1, 1), (1, 2, 2), (2, 4, 4)])
    assert got == {
        'version': '0.4',
        'name': 'mito_pred',
        'type': 'mode',
        'axes': [{'name': 'z', 'type': 'space'}, {'name': 'y', 'type': 'space'}, {'name': 'x', 'type': 'space'}],
        'datasets': [
            {'path': 'mito_pred', 'coordinateTransformations': [{'type': 'scale', 'scale': [1.0, 1.0, 1.0]}]},
            {'path': 'mito_pred_s1', 'coordinateTransformations': [{'type': 'scale', 'scale': [1.0, 2.0, 2.0]},
                                                                   {'type': 'translation', 'translation': [0.0, 0.5, 0.5]}]},
            {'path': 'mito_pred_s2', 'coordinateTransformations': [{'type': 'scale', 'scale': [2.0, 4.0, 4.0]},
                                                                   {'type': 'translation', 'translation': [0.5, 1.5, 1.5]}]},
        ],
    }
    json.dumps(got)


def test_group_attributes(tmp_path):
    from empanada_amd.zarr_utils import ZarrV2Group, open_zarr
    path = str(tmp_path / 'g.zarr')
    g = ZarrV2Group(path)
    a = g.create_dataset('labels', shape=(2, 3, 4), dtype=np.uint32, chunks=(1, None, None))
    a[...] = np.arange(24, dtype=np.uint32).reshape(2, 3, 4)
    with open(os.path.join(path, '.zgroup')) as fh:
        zgroup = fh.read()
    assert g.attrs == {} and not os.path.exists(os.path.join(path, '.zattrs'))
    g.update_attrs({'multiscales': [{'name': 'a'}], 'other': 1})
    g.update_attrs({'other': 2, 'third': [1, 2]})
    want = {'multiscales': [{'name': 'a'}], 'other': 2, 'third': [1, 2]}
    assert g.attrs == want
    g.attrs['other'] = 5                                            # a parsed copy: nothing is written behind the caller's back
    assert g.attrs == want
    assert ZarrV2Group(path).attrs == want and open_zarr(path, 'r').attrs == want
    with open(os.path.join(path, '.zattrs')) as fh:
        assert json.load(fh) == want
    with open(os.path.join(path, '.zgroup')) as fh:
        assert fh.read() == zgroup
    np.testing.assert_array_equal(np.asarray(ZarrV2Group(path)['labels']), np.arange(24, dtype=np.uint32).reshape(2, 3, 4))
    assert sorted(os.listdir(path)) == ['.zattrs', '.zgroup', 'labels']


def test_write_multiscales_keeps_other_entries(tmp_path):
    from empanada_amd.inference import driver, pyramid as P
    from empanada_amd.zarr_utils import ZarrV2Group
    g = ZarrV2Group(str(tmp_path / 'g.zarr'))
    g.update_attrs({'multiscales': [{'name': 'raw', 'datasets': []}, {'name': 'mito_pred', 'stale': True}], 'keep': 'me'})
    levels = P.plan((40, 72, 88), P.normalize(2), 0, 40)
    driver.write_multiscales(g, [1, 2], {1: 'mito', 2: 'er'}, levels)
    attrs = g.attrs
    assert attrs['keep'] == 'me'
    assert [e['name'] for e in attrs['multiscales']] == ['raw', 'mito_pred', 'er_pred']
    cum = [(1, 1, 1), (2, 2, 2), (4, 4, 4)]
    assert attrs['multiscales'][1] == P.multiscales('mito_pred', ['mito_pred', 'mito_pred_s1', 'mito_pred_s2'], cum)
    assert attrs['multiscales'][2] == P.multiscales('er_pred', ['er_pred', 'er_pred_s1', 'er_pred_s2'], cum)

    class Plain:                                                     # an `out` of another kind: attrs if it has them
        def __init__(self):
            self.attrs = {}
    o = Plain()
    driver.write_multiscales(o, [1], None, levels[:1])
    assert [e['name'] for e in o.attrs['multiscales']] == ['1_pred']
    driver.write_multiscales(object(), [1], None, levels[:1])      # none: skipped silently


def test_infer_volume_pyramid_errors_come_first(tmp_path):
    """before the engine, the volume's data or the GPU are looked at: placeholders are enough"""
    from empanada_amd.inference.driver import infer_volume
    from empanada_amd.zarr_utils import ZarrV2Group

    class Engine:
        thing_list = [1]
        label_divisor = 1000

    class Volume:
        shape = (41, 72, 88)

    g = ZarrV2Group(str(tmp_path / 'g.zarr'))
    kw = dict(norms=dict(mean=0.5, std=0.1), labels=[1], out=g)
    for bad in (0, 9, [(1, 1, 1)], [(2, 3, 2)], 'auto'):
        with pytest.raises(ValueError, match='pyramid'):
            infer_volume(Engine(), Volume(), pyramid=bad, **kw)
    assert os.listdir(g.path) == ['.zgroup']
