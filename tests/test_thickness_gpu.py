"""GPU: local thickness of the labelled objects -- emp_label_thick_* (csrc/emp_label_thick.hip) through
_hip.label_thickness, thickness.volume_thickness and infer_volume(..., thickness=).  The checker is
tests/thickness_ref.py's `thickness_fast`, a restatement of the definition in include/emp_hip.h (E10) on scipy's exact
Euclidean transform that shares nothing with the kernel and that tests/test_thickness_host.py checks against brute
force.  Every value is an integer and is compared bit for bit.  The engine and volume of the infer_volume cases are those
of tests/test_pyramid_gpu.py."""
import os
import queue
import sys
import time

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import thickness_ref as ref  # noqa: E402

from empanada_amd import synthetic as SY  # noqa: E402
from test_holes_host import planted_volume  # noqa: E402
from test_morph_host import SAMPLINGS, blobs  # noqa: E402
from test_pyramid_gpu import KW, NAMES, ORTHO, SHAPE, _dev, _engine, _free_port, _np, _run, case  # noqa: E402,F401 (fixture)

pytestmark = pytest.mark.gpu

SHAPES = [(13, 21, 37), (5, 16, 64), (6, 9, 1), (1, 9, 12), (3, 4, 300), (2, 70, 5)]
_CACHE = {}


def _u16(t):
    assert t.dtype == torch.uint16 and t.is_cuda
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def _thick(lab, cap=1024, sampling=(1, 1, 1), below=None, above=None, **kw):
    """(map, table) of _hip.label_thickness as numpy arrays"""
    from empanada_amd import _hip
    dev = lambda t: None if t is None else _dev(t)
    t2, table = _hip.label_thickness(dev(lab), cap, sampling, below=dev(below), above=dev(above), **kw)
    assert table.dtype == torch.int64 and table.is_cuda and table.dim() == 2 and table.shape[1] == 3
    assert tuple(t2.shape) == tuple(lab.shape)
    return _u16(t2), table.cpu().numpy()


def _check(lab, cap, sampling=(1, 1, 1), msg=''):
    want, d2 = ref.thickness_fast(lab, cap, sampling)
    info = {}
    got, table = _thick(lab, cap, sampling, info=info)
    np.testing.assert_array_equal(got, want, err_msg=msg)
    np.testing.assert_array_equal(table, ref.table_ref(lab, want), err_msg=msg)
    assert info['capped'] == int((d2 == cap).sum()) and info['candidates'] == int((lab != 0).sum()), msg
    return got, info


# ------------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_kernel_equals_the_checker_on_random_volumes(shape):
    for make in (planted_volume, blobs):
        for dtype in (np.uint8, np.uint32):
            lab = make(shape, dtype, seed=11)
            for sampling in SAMPLINGS:
                for cap in (2, 10, 1024):
                    _check(lab, cap, sampling, f'{make.__name__} {np.dtype(dtype).name} {sampling} cap {cap}')
    lab = planted_volume(shape, np.uint32, seed=5).view(np.int32)           # the bits of an int32 are taken as they are
    _check(lab, 10)


def test_reach_across_tiles():
    """balls that cover voxels of other tiles: two tiles away in z and y, and across the x-tile borders"""
    for lab in (ref.dumbbell(), ref.tube_and_ball()):
        got, info = _check(lab, 1024)
        assert info['capped'] == 0 and info['lists'] > 4
    t2 = _thick(ref.tube_and_ball(), 1024)[0]
    assert t2[0, 8, 64] == t2[16, 8, 64] == t2[8, 0, 64] == t2[8, 16, 64] == t2[8, 8, 64] >= 64
    assert t2[15, 4, 30] == t2[15, 4, 63 - 20] == t2[15, 4, 64 + 20] == t2[15, 4, 130] >= 9      # along the tube
    _check(ref.dumbbell(np.uint8), 1024, (1, 2, 1))
    _check(ref.tube_and_ball(), 1024, (3, 1, 1))


@pytest.mark.parametrize('cap', [10, 50])
def test_a_cap_that_bites(cap):
    lab = ref.dumbbell()
    got, info = _check(lab, cap)
    free = ref.thickness_fast(lab, 65535)[0]
    assert info['capped'] > 0 and (got != np.minimum(free, cap)).any()      # not a clamp of the uncapped result


def test_ids_above_2_31_sort_as_unsigned():
    lab = blobs((13, 21, 37), np.uint32, seed=2)
    lab[lab == 3] = 0x80000000
    _, table = _thick(lab.view(np.int32), 10)
    assert (table[:, 0] == 0x80000000).any() and (table[:, 0] == 0xFFFFFFFF).any() and (table[:, 0] < 2 ** 31).any()
    keys = [(a << 32) | b for a, b in table[:, :2].tolist()]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    np.testing.assert_array_equal(table, ref.table_ref(lab, ref.thickness_fast(lab, 10)[0]))


# ------------------------------------------------------------------------------------------------------ blocks and halos
def _tall():
    """(29, 21, 37) labels, never modified"""
    if 'tall' not in _CACHE:
        _CACHE['tall'] = blobs((29, 21, 37), np.uint32, seed=4)
    return _CACHE['tall']


@pytest.mark.parametrize('cap', [10, 26])
def test_blocks_equal_the_whole(cap):
    from empanada_amd import _hip
    lab = _tall()[8:21]                                                     # (13, 21, 37)
    want = ref.thickness_fast(lab, cap)[0]
    per = 21 * 37
    for slices, n_blocks in ((1, 13), (2, 7), (5, 3)):
        info = {}
        got, table = _thick(lab, cap, block_voxels=slices * per + 3, info=info)
        assert info['blocks'] == n_blocks
        np.testing.assert_array_equal(got, want, err_msg=f'{n_blocks} blocks')
        np.testing.assert_array_equal(table, ref.table_ref(lab, want), err_msg=f'{n_blocks} blocks')
    with pytest.raises(ValueError, match='single slice'):
        _hip.label_thickness(_dev(lab), cap, block_voxels=per - 1)


@pytest.mark.parametrize('cap', [10, 26])
def test_halo_stacks_cut_from_a_taller_volume(cap):
    """below / above stand for the volume outside the slab: with 2 h slices the map is the taller volume's, with fewer
    that of the volume cut there"""
    from empanada_amd.thickness import halo_slices
    tall = _tall()
    whole = ref.thickness_fast(tall, cap)[0]
    two_h = halo_slices(cap)
    z0, z1 = 10, 19
    maps = {}
    for k in (0, two_h // 2, two_h):
        lo, hi = tall[z0 - k:z0], tall[z1:z1 + k]
        got, table = _thick(tall[z0:z1], cap, below=lo if k else None, above=hi if k else None)
        want = ref.thickness_fast(tall[z0 - k:z1 + k], cap)[0][k:k + z1 - z0]
        np.testing.assert_array_equal(got, want, err_msg=f'{k} halo slices')
        np.testing.assert_array_equal(table, ref.table_ref(tall[z0:z1], want))
        maps[k] = got
    np.testing.assert_array_equal(maps[two_h], whole[z0:z1])
    assert (maps[0] != whole[z0:z1]).any()                                  # the data tell a halo from none
    # at the volume's ends the stacks are shorter than the halo, or absent
    got, _ = _thick(tall[0:9], cap, above=tall[9:9 + two_h])
    np.testing.assert_array_equal(got, whole[0:9])
    got, _ = _thick(tall[24:29], cap, below=tall[24 - two_h:24])
    np.testing.assert_array_equal(got, whole[24:29])


@pytest.mark.parametrize('offset', [1, 3])
def test_unaligned_slab(offset):
    """the slab and the halo stacks are views at an element offset: same map; the input is not written"""
    from empanada_amd import _hip
    for dtype, tdt in ((np.uint8, torch.uint8), (np.uint32, torch.int32)):
        tall = blobs((13, 9, 70), dtype, seed=6)
        flat = torch.zeros((tall.size + 8,), dtype=tdt, device='cuda')
        flat[offset:offset + tall.size] = _dev(tall).view(tdt).ravel()
        before = flat.clone()
        v = flat[offset:offset + tall.size].view(tall.shape)
        v = v.view(torch.uint32) if dtype == np.uint32 else v
        assert v.data_ptr() % (4 * v.element_size()) != 0
        t2, table = _hip.label_thickness(v[3:10], 5, below=v[0:3], above=v[10:13])
        want = ref.thickness_fast(tall, 5)[0][3:10]
        np.testing.assert_array_equal(_u16(t2), want)
        np.testing.assert_array_equal(table.cpu().numpy(), ref.table_ref(tall[3:10], want))
        assert torch.equal(flat, before)


def test_empty_and_degenerate_inputs():
    from empanada_amd import _hip
    for shape in ((0, 4, 4), (3, 0, 4), (3, 4, 0)):
        for tdt in (torch.uint8, torch.int32):
            info = {}
            t2, table = _hip.label_thickness(torch.zeros(shape, dtype=tdt, device='cuda'), info=info)
            assert tuple(t2.shape) == shape and t2.dtype == torch.uint16 and t2.is_cuda
            assert tuple(table.shape) == (0, 3) and table.dtype == torch.int64 and table.is_cuda
            assert info['blocks'] == 0 and info['capped'] == 0
    info = {}
    got, table = _thick(np.zeros((9, 10, 70), np.uint32), info=info)
    assert not got.any() and table.shape == (0, 3) and info['candidates'] == 0 and info['lists'] == 0
    _check(blobs((9, 10, 1), np.uint8, seed=1), 10)                         # W = 1
    own = np.arange(1, 5 * 6 * 70 + 1, dtype=np.uint32).reshape(5, 6, 70)   # every voxel its own label
    got, table = _thick(own)
    assert (got == 1).all() and table.tolist() == [[i, 1, 1] for i in range(1, own.size + 1)]
    full = np.full((9, 10, 70), 7, np.uint8)                                # one label fills the volume: cap everywhere
    got, info = _check(full, 50)
    assert (got == 50).all() and info['capped'] == full.size


def test_two_runs_are_bit_identical():
    from empanada_amd import _hip
    lab = _dev(ref.dumbbell())
    a, ta = _hip.label_thickness(lab, 50)
    b, tb = _hip.label_thickness(lab, 50)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16)) and torch.equal(ta, tb)


def test_volume_thickness(tmp_path):
    from empanada_amd import thickness as TH
    from empanada_amd.zarr_utils import ZarrV2Group
    vol = _tall()
    g = ZarrV2Group(str(tmp_path / 'lab.zarr'))
    ds = g.create_dataset('lab', shape=vol.shape, dtype=np.uint32, chunks=(1, None, None))
    ds.write_slab(0, vol)
    for r_cap, sampling in ((3, (1, 1, 1)), (5.1, (3, 1, 1))):
        cap = TH.check((r_cap, sampling))[1]
        want, d2 = ref.thickness_fast(vol, cap, sampling)
        for slab_rows in (3, 7, None):
            for source in (vol, ds, _dev(vol)):
                t2, table, capped = TH.volume_thickness(source, r_cap=r_cap, sampling=sampling, slab_rows=slab_rows)
                assert isinstance(t2, np.ndarray) and t2.dtype == np.uint16 and table.dtype == np.int64
                np.testing.assert_array_equal(t2, want, err_msg=f'{type(source).__name__} slab_rows {slab_rows}')
                np.testing.assert_array_equal(table, ref.table_ref(vol, want))
                assert capped == int((d2 == cap).sum())
    t2, table, capped = TH.volume_thickness(np.zeros((3, 4, 5), np.uint8), r_cap=2)
    assert not t2.any() and table.shape == (0, 3) and capped == 0
    for bad in (0, True, 2.0):
        with pytest.raises(ValueError, match='slab_rows'):
            TH.volume_thickness(vol, r_cap=2, slab_rows=bad)
    with pytest.raises(ValueError):
        TH.volume_thickness(vol[0], r_cap=2)
    with pytest.raises(ValueError):
        TH.volume_thickness(vol, r_cap=0.5)


# ------------------------------------------------------------------------------------------------------ infer_volume
PLAIN_KEYS = ['datasets', 'instances', 'volumes', 'z_range']
NEW_KEYS = ['thickness', 'thickness_maps', 'thickness_params']
R_CAP, CAP = 3, 9


def _assert_thickness(res, vols=None, cap=CAP, sampling=(1, 1, 1), r_cap=float(R_CAP)):
    """res['thickness'] and res['thickness_maps'] are the checker's of the (gathered) volume of the thing class"""
    lab = _np(res['volumes'][1]) if vols is None else vols[1]
    assert sorted(res['thickness']) == [1] and sorted(res['thickness_maps']) == [1]
    assert res['thickness_params'] == {'r_cap': r_cap, 'cap': cap, 'sampling': sampling}
    want, d2 = ref.thickness_fast(lab, cap, sampling)
    z0, z1 = res['z_range']
    np.testing.assert_array_equal(_u16(res['thickness_maps'][1]), want[z0:z1])
    table = res['thickness'][1]['table']
    assert isinstance(table, np.ndarray) and table.dtype == np.int64
    np.testing.assert_array_equal(table, ref.table_ref(lab, want))
    assert res['thickness'][1]['capped'] == int((d2 == cap).sum())
    return want


def test_infer_volume_plain_path_with_a_store(tmp_path, case):
    from empanada_amd import thickness as TH
    from empanada_amd.zarr_utils import ZarrV2Group
    eng, vol, vols, sets, counts = case(ORTHO)
    for name, compressor in (('raw.zarr', None), ('z.zarr', 'zlib')):
        path = tmp_path / name
        res = _run(eng, vol, path, axes=ORTHO, thickness=R_CAP, measure=True, compressor=compressor)
        want = _assert_thickness(res)
        assert want.max() > 1 and dict(res['instances']) == counts
        np.testing.assert_array_equal(_np(res['volumes'][1]), vols[1])
        np.testing.assert_array_equal(np.asarray(res['datasets'][1]), sets[1])
        g = ZarrV2Group(str(path), mode='r')
        ds = res['thickness_datasets'][1]
        assert sorted(res['thickness_datasets']) == [1] and sorted(ds) == ['map', 'table']
        assert ds['map'].path == os.path.join(str(path), 'mito_thickness') and 'mito_thickness' in g
        assert ds['map'].dtype == np.uint16 and tuple(ds['map'].shape) == SHAPE
        assert tuple(ds['map'].chunks) == (1,) + SHAPE[1:] and ds['map'].codec is None          # always raw chunks
        np.testing.assert_array_equal(np.asarray(g['mito_thickness']), want)
        np.testing.assert_array_equal(np.asarray(g['mito_thickness_table']).reshape(-1, 3), res['thickness'][1]['table'])
        attrs = g.attrs
        assert attrs['thickness'] == {'columns': list(TH.COLUMNS), 'r_cap': 3.0, 'cap': 9, 'sampling': [1, 1, 1],
                                      'map': 'squared radius, diameter = 2 sqrt'}
        assert sorted(attrs) == ['objects', 'thickness']                                        # what was there survives
    # thickness=None: the parent's keys and the parent's datasets, nothing else
    plain = _run(eng, vol, tmp_path / 'n.zarr', axes=ORTHO)
    assert sorted(plain) == PLAIN_KEYS
    assert sorted(os.listdir(str(tmp_path / 'n.zarr'))) == ['.zgroup', 'er_pred', 'mito_pred']
    # without a store, with a sampling
    bare = _run(eng, vol, None, axes=ORTHO, thickness=(4, (2, 1, 1)))
    _assert_thickness(bare, cap=16, sampling=(2, 1, 1), r_cap=4.0)
    assert sorted(bare) == sorted(PLAIN_KEYS + NEW_KEYS)
    with pytest.raises(ValueError, match='r_cap'):
        _run(eng, vol, None, axes=ORTHO, thickness=0)


def test_infer_volume_stack_mode_and_windows(tmp_path, case):
    eng, vol, vols, _, counts = case(('xy',))
    res = _run(eng, vol, None, axes=('xy',), thickness=R_CAP)
    _assert_thickness(res)
    assert dict(res['instances']) == counts
    np.testing.assert_array_equal(_np(res['volumes'][1]), vols[1])
    kw = dict(axes=('xy',), batch_pixels=4 * 96 * 96, window_slices=8)      # 4 slices per model call, windows of 8
    win = _run(eng, vol, tmp_path / 'w.zarr', thickness=R_CAP, **kw)
    assert win['windows']['xy'] > 1
    want = _assert_thickness(win)
    np.testing.assert_array_equal(np.asarray(win['thickness_datasets'][1]['map']), want)
    assert sorted(_run(eng, vol, None, **kw)) == sorted(PLAIN_KEYS + ['windows', 'head_bytes'])


def test_infer_volume_pipeline(tmp_path, case):
    from empanada_amd.inference.pipeline import VolumePipeline
    eng, vol, vols, sets, counts = case(ORTHO)
    pipe = VolumePipeline(eng, tune=False, graph=True, overlap=True, batch_pixels=1 << 22)
    try:
        res = _run(eng, vol, tmp_path / 'a.zarr', axes=ORTHO, thickness=R_CAP, pipeline=pipe)
        want = _assert_thickness(res)
        assert dict(res['instances']) == counts
        np.testing.assert_array_equal(_np(res['volumes'][1]), vols[1])
        np.testing.assert_array_equal(np.asarray(res['thickness_datasets'][1]['map']), want)
        plain = _run(eng, vol, tmp_path / 'b.zarr', axes=ORTHO, pipeline=pipe)
        assert sorted(plain) == sorted(PLAIN_KEYS + ['pipeline'])
        assert sorted(os.listdir(str(tmp_path / 'b.zarr'))) == ['.zgroup', 'er_pred', 'mito_pred']
    finally:
        pipe.close()


def test_infer_volume_with_morph_and_split_objects(case):
    """the map is of the repaired labels"""
    eng, vol, vols, _, _ = case(ORTHO)
    res = _run(eng, vol, None, axes=ORTHO, thickness=R_CAP, morph=('open', 1), split_objects=6)
    repaired = _np(res['volumes'][1])
    assert (repaired != vols[1]).any() and repaired.any()
    _assert_thickness(res)
    assert (_u16(res['thickness_maps'][1]) != ref.thickness_fast(vols[1], CAP)[0]).any()


def test_a_class_without_objects(tmp_path):
    """the step infer_volume applies to its result, on volumes of which one is empty: it has a (0, 3) table, which the
    store holds as a zero-row array; a store that cannot is recorded as None"""
    from empanada_amd.inference import driver
    from empanada_amd.zarr_utils import ZarrV2Group
    things = np.zeros((4, 6, 9), np.uint32)
    things[1:3, 0:3, 3:7] = 1001
    things[0, 2:4, 4:6] = 1002
    vols = {1: torch.zeros((4, 6, 9), dtype=torch.int32, device='cuda').view(torch.uint32),
            2: _dev(np.ones((4, 6, 9), np.uint8)), 3: _dev(things)}

    def run(out):
        return driver._thickened({'volumes': dict(vols), 'z_range': (0, 4)}, (2.0, 4, (1, 1, 1)), [1, 3], (4, 6, 9),
                                 {1: 'mito', 2: 'er', 3: 'ld'}, out, None)

    res = run(ZarrV2Group(str(tmp_path / 'z.zarr')))
    assert sorted(res['thickness']) == [1, 3]                               # thing classes only
    assert res['thickness'][1]['table'].shape == (0, 3) and res['thickness'][1]['table'].dtype == np.int64
    assert not _u16(res['thickness_maps'][1]).any() and res['thickness'][1]['capped'] == 0
    ds = res['thickness_datasets'][1]
    assert ds['table'] is not None and ds['table'].shape == (0, 3) and not np.asarray(ds['map']).any()
    want = ref.thickness_fast(things, 4)[0]
    np.testing.assert_array_equal(_u16(res['thickness_maps'][3]), want)
    np.testing.assert_array_equal(res['thickness'][3]['table'], ref.table_ref(things, want))
    np.testing.assert_array_equal(np.asarray(res['thickness_datasets'][3]['map']), want)

    class NoEmpty(ZarrV2Group):
        def create_dataset(self, name, shape, **kw):
            if 0 in tuple(shape):
                raise ValueError("no zero-length axes here")
            return super().create_dataset(name, shape=shape, **kw)

    res = run(NoEmpty(str(tmp_path / 'y.zarr')))
    assert res['thickness_datasets'][1]['table'] is None and res['thickness_datasets'][3]['table'] is not None
    assert sorted(os.listdir(str(tmp_path / 'y.zarr'))) == ['.zattrs', '.zgroup', 'ld_thickness', 'ld_thickness_table',
                                                           'mito_thickness']


# ----------------------------------------------------------------------------------------------- two ranks over gloo
def _rank(rank, world, port, path, q):
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        eng, vol = _engine(), SY.em_volume(SHAPE, seed=3)
        res = _run(eng, vol, path, axes=ORTHO, group=dist.group.WORLD, thickness=(3, (2, 1, 1)))
        q.put((rank, tuple(res['z_range']), res['thickness'], res['thickness_params'], dict(res['instances']),
               _u16(res['thickness_maps'][1]), np.asarray(res['thickness_datasets'][1]['table']).reshape(-1, 3)))
    finally:
        dist.destroy_process_group()


def test_infer_volume_two_ranks(tmp_path, case):
    import torch.multiprocessing as mp
    from empanada_amd.zarr_utils import ZarrV2Group
    eng, vol, vols, sets, counts = case(ORTHO)
    want, d2 = ref.thickness_fast(vols[1], 9, (2, 1, 1))
    table = ref.table_ref(vols[1], want)
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    path = str(tmp_path / 'two.zarr')
    port = _free_port()
    procs = [ctx.Process(target=_rank, args=(r, 2, port, path, q)) for r in range(2)]
    for p in procs:
        p.start()
    got, deadline = {}, time.monotonic() + 240                 # the ranks' own time limit: they are ended, not waited for
    try:
        while len(got) < 2:                                     # a rank that died is reported at once
            try:
                item = q.get(timeout=1)
                got[item[0]] = item[1:]
            except queue.Empty:
                dead = [p.exitcode for p in procs if not p.is_alive() and p.exitcode != 0]
                assert not dead, f"a rank ended with exit code {dead[0]} before it reported"
                assert any(p.is_alive() for p in procs) or not q.empty(), "the ranks ended without reporting"
                assert time.monotonic() < deadline, "the ranks did not report within their time limit"
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
    assert got[0][0] == (0, 20) and got[1][0] == (20, 40)
    g = ZarrV2Group(path, mode='r')
    for r in (0, 1):
        z0, z1 = got[r][0]
        assert got[r][2] == {'r_cap': 3.0, 'cap': 9, 'sampling': (2, 1, 1)} and got[r][3] == counts
        np.testing.assert_array_equal(got[r][1][1]['table'], table, err_msg=f'rank {r}')
        assert got[r][1][1]['capped'] == int((d2 == 9).sum())
        np.testing.assert_array_equal(got[r][4], want[z0:z1], err_msg=f'rank {r} map')
        np.testing.assert_array_equal(got[r][5], table, err_msg=f'rank {r} dataset')
    np.testing.assert_array_equal(np.asarray(g[NAMES[1]]), sets[1])
    np.testing.assert_array_equal(np.asarray(g['mito_thickness']), want)
