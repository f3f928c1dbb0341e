"""GPU: _hip.shape_labels (csrc/emp_label_shape.hip) against tests/shape_ref.py bit for bit -- tile borders, the
overflow of the tile's table, halos, blocks, alignment, degenerate inputs -- and `shapes=` through infer_volume."""
import os
import queue
import sys
import time

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import shape_ref as ref  # noqa: E402

from empanada_amd import synthetic as SY  # noqa: E402
from test_holes_host import planted_volume  # noqa: E402
from test_morph_host import blobs  # noqa: E402
from test_pyramid_gpu import KW, NAMES, ORTHO, SHAPE, _dev, _engine, _free_port, _np, _run, case  # noqa: E402,F401 (fixture)

pytestmark = pytest.mark.gpu

SHAPES = [(13, 21, 37), (5, 16, 64), (6, 9, 1), (1, 9, 12), (3, 4, 300), (2, 70, 5), (17, 19, 130)]


def _table(lab, **kw):
    from empanada_amd import _hip
    t = _hip.shape_labels(lab if isinstance(lab, torch.Tensor) else _dev(lab), **kw)
    assert t.dtype == torch.int64 and t.is_cuda and t.dim() == 2 and t.shape[1] == 26
    return t.cpu().numpy()


def _check(lab, msg='', **kw):
    np.testing.assert_array_equal(_table(lab, **kw), ref.shape_table(lab, z_base=kw.get('z_base', 0)), err_msg=msg)


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_kernel_equals_the_checker_on_random_volumes(shape):
    for dtype in (np.uint8, np.uint32):
        info = {}
        _check(planted_volume(shape, dtype, seed=sum(shape)), f'planted {dtype.__name__}', info=info)
        assert info['blocks'] == 1 and info['tiles'] >= 1 and info['work_bytes'] > 0
        _check(blobs(shape, dtype, seed=sum(shape)), f'blobs {dtype.__name__}', z_base=7)


def test_int32_bits_are_taken_as_they_are():
    a = blobs((5, 9, 70), np.uint32, seed=2)                         # one label is 2^32 - 1
    got = _table(torch.from_numpy(a.view(np.int32)).cuda())
    np.testing.assert_array_equal(got, ref.shape_table(a))
    assert got[-1, 0] == 2 ** 32 - 1


def test_a_tile_with_more_labels_than_its_table_has_slots():
    rng = np.random.default_rng(5)
    lab = rng.integers(1, 201, size=(9, 10, 70)).astype(np.uint32)
    info = {}
    _check(lab, info=info)
    assert info['spilled'] > 0 and info['tiles'] == 8              # 2 x 2 x 2 tiles, all with labels
    calm = {}
    _check(np.full((9, 10, 70), 3, np.uint8), info=calm)
    assert calm['spilled'] == 0


def test_ids_above_2_31_sort_as_unsigned():
    lab = np.zeros((4, 9, 66), np.uint32)
    lab[0:2, 1:5, 2:60] = 2 ** 31 + 7
    lab[2:4, 2:8, 60:66] = 5
    lab[1:3, 6:9, 3:9] = 2 ** 32 - 1
    got = _table(lab)
    assert got[:, 0].tolist() == [5, 2 ** 31 + 7, 2 ** 32 - 1]
    np.testing.assert_array_equal(got, ref.shape_table(lab))


def test_identities_with_measure_labels():
    from empanada_amd import _hip
    for lab in (planted_volume((13, 21, 130), np.uint32, seed=1), blobs((9, 17, 70), np.uint8, seed=2)):
        dev = _dev(lab)
        m = _hip.measure_labels(dev, z_base=3).cpu().numpy()
        s = _table(dev, z_base=3)
        np.testing.assert_array_equal(s[:, 0:2], m[:, 0:2])
        np.testing.assert_array_equal(s[:, 2:5], m[:, 8:11])
        np.testing.assert_array_equal(s[:, [19, 13, 11]], m[:, 11:14])


def _tall():
    return planted_volume((29, 11, 70), np.uint32, seed=8, cell=5)


def test_blocks_equal_the_whole():
    tall = _tall()
    want = ref.shape_table(tall, z_base=2)
    for per in (1, 2, 3):
        info = {}
        got = _table(tall, z_base=2, block_voxels=per * 11 * 70, info=info)
        assert info['blocks'] == -(-29 // per)
        np.testing.assert_array_equal(got, want, err_msg=f'{per} slices per block')


def test_slabs_cut_from_a_taller_volume():
    from empanada_amd.shapes import merge_tables
    tall = _tall()
    dev = _dev(tall)
    want = ref.shape_table(tall, z_base=100)
    cuts = [0, 1, 9, 16, 17, 29]
    parts = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        below, above = (dev[a - 1] if a else None), (dev[b] if b < 29 else None)
        got = _table(dev[a:b], below=below, above=above, z_base=100 + a)
        np.testing.assert_array_equal(got, ref.shape_table(tall[a:b], None if below is None else tall[a - 1],
                                                           None if above is None else tall[b], z_base=100 + a))
        parts.append(got)
    np.testing.assert_array_equal(merge_tables(parts[::-1]), want)
    on_device = merge_tables([torch.from_numpy(p).cuda() for p in parts])
    assert on_device.is_cuda
    np.testing.assert_array_equal(on_device.cpu().numpy(), want)


@pytest.mark.parametrize('offset', [1, 3])
def test_unaligned_slab(offset):
    """the slab and its neighbour slices are views at an element offset: same table; the input is not written"""
    for dtype, tdt in ((np.uint8, torch.uint8), (np.uint32, torch.int32)):
        tall = blobs((13, 9, 70), dtype, seed=6)
        flat = torch.zeros((tall.size + 8,), dtype=tdt, device='cuda')
        flat[offset:offset + tall.size] = _dev(tall).view(tdt).ravel()
        before = flat.clone()
        v = flat[offset:offset + tall.size].view(tall.shape)
        v = v.view(torch.uint32) if dtype == np.uint32 else v
        assert v.data_ptr() % (4 * v.element_size()) != 0
        got = _table(v[3:10], below=v[2], above=v[10], z_base=3)
        np.testing.assert_array_equal(got, ref.shape_table(tall[3:10], tall[2], tall[10], z_base=3))
        assert torch.equal(flat, before)


def test_empty_and_degenerate_inputs():
    from empanada_amd import _hip
    for shape in ((0, 4, 4), (3, 0, 4), (3, 4, 0)):
        for tdt in (torch.uint8, torch.int32):
            info = {}
            t = _hip.shape_labels(torch.zeros(shape, dtype=tdt, device='cuda'), info=info)
            assert tuple(t.shape) == (0, 26) and t.dtype == torch.int64 and t.is_cuda
            assert info == {'blocks': 0, 'tiles': 0, 'spilled': 0, 'work_bytes': 0}
    info = {}
    assert _table(np.zeros((9, 10, 70), np.uint32), info=info).shape == (0, 26)
    assert info['blocks'] == 1 and info['tiles'] == 0
    own = np.arange(1, 3 * 4 * 66 + 1, dtype=np.uint32).reshape(3, 4, 66)   # every voxel its own label
    got = _table(own)
    np.testing.assert_array_equal(got, ref.shape_table(own))
    assert (got[:, 11:24] == 2).all() and (got[:, 24] == 8).all() and (got[:, 25] == 12).all()
    # the last slice the limits allow, and one past it
    one = np.full((1, 3, 5), 9, np.uint8)
    np.testing.assert_array_equal(_table(one, z_base=2 ** 20 - 1), ref.shape_table(one, z_base=2 ** 20 - 1))
    lab = _dev(one)
    with pytest.raises(ValueError, match='2\\^20|1048576'):
        _hip.shape_labels(lab, z_base=2 ** 20)
    for bad in (dict(z_base=-1), dict(z_base=1.5), dict(below=lab), dict(above=lab[0].cpu()),
                dict(below=lab[0].to(torch.int32)), dict(block_voxels=0), dict(block_voxels=14)):
        with pytest.raises(ValueError):
            _hip.shape_labels(lab, **bad)
    for bad in (lab.cpu(), lab[0], lab.to(torch.int64), lab.to(torch.float32), lab[:, :, ::2]):
        with pytest.raises(ValueError):
            _hip.shape_labels(bad)
    # the library refuses what the wrapper would have caught, before any launch
    lib = _hip.load()
    c = torch.zeros((2,), dtype=torch.int64, device='cuda')
    assert lib.emp_label_shape(lab.data_ptr(), 1, 1, 3, 5, None, None, 2 ** 20, None, 0, None, c.data_ptr(), None) == -1
    assert b'2^20' in lib.emp_last_error()
    assert lib.emp_label_shape(lab.data_ptr(), 2, 1, 3, 5, None, None, 0, None, 0, None, c.data_ptr(), None) == -1
    assert lib.emp_label_shape_labels(lab.data_ptr(), 1, 1, 3, 5, None, 1, None, 0, None, None, None) == -1
    assert lib.emp_label_shape_work_bytes(-1) == -1


def test_two_runs_are_bit_identical():
    rng = np.random.default_rng(9)
    lab = _dev(rng.integers(0, 60, size=(17, 19, 130)).astype(np.uint32))       # overflowing tiles among them
    a, b = _table(lab), _table(lab)
    assert np.array_equal(a, b) and len(a) == 59


def test_thinning_keeps_the_euler_number():
    from empanada_amd import _hip
    vol = ref.planted_objects()
    before = _table(vol)
    assert before[:, 0].tolist() == [5, 9, 200] and ref.euler(before).tolist() == [1, 0, 1]
    np.testing.assert_array_equal(before, ref.shape_table(vol))
    skel = _hip.label_thin(_dev(vol))
    after = _table(skel)
    assert (after[:, 1] < before[:, 1]).all()
    np.testing.assert_array_equal(after[:, 0], before[:, 0])
    np.testing.assert_array_equal(ref.euler(after), ref.euler(before))


def test_volume_shapes(tmp_path):
    from empanada_amd import shapes as SH
    from empanada_amd.zarr_utils import ZarrV2Group
    vol = _tall()
    g = ZarrV2Group(str(tmp_path / 'lab.zarr'))
    ds = g.create_dataset('lab', shape=vol.shape, dtype=np.uint32, chunks=(1, None, None))
    ds.write_slab(0, vol)
    want = ref.shape_table(vol)
    for slab_rows in (4, None):
        for source in (vol, ds, _dev(vol)):
            got = SH.volume_shapes(source, slab_rows=slab_rows)
            assert isinstance(got, np.ndarray) and got.dtype == np.int64
            np.testing.assert_array_equal(got, want, err_msg=f'{type(source).__name__} slab_rows {slab_rows}')
    assert SH.volume_shapes(np.zeros((3, 4, 5), np.uint8)).shape == (0, 26)
    with pytest.raises(ValueError, match='slab_rows'):
        SH.volume_shapes(vol, slab_rows=0)
    with pytest.raises(ValueError):
        SH.volume_shapes(vol[0])


# ------------------------------------------------------------------------------------------------------ infer_volume
PLAIN_KEYS = ['datasets', 'instances', 'volumes', 'z_range']
NEW_KEYS = ['shape_spacing', 'shapes']


def _assert_shapes(res, vols=None, spacing=(1.0, 1.0, 1.0)):
    """res['shapes'] is the checker's table of the (gathered) volume of every class"""
    assert sorted(res['shapes']) == [1, 2] and res['shape_spacing'] == spacing
    for c in (1, 2):
        lab = _np(res['volumes'][c]) if vols is None else vols[c]
        table = res['shapes'][c]
        assert isinstance(table, np.ndarray) and table.dtype == np.int64
        np.testing.assert_array_equal(table, ref.shape_table(lab), err_msg=f'class {c}')
    assert res['shapes'][2].shape[0] <= 1                          # a stuff class is one label


def test_infer_volume_plain_path_with_a_store(tmp_path, case):
    from empanada_amd import shapes as SH
    from empanada_amd.zarr_utils import ZarrV2Group
    eng, vol, vols, sets, counts = case(ORTHO)
    path = tmp_path / 'raw.zarr'
    res = _run(eng, vol, path, axes=ORTHO, shapes=True, measure=True)
    _assert_shapes(res)
    assert dict(res['instances']) == counts
    np.testing.assert_array_equal(_np(res['volumes'][1]), vols[1])
    np.testing.assert_array_equal(np.asarray(res['datasets'][1]), sets[1])
    np.testing.assert_array_equal(res['shapes'][1][:, :2], res['objects'][1][:, :2])
    g = ZarrV2Group(str(path), mode='r')
    assert sorted(res['shape_datasets']) == [1, 2]
    for c, name in ((1, 'mito_shapes'), (2, 'er_shapes')):
        assert res['shape_datasets'][c].path == os.path.join(str(path), name) and name in g
        np.testing.assert_array_equal(np.asarray(g[name]).reshape(-1, 26), res['shapes'][c])
    attrs = g.attrs
    assert attrs['shapes'] == {'columns': list(SH.COLUMNS), 'spacing': [1.0, 1.0, 1.0]}
    assert sorted(attrs) == ['objects', 'shapes']                                           # what was there survives
    d = SH.derive(res['shapes'][1], res['shape_spacing'])
    assert np.isfinite(d['surface_area']).all() and (d['sphericity'] > 0).all() and (d['axes'][:, 0] > 0).all()
    # shapes=None: the parent's keys and the parent's datasets, nothing else
    plain = _run(eng, vol, tmp_path / 'n.zarr', axes=ORTHO)
    assert sorted(plain) == PLAIN_KEYS
    assert sorted(os.listdir(str(tmp_path / 'n.zarr'))) == ['.zgroup', 'er_pred', 'mito_pred']
    # without a store, with a spacing
    bare = _run(eng, vol, None, axes=ORTHO, shapes=(3, 1, 1))
    _assert_shapes(bare, spacing=(3.0, 1.0, 1.0))
    assert sorted(bare) == sorted(PLAIN_KEYS + NEW_KEYS)
    with pytest.raises(ValueError, match='shapes must be'):
        _run(eng, vol, None, axes=ORTHO, shapes=(1, 1))


def test_infer_volume_stack_mode_and_windows(tmp_path, case):
    eng, vol, vols, _, counts = case(('xy',))
    res = _run(eng, vol, None, axes=('xy',), shapes=True)
    _assert_shapes(res)
    assert dict(res['instances']) == counts
    np.testing.assert_array_equal(_np(res['volumes'][1]), vols[1])
    kw = dict(axes=('xy',), batch_pixels=4 * 96 * 96, window_slices=8)      # 4 slices per model call, windows of 8
    win = _run(eng, vol, tmp_path / 'w.zarr', shapes=True, **kw)
    assert win['windows']['xy'] > 1
    _assert_shapes(win)
    np.testing.assert_array_equal(np.asarray(win['shape_datasets'][1]).reshape(-1, 26), win['shapes'][1])
    assert sorted(_run(eng, vol, None, **kw)) == sorted(PLAIN_KEYS + ['windows', 'head_bytes'])


def test_infer_volume_pipeline(tmp_path, case):
    from empanada_amd.inference.pipeline import VolumePipeline
    eng, vol, vols, sets, counts = case(ORTHO)
    pipe = VolumePipeline(eng, tune=False, graph=True, overlap=True, batch_pixels=1 << 22)
    try:
        res = _run(eng, vol, tmp_path / 'a.zarr', axes=ORTHO, shapes=True, pipeline=pipe)
        _assert_shapes(res)
        assert dict(res['instances']) == counts
        np.testing.assert_array_equal(_np(res['volumes'][1]), vols[1])
        np.testing.assert_array_equal(np.asarray(res['shape_datasets'][1]).reshape(-1, 26), res['shapes'][1])
        plain = _run(eng, vol, tmp_path / 'b.zarr', axes=ORTHO, pipeline=pipe)
        assert sorted(plain) == sorted(PLAIN_KEYS + ['pipeline'])
        assert sorted(os.listdir(str(tmp_path / 'b.zarr'))) == ['.zgroup', 'er_pred', 'mito_pred']
    finally:
        pipe.close()


def test_infer_volume_with_split_objects_and_fill_holes(case):
    """the table is of the repaired labels, whose objects are single pieces: euler = 1 - tunnels + cavities"""
    from scipy.ndimage import label
    from empanada_amd import shapes as SH
    eng, vol, vols, _, _ = case(ORTHO)
    res = _run(eng, vol, None, axes=ORTHO, shapes=True, split_objects=26, fill_holes=True)
    repaired = _np(res['volumes'][1])
    assert repaired.any()
    _assert_shapes(res)
    d = SH.derive(res['shapes'][1])
    for lab, e in zip(d['label'], d['euler']):
        mask = repaired == lab
        assert label(mask, structure=np.ones((3, 3, 3), int))[1] == 1              # one piece ...
        cavities = label(~np.pad(mask, 1))[1] - 1                                   # ... that may enclose another object
        assert 1 + cavities - e >= 0                                                # the number of its tunnels


def test_a_class_without_objects(tmp_path):
    """the step infer_volume applies to its result, on volumes of which one is empty: it has a (0, 26) table, which the
    store holds as a zero-row array; a store that cannot is recorded as None"""
    from empanada_amd.inference import driver
    from empanada_amd.zarr_utils import ZarrV2Group
    things = np.zeros((4, 6, 9), np.uint32)
    things[1:3, 0:3, 3:7] = 1001
    things[0, 2:4, 4:6] = 1002
    vols = {1: torch.zeros((4, 6, 9), dtype=torch.int32, device='cuda').view(torch.uint32),
            2: _dev(np.ones((4, 6, 9), np.uint8)), 3: _dev(things)}
    names = {1: 'mito', 2: 'er', 3: 'ld'}

    def run(out):
        return driver._shaped({'volumes': dict(vols), 'z_range': (0, 4)}, (1.0, 1.0, 1.0), [1, 2, 3], names, out, None)

    res = run(ZarrV2Group(str(tmp_path / 'z.zarr')))
    assert sorted(res['shapes']) == [1, 2, 3]
    assert res['shapes'][1].shape == (0, 26) and res['shapes'][1].dtype == np.int64
    assert res['shape_datasets'][1] is not None and res['shape_datasets'][1].shape == (0, 26)
    np.testing.assert_array_equal(res['shapes'][2], ref.shape_table(np.ones((4, 6, 9), np.uint8)))
    np.testing.assert_array_equal(res['shapes'][3], ref.shape_table(things))
    np.testing.assert_array_equal(np.asarray(res['shape_datasets'][3]).reshape(-1, 26), res['shapes'][3])

    class NoEmpty(ZarrV2Group):
        def create_dataset(self, name, shape, **kw):
            if 0 in tuple(shape):
                raise ValueError("no zero-length axes here")
            return super().create_dataset(name, shape=shape, **kw)

    res = run(NoEmpty(str(tmp_path / 'y.zarr')))
    assert res['shape_datasets'][1] is None and res['shape_datasets'][3] is not None
    assert sorted(os.listdir(str(tmp_path / 'y.zarr'))) == ['.zattrs', '.zgroup', 'er_shapes', 'ld_shapes']


# ----------------------------------------------------------------------------------------------- two ranks over gloo
def _rank(rank, world, port, path, q):
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        eng, vol = _engine(), SY.em_volume(SHAPE, seed=3)
        res = _run(eng, vol, path, axes=ORTHO, group=dist.group.WORLD, shapes=(2, 1, 1))
        q.put((rank, tuple(res['z_range']), res['shapes'], res['shape_spacing'], dict(res['instances']),
               {c: np.asarray(a).reshape(-1, 26) for c, a in res['shape_datasets'].items()}))
    finally:
        dist.destroy_process_group()


def test_infer_volume_two_ranks(tmp_path, case):
    import torch.multiprocessing as mp
    from empanada_amd.zarr_utils import ZarrV2Group
    eng, vol, vols, sets, counts = case(ORTHO)
    want = {c: ref.shape_table(vols[c]) for c in (1, 2)}
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
        assert got[r][2] == (2.0, 1.0, 1.0) and got[r][3] == counts
        for c in (1, 2):
            np.testing.assert_array_equal(got[r][1][c], want[c], err_msg=f'rank {r} class {c}')
            np.testing.assert_array_equal(got[r][4][c], want[c], err_msg=f'rank {r} class {c} dataset')
    np.testing.assert_array_equal(np.asarray(g[NAMES[1]]), sets[1])
    assert g.attrs['shapes']['spacing'] == [2.0, 1.0, 1.0]
