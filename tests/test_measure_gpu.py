"""GPU: per-object measurements -- emp_label_measure (csrc/emp_measure.hip) through _hip.measure_labels,
measurements.volume_measurements and infer_volume(..., measure=).  The checker is tests/test_measure_host.py's
`measure_ref`, a numpy restatement of the definition in include/emp_hip.h (E2) that shares nothing with the kernel.
Every column is an integer and is compared bit for bit.  The engine and volume of the infer_volume cases are those of
tests/test_pyramid_gpu.py."""
import os
import queue
import time

import numpy as np
import pytest
import torch

from empanada_amd import synthetic as SY
from test_measure_host import N_COL, measure_ref
from test_pyramid_gpu import KW, NAMES, ORTHO, SHAPE, _dev, _engine, _free_port, _np, _run, case  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (1, 1, 2), (2, 2, 2), (3, 3, 5), (2, 5, 130), (2, 4, 259), (3, 2, 1031), (5, 64, 64)]
DTYPES = [np.uint8, np.uint32]
_CACHE = {}


def _measure(lab, below=None, above=None, **kw):
    from empanada_amd import _hip
    got = _hip.measure_labels(_dev(lab), None if below is None else _dev(below), None if above is None else _dev(above),
                              **kw)
    assert got.dtype == torch.int64 and got.is_cuda and got.dim() == 2 and got.shape[1] == N_COL
    return got.cpu().numpy()


def _contents(shape, dtype):
    """name -> array: nothing, one label everywhere, every voxel its own run, four letters with labels >= 2^31 (uint32),
    random boxes"""
    top = int(np.iinfo(dtype).max)
    rng = np.random.default_rng(int(np.prod(shape)) * 7 + np.dtype(dtype).itemsize)
    z, y, x = np.indices(shape)
    letters = np.array([0, 1, top // 2 + 1, top], dtype)
    boxes = np.zeros(shape, dtype)
    for label in range(1, 9):
        lo = [int(rng.integers(0, s)) for s in shape]
        hi = [int(rng.integers(a + 1, s + 1)) for a, s in zip(lo, shape)]
        boxes[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = label * 29 % 251 + 1
    return {'zero': np.zeros(shape, dtype), 'one': np.full(shape, 5, dtype),
            'checker': np.where((z + y + x) % 2 == 0, 2, top).astype(dtype),
            'alphabet': letters[rng.integers(0, 4, size=shape)], 'boxes': boxes}


# ------------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize('dtype', DTYPES, ids=['u8', 'u32'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_kernel_equals_the_restatement(shape, dtype):
    rng = np.random.default_rng(11)
    for name, lab in _contents(shape, dtype).items():
        other = _contents(shape, dtype)['alphabet'][0]                      # a neighbour slice unlike the end slices
        noise = rng.permutation(lab[-1].ravel()).reshape(lab[-1].shape)
        for below, above, z_base in ((None, None, 0), (None, None, 7), (lab[0], lab[-1], 7), (other, noise, 0),
                                     (lab[0], None, 0), (None, other, 7)):
            got = _measure(lab, below, above, z_base=z_base)
            np.testing.assert_array_equal(got, measure_ref(lab, below, above, z_base), err_msg=f'{name} {shape} z_base {z_base}')
        if name == 'zero':
            assert got.shape == (0, N_COL)
        if name == 'checker':                                               # the run total at its maximum
            info = {}
            from empanada_amd import _hip
            _hip.measure_labels(_dev(lab), info=info)
            assert info['runs'] == lab.size and info['blocks'] == 1


def test_cases_counted_by_hand():
    one = np.zeros((3, 3, 3), np.uint8)
    one[1, 2, 0] = 7
    assert _measure(one, z_base=5).tolist() == [[7, 1, 6, 2, 0, 7, 3, 1, 6, 2, 0, 2, 2, 2]]
    assert _measure(np.full((2, 2, 2), 3, np.uint32)).tolist() == [[3, 8, 0, 0, 0, 2, 2, 2, 4, 4, 4, 8, 8, 8]]
    v = np.array([[[5]]], np.uint8)
    assert _measure(v, below=np.array([[5]], np.uint8))[0, 11:].tolist() == [1, 2, 2]
    assert _measure(v, below=np.array([[6]], np.uint8))[0, 11:].tolist() == [2, 2, 2]


def test_empty_slabs():
    from empanada_amd import _hip
    for shape in ((0, 4, 4), (3, 0, 4), (3, 4, 0)):
        for tdt in (torch.uint8, torch.int32):
            got = _hip.measure_labels(torch.zeros(shape, dtype=tdt, device='cuda'))
            assert tuple(got.shape) == (0, N_COL) and got.dtype == torch.int64 and got.is_cuda


def test_int32_bits_are_taken_as_they_are():
    from empanada_amd import _hip
    a = _contents((3, 5, 130), np.uint32)['alphabet']                       # half the letters are negative as int32
    got = _hip.measure_labels(torch.from_numpy(a.view(np.int32)).cuda(), z_base=2)
    np.testing.assert_array_equal(got.cpu().numpy(), measure_ref(a, z_base=2))
    assert (got[:, 0] >= 2 ** 31).any()


@pytest.mark.parametrize('offset', [1, 2, 3])
def test_unaligned_slab_takes_the_narrow_path(offset):
    """the slab and its neighbour slices start 1, 2 or 3 elements off a 16-byte (uint32) / 4-byte (uint8) address: the
    rows' aligned lane grid shifts, neighbour groups are read voxel by voxel; same table"""
    from empanada_amd import _hip
    for dtype, tdt in ((np.uint32, torch.int32), (np.uint8, torch.uint8)):
        for shape in ((3, 6, 64), (2, 3, 259)):
            a = _contents(shape, dtype)['alphabet']
            ends = _contents((2,) + shape[1:], dtype)['boxes']
            flat = torch.zeros((a.size + ends.size + 32,), dtype=tdt, device='cuda')
            flat[offset:offset + a.size] = _dev(a).view(tdt).ravel()
            at = offset + a.size + (5 - offset)                             # the neighbour slices at yet another offset
            flat[at:at + ends.size] = _dev(ends).view(tdt).ravel()
            view = (lambda t: t.view(torch.uint32)) if dtype == np.uint32 else (lambda t: t)
            dev = view(flat[offset:offset + a.size]).view(a.shape)
            nb = view(flat[at:at + ends.size]).view(ends.shape)
            assert dev.data_ptr() % (4 * dev.element_size()) != 0 and dev.is_contiguous()
            got = _hip.measure_labels(dev, below=nb[0], above=nb[1], z_base=3)
            np.testing.assert_array_equal(got.cpu().numpy(), measure_ref(a, ends[0], ends[1], 3), err_msg=f'{dtype} {shape}')


def test_a_label_of_many_runs_beside_labels_of_one():
    """label 9 has one run in each of 700 rows -- many reduce segments of 16 runs, whose partial sums meet in one table
    row -- and sits between labels that own a single run each"""
    lab = np.zeros((7, 100, 40), np.uint32)
    lab[:, :, 3:30] = 9
    lab[0, 0, 35:38] = 4
    lab[6, 99, 0:2] = 0xFFFFFFF0
    lab[3, 50, 31] = 9                                                      # and a second run of it in one row
    got = _measure(lab, z_base=1)
    assert got[:, 0].tolist() == [4, 9, 0xFFFFFFF0] and got[1, 1] == 700 * 27 + 1
    np.testing.assert_array_equal(got, measure_ref(lab, z_base=1))


def test_a_run_across_a_chunk_border():
    """a wave takes 256 voxels of a row at a time: the run below spans three chunks and has exposed y and z faces on both
    sides of each border, so its exposure is the carried scan's difference across chunks"""
    for dtype in DTYPES:
        lab = np.zeros((3, 3, 700), dtype)
        lab[1, 1, 100:650] = 6
        lab[1, 0, 90:258] = 6                                               # covers part of the run from y - 1 ...
        lab[0, 1, 250:300] = 6                                              # ... from z - 1, across the border ...
        lab[2, 1, 500:520] = 8                                              # ... and another label from z + 1
        lab[1, 2, 255:257] = 6
        np.testing.assert_array_equal(_measure(lab), measure_ref(lab))


# ------------------------------------------------------------------------------------------------------ planted labels
def _planted():
    """(8, 256, 256) uint16 labels, fill 0.08, seed 4321: computed once, never modified"""
    if 'planted' not in _CACHE:
        lab = SY.planted_labels((8, 256, 256), fill=0.08, seed=4321)[0].astype(np.uint32)
        _CACHE['planted'] = (lab, measure_ref(lab))
    return _CACHE['planted']


def test_planted_labels_whole_and_in_blocks():
    from empanada_amd import _hip, measurements as M
    lab, want = _planted()
    assert len(want) == 66 and (want[:, 2] <= 3).all() and (want[:, 5] > 3).all()       # every object crosses z = 3
    np.testing.assert_array_equal(_measure(lab), want)
    for block, n_blocks in ((3 * 256 * 256, 3), (256 * 256, 8)):
        info = {}
        got = _hip.measure_labels(_dev(lab), block_voxels=block, info=info)
        assert info['blocks'] == n_blocks
        np.testing.assert_array_equal(got.cpu().numpy(), want)
    u8 = lab.astype(np.uint8)
    np.testing.assert_array_equal(_measure(u8, block_voxels=2 * 256 * 256), measure_ref(u8))
    # the data tell a block with its neighbour slices from one without: the halves measured blind give another table
    dev = _dev(lab)
    blind = M.merge_tables([_hip.measure_labels(dev[:4]), _hip.measure_labels(dev[4:], z_base=4)]).cpu().numpy()
    assert (blind != want).any() and (blind[:, :11] == want[:, :11]).all() and (blind[:, 11] > want[:, 11]).any()
    seen = M.merge_tables([_hip.measure_labels(dev[:4], above=dev[4]), _hip.measure_labels(dev[4:], below=dev[3], z_base=4)])
    np.testing.assert_array_equal(seen.cpu().numpy(), want)
    with pytest.raises(ValueError, match='single slice'):
        _hip.measure_labels(dev, block_voxels=256 * 256 - 1)
    for bad in (0, -1, 2 ** 31, 1.5, True):
        with pytest.raises(ValueError, match='block_voxels'):
            _hip.measure_labels(dev, block_voxels=bad)
    for kw in (dict(below=dev[0, :, :-1]), dict(above=dev[0].cpu()), dict(below=dev[0].view(torch.int32)), dict(z_base=-1),
               dict(z_base=1.0)):
        with pytest.raises(ValueError):
            _hip.measure_labels(dev, **kw)
    for bad in (dev[0], dev[:, :, ::2], dev.view(torch.int32).to(torch.int64)):
        with pytest.raises(ValueError):
            _hip.measure_labels(bad)


def test_volume_measurements(tmp_path):
    from empanada_amd import measurements as M
    from empanada_amd.zarr_utils import ZarrV2Group
    lab, want = _planted()
    ds = ZarrV2Group(str(tmp_path / 'gt.zarr')).create_dataset('lab', shape=lab.shape, dtype=np.uint32, chunks=(1, None, None))
    ds.write_slab(0, lab)
    for source in (lab, lab.astype(np.int64), _dev(lab), ds):
        for slab_rows in (1, 3, None):
            got = M.volume_measurements(source, slab_rows=slab_rows)
            assert isinstance(got, np.ndarray) and got.dtype == np.int64
            np.testing.assert_array_equal(got, want, err_msg=f'{type(source).__name__} slab_rows {slab_rows}')
    assert M.volume_measurements(np.zeros((3, 4, 5), np.uint8)).shape == (0, N_COL)
    for bad in (0, True, 2.0):
        with pytest.raises(ValueError, match='slab_rows'):
            M.volume_measurements(lab, slab_rows=bad)


# ------------------------------------------------------------------------------------------------------ infer_volume
PLAIN_KEYS = ['datasets', 'instances', 'volumes', 'z_range']


def _assert_objects(res, spacing=(1.0, 1.0, 1.0)):
    """res['objects'] is the checker's table of res['volumes']; one row per instance of a thing class"""
    from empanada_amd import measurements as M
    assert sorted(res['objects']) == [1, 2] and res['object_spacing'] == spacing
    for c in (1, 2):
        vol = _np(res['volumes'][c])
        table = res['objects'][c]
        assert isinstance(table, np.ndarray) and table.dtype == np.int64
        np.testing.assert_array_equal(table, measure_ref(vol), err_msg=f'class {c}')
    assert len(res['objects'][1]) == res['instances'][1] > 0
    assert res['objects'][2][:, 0].tolist() == [1]                          # a stuff class: label 1 alone
    d = M.derive(res['objects'][1], res['object_spacing'])
    assert (d['volume'] == res['objects'][1][:, 1] * spacing[0] * spacing[1] * spacing[2]).all()


def test_infer_volume_plain_path_with_a_store(tmp_path, case):
    from empanada_amd import measurements as M
    from empanada_amd.zarr_utils import ZarrV2Group
    eng, vol, vols, sets, counts = case(ORTHO)
    path = tmp_path / 'm.zarr'
    res = _run(eng, vol, path, axes=ORTHO, measure=(40., 8., 8.), pyramid=1)
    _assert_objects(res, (40.0, 8.0, 8.0))
    assert dict(res['instances']) == counts
    g = ZarrV2Group(str(path), mode='r')
    for c in (1, 2):
        np.testing.assert_array_equal(_np(res['volumes'][c]), vols[c])
        np.testing.assert_array_equal(np.asarray(res['datasets'][c]), sets[c])
        name = NAMES[c].replace('_pred', '_objects')
        ds = res['object_datasets'][c]
        assert ds.path == os.path.join(str(path), name) and name in g
        assert ds.dtype == np.int64 and ds.shape == res['objects'][c].shape and ds.chunks == ds.shape
        assert ds.meta['compressor'] is None
        np.testing.assert_array_equal(np.asarray(g[name]), res['objects'][c])
    attrs = g.attrs
    assert attrs['objects'] == {'columns': list(M.COLUMNS), 'spacing': [40.0, 8.0, 8.0]}
    assert [e['name'] for e in attrs['multiscales']] == [NAMES[1], NAMES[2]]          # what was there survives
    assert sorted(attrs) == ['multiscales', 'objects']
    d = M.derive(res['objects'][1], res['object_spacing'])
    t = res['objects'][1]
    assert (d['surface_area'] == t[:, 11] * 64.0 + t[:, 12] * 320.0 + t[:, 13] * 320.0).all()
    # measure=None: the parent's keys and the parent's datasets, nothing else
    plain = _run(eng, vol, tmp_path / 'n.zarr', axes=ORTHO)
    assert sorted(plain) == PLAIN_KEYS
    assert sorted(os.listdir(str(tmp_path / 'n.zarr'))) == ['.zgroup', 'er_pred', 'mito_pred']
    # without a store: the tables alone
    bare = _run(eng, vol, None, axes=ORTHO, measure=True)
    _assert_objects(bare)
    assert sorted(bare) == sorted(PLAIN_KEYS + ['objects', 'object_spacing'])
    np.testing.assert_array_equal(bare['objects'][1], res['objects'][1])


def test_infer_volume_stack_mode_and_windows(tmp_path, case):
    eng, vol, vols, _, counts = case(('xy',))
    res = _run(eng, vol, None, axes=('xy',), measure=True)
    _assert_objects(res)
    assert dict(res['instances']) == counts
    np.testing.assert_array_equal(_np(res['volumes'][1]), vols[1])
    kw = dict(axes=('xy',), batch_pixels=4 * 96 * 96, window_slices=8)      # 4 slices per model call, windows of 8
    win = _run(eng, vol, tmp_path / 'w.zarr', measure=True, **kw)
    assert win['windows']['xy'] > 1
    _assert_objects(win)
    np.testing.assert_array_equal(np.asarray(win['object_datasets'][1]), win['objects'][1])
    assert sorted(_run(eng, vol, None, **kw)) == sorted(PLAIN_KEYS + ['windows', 'head_bytes'])


def test_infer_volume_pipeline(tmp_path, case):
    from empanada_amd.inference.pipeline import VolumePipeline
    eng, vol, vols, sets, counts = case(ORTHO)
    pipe = VolumePipeline(eng, tune=False, graph=True, overlap=True, batch_pixels=1 << 22)
    try:
        res = _run(eng, vol, tmp_path / 'a.zarr', axes=ORTHO, measure=True, pipeline=pipe)
        _assert_objects(res)
        assert dict(res['instances']) == counts
        for c in (1, 2):
            np.testing.assert_array_equal(_np(res['volumes'][c]), vols[c])
            np.testing.assert_array_equal(np.asarray(res['object_datasets'][c]), res['objects'][c])
        plain = _run(eng, vol, tmp_path / 'b.zarr', axes=ORTHO, pipeline=pipe)
        assert sorted(plain) == sorted(PLAIN_KEYS + ['pipeline'])
        assert sorted(os.listdir(str(tmp_path / 'b.zarr'))) == ['.zgroup', 'er_pred', 'mito_pred']
    finally:
        pipe.close()


def test_a_class_without_objects(tmp_path):
    """the step infer_volume applies to its result, on volumes of which one is empty: that class has a (0, 14) table, which
    the store holds as a zero-row array; a store that cannot is recorded as None"""
    from empanada_amd.inference import driver
    from empanada_amd.zarr_utils import ZarrV2Group
    full = np.zeros((4, 6, 9), np.uint8)
    full[1:3, 2:5, 3:8] = 1
    vols = {1: torch.zeros((4, 6, 9), dtype=torch.int32, device='cuda').view(torch.uint32), 2: _dev(full)}

    def run(out):
        return driver._measured({'volumes': vols, 'z_range': (3, 7)}, (1.0, 1.0, 1.0), [1, 2], {1: 'mito', 2: 'er'}, out, None)

    res = run(ZarrV2Group(str(tmp_path / 'z.zarr')))
    assert res['objects'][1].shape == (0, N_COL) and res['objects'][1].dtype == np.int64
    np.testing.assert_array_equal(res['objects'][2], measure_ref(full, z_base=3))
    ds = res['object_datasets'][1]
    assert ds is not None and ds.shape == (0, N_COL) and ds.dtype == np.int64 and np.asarray(ds).shape == (0, N_COL)
    np.testing.assert_array_equal(np.asarray(res['object_datasets'][2]), res['objects'][2])

    class NoEmpty(ZarrV2Group):
        def create_dataset(self, name, shape, **kw):
            if 0 in tuple(shape):
                raise ValueError("no zero-length axes here")
            return super().create_dataset(name, shape=shape, **kw)

    res = run(NoEmpty(str(tmp_path / 'y.zarr')))
    assert res['object_datasets'][1] is None and sorted(os.listdir(str(tmp_path / 'y.zarr'))) == ['.zattrs', '.zgroup', 'er_objects']
    np.testing.assert_array_equal(np.asarray(res['object_datasets'][2]), res['objects'][2])


# ----------------------------------------------------------------------------------------------- two ranks over gloo
def _rank(rank, world, port, path, q):
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        eng, vol = _engine(), SY.em_volume(SHAPE, seed=3)
        res = _run(eng, vol, path, axes=ORTHO, group=dist.group.WORLD, measure=(2.0, 1.0, 1.0))
        q.put((rank, tuple(res['z_range']), res['objects'], res['object_spacing'], dict(res['instances']),
               {c: np.asarray(a) for c, a in res['object_datasets'].items()}))
    finally:
        dist.destroy_process_group()


def test_infer_volume_two_ranks(tmp_path, case):
    import torch.multiprocessing as mp
    from empanada_amd.zarr_utils import ZarrV2Group
    eng, vol, vols, sets, counts = case(ORTHO)
    want = {c: measure_ref(vols[c]) for c in (1, 2)}
    crossing = (want[1][:, 2] < 20) & (want[1][:, 5] > 20)
    assert crossing.any(), "no object crosses the border between the two ranks' slabs"
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
            np.testing.assert_array_equal(got[r][4][c], want[c], err_msg=f'rank {r} dataset of class {c}')
    for c in (1, 2):
        np.testing.assert_array_equal(np.asarray(g[NAMES[c]]), sets[c])
        np.testing.assert_array_equal(np.asarray(g[NAMES[c].replace('_pred', '_objects')]), want[c])
    assert g.attrs['objects']['spacing'] == [2.0, 1.0, 1.0]
