"""GPU: the surface meshes (emp_label_mesh.hip; include/emp_hip.h, E7) bit for bit against the numpy checker
(mesh_ref.py), the smoothing against its float64 smoother, and infer_volume(mesh=) on every path."""
import os
import queue
import time

import numpy as np
import pytest
import torch

from empanada_amd import meshes as MS
from empanada_amd import synthetic as SY
from mesh_ref import emit_ref, finish_ref, hand_cases, mesh_ref, neighbours_ref, random_volume, taubin_ref
from test_measure_host import measure_ref
from test_pyramid_gpu import KW, NAMES, ORTHO, SHAPE, _dev, _engine, _free_port, _np, _run, case  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

# W of 1, one below, at and above a wave, and two waves; single-row and single-slice volumes
SHAPES = [(1, 1, 1), (1, 1, 67), (5, 1, 64), (5, 7, 67), (3, 33, 130), (9, 16, 64)]
# max |device float32 - float64 checker| after 10 Taubin iterations over SHAPES, measured on an MI355X, was 5.347e-05 =
# 2^-14.19 voxel, at (3, 33, 130) (profiles/label_mesh.md); 16 x that = 8.56e-04, rounded up to a power of two.  It must
# not exceed 2^-10 voxel, and does not.
SMOOTH_TOL = 2.0 ** -10
assert SMOOTH_TOL <= 2.0 ** -10
_CACHE = {}


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _mesh(vol, **kw):
    """(raw keys, raw quad keys, raw codes, finished mesh as numpy arrays) of a host volume"""
    from empanada_amd import _hip
    dev = _dev(vol)
    keys, (qk, qd) = _hip.label_mesh(dev, **kw)
    v, q, o = _hip.mesh_finish(keys, (qk, qd), vol.shape)
    return _u64(keys), _u64(qk), qd.cpu().numpy(), {'vertices': v.cpu().numpy(), 'quads': q.cpu().numpy(),
                                                    'objects': o.cpu().numpy()}


def _assert_mesh(got, want):
    for k in ('vertices', 'quads', 'objects'):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


@pytest.mark.parametrize('dtype', [np.uint8, np.uint32], ids=['u8', 'u32'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_label_mesh_equals_the_checker(shape, dtype):
    vol = random_volume(shape, seed=sum(shape), dtype=dtype, big=dtype == np.uint32)
    info = {}
    keys, qk, qd, got = _mesh(vol, info=info)
    # corner order is ascending in the corner, not in the key: sort what one call emitted by corner
    wk, wq, wd = emit_ref(vol)
    np.testing.assert_array_equal(np.sort(keys), wk)
    corner = keys & np.uint64(0xffffffff)
    assert (np.diff(corner.astype(np.int64)) >= 0).all()
    np.testing.assert_array_equal(qk, wq)
    np.testing.assert_array_equal(qd, wd)
    _assert_mesh(got, mesh_ref(vol))
    assert info['blocks'] == 1 and info['vertices'] == len(wk) and info['quads'] == len(wq) and info['work_bytes'] > 0
    if dtype == np.uint32 and (vol >= 2 ** 31).any():
        assert got['objects'][-1, 0] == 2 ** 31 + 7


@pytest.mark.parametrize('name', list(hand_cases()))
def test_hand_cases(name):
    vol = hand_cases()[name]
    got = _mesh(vol)[3]
    _assert_mesh(got, mesh_ref(vol))
    counts = {'one': (8, 6), 'edge': (14, 12), 'corner': (15, 12), 'pair': (16, 12), 'eight': (64, 48), 'ends': (16, 12),
              'full': (60 - 6, 2 * (6 + 12 + 8))}[name]
    assert (len(got['vertices']), len(got['quads'])) == counts


def test_int32_bits_are_taken_as_they_are():
    from empanada_amd import _hip
    vol = random_volume((3, 5, 9), seed=11, big=True)
    keys, (qk, qd) = _hip.label_mesh(torch.from_numpy(vol.view(np.int32)).cuda())
    _assert_mesh(dict(zip(('vertices', 'quads', 'objects'),
                          (t.cpu().numpy() for t in _hip.mesh_finish(keys, (qk, qd), vol.shape)))), mesh_ref(vol))


@pytest.mark.parametrize('dtype', [np.uint8, np.uint32], ids=['u8', 'u32'])
def test_neighbour_slices_stand_for_the_volume_around(dtype):
    from empanada_amd import _hip
    big = random_volume((9, 16, 64), seed=21, dtype=dtype)
    for z0, z1, top in ((2, 6, False), (0, 4, False), (5, 9, True), (3, 4, False), (2, 6, True)):
        kw = dict(below=big[z0 - 1] if z0 else None, above=big[z1] if z1 < 9 else None, z_base=z0, top=top)
        keys, (qk, qd) = _hip.label_mesh(_dev(big[z0:z1]), depth=9, **{k: (_dev(v) if isinstance(v, np.ndarray) else v)
                                                                      for k, v in kw.items()})
        wk, wq, wd = emit_ref(big[z0:z1], **kw)
        np.testing.assert_array_equal(np.sort(_u64(keys)), wk, err_msg=f'{z0}:{z1}')
        np.testing.assert_array_equal(_u64(qk), wq)
        np.testing.assert_array_equal(qd.cpu().numpy(), wd)
    # the slabs of a partition, each with its true neighbour slices, concatenate to the whole
    parts = [_hip.label_mesh(_dev(big[a:b]), below=_dev(big[a - 1]) if a else None, above=_dev(big[b]) if b < 9 else None,
                             z_base=a, depth=9, top=b == 9) for a, b in ((0, 2), (2, 3), (3, 9))]
    keys = torch.cat([p[0] for p in parts])
    quads = (torch.cat([p[1][0] for p in parts]), torch.cat([p[1][1] for p in parts]))
    got = dict(zip(('vertices', 'quads', 'objects'), (t.cpu().numpy() for t in _hip.mesh_finish(keys, quads, big.shape))))
    _assert_mesh(got, mesh_ref(big))


@pytest.mark.parametrize('offset', [1, 2, 3])
def test_unaligned_slab_takes_the_narrow_path(offset):
    """the slab starts 1, 2 or 3 elements off a 16-byte (uint32) / 4-byte (uint8) address and its neighbour slices at yet
    another offset; W = 7 cuts a group at both ends of every row, and the rows of 7 elements put the aligned load and the
    voxel-by-voxel one on different rows: same keys, same quads, same mesh"""
    from empanada_amd import _hip
    shape = (3, 5, 7)
    for dtype, tdt in ((np.uint32, torch.int32), (np.uint8, torch.uint8)):
        a = random_volume(shape, seed=40 + offset, density=0.5, dtype=dtype, big=dtype == np.uint32)
        ends = random_volume((2,) + shape[1:], seed=50 + offset, density=0.5, dtype=dtype)
        flat = torch.zeros((a.size + ends.size + 32,), dtype=tdt, device='cuda')
        flat[offset:offset + a.size] = _dev(a).view(tdt).ravel()
        at = offset + a.size
        at += (offset + 2 - at) % 4                                         # the neighbour slices at yet another offset
        flat[at:at + ends.size] = _dev(ends).view(tdt).ravel()
        view = (lambda t: t.view(torch.uint32)) if dtype == np.uint32 else (lambda t: t)
        dev = view(flat[offset:offset + a.size]).view(a.shape)
        nb = view(flat[at:at + ends.size]).view(ends.shape)
        assert dev.data_ptr() % (4 * dev.element_size()) != 0 and dev.is_contiguous()
        assert nb.data_ptr() % (4 * nb.element_size()) != dev.data_ptr() % (4 * dev.element_size())
        keys, (qk, qd) = _hip.label_mesh(dev, below=nb[0], above=nb[1], z_base=2)
        wk, wq, wd = emit_ref(a, below=ends[0], above=ends[1], z_base=2)
        np.testing.assert_array_equal(np.sort(_u64(keys)), wk, err_msg=str(dtype))
        np.testing.assert_array_equal(_u64(qk), wq, err_msg=str(dtype))
        np.testing.assert_array_equal(qd.cpu().numpy(), wd, err_msg=str(dtype))
        got = dict(zip(('vertices', 'quads', 'objects'),
                       (t.cpu().numpy() for t in _hip.mesh_finish(keys, (qk, qd), shape))))
        _assert_mesh(got, finish_ref(wk, wq, wd, shape[1], shape[2]))
        assert len(wq) and (a != 0).any() and (ends != 0).any()


@pytest.mark.parametrize('slices', [1, 2])
def test_z_blocks_equal_the_uncut_call(slices):
    from empanada_amd import _hip
    vol = random_volume((5, 7, 67), seed=31)
    dev = _dev(vol)
    whole = _hip.label_mesh(dev)
    info = {}
    cut = _hip.label_mesh(dev, block_voxels=slices * 7 * 67, info=info)
    assert info['blocks'] == -(-5 // slices)
    assert torch.equal(cut[0], whole[0]) and torch.equal(cut[1][0], whole[1][0]) and torch.equal(cut[1][1], whole[1][1])
    assert info['vertices'] == whole[0].numel() and info['quads'] == whole[1][0].numel()


def test_empty_and_all_zero_slabs():
    from empanada_amd import _hip
    for shape in ((0, 4, 5), (3, 4, 5)):
        info = {}
        keys, (qk, qd) = _hip.label_mesh(torch.zeros(shape, dtype=torch.uint8, device='cuda'), info=info)
        assert keys.shape == (0,) and qk.shape == (0,) and qd.shape == (0,) and info['vertices'] == info['quads'] == 0
        assert keys.dtype == torch.int64 and qk.dtype == torch.int64 and qd.dtype == torch.int32
        v, q, o = _hip.mesh_finish(keys, (qk, qd), shape)
        assert v.shape == (0, 3) and q.shape == (0, 4) and o.shape == (0, 5)
        assert v.dtype == torch.int32 and q.dtype == torch.int32 and o.dtype == torch.int64
        p = _hip.mesh_smooth(v, q, 3)
        assert p.shape == (0, 3) and p.dtype == torch.float32


def test_refusals():
    from empanada_amd import _hip
    slab = torch.ones((2, 3, 4), dtype=torch.uint8, device='cuda')
    plane = torch.zeros((3, 4), dtype=torch.uint8, device='cuda')
    bad = [dict(slab=slab.cpu()), dict(slab=slab.float()), dict(slab=slab[0]), dict(slab=slab[:, :, ::2]),
           dict(below=plane[:2]), dict(above=plane.int()), dict(below=plane.cpu()), dict(above=plane.t().contiguous().t()),
           dict(z_base=-1), dict(z_base=1.5), dict(z_base=True), dict(depth=1), dict(z_base=4, depth=5), dict(top=1),
           dict(block_voxels=0), dict(block_voxels=2 ** 26 + 1), dict(block_voxels=11)]
    for kw in bad:
        with pytest.raises(ValueError, match='label_mesh'):
            _hip.label_mesh(**{'slab': slab, **kw})
    # the corner limit, through the wrapper's arithmetic: (depth + 1) * 4 * 5 corners
    limit = 2 ** 32 // 20 - 1
    keys, _ = _hip.label_mesh(slab, z_base=limit - 2, depth=limit)
    assert int(_u64(keys).max() & np.uint64(0xffffffff)) == (limit + 1) * 20 - 1
    with pytest.raises(ValueError, match=r'2\^32'):
        _hip.label_mesh(slab, depth=limit + 1)
    keys, quads = _hip.label_mesh(slab)
    for args in ((keys, quads[0], (2, 3, 4)), (keys.int(), quads, (2, 3, 4)), (keys, (quads[0], quads[1][:1]), (2, 3, 4)),
                 (keys, (quads[0].cpu(), quads[1]), (2, 3, 4)), (keys, quads, (0, 4)), (keys, quads, (2 ** 16, 2 ** 16))):
        with pytest.raises(ValueError, match='mesh_finish'):
            _hip.mesh_finish(*args)
    v, q, _ = _hip.mesh_finish(keys, quads, (2, 3, 4))
    for args in ((v, q, -1), (v, q, 1.5), (v, q, True), (v.float(), q, 1), (v, q[:, :3], 1), (v, q, 1, 2.0), (v, q, 1, 0.5, 'x')):
        with pytest.raises(ValueError, match='mesh_'):
            _hip.mesh_smooth(*args)
    with pytest.raises(ValueError, match='iterations'):
        MS.mesh_volume(slab, iterations=-1)


# ------------------------------------------------------------------------------------------------------ smoothing
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_smoothing(shape):
    from empanada_amd import _hip
    vol = random_volume(shape, seed=sum(shape), big=True)
    want = mesh_ref(vol)
    dev = _dev(vol)
    keys, quads = _hip.label_mesh(dev)
    v, q, _ = _hip.mesh_finish(keys, quads, shape)
    np.testing.assert_array_equal(_hip.mesh_neighbours(v, q).cpu().numpy(), neighbours_ref(want['vertices'], want['quads']))
    np.testing.assert_array_equal(_hip.mesh_smooth(v, q, 0).cpu().numpy(), want['vertices'].astype(np.float32))
    got = _hip.mesh_smooth(v, q, 10)
    assert got.dtype == torch.float32 and got.shape == v.shape
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - taubin_ref(want['vertices'], want['quads'], 10)).max(initial=0.0))
    print(f"smoothing {shape}: max |device - checker| = {err:.3e} = 2^{np.log2(max(err, 1e-300)):.2f}")
    assert err <= SMOOTH_TOL
    assert torch.equal(_hip.mesh_smooth(v, q, 10), got)                         # run to run
    assert torch.equal(v, torch.from_numpy(want['vertices']).cuda())            # the input stays


# ------------------------------------------------------------------------------------------------------ ranks
RANK_BOUNDS = [(0, 4, 9), (0, 1, 9), (0, 0, 9), (0, 9, 9)]


def _rank_volume():
    return random_volume((9, 16, 64), seed=41, big=True)


def _rank(rank, world, port, q, infer):
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        vol, out = _rank_volume(), []
        for b in RANK_BOUNDS:
            for it in (0, 2):
                m = MS.mesh_volume(_dev(vol[b[rank]:b[rank + 1]]), dist.group.WORLD, b[rank], 9, it)
                out.append({k: v.cpu().numpy() for k, v in m.items()})
        res = None
        if infer:
            eng, em = _engine(), SY.em_volume(SHAPE, seed=3)
            r = _run(eng, em, None, axes=ORTHO, group=dist.group.WORLD, mesh=True, measure=True)
            res = (tuple(r['z_range']), r['meshes'], r['objects'])
        q.put((rank, out, res))
    finally:
        dist.destroy_process_group()


def test_two_ranks(case):
    """every rank holds the whole mesh of the single-rank call, whichever way the slices are dealt -- one split leaves a
    rank empty.  Also infer_volume(mesh=) over two ranks."""
    import torch.multiprocessing as mp
    eng, em, vols, sets, counts = case(ORTHO)
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank, args=(r, 2, port, q, True)) for r in range(2)]
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
    vol = _rank_volume()
    want = mesh_ref(vol)
    smooth = taubin_ref(want['vertices'], want['quads'], 2)
    i = 0
    for b in RANK_BOUNDS:
        for it in (0, 2):
            for r in (0, 1):
                m = got[r][0][i]
                if it == 0:
                    _assert_mesh(m, want)
                else:
                    assert m['vertices'].dtype == np.float32 and np.abs(m['vertices'] - smooth).max() <= SMOOTH_TOL
                    np.testing.assert_array_equal(m['quads'], want['quads'])
                    np.testing.assert_array_equal(m['objects'], want['objects'])
            np.testing.assert_array_equal(got[0][0][i]['vertices'], got[1][0][i]['vertices'])
            i += 1
    want = mesh_ref(vols[1])
    assert got[0][1][0] == (0, 20) and got[1][1][0] == (20, 40)
    for r in (0, 1):
        assert list(got[r][1][1]) == [1]
        _assert_mesh(got[r][1][1][1], want)
        np.testing.assert_array_equal(got[r][1][2][1], measure_ref(vols[1]))


# ------------------------------------------------------------------------------------------------------ infer_volume
def _want(vols):
    key = ('mesh', id(vols[1]))
    if key not in _CACHE:
        _CACHE[key] = mesh_ref(vols[1])
    return _CACHE[key]


def _assert_meshed(res, vols, iterations=0):
    want = _want(vols)
    assert list(res['meshes']) == [1]                                           # a stuff class has no mesh
    got = res['meshes'][1]
    assert all(isinstance(a, np.ndarray) for a in got.values())
    if iterations == 0:
        _assert_mesh(got, want)
    else:
        assert got['vertices'].dtype == np.float32
        err = np.abs(got['vertices'] - taubin_ref(want['vertices'], want['quads'], iterations)).max()
        assert err <= SMOOTH_TOL
        np.testing.assert_array_equal(got['quads'], want['quads'])
        np.testing.assert_array_equal(got['objects'], want['objects'])
    if 'objects' in res:
        # measure= counts the faces that mesh= emits: per object and axis, and the rows carry the same labels
        table = res['objects'][1]
        np.testing.assert_array_equal(got['objects'][:, 0], table[:, 0])
        p = want['vertices'][got['quads']]
        axis = (p.max(axis=1) == p.min(axis=1)).argmax(axis=1)
        for row, (_, _, _, q0, q1) in zip(table, got['objects']):
            assert np.bincount(axis[q0:q1], minlength=3).tolist() == row[11:14].tolist()
    if 'mesh_datasets' in res:
        for k, ds in res['mesh_datasets'][1].items():
            a = np.asarray(ds[...])
            assert a.dtype == got[k].dtype
            np.testing.assert_array_equal(a, got[k])


def test_infer_volume_plain_path_with_a_store(tmp_path, case):
    from empanada_amd.zarr_utils import ZarrV2Group
    eng, vol, vols, sets, counts = case(ORTHO)
    res = _run(eng, vol, tmp_path / 'm.zarr', axes=ORTHO, mesh=True, measure=True)
    _assert_meshed(res, vols)
    assert dict(res['instances']) == counts and _np(res['volumes'][1]).tobytes() == vols[1].tobytes()
    root = ZarrV2Group(str(tmp_path / 'm.zarr'))
    assert {'mito_mesh_vertices', 'mito_mesh_quads', 'mito_mesh_objects'} <= set(os.listdir(root.path))
    assert not any(n.startswith('er_mesh') for n in os.listdir(root.path))
    assert root.attrs['meshes'] == {'axes': 'zyx', 'object_columns': list(MS.OBJECT_COLUMNS), 'iterations': 0}
    assert 'objects' in root.attrs                                              # beside what measure= wrote
    smooth = _run(eng, vol, tmp_path / 's.zarr', axes=ORTHO, mesh=3)
    _assert_meshed(smooth, vols, 3)
    assert ZarrV2Group(str(tmp_path / 's.zarr')).attrs['meshes']['iterations'] == 3
    # a class without objects: zero-row arrays, in the store where it can hold them
    none = _run(eng, vol, tmp_path / 'z.zarr', axes=ORTHO, mesh=2, min_size=10 ** 9)
    m = none['meshes'][1]
    assert m['vertices'].shape == (0, 3) and m['quads'].shape == (0, 4) and m['objects'].shape == (0, 5)
    assert m['vertices'].dtype == np.float32
    ds = none['mesh_datasets'][1]
    assert ds is None or all(tuple(ds[k].shape) == m[k].shape for k in m)


def test_mesh_none_adds_no_key_and_no_launch(case, monkeypatch):
    from empanada_amd import _hip
    eng, vol, vols, sets, counts = case(ORTHO)
    for name in ('label_mesh', 'mesh_finish', 'mesh_smooth'):
        monkeypatch.setattr(_hip, name, lambda *a, _n=name, **k: pytest.fail(f"{_n} was called"))
    monkeypatch.setattr(MS, 'mesh_volume', lambda *a, **k: pytest.fail("mesh_volume was called"))
    off = _run(eng, vol, None, axes=ORTHO, mesh=None)
    assert sorted(off) == ['datasets', 'instances', 'volumes', 'z_range'] and dict(off['instances']) == counts
    for c in (1, 2):
        assert _np(off['volumes'][c]).tobytes() == vols[c].tobytes()


def test_infer_volume_after_the_repairs(case):
    """the mesh is that of the FINAL volume: after morph, separate, split_objects and fill_holes"""
    eng, vol, vols, sets, counts = case(ORTHO)
    res = _run(eng, vol, None, axes=ORTHO, morph=('open', 1), split_objects=6, fill_holes=True, mesh=True, measure=True)
    final = _np(res['volumes'][1])
    assert final.tobytes() != vols[1].tobytes()
    _assert_mesh(res['meshes'][1], mesh_ref(final))
    np.testing.assert_array_equal(res['meshes'][1]['objects'][:, 0], res['objects'][1][:, 0])


def test_infer_volume_stack_mode_and_windows(tmp_path, case):
    eng, vol, vols, _, counts = case(('xy',))
    _assert_meshed(_run(eng, vol, None, axes=('xy',), mesh=True, measure=True), vols)
    kw = dict(axes=('xy',), batch_pixels=4 * 96 * 96, window_slices=8)      # 4 slices per model call, windows of 8
    win = _run(eng, vol, tmp_path / 'w.zarr', mesh=3, **kw)
    assert win['windows']['xy'] > 1
    _assert_meshed(win, vols, 3)


def test_infer_volume_pipeline(tmp_path, case):
    from empanada_amd.inference.pipeline import VolumePipeline
    eng, vol, vols, sets, counts = case(ORTHO)
    pipe = VolumePipeline(eng, tune=False, graph=True, overlap=True, batch_pixels=1 << 22)
    try:
        for i, mesh in enumerate((True, 3)):
            res = _run(eng, vol, tmp_path / f'{i}.zarr', axes=ORTHO, mesh=mesh, measure=True, pipeline=pipe)
            _assert_meshed(res, vols, 0 if mesh is True else mesh)
        off = _run(eng, vol, None, axes=ORTHO, pipeline=pipe)
        assert 'meshes' not in off and dict(off['instances']) == counts
    finally:
        pipe.close()


def test_infer_volume_rejects_a_bad_mesh_before_any_work(case):
    eng, vol, _, _, _ = case(ORTHO)
    before = torch.cuda.memory_allocated()
    for bad in (False, -1, 1.5, 'yes', (1, 2)):
        with pytest.raises(ValueError, match='mesh'):
            _run(eng, vol, None, axes=ORTHO, mesh=bad)
    assert torch.cuda.memory_allocated() == before
