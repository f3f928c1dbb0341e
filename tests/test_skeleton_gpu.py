"""GPU: _hip.skel_classify equals the checker's predicates and is invariant under the cube's symmetries; _hip.label_thin
equals the sequential thinning of skeleton_ref.py -- bit for bit -- over tile borders, z-blocks, halos and ranks;
_hip.label_graph / graph_finish equal the checker's graph; infer_volume(skeleton=) thins the final volumes on every
path."""
import itertools
import os
import queue
import time

import numpy as np
import pytest
import torch
from scipy import ndimage
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

import skeleton_ref as ref
from empanada_amd import skeletons as SK
from empanada_amd import synthetic as SY
from test_pyramid_gpu import KW, NAMES, ORTHO, SHAPE, _dev, _engine, _free_port, _np, _run, case  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (2, 3, 5), (9, 9, 65), (3, 17, 130), (20, 24, 40), (17, 10, 70)]
KEYS = ('vertices', 'degree', 'edges', 'objects')
_CACHE = {}


def _classify(masks):
    from empanada_amd import _hip
    return _hip.skel_classify(torch.from_numpy(np.asarray(masks, np.int64).astype(np.uint32).view(np.int32)).cuda()).cpu().numpy()


# ------------------------------------------------------------------------------------------------------ the predicate
def test_skel_classify_equals_the_checker():
    few = [0] + [1 << a for a in range(26)] + [(1 << a) | (1 << b) for a in range(26) for b in range(a + 1, 26)]
    assert len(few) == 352
    rng = np.random.default_rng(26)
    rand = [int(m) for d in np.linspace(0.1, 0.9, 8) for m in
            (rng.random((512, 26)) < d).astype(np.int64) @ (1 << np.arange(26, dtype=np.int64))]
    assert len(rand) == 4096
    masks = few + [m ^ 0x3ffffff for m in few] + rand
    got = _classify(masks)
    want = np.array([ref.classify(m) for m in masks], np.uint8)
    np.testing.assert_array_equal(got, want)
    assert set(np.unique(got)) == {0, 1, 2}
    np.testing.assert_array_equal(_classify([m | 0xfc000000 for m in rand[:64]]), want[-4096:][:64])   # bits 26 .. 31


def _symmetries():
    """the 48 symmetries of the cube as permutations of the 26 bit positions"""
    index = {tuple(o): n for n, o in enumerate(ref.OFFSETS)}
    out = []
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1, -1), repeat=3):
            out.append(np.array([index[tuple(int(signs[a] * o[perm[a]]) for a in range(3))] for o in ref.OFFSETS]))
    return out


def test_skel_classify_is_invariant_under_the_symmetries_of_the_cube():
    from empanada_amd import _hip
    g = torch.Generator(device='cuda').manual_seed(48)
    bits = torch.rand((1 << 20, 26), device='cuda', generator=g) < torch.rand((1 << 20, 1), device='cuda', generator=g)
    weights = (1 << torch.arange(26, device='cuda', dtype=torch.int64))
    first = _hip.skel_classify((bits.long() * weights).sum(1).to(torch.int32))
    assert len(torch.unique(first)) == 3
    syms = _symmetries()
    assert len({tuple(s) for s in syms}) == 48
    for s in syms:
        moved = (bits[:, torch.from_numpy(s).cuda()].long() * weights).sum(1).to(torch.int32)
        assert torch.equal(_hip.skel_classify(moved.contiguous()), first)


# ------------------------------------------------------------------------------------------------------ the volumes
def crossing(shape):
    """thin objects across tile faces, edges and the tile corner (8, 8, 64); label 2 is 26-adjacent to label 1"""
    D, H, W = shape
    v = np.zeros(shape, np.uint8)
    cz, cy, cx = min(8, D // 2), min(8, H // 2), min(64, W // 2)
    v[max(cz - 1, 0):cz + 2, max(cy - 1, 0):cy + 2, :] = 1                  # along x, around the tile edge z = y = 8
    v[:, max(cy - 1, 0):cy + 2, max(cx - 2, 0):cx + 1] = 1                  # along z, against the face x = 64
    v[max(cz - 2, 0):cz + 1, :, cx + 1:cx + 4] = 2                          # along y, another label, touching
    for i in range(min(D, H)):                                              # a one-voxel diagonal through the corner
        x = cx - cz + i + 6
        if 0 <= x < W and v[i, i, x] == 0:
            v[i, i, x] = 3
    return v


def volumes(shape):
    """name -> uint32 volume with labels <= 255"""
    if shape not in _CACHE:
        out = {'solid': np.full(shape, 7, np.uint32), 'zero': np.zeros(shape, np.uint32),
               'crossing': crossing(shape).astype(np.uint32)}
        for seed in (0, 1):
            n = ref.noise(shape, seed + sum(shape))
            out[f'noise{seed}'] = np.where(n != 0, (n - 1) % 250 + 1, 0).astype(np.uint32)
        for name in ('bar', 'ball', 'torus', 'touching'):
            out[name] = ref.in_shape(getattr(ref, name)(), shape).astype(np.uint32)
        _CACHE[shape] = {k: (v, ref.thin(v)) for k, v in out.items()}
    return _CACHE[shape]


def _thin(vol, **kw):
    from empanada_amd import _hip
    dev = _dev(vol)
    info = {}
    got = _hip.label_thin(dev, info=info, **kw)
    assert got.dtype == dev.dtype and got.is_cuda and tuple(got.shape) == vol.shape
    np.testing.assert_array_equal(_np(dev), vol)                                # the input is not written
    return _np(got), info


@pytest.mark.parametrize('dtype', [np.uint8, np.uint32], ids=['u8', 'u32'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_label_thin_equals_the_checker(shape, dtype):
    for name, (vol, (want, iterations, deleted)) in volumes(shape).items():
        got, info = _thin(vol.astype(dtype))
        np.testing.assert_array_equal(got, want.astype(dtype), err_msg=name)
        assert info['iterations'] == iterations and info['voxels_deleted'] == deleted, name
        assert info['blocks'] == 1 and info['work_bytes'] >= vol.size
        if not vol.any():
            assert info['active_tiles'] == 0 and info['launches'] == 0


def test_counted_cases_and_the_ypsilon():
    v = volumes((20, 24, 40))
    for name, voxels, iterations in (('bar', 25, 5), ('ball', 1, 9), ('torus', 44, None)):
        got, info = _thin(v[name][0].astype(np.uint8))
        assert int((got != 0).sum()) == voxels and iterations in (None, info['iterations'])
    got, _ = _thin(v['touching'][0].astype(np.uint8))
    assert int((got == 1).sum()) == 1 and int((got == 2).sum()) == 1
    y = ref.ypsilon()
    got, _ = _thin(y)
    np.testing.assert_array_equal(got, ref.thin(y)[0].astype(np.uint8))
    assert ref.topology(got) == ref.topology(y)
    g = ref.graph(got)
    assert (g['degree'] == 1).sum() >= 3                                        # three arms end somewhere


def test_int32_bits_are_taken_as_they_are():
    from empanada_amd import _hip
    vol, (want, _, _) = volumes((17, 10, 70))['noise0']
    big = np.where(vol != 0, vol | np.uint32(0x80000000), 0).astype(np.uint32)
    big[vol == 3] = 2 ** 32 - 1
    got = _hip.label_thin(torch.from_numpy(big.view(np.int32)).cuda())
    assert got.dtype == torch.int32
    np.testing.assert_array_equal(got.cpu().numpy().view(np.uint32), np.where(want != 0, big, 0))


def test_ball_stopped_after_two_iterations():
    """an explicit max_iterations that is reached stops the thinning without an error: the twice-thinned ball.  With the
    default limit the ball needs 9 iterations."""
    ball = ref.ball()
    got, info = _thin(ball, max_iterations=2)
    want, iterations, _ = ref.thin(ball, max_iterations=2)
    assert iterations == 2 and info['iterations'] == 2
    np.testing.assert_array_equal(got, want.astype(np.uint8))
    assert 1 < int((got != 0).sum()) < int(ball.sum())


def test_empty_slabs_and_refusals():
    from empanada_amd import _hip
    empty = torch.zeros((0, 5, 7), dtype=torch.uint8, device='cuda')
    info = {}
    assert tuple(_hip.label_thin(empty, info=info).shape) == (0, 5, 7) and info['blocks'] == 0
    t = _hip.LabelThin(empty)
    assert t.ends() is None and t.iterate() == 0
    lab = torch.ones((4, 6, 8), dtype=torch.uint8, device='cuda')
    st = torch.ones((6, 8), dtype=torch.uint8, device='cuda')
    for bad, match in ((dict(slab=lab.permute(0, 2, 1)), 'contiguous'), (dict(slab=lab.float()), 'dtype'),
                       (dict(slab=lab[0]), r'\(D, H, W\)'), (dict(slab=lab, z_base=-1), 'z_base'),
                       (dict(slab=lab, z_base=1.0), 'z_base'), (dict(slab=lab, block_voxels=0), 'block_voxels'),
                       (dict(slab=lab, block_voxels=47), 'single slice'), (dict(slab=lab, max_iterations=0), 'max_iterations'),
                       (dict(slab=lab, max_iterations=True), 'max_iterations'), (dict(slab=lab, below=st), 'labels, state'),
                       (dict(slab=lab, below=(st, st.int())), 'dtype'), (dict(slab=lab, above=(st[:3], st)), 'expected'),
                       (dict(slab=lab, above=(st.cpu(), st)), 'GPU')):
        with pytest.raises(ValueError, match=match):
            _hip.label_thin(**bad)
    t = _hip.LabelThin(lab)
    with pytest.raises(ValueError, match='subfield'):
        t.run_pass(8)
    with pytest.raises(ValueError, match='overlap|expected|dtype'):
        t.paint(out=torch.zeros((4, 6, 9), dtype=torch.uint8, device='cuda'))
    wide = torch.full((2, 3, 4), 300, dtype=torch.int32, device='cuda')
    with pytest.raises(ValueError, match='255'):
        _hip.LabelThin(wide).paint(dtype=torch.uint8)


def test_the_iteration_limits(monkeypatch):
    """the call never loops without bound: with a counter that always reports a deletion the default limit, max(D, H, W)
    + 2, is a RuntimeError and an explicit one returns the volume as it then is"""
    from empanada_amd import _hip
    lab = torch.ones((4, 6, 8), dtype=torch.uint8, device='cuda')
    monkeypatch.setattr(_hip.LabelThin, 'deleted', lambda self: 1)
    info = {}
    with pytest.raises(RuntimeError, match='not settled after 10'):
        _hip.label_thin(lab, info=info)
    assert info['iterations'] == 10
    assert tuple(_hip.label_thin(lab, max_iterations=3, info=info).shape) == (4, 6, 8) and info['iterations'] == 3


# ------------------------------------------------------------------------------------------------------ partitions
def _partition_case():
    if 'partition' not in _CACHE:
        shape = (12, 10, 70)
        n = ref.noise(shape, 77)
        vol = np.where(n != 0, (n - 1) % 250 + 1, 0).astype(np.uint8)
        c = crossing(shape)
        vol = np.where(c != 0, c + 250, vol).astype(np.uint8)
        _CACHE['partition'] = (vol, ref.thin(vol))
    return _CACHE['partition']


def test_every_z_cut_in_lock_step_equals_the_whole():
    from empanada_amd import _hip
    vol, (want, iterations, deleted) = _partition_case()
    for cut in range(1, vol.shape[0]):
        a, b = _hip.LabelThin(_dev(vol[:cut]), 0), _hip.LabelThin(_dev(vol[cut:]), cut)
        while True:
            a.mark(None, b.ends()[0]), b.mark(a.ends()[1], None)
            for s in range(8):
                a.run_pass(s, None, b.ends()[0]), b.run_pass(s, a.ends()[1], None)
            if a.deleted() + b.deleted() == 0:
                break
            assert a.iterations <= iterations
        got = np.concatenate([_np(a.paint()), _np(b.paint())])
        np.testing.assert_array_equal(got, want.astype(np.uint8), err_msg=f'cut {cut}')
        assert a.iterations == b.iterations == iterations and a.voxels_deleted + b.voxels_deleted == deleted


def test_z_blocks_and_an_odd_z_base():
    vol, (want, iterations, deleted) = _partition_case()
    got, info = _thin(vol, block_voxels=4 * 700)
    assert info['blocks'] == 3 and info['iterations'] == iterations and info['voxels_deleted'] == deleted
    np.testing.assert_array_equal(got, want.astype(np.uint8))
    got, info = _thin(vol, block_voxels=700)
    assert info['blocks'] == 12
    np.testing.assert_array_equal(got, want.astype(np.uint8))
    # the slab from slice 1 on, under the volume's own numbering, with the true slice below it held fixed
    lower = vol.copy()
    lower[0] = 0
    whole = ref.thin(lower)[0]
    got, _ = _thin(lower[1:], z_base=1)
    np.testing.assert_array_equal(got, whole[1:].astype(np.uint8))
    np.testing.assert_array_equal(got, ref.thin(lower[1:], z_base=1)[0].astype(np.uint8))
    halo = (_dev(lower[0]), torch.ones(lower.shape[1:], dtype=torch.uint8, device='cuda'))   # alive, but label 0
    np.testing.assert_array_equal(_thin(lower[1:], z_base=1, below=halo, above=halo)[0], whole[1:].astype(np.uint8))
    other = ref.thin(lower[1:], z_base=0)[0]
    assert not np.array_equal(other, whole[1:])                                 # the parity of z_base matters
    np.testing.assert_array_equal(_thin(lower[1:], z_base=0)[0], other.astype(np.uint8))
    np.testing.assert_array_equal(_thin(lower[1:], z_base=2)[0], other.astype(np.uint8))


# ------------------------------------------------------------------------------------------------------ the graph
def _graph(vol, **kw):
    from empanada_amd import _hip
    info = {}
    v, e = _hip.label_graph(_dev(vol), info=info, **kw)
    return v, e, info


def _finish(v, e, shape):
    from empanada_amd import _hip
    vertices, degree, edges, objects, order = _hip.graph_finish(v, e, shape)
    assert order.dtype == torch.int32 and sorted(order.tolist()) == list(range(len(order)))
    return {'vertices': vertices.cpu().numpy(), 'degree': degree.cpu().numpy(), 'edges': edges.cpu().numpy(),
            'objects': objects.cpu().numpy()}


def _assert_graph(got, want):
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


def _arbiters(g, vol):
    """sum of the degrees = twice the edges, per object; the graph's components are the 26-components of the volume"""
    v, e = g['vertices'], g['edges']
    assert len(e) == 0 or (e[:, 0] < e[:, 1]).all()
    for label, v0, v1, e0, e1, iso, ends, junc in g['objects']:
        d = g['degree'][v0:v1]
        assert d.sum() == 2 * (e1 - e0)
        assert (iso, ends, junc) == ((d == 0).sum(), (d == 1).sum(), (d >= 3).sum())
        assert ((e[e0:e1] >= v0) & (e[e0:e1] < v1)).all()
        n = v1 - v0
        adj = coo_matrix((np.ones(e1 - e0), (e[e0:e1, 0] - v0, e[e0:e1, 1] - v0)), shape=(n, n))
        assert connected_components(adj, directed=False)[0] == \
            ndimage.label(ref.as_u32(vol) == np.uint32(label), structure=np.ones((3, 3, 3)))[1]


@pytest.mark.parametrize('dtype', [np.uint8, np.uint32], ids=['u8', 'u32'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_label_graph_equals_the_checker(shape, dtype):
    for name, (vol, (skel, _, _)) in volumes(shape).items():
        if name == 'solid' and np.prod(shape) > 2000:
            continue
        for s in ((skel,) if name != 'solid' else (skel, vol)):                  # a solid block is no skeleton
            s = s.astype(dtype)
            v, e, info = _graph(s)
            got = _finish(v, e, shape)
            want = ref.graph(s)
            _assert_graph(got, want)
            assert info['vertices'] == len(want['vertices']) and info['edges'] == len(want['edges'])
            _arbiters(got, s)


def _sparse(shape, seed, density=0.2, big=False):
    rng = np.random.default_rng(seed)
    labels = np.array([0, 1, 2, 200, 2 ** 31 + 5, 2 ** 32 - 1] if big else [0, 1, 2, 200], np.uint32)
    v = labels[rng.integers(1, len(labels), shape)]
    v[rng.random(shape) >= density] = 0
    return v


def test_graph_of_a_random_sparse_volume_and_of_z_blocks():
    from empanada_amd import _hip
    shape = (7, 9, 67)
    vol = _sparse(shape, 5, big=True)
    want = ref.graph(vol)
    v, e, _ = _graph(vol)
    got = _finish(v, e, shape)
    _assert_graph(got, want)
    _arbiters(got, vol)
    assert got['objects'][-1, 0] == 2 ** 32 - 1 and (got['degree'] >= 3).any()
    v2, e2, info = _graph(vol, block_voxels=3 * 9 * 67)
    assert info['blocks'] == 3
    assert all(torch.equal(a, b) for a, b in zip(v + e, v2 + e2))                 # bit-identical from any z-partition
    # two slabs with each other's end slices, concatenated in z order
    lo = _hip.label_graph(_dev(vol[:4]), above=_dev(vol[4]), z_base=0, depth=7)
    hi = _hip.label_graph(_dev(vol[4:]), below=_dev(vol[3]), z_base=4, depth=7)
    joined = [tuple(torch.cat([a, b]) for a, b in zip(lo[i], hi[i])) for i in (0, 1)]
    _assert_graph(_finish(joined[0], joined[1], shape), want)
    # int32 bits as they are; an all-zero and an empty slab
    v3 = _hip.label_graph(torch.from_numpy(vol.view(np.int32)).cuda())
    assert torch.equal(v3[0][0], v[0])
    zero = _graph(np.zeros((3, 4, 5), np.uint8))
    assert zero[0][0].numel() == 0 and zero[1][0].numel() == 0
    g = _finish(zero[0], zero[1], (4, 5))
    assert g['vertices'].shape == (0, 3) and g['edges'].shape == (0, 2) and g['objects'].shape == (0, 8)
    with pytest.raises(ValueError, match='2\\^32'):
        _hip.label_graph(_dev(vol), depth=2 ** 32)
    with pytest.raises(ValueError, match='single slice'):
        _hip.label_graph(_dev(vol), block_voxels=100)
    with pytest.raises(ValueError, match='expected|shape'):
        _hip.label_graph(_dev(vol), below=_dev(vol[0, :4]))


# ------------------------------------------------------------------------------------------------------ ranks
RANK_BOUNDS = [(0, 5, 12), (0, 1, 12), (0, 0, 12), (0, 12, 12)]


def _rank(rank, world, port, q, infer):
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        vol, out = _partition_case()[0], []
        for b in RANK_BOUNDS:
            part = _dev(vol[b[rank]:b[rank + 1]])
            thin = _np(SK.thin_volume(part, dist.group.WORLD, b[rank]))
            s = SK.skeleton_volume(part, dist.group.WORLD, b[rank], 12, 9, (1, 1, 1))
            out.append((thin, {k: v.cpu().numpy() for k, v in s.items()}))
        res = None
        if infer:
            eng, em = _engine(), SY.em_volume(SHAPE, seed=3)
            r = _run(eng, em, None, axes=ORTHO, group=dist.group.WORLD, skeleton=True)
            res = (tuple(r['z_range']), r['skeletons'])
        q.put((rank, out, res))
    finally:
        dist.destroy_process_group()


def _radius2(vol, vertices, cap, sampling=(1, 1, 1)):
    from empanada_amd import _hip
    edt = _hip.label_edt(_dev(vol), sampling, cap).cpu().numpy()
    return edt[vertices[:, 0], vertices[:, 1], vertices[:, 2]].astype(np.int32)


def _want_skeleton(vol, cap=4096, sampling=(1, 1, 1)):
    want = ref.graph(ref.thin(vol)[0])
    want['radius2'] = _radius2(vol, want['vertices'], cap, sampling)
    return want


def _assert_skeleton(got, want):
    _assert_graph(got, want)
    assert got['radius2'].dtype == np.int32
    np.testing.assert_array_equal(got['radius2'], want['radius2'])


def test_two_ranks(case):
    """every rank's slab is its part of the single-rank skeleton and every rank holds the whole graph, whichever way the
    slices are dealt -- one split leaves a rank empty.  Also infer_volume(skeleton=) over two ranks."""
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
    vol, (thin, _, _) = _partition_case()
    want = _want_skeleton(vol, cap=9)
    assert want['radius2'].max() <= 9
    for i, b in enumerate(RANK_BOUNDS):
        for r in (0, 1):
            np.testing.assert_array_equal(got[r][0][i][0], thin[b[r]:b[r + 1]].astype(np.uint8))
            _assert_skeleton(got[r][0][i][1], want)
    want = _want_skeleton(vols[1])
    assert got[0][1][0] == (0, 20) and got[1][1][0] == (20, 40)
    for r in (0, 1):
        assert list(got[r][1][1]) == [1]
        _assert_skeleton(got[r][1][1][1], want)


# ------------------------------------------------------------------------------------------------------ infer_volume
def _want(vols):
    key = ('skeleton', id(vols[1]))
    if key not in _CACHE:
        _CACHE[key] = _want_skeleton(vols[1])
    return _CACHE[key]


def _assert_skeletonized(res, vols):
    want = _want(vols)
    assert list(res['skeletons']) == [1]                                        # a stuff class has no skeleton
    got = res['skeletons'][1]
    assert all(isinstance(a, np.ndarray) for a in got.values()) and sorted(got) == sorted(KEYS + ('radius2',))
    _assert_skeleton(got, want)
    if 'skeleton_datasets' in res:
        for k, ds in res['skeleton_datasets'][1].items():
            a = np.asarray(ds[...])
            assert a.dtype == got[k].dtype
            np.testing.assert_array_equal(a, got[k])


def test_infer_volume_plain_path_with_a_store(tmp_path, case):
    from empanada_amd.zarr_utils import ZarrV2Group
    eng, vol, vols, sets, counts = case(ORTHO)
    res = _run(eng, vol, tmp_path / 's.zarr', axes=ORTHO, skeleton=True, measure=True)
    _assert_skeletonized(res, vols)
    assert dict(res['instances']) == counts and _np(res['volumes'][1]).tobytes() == vols[1].tobytes()
    got = res['skeletons'][1]
    assert len(got['vertices']) and len(got['edges'])
    np.testing.assert_array_equal(got['objects'][:, 0], res['objects'][1][:, 0])    # the rows of measure's table
    _arbiters(got, ref.thin(vols[1])[0])
    d = SK.derive(got)
    assert (d['length'] >= 0).all() and (d['max_radius'] >= 1).all()
    root = ZarrV2Group(str(tmp_path / 's.zarr'))
    assert {f'mito_skeleton_{k}' for k in KEYS + ('radius2',)} <= set(os.listdir(root.path))
    assert not any(n.startswith('er_skeleton') for n in os.listdir(root.path))
    assert root.attrs['skeletons'] == {'axes': 'zyx', 'object_columns': list(SK.OBJECT_COLUMNS), 'r_cap': 64.0,
                                       'sampling': [1, 1, 1]}
    assert 'objects' in root.attrs                                              # beside what measure= wrote
    # a cap and a sampling of the caller's: only the radius changes
    capped = _run(eng, vol, tmp_path / 'c.zarr', axes=ORTHO, skeleton=(2, (2, 1, 1)))
    _assert_graph(capped['skeletons'][1], _want(vols))
    np.testing.assert_array_equal(capped['skeletons'][1]['radius2'], _radius2(vols[1], got['vertices'], 4, (2, 1, 1)))
    assert capped['skeletons'][1]['radius2'].max() == 4
    assert ZarrV2Group(str(tmp_path / 'c.zarr')).attrs['skeletons']['sampling'] == [2, 1, 1]
    # a class without objects: zero-row arrays, in the store where it can hold them
    none = _run(eng, vol, tmp_path / 'z.zarr', axes=ORTHO, skeleton=True, min_size=10 ** 9)
    s = none['skeletons'][1]
    assert s['vertices'].shape == (0, 3) and s['edges'].shape == (0, 2) and s['objects'].shape == (0, 8)
    assert s['degree'].shape == (0,) and s['radius2'].shape == (0,)
    ds = none['skeleton_datasets'][1]
    assert ds is None or all(tuple(ds[k].shape) == s[k].shape for k in s)


def test_skeleton_none_adds_no_key_and_no_launch(case, monkeypatch):
    from empanada_amd import _hip
    eng, vol, vols, sets, counts = case(ORTHO)
    for name in ('label_thin', 'LabelThin', 'label_graph', 'graph_finish'):
        monkeypatch.setattr(_hip, name, lambda *a, _n=name, **k: pytest.fail(f"{_n} was called"))
    monkeypatch.setattr(SK, 'skeleton_volume', lambda *a, **k: pytest.fail("skeleton_volume was called"))
    off = _run(eng, vol, None, axes=ORTHO, skeleton=None)
    assert sorted(off) == ['datasets', 'instances', 'volumes', 'z_range'] and dict(off['instances']) == counts
    for c in (1, 2):
        assert _np(off['volumes'][c]).tobytes() == vols[c].tobytes()


def test_infer_volume_after_the_repairs(case):
    """the skeleton is that of the FINAL volume: after morph, separate, split_objects and fill_holes"""
    eng, vol, vols, sets, counts = case(ORTHO)
    res = _run(eng, vol, None, axes=ORTHO, morph=('open', 1), separate=(2, 4), split_objects=6, fill_holes=True,
               skeleton=True, measure=True)
    final = _np(res['volumes'][1])
    assert final.tobytes() != vols[1].tobytes()
    _assert_skeleton(res['skeletons'][1], _want_skeleton(final))
    np.testing.assert_array_equal(res['skeletons'][1]['objects'][:, 0], res['objects'][1][:, 0])


def test_infer_volume_stack_mode_and_windows(tmp_path, case):
    eng, vol, vols, _, counts = case(('xy',))
    _assert_skeletonized(_run(eng, vol, None, axes=('xy',), skeleton=True), vols)
    kw = dict(axes=('xy',), batch_pixels=4 * 96 * 96, window_slices=8)      # 4 slices per model call, windows of 8
    win = _run(eng, vol, tmp_path / 'w.zarr', skeleton=64, **kw)
    assert win['windows']['xy'] > 1
    _assert_skeletonized(win, vols)


def test_infer_volume_pipeline(tmp_path, case):
    from empanada_amd.inference.pipeline import VolumePipeline
    eng, vol, vols, sets, counts = case(ORTHO)
    pipe = VolumePipeline(eng, tune=False, graph=True, overlap=True, batch_pixels=1 << 22)
    try:
        res = _run(eng, vol, tmp_path / 'p.zarr', axes=ORTHO, skeleton=True, pipeline=pipe)
        _assert_skeletonized(res, vols)
        off = _run(eng, vol, None, axes=ORTHO, pipeline=pipe)
        assert 'skeletons' not in off and dict(off['instances']) == counts
    finally:
        pipe.close()


def test_infer_volume_rejects_a_bad_skeleton_before_any_work(case):
    eng, vol, _, _, _ = case(ORTHO)
    before = torch.cuda.memory_allocated()
    for bad in (False, -1, 0, 300, 'yes', (1, 2), (3, (1, 1, 0))):
        with pytest.raises(ValueError, match='skeleton'):
            _run(eng, vol, None, axes=ORTHO, skeleton=bad)
    assert torch.cuda.memory_allocated() == before
