"""GPU: 3D connected components -- emp_label_components / emp_label_components_paint (csrc/emp_components.hip) through
_hip.label_components, components.split_volume and infer_volume(..., split_objects=).  The checker is
tests/test_components_host.py's `components_ref`, a scipy.ndimage restatement of the definition in include/emp_hip.h
(E3) that shares nothing with the kernel.  Everything is compared bit for bit.  The engine and volume of the
infer_volume cases are those of tests/test_pyramid_gpu.py."""
import os
import queue
import time

import numpy as np
import pytest
import torch

from empanada_amd import components as CP
from empanada_amd import synthetic as SY
from test_components_host import CONNECTIVITIES, N_COL, components_ref, random_labels, split_ref
from test_measure_host import measure_ref
from test_pyramid_gpu import KW, NAMES, ORTHO, SHAPE, _dev, _engine, _free_port, _np, _run, case  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (1, 1, 70), (3, 1, 5), (1, 9, 1), (5, 6, 7), (4, 5, 64), (3, 4, 300)]
DTYPES = [np.uint8, np.uint32]
_CACHE = {}


def _label(lab, connectivity, **kw):
    from empanada_amd import _hip
    lc = _hip.label_components(lab if isinstance(lab, torch.Tensor) else _dev(lab), connectivity, **kw)
    assert lc.table.dtype == torch.int64 and lc.table.is_cuda and lc.table.dim() == 2 and lc.table.shape[1] == N_COL
    return lc


def _check(lab, connectivity, z_base=0, msg='', **kw):
    """table and numbered volume of the kernel against the restatement; returns the LabelComponents"""
    want, comp = components_ref(lab, connectivity, z_base)
    lc = _label(lab, connectivity, z_base=z_base, **kw)
    np.testing.assert_array_equal(lc.table.cpu().numpy(), want, err_msg=f'{msg} {lab.shape} c{connectivity}')
    numbered = lc.paint(torch.arange(1, lc.n + 1, device='cuda'), dtype=torch.uint32)
    assert numbered.dtype == torch.uint32 and tuple(numbered.shape) == lab.shape
    np.testing.assert_array_equal(_np(numbered).astype(np.int64), comp + 1, err_msg=f'{msg} {lab.shape} c{connectivity}')
    return lc


# ------------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize('dtype', DTYPES, ids=['u8', 'u32'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_kernel_equals_the_restatement(shape, dtype):
    for n_labels, density in ((1, 0.2), (3, 0.5), (5, 0.9), (2, 0.5), (1, 0.9)):
        lab = random_labels(shape, n_labels, density, seed=n_labels * 100 + int(density * 10), dtype=dtype)
        if shape == (3, 4, 300):
            lab[1, 2, 250:262] = 1                                          # a run across the border of a wave's pass
        for connectivity in CONNECTIVITIES:
            _check(lab, connectivity, z_base=3 if n_labels == 3 else 0, msg=f'{n_labels} labels fill {density}')


def _contacts():
    """name -> (two voxel positions of a 3x3x3 cube, the connectivities that join them)"""
    return {'face_z': ((1, 1, 1), (2, 1, 1), (6, 18, 26)), 'face_y': ((1, 1, 1), (1, 0, 1), (6, 18, 26)),
            'face_x': ((1, 1, 1), (1, 1, 2), (6, 18, 26)),
            'edge_zy': ((1, 1, 1), (0, 2, 1), (18, 26)), 'edge_zx': ((1, 1, 1), (2, 1, 0), (18, 26)),
            'edge_yx': ((1, 1, 1), (1, 0, 2), (18, 26)), 'edge_zy2': ((1, 1, 1), (2, 2, 1), (18, 26)),
            'corner_a': ((1, 1, 1), (0, 0, 0), (26,)), 'corner_b': ((1, 1, 1), (2, 0, 2), (26,)),
            'corner_c': ((1, 1, 1), (0, 2, 0), (26,)), 'corner_d': ((1, 1, 1), (2, 2, 2), (26,)),
            'apart': ((0, 1, 1), (2, 1, 1), ())}


@pytest.mark.parametrize('dtype', DTYPES, ids=['u8', 'u32'])
def test_connectivity_probes(dtype):
    for name, (p, q, joined) in _contacts().items():
        for size, shift in ((3, 0), (2, 1)):
            if size == 2 and (name == 'apart' or min(min(p), min(q)) - shift < 0 or max(max(p), max(q)) - shift > 1):
                continue
            p2, q2 = tuple(v - shift for v in p), tuple(v - shift for v in q)
            same = np.zeros((size,) * 3, dtype)
            same[p2] = same[q2] = 7
            other = same.copy()
            other[q2] = 8
            for connectivity in CONNECTIVITIES:
                lc = _check(same, connectivity, msg=name)
                assert lc.n == (1 if connectivity in joined else 2), (name, size, connectivity)
                assert _check(other, connectivity, msg=name).n == 2          # different labels never join
    z, y, x = np.indices((8, 8, 8))
    checker = ((z + y + x) % 2 == 0).astype(dtype) * 5
    assert [_check(checker, c, msg='checkerboard').n for c in CONNECTIVITIES] == [256, 1, 1]
    both = np.where((z + y + x) % 2 == 0, 5, 6).astype(dtype)                # two checkerboards, one inside the other
    assert [_check(both, c, msg='checkerboards').n for c in CONNECTIVITIES] == [512, 2, 2]


def _spiral2d(n):
    g = np.zeros((n, n), bool)
    y = x = 0
    dy, dx = 0, 1
    g[0, 0] = True
    path = [(0, 0)]
    while True:
        for _ in range(2):
            ny, nx, ay, ax = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            if 0 <= ny < n and 0 <= nx < n and not g[ny, nx] and not (0 <= ay < n and 0 <= ax < n and g[ay, ax]):
                y, x = ny, nx
                g[y, x] = True
                path.append((y, x))
                break
            dy, dx = dx, -dy
        else:
            return g, path


def test_late_joins():
    """sets that stay apart until the last row of the last slice, and long thin paths: many unions down one chain"""
    u = np.zeros((1, 6, 5), np.uint8)
    u[0, :, 0] = u[0, :, 4] = u[0, 5, :] = 2
    comb = np.zeros((4, 5, 9), np.uint32)
    comb[:, :, ::2] = 9
    teeth = comb.copy()
    comb[-1, -1, :] = 9
    g, path = _spiral2d(11)
    assert g.sum() > 60 and not g.all()
    snake = np.zeros((5, 11, 11), np.uint8)                                  # one voxel thick: up at the end, down at the start
    snake[0::2] = g
    snake[(1,) + path[-1]] = snake[(3,) + path[0]] = 1
    pair = np.where(np.broadcast_to(g, (3, 11, 11)), 4, 3).astype(np.uint32)  # the spiral and the spiral between its arms
    pair[1] = 0
    pair[(1,) + path[-1]] = 4
    pair[1, 1, 0] = 3
    for connectivity in CONNECTIVITIES:
        assert _check(u, connectivity, msg='U').n == 1
        assert _check(teeth, connectivity, msg='teeth').n == 5
        assert _check(comb, connectivity, msg='comb').n == 1
        _check(snake, connectivity, msg='snake')
        _check(pair, connectivity, msg='two spirals')
    assert _label(snake, 6).n == 1 and _label(pair, 6).n == 2
    assert _label(snake[0:1], 6).n == 1


def test_large_labels_and_int32_input():
    from empanada_amd import _hip
    values = [1, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1]
    lab = random_labels((3, 5, 70), 4, 0.6, seed=5, values=values)
    for connectivity in CONNECTIVITIES:
        _check(lab, connectivity, z_base=2)
        want, comp = components_ref(lab, connectivity, 2)
        lc = _hip.label_components(torch.from_numpy(lab.view(np.int32)).cuda(), connectivity, z_base=2)
        np.testing.assert_array_equal(lc.table.cpu().numpy(), want)
        assert (lc.table[:, 0] >= 2 ** 31).any()
        back = lc.paint(lc.table[:, 0])                                     # every component its own label: the input
        assert back.dtype == torch.int32
        np.testing.assert_array_equal(back.cpu().numpy().view(np.uint32), lab)


def test_all_zero_and_empty_slabs():
    from empanada_amd import _hip
    for tdt in (torch.uint8, torch.int32):
        for shape in ((0, 4, 4), (3, 0, 4), (3, 4, 0), (2, 3, 4)):
            lc = _hip.label_components(torch.zeros(shape, dtype=tdt, device='cuda'), 18)
            assert tuple(lc.table.shape) == (0, N_COL) and lc.table.dtype == torch.int64 and lc.table.is_cuda and lc.n == 0
            out = lc.paint(torch.zeros((0,), dtype=torch.int64), dtype=torch.uint8)
            assert tuple(out.shape) == shape and out.dtype == torch.uint8 and not out.any()


@pytest.mark.parametrize('offset', [1, 2, 3])
def test_unaligned_slab_takes_the_narrow_path(offset):
    """the slab, and the output painted into, start 1, 2 or 3 elements off a 16-byte (uint32) / 4-byte (uint8) address"""
    from empanada_amd import _hip
    for dtype, tdt in ((np.uint32, torch.int32), (np.uint8, torch.uint8)):
        for shape in ((3, 6, 64), (2, 3, 259)):
            a = random_labels(shape, 3, 0.6, seed=offset, dtype=dtype)
            flat = torch.zeros((a.size + 32,), dtype=tdt, device='cuda')
            flat[offset:offset + a.size] = _dev(a).view(tdt).ravel()
            dev = flat[offset:offset + a.size].view(a.shape)
            assert dev.data_ptr() % (4 * dev.element_size()) != 0 and dev.is_contiguous()
            want, comp = components_ref(a, 26, 1)
            lc = _hip.label_components(dev, 26, z_base=1)
            np.testing.assert_array_equal(lc.table.cpu().numpy(), want, err_msg=f'{dtype} {shape}')
            for odt in (torch.int32, torch.uint8):
                buf = torch.full((a.size + 32,), 77, dtype=odt, device='cuda')
                out = buf[offset:offset + a.size].view(a.shape)
                lut = torch.arange(lc.n, device='cuda') % 251 + 1
                assert lc.paint(lut, out=out) is out
                np.testing.assert_array_equal(out.cpu().numpy().astype(np.int64),
                                              np.where(comp >= 0, np.append(lut.cpu().numpy(), 0)[comp], 0))
                assert (buf[:offset] == 77).all() and (buf[offset + a.size:] == 77).all()     # nothing outside


# ------------------------------------------------------------------------------------------------------ paint
def test_paint():
    from empanada_amd import _hip
    mask = (random_labels((4, 7, 37), 1, 0.35, seed=8, dtype=np.uint8) > 0).astype(np.uint8)
    want, comp = components_ref(mask, 6)
    n = len(want)
    assert n > 20
    dev = _dev(mask)
    lc = _hip.label_components(dev, 6)
    # a uint8 mask becomes uint32 instances, with values no byte holds
    lut = 1000 + np.arange(n, dtype=np.int64) * 70001
    inst = lc.paint(lut, dtype=torch.uint32)
    assert inst.dtype == torch.uint32
    np.testing.assert_array_equal(_np(inst).astype(np.int64), np.where(comp >= 0, np.append(lut, 0)[comp], 0))
    # zeros in the lut erase; into a given tensor whose old content goes
    lut0 = np.where(np.arange(n) % 3 == 0, 0, np.arange(n) % 200 + 1)
    out = torch.full(mask.shape, 9, dtype=torch.uint8, device='cuda')
    assert lc.paint(lut0, out=out) is out
    np.testing.assert_array_equal(out.cpu().numpy(), np.where(comp >= 0, np.append(lut0, 0)[comp], 0))
    # a slice range only: the other slices of `out` stay as they are
    out = torch.full(mask.shape, 9, dtype=torch.int32, device='cuda')
    lc.paint(lut, out=out, z_range=(1, 3))
    full = np.where(comp >= 0, np.append(lut, 0)[comp], 0)
    np.testing.assert_array_equal(out[1:3].cpu().numpy(), full[1:3])
    assert (out[0] == 9).all() and (out[3] == 9).all()
    plane = lc.paint_slice(torch.from_numpy(lut).cuda(), 2)
    np.testing.assert_array_equal(_np(plane).astype(np.int64), full[2])
    # a value above 255 into uint8 is refused with nothing written, and so are the other argument errors
    before = dev.clone()
    out = torch.full(mask.shape, 9, dtype=torch.uint8, device='cuda')
    for target in (dict(out=dev), dict(out=out), dict(dtype=torch.uint8)):
        with pytest.raises(ValueError, match='cannot hold'):
            lc.paint(np.where(np.arange(n) == n - 1, 256, 1), **target)
    assert torch.equal(dev, before) and (out == 9).all()
    for bad in (dict(lut=lut[:-1]), dict(lut=lut, out=out[:, :, :-1]), dict(lut=lut, out=out.cpu()),
                dict(lut=lut.astype(np.float32)), dict(lut=lut, dtype=torch.int64), dict(lut=lut, z_range=(2, 5)),
                dict(lut=-lut)):
        with pytest.raises(ValueError):
            lc.paint(**bad)
    assert torch.equal(dev, before)
    # in place: lut zeros erase, the rest is renumbered, the background is not written
    lut8 = np.where(np.arange(n) % 4 == 0, 0, np.arange(n) % 250 + 1)
    assert lc.paint(lut8, out=dev) is dev
    np.testing.assert_array_equal(dev.cpu().numpy(), np.where(comp >= 0, np.append(lut8, 0)[comp], 0))


@pytest.mark.parametrize('dtype', DTYPES, ids=['u8', 'u32'])
def test_blocks_give_the_table_and_the_volume_of_the_whole(dtype):
    lab = random_labels((6, 7, 33), 3, 0.5, seed=21, dtype=dtype)
    for connectivity in CONNECTIVITIES:
        want, comp = components_ref(lab, connectivity, 4)
        for per, n_blocks in ((6, 1), (3, 2), (2, 3), (1, 6), (4, 2)):
            info = {}
            lc = _check(lab, connectivity, z_base=4, block_voxels=per * 7 * 33 + 5, info=info, msg=f'{n_blocks} blocks')
            assert info['blocks'] == n_blocks and info['runs'] > 0 and info['work_bytes'] > 0
            dev = _dev(lab)
            from empanada_amd import _hip
            lc = _hip.label_components(dev, connectivity, block_voxels=per * 7 * 33)
            lut = np.arange(lc.n) % 200 + 1
            lc.paint(lut, out=dev, z_range=(1, 5))                          # in place, across the blocks' borders
            painted = np.where(comp >= 0, np.append(lut, 0)[comp], 0)
            np.testing.assert_array_equal(_np(dev)[1:5], painted[1:5])
            np.testing.assert_array_equal(_np(dev)[[0, 5]], lab[[0, 5]])


# ------------------------------------------------------------------------------------------------------ split_volume
def _planted():
    """a (12, 20, 24) uint32 volume with known defects, min_size 20 / min_span 2 in mind:
    label 3: a 6x6x6 body, a 3x3x3 piece of 27 voxels (stays, new label) and a 2-voxel crumb (goes);
    label 5: one 4x4x4 box, whole;
    label 8: two equal 3x3x3 pieces -- the one met first keeps the label -- touching label 5 by a face, which never joins;
    label 9: a 1 x 5 x 5 sheet (25 voxels, span 1 along z: goes) and a corner contact: one piece for 26, two for 6 / 18;
    label 11: two crumbs of 4 voxels: the label vanishes"""
    v = np.zeros((12, 20, 24), np.uint32)
    v[0:6, 0:6, 0:6] = 3
    v[8:11, 1:4, 1:4] = 3
    v[7, 12, 0:2] = 3
    v[0:4, 8:12, 8:12] = 5
    v[0:3, 8:11, 12:15] = 8
    v[6:9, 14:17, 18:21] = 8
    v[11, 0:5, 10:15] = 9
    v[4:7, 14:17, 4:7] = 9
    v[7:10, 17:20, 7:10] = 9                                                # (6, 16, 6) and (7, 17, 7): a corner
    v[2, 18, 20:24] = 11
    v[10, 9, 20:24] = 11
    return v


def test_split_volume_on_a_planted_volume():
    from empanada_amd import _hip
    from empanada_amd.components import split_volume
    v = _planted()
    expect = {26: dict(objects_in=5, objects_split=4, pieces_added=2, pieces_removed=4, objects_out=6),
              6: dict(objects_in=5, objects_split=4, pieces_added=3, pieces_removed=4, objects_out=7)}
    for connectivity in (26, 6):
        want, stats, _ = split_ref(v, connectivity, min_size=20, min_span=2)
        assert stats == expect[connectivity]                                 # the plant is what its docstring says
        dev = _dev(v)
        got, got_stats = split_volume(dev, connectivity, min_size=20, min_span=2)
        assert got is dev and got_stats == stats
        out = _np(dev)
        np.testing.assert_array_equal(out, want)
        assert out[8, 1, 1] == 12 and out[7, 12, 0] == 0 and out[0, 0, 0] == 3          # piece, crumb, body
        assert out[0, 8, 12] == 8 and out[6, 14, 18] == 13 and out[11, 0, 10] == 0 and out[2, 18, 20] == 0
        # the output's components are exactly its labels
        again = _hip.label_components(dev, connectivity)
        assert again.n == stats['objects_out'] == len(np.unique(out)) - 1
        lut2, stats2 = CP.plan(again.table, 20, 2)
        assert stats2['objects_split'] == 0 and stats2['pieces_removed'] == 0
        # into another tensor, without filters, with a z_base: nothing is erased
        src = _dev(v)
        out2 = torch.zeros(v.shape, dtype=torch.int32, device='cuda')
        got2, s2 = split_volume(src, connectivity, z_base=7, out=out2)
        assert got2 is out2 and s2['pieces_removed'] == 0 and s2['objects_out'] == s2['objects_in'] + s2['pieces_added']
        np.testing.assert_array_equal(out2.cpu().numpy().view(np.uint32), split_ref(v, connectivity)[0])
        np.testing.assert_array_equal(_np(src), v)
    stuff = (v > 0).astype(np.uint8)                                          # a uint8 slab in place
    dev = _dev(stuff)
    _, s = split_volume(dev, 18, min_size=10)
    np.testing.assert_array_equal(dev.cpu().numpy(), split_ref(stuff, 18, min_size=10)[0])
    assert s['objects_in'] == 1 and s['objects_split'] == 1


# ------------------------------------------------------------------------------------------------------ infer_volume
def _wanted(vols, connectivity=26):
    key = (id(vols[1]), connectivity)
    if key not in _CACHE:
        _CACHE[key] = split_ref(vols[1], connectivity, min_size=KW['min_size'], min_span=KW['min_span'])[:2]
    return _CACHE[key]


def _assert_split(res, vols, connectivity=26):
    want, stats = _wanted(vols, connectivity)
    np.testing.assert_array_equal(_np(res['volumes'][1]), want)
    np.testing.assert_array_equal(_np(res['volumes'][2]), vols[2])          # a stuff class stays as it is
    assert res['split'] == {1: stats} and res['instances'][1] == stats['objects_out'] == len(np.unique(want)) - 1
    assert stats['objects_in'] == len(np.unique(vols[1])) - 1
    if 'objects' in res:
        for c in (1, 2):
            np.testing.assert_array_equal(res['objects'][c], measure_ref(_np(res['volumes'][c])))
        assert len(res['objects'][1]) == res['instances'][1]
    for c, ds in res['datasets'].items():
        if ds is not None:
            np.testing.assert_array_equal(np.asarray(ds[...]), _np(res['volumes'][c]))


def test_infer_volume_plain_path_with_a_store(tmp_path, case):
    eng, vol, vols, sets, counts = case(ORTHO)
    res = _run(eng, vol, tmp_path / 's.zarr', axes=ORTHO, split_objects=26, measure=True, pyramid=1, compressor='zlib')
    _assert_split(res, vols)
    from empanada_amd.inference import pyramid as pyr
    np.testing.assert_array_equal(_np(res['pyramid'][1][0]), _np(pyr.build(res['volumes'][1], [(2, 2, 2)])[0]))
    _assert_split(_run(eng, vol, None, axes=ORTHO, split_objects=6), vols, 6)
    # off: the parent's keys and the parent's volumes, with the argument and without it
    off = _run(eng, vol, tmp_path / 'n.zarr', axes=ORTHO, split_objects=None)
    assert sorted(off) == ['datasets', 'instances', 'volumes', 'z_range'] and dict(off['instances']) == counts
    for c in (1, 2):
        np.testing.assert_array_equal(_np(off['volumes'][c]), vols[c])
        np.testing.assert_array_equal(np.asarray(off['datasets'][c][...]), sets[c])


def test_infer_volume_stack_mode_and_windows(tmp_path, case):
    eng, vol, vols, _, counts = case(('xy',))
    _assert_split(_run(eng, vol, None, axes=('xy',), split_objects=26, measure=True), vols)
    kw = dict(axes=('xy',), batch_pixels=4 * 96 * 96, window_slices=8)      # 4 slices per model call, windows of 8
    win = _run(eng, vol, tmp_path / 'w.zarr', split_objects=26, **kw)
    assert win['windows']['xy'] > 1
    _assert_split(win, vols)


def test_infer_volume_pipeline(tmp_path, case):
    from empanada_amd.inference.pipeline import VolumePipeline
    eng, vol, vols, sets, counts = case(ORTHO)
    pipe = VolumePipeline(eng, tune=False, graph=True, overlap=True, batch_pixels=1 << 22)
    try:
        res = _run(eng, vol, tmp_path / 'a.zarr', axes=ORTHO, split_objects=26, measure=True, pipeline=pipe)
        _assert_split(res, vols)
        off = _run(eng, vol, None, axes=ORTHO, pipeline=pipe)
        assert 'split' not in off and dict(off['instances']) == counts
        np.testing.assert_array_equal(_np(off['volumes'][1]), vols[1])
    finally:
        pipe.close()


# ----------------------------------------------------------------------------------------------- two ranks over gloo
def _rank(rank, world, port, path, q):
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        from empanada_amd.components import split_volume
        v = _planted()
        z0, z1 = (0, 7) if rank == 0 else (7, 12)                            # the cut goes through objects and a seam pair
        dev = _dev(v[z0:z1])
        _, planted_stats = split_volume(dev, 26, min_size=20, min_span=2, group=dist.group.WORLD, z_base=z0)
        eng, vol = _engine(), SY.em_volume(SHAPE, seed=3)
        res = _run(eng, vol, path, axes=ORTHO, group=dist.group.WORLD, split_objects=26, measure=True)
        q.put((rank, tuple(res['z_range']), _np(res['volumes'][1]), res['split'], dict(res['instances']), res['objects'],
               _np(dev), planted_stats))
    finally:
        dist.destroy_process_group()


def test_two_ranks(tmp_path, case):
    import torch.multiprocessing as mp
    from empanada_amd.zarr_utils import ZarrV2Group
    eng, vol, vols, sets, counts = case(ORTHO)
    want, stats = _wanted(vols)
    planted_want, planted_stats, _ = split_ref(_planted(), 26, min_size=20, min_span=2)
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
    np.testing.assert_array_equal(np.concatenate([got[0][1], got[1][1]]), want)
    np.testing.assert_array_equal(np.concatenate([got[0][5], got[1][5]]), planted_want)
    for r in (0, 1):
        assert got[r][2] == {1: stats} and got[r][3][1] == stats['objects_out'] and got[r][6] == planted_stats
        np.testing.assert_array_equal(got[r][4][1], measure_ref(want))
    np.testing.assert_array_equal(np.asarray(ZarrV2Group(path, mode='r')[NAMES[1]]), want)
