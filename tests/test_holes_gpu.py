"""GPU: the cavity table of _hip.label_holes, the plan and the volume painted in place equal the checker of
test_holes_host.py (scipy.ndimage.label on the zero voxels, numpy shifts for the wall labels) -- exact integers, no
tolerance -- and infer_volume(fill_holes=) fills the volumes before anything reads them, on every path."""
import os
import queue
import time

import numpy as np
import pytest
import torch

from empanada_amd import holes as HO
from empanada_amd import synthetic as SY
from test_components_host import split_ref
from test_holes_host import N_COL, NO_LABEL, components_of, fill_ref, holes_ref, plan_ref, planted_volume
from test_measure_host import measure_ref
from test_pyramid_gpu import KW, NAMES, ORTHO, SHAPE, _dev, _engine, _free_port, _np, _run, case  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

DTYPES = [np.uint8, np.uint32]
_CACHE = {}


def _check(vol, below=None, above=None, z_base=0, max_voxels=None, msg='', **kw):
    """label_holes of a device copy of `vol`: table == checker, plan == definition and, without neighbour slices, the
    volume painted in place == the checker's; returns (LabelHoles, painted numpy volume)"""
    from empanada_amd import _hip
    dev = _dev(vol)
    lh = _hip.label_holes(dev, below=None if below is None else _dev(below), above=None if above is None else _dev(above),
                          z_base=z_base, **kw)
    want = holes_ref(vol, below, above, z_base)
    assert lh.table.dtype == torch.int64 and lh.table.is_cuda and tuple(lh.table.shape) == (lh.n, N_COL)
    np.testing.assert_array_equal(lh.table.cpu().numpy(), want, err_msg=msg)
    shape = (z_base + vol.shape[0] + (above is not None), vol.shape[1], vol.shape[2])   # the volume the slab is part of
    lut, stats = HO.plan(want, shape, max_voxels)
    want_lut, want_stats = plan_ref(want, shape, max_voxels)
    assert lut.astype(np.int64).tolist() == want_lut.tolist() and stats == want_stats, msg
    assert lh.paint(lut) is dev
    painted = _np(dev)
    if below is None and above is None and z_base == 0:
        np.testing.assert_array_equal(painted, fill_ref(vol, max_voxels)[0], err_msg=msg)
    k = components_of(vol)
    np.testing.assert_array_equal(painted, np.where(k >= 0, np.append(lut, 0)[k].astype(vol.dtype), vol), err_msg=msg)
    return lh, painted


# ------------------------------------------------------------------------------------------------------ random volumes
@pytest.mark.parametrize('dtype', DTYPES, ids=['u8', 'u32'])
@pytest.mark.parametrize('shape', [(13, 21, 37), (5, 16, 64), (6, 9, 1), (1, 9, 12), (3, 4, 300)],
                         ids=lambda s: 'x'.join(map(str, s)))
def test_kernel_equals_the_checker(shape, dtype):
    for seed in (0, 1):
        vol = planted_volume(shape, dtype, seed)
        lh, painted = _check(vol, msg=f'seed {seed}')
        if shape[0] == 1 or shape[2] == 1:                      # every cavity is open: nothing is written
            np.testing.assert_array_equal(painted, vol)
        elif shape[0] > 3:
            assert (painted != vol).any()
        _check(vol, z_base=7, max_voxels=1, msg=f'seed {seed}, z_base, cap')
    vol = planted_volume(shape, dtype, 2)
    if shape[0] > 2:
        _check(vol[1:-1], below=vol[0], above=vol[-1], z_base=1, msg='neighbour slices')
    else:
        _check(vol, below=planted_volume(shape, dtype, 3)[0], above=planted_volume(shape, dtype, 4)[0], z_base=1,
               msg='neighbour slices')


# ------------------------------------------------------------------------------------------------------ probes
def _solid(n=7, lab=5, dtype=np.uint32):
    v = np.full((n, n, n), lab, dtype)
    v[3, 3, 3] = 0
    return v


@pytest.mark.parametrize('dtype', DTYPES, ids=['u8', 'u32'])
def test_probes(dtype):
    # a 1-voxel cavity
    v = _solid(dtype=dtype)
    lh, p = _check(v)
    assert lh.n == 1 and p[3, 3, 3] == 5 and lh.table[0].tolist() == [1, 3 * 49 + 3 * 7 + 3, 3, 3, 3, 4, 4, 4, 5, 5]
    # opened through each of the six faces in turn
    for a in range(3):
        for side in (slice(0, 4), slice(3, 7)):
            v = _solid(dtype=dtype)
            idx = [3, 3, 3]
            idx[a] = side
            v[tuple(idx)] = 0
            lh, p = _check(v, msg=f'axis {a} {side}')
            assert lh.n == 1 and int(lh.table[0, 0]) == 4
            np.testing.assert_array_equal(p, v)
    # the only leak runs across an edge / a corner: closed, filled; the tunnel itself is open
    for tunnel in ((slice(0, 3), 2, 3), (slice(0, 3), 2, 2), (2, 3, slice(4, 7)), (4, slice(4, 7), 4)):
        v = _solid(dtype=dtype)
        v[tunnel] = 0
        lh, p = _check(v, msg=str(tunnel))
        assert lh.n == 2 and p[3, 3, 3] == 5 and (p[tunnel] == 0).all() and (p != v).sum() == 1
    # wall voxels that touch only across an edge and a corner do not enter the wall labels
    v = _solid(dtype=dtype)
    v[2, 2, 3], v[2, 2, 2], v[4, 3, 4] = 9, 8, 2
    lh, p = _check(v)
    assert lh.table[0, 8:].tolist() == [5, 5] and p[3, 3, 3] == 5
    # a two-label wall, along every axis: shared, left
    for nb in ((3, 3, 4), (3, 3, 2), (3, 2, 3), (3, 4, 3), (2, 3, 3), (4, 3, 3)):
        v = _solid(dtype=dtype)
        v[nb] = 200
        lh, p = _check(v, msg=str(nb))
        assert lh.table[0, 8:].tolist() == [5, 200] and p[3, 3, 3] == 0
    # an object nested in a cavity of another: the shell is shared and left; the inner object's own cavity is filled
    v = np.full((9, 9, 9), 5, dtype)
    v[1:8, 1:8, 1:8] = 0
    v[2:7, 2:7, 2:7] = 6
    v[4, 4, 4] = 0
    lh, p = _check(v)
    assert lh.n == 2 and lh.table[:, 8:].tolist() == [[5, 6], [6, 6]] and p[4, 4, 4] == 6 and (p != v).sum() == 1
    _, s = HO.plan(lh.table, v.shape)
    assert s == dict(cavities=2, filled=1, voxels_filled=1, shared=1, too_large=0)


def test_late_joins():
    """combs whose teeth meet only in the last row / the last slice, and a serpentine: runs that are united long after
    they were met in raster order"""
    v = np.full((3, 11, 21), 5, np.uint8)
    v[1, 1:10, 1:20:2] = 0
    v[1, 9, 1:20] = 0
    lh, p = _check(v)
    assert lh.n == 1 and (p == 5).all()
    v = np.full((8, 5, 21), 5, np.uint32)
    v[1:7, 2, 1:20:2] = 0
    v[6, 2, 1:20] = 0
    lh, p = _check(v)
    assert lh.n == 1 and (p == 5).all()
    v[6, 2, 10], v[7, 2, 3] = 5, 7                              # two combs now, the first with a second wall label
    lh, p = _check(v)
    assert lh.n == 2 and lh.table[:, 8:].tolist() == [[5, 7], [5, 5]]
    assert (p[:, :, :10] == v[:, :, :10]).all() and (p[:, :, 10:] == 5).all()
    n = 15                                                      # a serpentine: every row hangs on the one before it
    s = np.full((n, n), 5, np.uint32)
    for i, y in enumerate(range(1, n - 1, 2)):
        s[y, 1:n - 1] = 0
        if y + 2 < n - 1:
            s[y + 1, n - 2 if i % 2 == 0 else 1] = 0
    v = np.full((3, n, n), 5, np.uint32)
    v[1] = s
    lh, p = _check(v)
    assert lh.n == 1 and int(lh.table[0, 0]) == 7 * 13 + 6 and (p == 5).all()


def test_large_labels_and_int32_input():
    from empanada_amd import _hip
    big, top = 2 ** 31, 2 ** 32 - 1
    v = np.full((5, 7, 16), top, np.uint32)
    v[:, :, 5:10] = big
    v[:, :, 10:] = 3
    v[2, 3, 2] = 0                                              # walled by 2^32 - 1 alone
    v[2, 3, 4] = 0                                              # 2^32 - 1 and 2^31
    v[2, 3, 7] = 0                                              # 2^31 alone
    v[2, 3, 9] = 0                                              # 2^31 and 3
    lh, p = _check(v)
    assert lh.table[:, 8:].tolist() == [[top, top], [big, top], [big, big], [3, big]]
    assert p[2, 3, [2, 4, 7, 9]].tolist() == [top, 0, big, 0]
    dev = torch.from_numpy(v.view(np.int32)).cuda()             # the bits of an int32 are taken as they are
    lh = _hip.label_holes(dev)
    np.testing.assert_array_equal(lh.table.cpu().numpy(), holes_ref(v))
    lut, _ = HO.plan(lh.table, v.shape)
    assert lh.paint(lut) is dev and dev.dtype == torch.int32
    np.testing.assert_array_equal(dev.cpu().numpy().view(np.uint32), p)
    with pytest.raises(ValueError, match='cannot hold'):        # a uint8 slab cannot take a label above 255
        lh8 = _hip.label_holes(_dev(np.zeros((1, 2, 2), np.uint8)))
        lh8.paint(np.array([256]))


def test_all_zero_no_zero_and_empty_slabs():
    from empanada_amd import _hip
    for dtype in DTYPES:
        v = np.zeros((3, 5, 70), dtype)
        lh, p = _check(v)
        assert lh.table.tolist() == [[3 * 5 * 70, 0, 0, 0, 0, 3, 5, 70, NO_LABEL, 0]] and not p.any()
        lh, p = _check(np.full((3, 5, 70), 9, dtype))
        assert lh.n == 0 and (p == 9).all()
        tdt = torch.uint8 if dtype == np.uint8 else torch.uint32
        for shape in ((0, 5, 7), (0, 1, 1)):
            info = {}
            lh = _hip.label_holes(torch.zeros(shape, dtype=tdt, device='cuda'), info=info)
            assert tuple(lh.table.shape) == (0, N_COL) and lh.table.dtype == torch.int64 and lh.n == 0
            assert info == dict(blocks=0, runs=0, work_bytes=0)
            assert tuple(lh.paint(np.zeros((0,), np.int64)).shape) == shape
    for bad in (dict(below=torch.zeros((5, 7), dtype=torch.uint8, device='cuda')),
                dict(above=torch.zeros((5, 70), dtype=torch.int32, device='cuda')),
                dict(above=torch.zeros((5, 70), dtype=torch.uint8))):
        with pytest.raises(ValueError, match='label_holes'):
            _hip.label_holes(torch.zeros((3, 5, 70), dtype=torch.uint8, device='cuda'), **bad)
    with pytest.raises(ValueError, match='contiguous'):
        _hip.label_holes(torch.zeros((3, 5, 70), dtype=torch.uint8, device='cuda')[:, :, ::2])
    with pytest.raises(ValueError, match='D, H, W'):
        _hip.label_holes(torch.zeros((5, 70), dtype=torch.uint8, device='cuda'))


@pytest.mark.parametrize('offset', [1, 2, 3])
def test_unaligned_slab_takes_the_narrow_path_and_nothing_else_is_written(offset):
    """the slab starts 1, 2 or 3 elements off a 16-byte (uint32) / 4-byte (uint8) address inside a larger buffer; after
    the painting in place the whole buffer, guard margins included, differs from before in filled cavities alone"""
    from empanada_amd import _hip
    for dtype, tdt in ((np.uint32, torch.int32), (np.uint8, torch.uint8)):
        for shape in ((3, 6, 64), (4, 5, 259)):
            a = planted_volume(shape, dtype, seed=offset)
            flat = torch.full((a.size + 64,), 77, dtype=tdt, device='cuda')
            flat[16 + offset:16 + offset + a.size] = _dev(a).view(tdt).ravel()
            dev = flat[16 + offset:16 + offset + a.size].view(a.shape)
            assert dev.data_ptr() % (4 * dev.element_size()) != 0 and dev.is_contiguous()
            nb = planted_volume((2,) + shape[1:], dtype, seed=9)
            below, above = _dev(nb[0]).view(tdt), _dev(nb[1]).view(tdt)
            lh = _hip.label_holes(dev, below=below, above=above, z_base=2)
            np.testing.assert_array_equal(lh.table.cpu().numpy(), holes_ref(a, nb[0], nb[1], 2), err_msg=f'{dtype} {shape}')
            lh = _hip.label_holes(dev)
            want, _, t = fill_ref(a)
            np.testing.assert_array_equal(lh.table.cpu().numpy(), t)
            lh.paint(HO.plan(lh.table, shape)[0])
            whole = np.full(a.size + 64, 77, dtype)
            whole[16 + offset:16 + offset + a.size] = want.ravel()
            np.testing.assert_array_equal(flat.cpu().numpy().view(dtype), whole)
            assert (want != a).any()


# ------------------------------------------------------------------------------------------------------ z-blocks
def _seams_volume(dtype):
    """(6, 9, 12), three blocks of two slices: a cavity through both seams, one whose second wall label lies in the next
    block alone, one open only through another block, and one closed inside a block"""
    v = np.full((6, 9, 12), 4, dtype)
    v[1:5, 2, 2] = 0                                            # z 1 .. 4: in all three blocks, closed, filled
    v[1, 5, 5], v[2, 5, 5] = 0, 7                               # in block 0; its wall label 7 is in block 1
    v[3:6, 6, 8] = 0                                            # reaches z = 5: the piece in block 1 is open through block 2
    v[2:4, 3, 9:11] = 0                                         # inside block 1, closed
    v[0:3, 7, 3] = 0                                            # open through z = 0, continues into block 1
    return v


@pytest.mark.parametrize('dtype', DTYPES, ids=['u8', 'u32'])
def test_blocks_give_the_table_and_the_volume_of_the_whole(dtype):
    from empanada_amd import _hip
    for vol in (_seams_volume(dtype), planted_volume((6, 7, 33), dtype, seed=3)):
        H, W = vol.shape[1:]
        whole = _hip.label_holes(_dev(vol), z_base=4)
        for per, n_blocks in ((6, 1), (2, 3), (3, 2), (1, 6), (4, 2)):
            info = {}
            lh, painted = _check(vol, z_base=4, block_voxels=per * H * W + 5, info=info, msg=f'{n_blocks} blocks')
            assert info['blocks'] == n_blocks and info['runs'] > 0 and info['work_bytes'] > 0
            assert torch.equal(lh.table, whole.table)
            dev = _dev(vol)                                     # the volume: equal to the undivided call's
            lh = _hip.label_holes(dev, block_voxels=per * H * W)
            lh.paint(HO.plan(lh.table, vol.shape)[0])
            np.testing.assert_array_equal(_np(dev), fill_ref(vol)[0])
            ids = torch.arange(1, lh.n + 1, device='cuda')      # a slice painted with ids, across the blocks
            k = components_of(vol)
            for z in (0, 2, 5):
                lh2 = _hip.label_holes(_dev(vol), block_voxels=per * H * W)
                np.testing.assert_array_equal(_np(lh2.paint_slice(ids, z)).astype(np.int64), k[z] + 1)
    v = _seams_volume(dtype)
    got, s, t = fill_ref(v)
    assert s == dict(cavities=3, filled=2, voxels_filled=8, shared=1, too_large=0)
    assert got[1, 5, 5] == 0 and (got[3:6, 6, 8] == 0).all() and (got[1:5, 2, 2] == 4).all()


# ------------------------------------------------------------------------------------------------------ fill_volume
def _planted():
    """a (12, 20, 24) uint32 volume of two touching objects with cavities of every fate, cut at z = 7 by two ranks"""
    v = np.zeros((12, 20, 24), np.uint32)
    v[1:11, 1:19, 1:12] = 3
    v[1:11, 1:19, 12:23] = 70000
    v[5:9, 4, 4] = 0                                            # across the cut, walled by 3: filled
    v[6, 10, 16:19] = 0                                         # below the cut, walled by 70000: filled
    v[7, 10, 5] = 0                                             # first slice above the cut: filled
    v[6:8, 14, 11:13] = 0                                       # across the cut and the objects' border: shared
    v[3:8, 16, 20] = 0
    v[7, 16, 20:24] = 0                                         # opened through x = 23 above the cut: the part below too
    v[2:5, 8, 8] = 0                                            # 3 voxels
    return v


def test_fill_volume_on_a_planted_volume():
    from empanada_amd.holes import fill_volume
    v = _planted()
    for cap in (None, 3, 2):
        want, stats, _ = fill_ref(v, cap)
        dev = _dev(v)
        out, s = fill_volume(dev, v.shape, cap)
        assert out is dev and s == stats
        np.testing.assert_array_equal(_np(dev), want)
    assert fill_ref(v)[1] == dict(cavities=5, filled=4, voxels_filled=11, shared=1, too_large=0)
    assert fill_ref(v, 2)[1] == dict(cavities=5, filled=1, voxels_filled=1, shared=1, too_large=3)
    # a slab of a taller volume: z_base moves it off the border, and the slab's own ends stay open without neighbours
    dev = _dev(v[1:11])
    _, s = fill_volume(dev, (14, 20, 24), z_base=2)
    pad = np.zeros((14, 20, 24), np.uint32)
    pad[2:12] = v[1:11]
    np.testing.assert_array_equal(_np(dev), fill_ref(pad)[0][2:12])
    stuff = (v > 0).astype(np.uint8)                            # a uint8 slab: the shared cavity has one wall label now
    dev = _dev(stuff)
    _, s = fill_volume(dev, v.shape)
    np.testing.assert_array_equal(dev.cpu().numpy(), fill_ref(stuff)[0])
    assert s['filled'] == 5 and s['shared'] == 0


# ------------------------------------------------------------------------------------------------------ infer_volume
def _cavities(vol):
    """voxels to punch out of the heads' objects: (n, 3) global coordinates of voxels whose six neighbours carry their
    own label -- singles spread over the volume and columns of two and three along z, one of them across z = 19 | 20,
    the seam of two ranks"""
    v = vol.astype(np.int64)
    inner = v[1:-1, 1:-1, 1:-1]
    ok = inner > 0
    for a in range(3):
        for sl in (slice(0, -2), slice(2, None)):
            idx = [slice(1, -1)] * 3
            idx[a] = sl
            ok &= v[tuple(idx)] == inner
    deep = np.zeros(v.shape, bool)
    deep[1:-1, 1:-1, 1:-1] = ok
    column = deep[:-1] & deep[1:] & (v[:-1] == v[1:])          # (z, y, x) and (z + 1, y, x) both deep in one object
    picks = []
    seam = np.argwhere(column[19])                              # across z = 19 | 20 where an object allows it
    z = 19 if len(seam) else int(np.argwhere(column)[0][0])
    seam = np.argwhere(column[z])
    y, x = (int(i) for i in seam[len(seam) // 2])
    picks += [(z, y, x), (z + 1, y, x)]
    singles = np.argwhere(deep)
    for z, y, x in singles[::max(1, len(singles) // 9)]:
        if all(max(abs(z - p[0]), abs(y - p[1]), abs(x - p[2])) > 2 for p in picks):
            picks.append((z, y, x))
    assert len(picks) >= 5
    return np.array(picks, np.int64)


def _punching(monkeypatch_setattr, coords):
    """the consensus and the stack's painting with the cavities punched into what they return: what split_objects and
    fill_holes then see"""
    from empanada_amd.inference import sharded

    def punch(vols, zs):
        z0, z1 = int(zs[0]), int(zs[1])
        sel = coords[(coords[:, 0] >= z0) & (coords[:, 0] < z1)]
        if len(sel) and 1 in vols:
            vols[1] = vols[1].contiguous()
            z, y, x = (torch.from_numpy(sel[:, a] - (z0 if a == 0 else 0)).to(vols[1].device) for a in range(3))
            flat = vols[1].view(torch.int32).view(-1)
            flat[(z * vols[1].shape[1] + y) * vols[1].shape[2] + x] = 0
        return vols

    consensus, plane = sharded.consensus_volume, sharded.plane_volume

    def consensus_volume(*a, **k):
        cons, vols, zs = consensus(*a, **k)
        return cons, punch(vols, zs), zs

    def plane_volume(*a, **k):
        vols, zs, counts = plane(*a, **k)
        return punch(vols, zs), zs, counts

    monkeypatch_setattr(sharded, 'consensus_volume', consensus_volume)
    monkeypatch_setattr(sharded, 'plane_volume', plane_volume)


def _wanted(vols, split=None):
    key = (id(vols[1]), split)
    if key not in _CACHE:
        coords = _cavities(vols[1])
        punched = vols[1].copy()
        punched[tuple(coords.T)] = 0
        if split is not None:
            punched = split_ref(punched, split, min_size=KW['min_size'], min_span=KW['min_span'])[0]
        want, stats, _ = fill_ref(punched)
        if split is None:                                       # every planted cavity is closed again
            assert stats['filled'] >= len(coords) - 1 and (want[tuple(coords.T)] == vols[1][tuple(coords.T)]).all()
        _CACHE[key] = (coords, punched, want, stats)
    return _CACHE[key]


def _assert_filled(res, vols, split=None):
    coords, punched, want, stats = _wanted(vols, split)
    np.testing.assert_array_equal(_np(res['volumes'][1]), want)
    np.testing.assert_array_equal(_np(res['volumes'][2]), vols[2])          # a stuff class stays as it is
    assert res['filled'] == {1: stats} and stats['voxels_filled'] == int((want != punched).sum()) > 0
    if 'objects' in res:
        for c in (1, 2):
            np.testing.assert_array_equal(res['objects'][c], measure_ref(_np(res['volumes'][c])))
    for c, ds in res['datasets'].items():
        if ds is not None:
            np.testing.assert_array_equal(np.asarray(ds[...]), _np(res['volumes'][c]))


def test_infer_volume_plain_path_with_a_store(tmp_path, case, monkeypatch):
    eng, vol, vols, sets, counts = case(ORTHO)
    _punching(monkeypatch.setattr, _wanted(vols)[0])
    res = _run(eng, vol, tmp_path / 's.zarr', axes=ORTHO, fill_holes=True, measure=True, pyramid=1, compressor='zlib')
    _assert_filled(res, vols)
    assert dict(res['instances']) == counts                                # objects only grow
    from empanada_amd.inference import pyramid as pyr
    np.testing.assert_array_equal(_np(res['pyramid'][1][0]), _np(pyr.build(res['volumes'][1], [(2, 2, 2)])[0]))
    # a cap of one voxel leaves the columns of two: too_large
    capped = _run(eng, vol, None, axes=ORTHO, fill_holes=1)
    coords, punched, want, stats = _wanted(vols)
    want1, stats1, _ = fill_ref(punched, 1)
    np.testing.assert_array_equal(_np(capped['volumes'][1]), want1)
    assert capped['filled'] == {1: stats1} and stats1['too_large'] >= 1
    # together with split_objects: the split sees the punched volume, the filling what the split left
    both = _run(eng, vol, None, axes=ORTHO, split_objects=26, fill_holes=True, measure=True)
    _assert_filled(both, vols, 26)
    assert 'split' in both
    # off: the parent's keys, and the punched volumes as they are
    off = _run(eng, vol, tmp_path / 'n.zarr', axes=ORTHO, fill_holes=None)
    assert sorted(off) == ['datasets', 'instances', 'volumes', 'z_range'] and dict(off['instances']) == counts
    np.testing.assert_array_equal(_np(off['volumes'][1]), punched)


def test_infer_volume_stack_mode_and_windows(tmp_path, case, monkeypatch):
    eng, vol, vols, _, counts = case(('xy',))
    _punching(monkeypatch.setattr, _wanted(vols)[0])
    _assert_filled(_run(eng, vol, None, axes=('xy',), fill_holes=True, measure=True), vols)
    kw = dict(axes=('xy',), batch_pixels=4 * 96 * 96, window_slices=8)      # 4 slices per model call, windows of 8
    win = _run(eng, vol, tmp_path / 'w.zarr', fill_holes=True, **kw)
    assert win['windows']['xy'] > 1
    _assert_filled(win, vols)


def test_infer_volume_pipeline(tmp_path, case, monkeypatch):
    from empanada_amd.inference.pipeline import VolumePipeline
    eng, vol, vols, sets, counts = case(ORTHO)
    _punching(monkeypatch.setattr, _wanted(vols)[0])
    pipe = VolumePipeline(eng, tune=False, graph=True, overlap=True, batch_pixels=1 << 22)
    try:
        res = _run(eng, vol, tmp_path / 'a.zarr', axes=ORTHO, fill_holes=True, measure=True, pipeline=pipe)
        _assert_filled(res, vols)
        off = _run(eng, vol, None, axes=ORTHO, pipeline=pipe)
        assert 'filled' not in off and dict(off['instances']) == counts
    finally:
        pipe.close()


# ----------------------------------------------------------------------------------------------- two ranks over gloo
def _rank(rank, world, port, path, coords, q):
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        from empanada_amd.holes import fill_volume
        from empanada_amd.inference import sharded
        v = _planted()
        z0, z1 = (0, 7) if rank == 0 else (7, 12)                            # the cut goes through three cavities
        dev = _dev(v[z0:z1])
        _, planted_stats = fill_volume(dev, v.shape, group=dist.group.WORLD, z_base=z0)
        _punching(lambda obj, name, value: setattr(obj, name, value), coords)
        eng, vol = _engine(), SY.em_volume(SHAPE, seed=3)
        res = _run(eng, vol, path, axes=ORTHO, group=dist.group.WORLD, fill_holes=True, measure=True)
        q.put((rank, tuple(res['z_range']), _np(res['volumes'][1]), res['filled'], dict(res['instances']), res['objects'],
               _np(dev), planted_stats))
    finally:
        dist.destroy_process_group()


def test_two_ranks(tmp_path, case):
    import torch.multiprocessing as mp
    from empanada_amd.zarr_utils import ZarrV2Group
    eng, vol, vols, sets, counts = case(ORTHO)
    coords, punched, want, stats = _wanted(vols)
    assert coords[0].tolist()[0] == 19 and coords[1].tolist()[0] == 20, "no planted cavity crosses the ranks' seam"
    planted_want, planted_stats, _ = fill_ref(_planted())
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    path = str(tmp_path / 'two.zarr')
    port = _free_port()
    procs = [ctx.Process(target=_rank, args=(r, 2, port, path, coords, q)) for r in range(2)]
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
        assert got[r][2] == {1: stats} and got[r][3] == counts and got[r][6] == planted_stats
        np.testing.assert_array_equal(got[r][4][1], measure_ref(want))
    np.testing.assert_array_equal(np.asarray(ZarrV2Group(path, mode='r')[NAMES[1]]), want)
