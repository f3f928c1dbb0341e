"""GPU: _hip.label_edt / label_erode / label_dilate and morphology.morph_volume equal the checker of test_morph_host.py
(scipy's exact transform label by label, numpy shifts over the ball's offsets) -- exact integers, no tolerance -- over
halos, z-blocks and ranks, and infer_volume(morph=) reshapes the volumes before anything else reads them, on every
path."""
import os
import queue
import time

import numpy as np
import pytest
import torch

from empanada_amd import morphology as MO
from empanada_amd import synthetic as SY
from test_components_host import split_ref
from test_holes_host import fill_ref, planted_volume
from test_measure_host import measure_ref
from test_morph_host import R2S, REFS, SAMPLINGS, blobs, close_ref, dilate_ref, edt_ref, erode_ref, morph_ref, open_ref
from test_pyramid_gpu import KW, NAMES, ORTHO, SHAPE, _dev, _engine, _free_port, _np, _run, case  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

DTYPES = [np.uint8, np.uint32]
OPS = ('erode', 'dilate', 'open', 'close')
_CACHE = {}


def _halo(t):
    return None if t is None else _dev(t)


def _edt(vol, sampling=(1, 1, 1), cap=65535, below=None, above=None, **kw):
    from empanada_amd import _hip
    out = _hip.label_edt(_dev(vol), sampling, cap, below=_halo(below), above=_halo(above), **kw)
    assert out.dtype == torch.uint16 and out.is_cuda and tuple(out.shape) == vol.shape
    return out.view(torch.int16).cpu().numpy().view(np.uint16)


def _step(op, vol, r2, sampling=(1, 1, 1), below=None, above=None, **kw):
    from empanada_amd import _hip
    dev = _dev(vol)
    fn = _hip.label_erode if op == 'erode' else _hip.label_dilate
    out = fn(dev, r2, sampling, below=_halo(below), above=_halo(above), **kw)
    assert out.dtype == dev.dtype and out.is_cuda and tuple(out.shape) == vol.shape and out.data_ptr() != dev.data_ptr()
    np.testing.assert_array_equal(_np(dev), vol)                # the input is not written
    return _np(out)


def _morph(op, vol, r2, sampling=(1, 1, 1)):
    out, stats = MO.morph_volume(_dev(vol), vol.shape, op, r2, sampling)
    got = _np(out)
    assert stats == dict(op=op, r2=r2, sampling=tuple(sampling), voxels_removed=int(((vol != 0) & (got == 0)).sum()),
                         voxels_added=int(((vol == 0) & (got != 0)).sum()))
    return got


# ------------------------------------------------------------------------------------------------------ random volumes
@pytest.mark.parametrize('dtype', DTYPES, ids=['u8', 'u32'])
@pytest.mark.parametrize('shape', [(13, 21, 37), (5, 16, 64), (6, 9, 1), (1, 9, 12), (3, 4, 300), (2, 70, 5)],
                         ids=lambda s: 'x'.join(map(str, s)))
def test_kernels_equal_the_checker(shape, dtype):
    for seed in (0, 1):
        vol = planted_volume(shape, dtype, seed)
        for sampling in SAMPLINGS:
            msg = f'seed {seed}, sampling {sampling}'
            for cap in (2, 10, 65535):
                np.testing.assert_array_equal(_edt(vol, sampling, cap), edt_ref(vol, sampling, cap), err_msg=f'{msg}, cap {cap}')
            for r2 in R2S:
                er, di = erode_ref(vol, r2, sampling), dilate_ref(vol, r2, sampling)
                assert (er != vol).any() and (di != vol).any(), f'{msg}: r2 {r2} changes nothing'
                np.testing.assert_array_equal(_step('erode', vol, r2, sampling), er, err_msg=f'{msg}, erode {r2}')
                np.testing.assert_array_equal(_step('dilate', vol, r2, sampling), di, err_msg=f'{msg}, dilate {r2}')
                want = dilate_ref(er, r2, sampling)
                np.testing.assert_array_equal(_morph('open', vol, r2, sampling), want, err_msg=f'{msg}, open {r2}')
                want = np.where(vol != 0, vol, erode_ref(di, r2, sampling))
                np.testing.assert_array_equal(_morph('close', vol, r2, sampling), want, err_msg=f'{msg}, close {r2}')
    vol = blobs(shape, dtype, seed=2)                            # solid objects: distances beyond the first steps
    np.testing.assert_array_equal(_edt(vol), edt_ref(vol))
    for op in OPS:
        for r2 in (1, 4, 9):
            np.testing.assert_array_equal(_morph(op, vol, r2), REFS[op](vol, r2), err_msg=f'{op} {r2}')


# ------------------------------------------------------------------------------------------------------ probes
@pytest.mark.parametrize('dtype', DTYPES, ids=['u8', 'u32'])
def test_probes(dtype):
    # one label fills the volume: no candidate anywhere, cap everywhere, and the erosion keeps all
    solid = np.full((4, 5, 70), 9, dtype)
    for cap in (1, 77, 65535):
        assert (_edt(solid, cap=cap) == cap).all()
    for r2 in (1, 25, 65534):
        np.testing.assert_array_equal(_step('erode', solid, r2), solid)
        np.testing.assert_array_equal(_step('dilate', solid, r2), solid)
    # a single voxel
    one = np.zeros((5, 7, 9), dtype)
    one[2, 3, 4] = 6
    assert _edt(one).sum() == 1 and _edt(one, (3, 2, 1))[2, 3, 4] == 1 and _edt(one, (3, 2, 2))[2, 3, 4] == 4
    assert not _step('erode', one, 1).any() and not _morph('open', one, 1).any()
    np.testing.assert_array_equal(_step('dilate', one, 3), dilate_ref(one, 3))
    assert (_step('dilate', one, 3) == 6).sum() == 27 and (_step('dilate', one, 2) == 6).sum() == 19
    assert (_step('dilate', one, 1) == 6).sum() == 7 and (_step('dilate', one, 9, (3, 1, 1)) == 6).sum() == 29 + 2
    np.testing.assert_array_equal(_morph('close', one, 2), one)
    # two labels touching: the erosion opens a gap on both sides, along every axis
    for axis in range(3):
        two = np.zeros((8, 8, 8), dtype)
        idx = [slice(None)] * 3
        idx[axis] = slice(0, 4)
        two[tuple(idx)] = 3
        idx[axis] = slice(4, 8)
        two[tuple(idx)] = 7
        got = _step('erode', two, 1)
        np.testing.assert_array_equal(got, erode_ref(two, 1))
        line = np.moveaxis(got, axis, 0)[:, 3, 3].tolist()
        assert line == [3, 3, 3, 0, 0, 7, 7, 7]                # the faces of the volume do not erode
        d = np.moveaxis(_edt(two), axis, 0)[:, 3, 3].tolist()
        assert d == [16, 9, 4, 1, 1, 4, 9, 16]
    # a label on a face is not eroded from that face
    face = np.zeros((6, 6, 6), dtype)
    face[0:3, 0:4, 2:6] = 5
    got = _step('erode', face, 1)
    want = np.zeros_like(face)
    want[0:2, 0:3, 3:6] = 5
    np.testing.assert_array_equal(got, want)
    # a gap voxel as far from 3 as from 7 becomes 7; with 7 farther by one it becomes 3
    gap = np.zeros((3, 3, 9), dtype)
    gap[:, :, 0:2], gap[:, :, 3:5] = 3, 7
    assert (_step('dilate', gap, 1)[:, :, 2] == 7).all()
    gap = np.zeros((3, 3, 9), dtype)
    gap[:, :, 0:2], gap[:, :, 4:6] = 3, 7
    got = _step('dilate', gap, 4)
    assert (got[:, :, 2] == 3).all() and (got[:, :, 3] == 7).all() and (got[:, :, 6:8] == 7).all() and not got[:, :, 8].any()
    for axis in (0, 1):                                         # the tie along y and along z
        tie = np.zeros((5, 5, 5), dtype)
        idx = [2, 2, 2]
        idx[axis] = 1
        tie[tuple(idx)] = 7
        idx[axis] = 3
        tie[tuple(idx)] = 3
        assert _step('dilate', tie, 1)[2, 2, 2] == 7
        tie[tuple(idx)] = 9
        assert _step('dilate', tie, 1)[2, 2, 2] == 9
    # the dilation never changes a non-zero voxel
    vol = planted_volume((7, 9, 30), dtype, 5)
    for r2 in (1, 9):
        got = _step('dilate', vol, r2)
        assert (got[vol != 0] == vol[vol != 0]).all() and (got != vol).any()


def test_the_opening_of_a_dumbbell_removes_exactly_the_bridge():
    v = np.zeros((9, 9, 19), np.uint32)
    v[2:7, 2:7, 2:7] = 4
    v[2:7, 2:7, 12:17] = 4
    v[4, 4, 7:12] = 4                                           # a bridge of one voxel's width
    got = _morph('open', v, 3)                                  # the 26-neighbourhood: a box is open under it already
    want = v.copy()
    want[4, 4, 7:12] = 0
    np.testing.assert_array_equal(got, open_ref(v, 3))
    np.testing.assert_array_equal(got, want)
    got1 = _morph('open', v, 1)                                 # the 6-neighbourhood also rounds the boxes' edges off
    np.testing.assert_array_equal(got1, open_ref(v, 1))
    assert (got1[4, 4, 8:11] == 0).all() and ((got1 != 0) <= (v != 0)).all()
    from empanada_amd import components
    out, stats = components.split_volume(_dev(got), 6, None, None)
    assert stats['objects_in'] == 1 and stats['objects_out'] == 2


def test_large_labels_and_int32_input():
    from empanada_amd import _hip
    top, big = 0xffffffff, 0x80000000
    v = np.zeros((5, 6, 12), np.uint32)
    v[1:4, 1:5, 1:5], v[1:4, 1:5, 5:9], v[1:4, 1:5, 10] = top, big, 3
    for op in OPS:
        for r2 in (1, 3):
            np.testing.assert_array_equal(_morph(op, v, r2), REFS[op](v, r2), err_msg=f'{op} {r2}')
    got = _step('dilate', v, 1)
    assert (got[1:4, 1:5, 9] == big).all() and got[2, 2, 0] == top and got[0, 2, 4] == top and got[0, 2, 5] == big
    np.testing.assert_array_equal(_edt(v), edt_ref(v))
    dev = torch.from_numpy(v.view(np.int32)).cuda()             # the bits of an int32 are taken as they are
    out = _hip.label_dilate(dev, 1)
    assert out.dtype == torch.int32
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), got)
    out = _hip.label_erode(dev, 1)
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), erode_ref(v, 1))


def test_empty_slabs_and_argument_errors():
    from empanada_amd import _hip
    for tdt in (torch.uint8, torch.uint32):
        for shape in ((0, 5, 7), (0, 1, 1)):
            empty = torch.zeros(shape, dtype=tdt, device='cuda')
            info = {}
            out = _hip.label_edt(empty, info=info)
            assert tuple(out.shape) == shape and out.dtype == torch.uint16 and info == dict(blocks=0, work_bytes=0)
            for fn in (_hip.label_erode, _hip.label_dilate):
                out = fn(empty, 4)
                assert tuple(out.shape) == shape and out.dtype == tdt
            out, stats = MO.morph_volume(empty, (9,) + shape[1:], 'open', 1)
            assert tuple(out.shape) == shape and stats['voxels_removed'] == stats['voxels_added'] == 0
    slab = torch.zeros((3, 5, 70), dtype=torch.uint8, device='cuda')
    for bad in (dict(below=torch.zeros((5, 70), dtype=torch.uint8, device='cuda')),
                dict(below=torch.zeros((1, 5, 7), dtype=torch.uint8, device='cuda')),
                dict(above=torch.zeros((1, 5, 70), dtype=torch.int32, device='cuda')),
                dict(above=torch.zeros((1, 5, 70), dtype=torch.uint8)),
                dict(above=torch.zeros((2, 5, 140), dtype=torch.uint8, device='cuda')[:, :, ::2])):
        for fn, args in ((_hip.label_edt, ()), (_hip.label_erode, (1,)), (_hip.label_dilate, (1,))):
            with pytest.raises(ValueError, match='label_'):
                fn(slab, *args, **bad)
    with pytest.raises(ValueError, match='contiguous'):
        _hip.label_erode(torch.zeros((3, 5, 70), dtype=torch.uint8, device='cuda')[:, :, ::2], 1)
    with pytest.raises(ValueError, match='D, H, W'):
        _hip.label_dilate(torch.zeros((5, 70), dtype=torch.uint8, device='cuda'), 1)
    with pytest.raises(ValueError, match='single slice'):
        _hip.label_erode(slab, 1, block_voxels=5 * 70 - 1)
    with pytest.raises(ValueError, match='operation'):
        MO.morph_volume(slab, (3, 5, 70), 'thin', 1)


@pytest.mark.parametrize('offset', [1, 2, 3])
def test_unaligned_slab_takes_the_narrow_path(offset):
    """the slab starts 1, 2 or 3 elements off a 16-byte (uint32) / 4-byte (uint8) address inside a larger buffer"""
    from empanada_amd import _hip
    for dtype, tdt in ((np.uint32, torch.int32), (np.uint8, torch.uint8)):
        for shape in ((3, 6, 64), (4, 5, 259)):
            a = blobs(shape, dtype, seed=offset)
            flat = torch.full((a.size + 64,), 77, dtype=tdt, device='cuda')
            flat[16 + offset:16 + offset + a.size] = _dev(a).view(tdt).ravel()
            dev = flat[16 + offset:16 + offset + a.size].view(a.shape)
            assert dev.data_ptr() % (4 * dev.element_size()) != 0 and dev.is_contiguous()
            out = _hip.label_edt(dev)
            np.testing.assert_array_equal(out.view(torch.int16).cpu().numpy().view(np.uint16), edt_ref(a), err_msg=str(shape))
            out = _hip.label_erode(dev, 2)
            np.testing.assert_array_equal(out.cpu().numpy().view(dtype), erode_ref(a, 2), err_msg=str(shape))
            out = _hip.label_dilate(dev, 2)
            np.testing.assert_array_equal(out.cpu().numpy().view(dtype), dilate_ref(a, 2), err_msg=str(shape))


# ------------------------------------------------------------------------------------------------------ halos and blocks
def _whole(dtype):
    if ('whole', dtype) not in _CACHE:
        vol = np.concatenate([planted_volume((6, 10, 11), dtype, 7, punch=0.02, cell=5), blobs((6, 10, 11), dtype, 8)])
        want = {('edt', s, cap): edt_ref(vol, s, cap) for s in ((1, 1, 1), (2, 1, 1)) for cap in (5, 30)}
        for s in ((1, 1, 1), (2, 1, 1)):
            for r2 in (1, 4, 9):
                if r2 >= min(s) ** 2:
                    want.update({(op, s, r2): REFS[op](vol, r2, s) for op in OPS})
        _CACHE['whole', dtype] = (vol, want)
    return _CACHE['whole', dtype]


@pytest.mark.parametrize('dtype', DTYPES, ids=['u8', 'u32'])
def test_every_z_cut_with_its_halo_stacks_equals_the_whole(dtype):
    import math
    vol, want = _whole(dtype)
    assert vol.shape == (12, 10, 11)
    for (what, s, bound), full in want.items():
        if what in ('open', 'close'):
            continue
        h = math.isqrt(bound - 1 if what == 'edt' else bound) // s[0]
        for z0, z1 in ((0, 5), (5, 12), (3, 4), (1, 11), (11, 12), (4, 9)):
            for extra in (0, 2):                               # the halo that is needed, and a deeper one
                below = vol[max(0, z0 - h - extra):z0] if z0 and h + extra else None
                above = vol[z1:z1 + h + extra] if z1 < 12 and h + extra else None
                if what == 'edt':
                    got = _edt(vol[z0:z1], s, bound, below, above)
                else:
                    got = _step(what, vol[z0:z1], bound, s, below, above)
                np.testing.assert_array_equal(got, full[z0:z1], err_msg=f'{what} {s} {bound}: [{z0}, {z1}) + {extra}')


@pytest.mark.parametrize('dtype', DTYPES, ids=['u8', 'u32'])
def test_blocks_equal_the_undivided_call(dtype, monkeypatch):
    from empanada_amd import _hip
    vol, want = _whole(dtype)
    H, W = vol.shape[1:]
    for per in (1, 3):
        for (what, s, bound), full in want.items():
            info = {}
            kw = dict(block_voxels=per * H * W + 5, info=info)
            if what == 'edt':
                got = _edt(vol, s, bound, **kw)
            elif what in ('erode', 'dilate'):
                got = _step(what, vol, bound, s, **kw)
            else:                                               # the compound operations through morph_volume
                for name in ('label_erode', 'label_dilate'):
                    monkeypatch.setattr(_hip, name, lambda *a, _f=getattr(_hip, name), **k: _f(*a, **dict(k, **kw)))
                got = _morph(what, vol, bound, s)
                monkeypatch.undo()
            assert info['blocks'] == 12 // per and info['work_bytes'] > 0
            np.testing.assert_array_equal(got, full, err_msg=f'{what} {s} {bound}: blocks of {per}')
    # a block at the slab's end is continued by the caller's stacks
    for what, bound in (('erode', 9), ('dilate', 9)):
        got = _step(what, vol[2:10], bound, (1, 1, 1), vol[0:2], vol[10:12], block_voxels=2 * H * W)
        np.testing.assert_array_equal(got, want[what, (1, 1, 1), 9][2:10])
    got = _edt(vol[2:10], (1, 1, 1), 30, vol[0:2], vol[10:12], block_voxels=H * W)
    np.testing.assert_array_equal(got, want['edt', (1, 1, 1), 30][2:10])


# ------------------------------------------------------------------------------------------------------ ranks
RANK_CASES = [('erode', 4, (1, 1, 1)), ('dilate', 9, (1, 1, 1)), ('open', 4, (1, 1, 1)), ('close', 4, (1, 1, 1)),
              ('open', 9, (2, 1, 1)), ('close', 2, (1, 1, 1)), ('open', 1, (1, 1, 1))]
RANK_BOUNDS = {2: [(0, 7, 12), (0, 1, 12), (0, 0, 12)], 3: [(0, 4, 8, 12), (0, 5, 6, 12), (0, 3, 3, 12), (0, 1, 2, 12)]}


def _rank(rank, world, port, q, infer_path):
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        vol, _ = _whole(np.uint32)
        out = []
        for b in RANK_BOUNDS[world]:
            for op, r2, s in RANK_CASES:
                new, stats = MO.morph_volume(_dev(vol[b[rank]:b[rank + 1]]), vol.shape, op, r2, s, group=dist.group.WORLD,
                                             z_base=b[rank])
                out.append((_np(new), stats))
        res = None
        if infer_path is not None:
            eng, em = _engine(), SY.em_volume(SHAPE, seed=3)
            r = _run(eng, em, infer_path, axes=ORTHO, group=dist.group.WORLD, morph=('open', 2), measure=True)
            res = (tuple(r['z_range']), _np(r['volumes'][1]), r['morph'], dict(r['instances']), r['objects'])
        q.put((rank, out, res))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize('world', [2, 3])
def test_ranks(world, tmp_path, case):
    """every rank's slab is its part of the single-rank result and the stats are the same on all ranks; the bounds
    include a rank with fewer slices than the halo and an empty rank.  World 2 also runs infer_volume(morph=)."""
    import torch.multiprocessing as mp
    from empanada_amd.zarr_utils import ZarrV2Group
    vol, _ = _whole(np.uint32)
    path = str(tmp_path / 'two.zarr') if world == 2 else None
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank, args=(r, world, port, q, path)) for r in range(world)]
    for p in procs:
        p.start()
    got, deadline = {}, time.monotonic() + 240                 # the ranks' own time limit: they are ended, not waited for
    try:
        while len(got) < world:                                 # a rank that died is reported at once
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
    i = 0
    for b in RANK_BOUNDS[world]:
        for op, r2, s in RANK_CASES:
            want = REFS[op](vol, r2, s)
            stats = dict(op=op, r2=r2, sampling=s, voxels_removed=int(((vol != 0) & (want == 0)).sum()),
                         voxels_added=int(((vol == 0) & (want != 0)).sum()))
            assert stats['voxels_removed'] + stats['voxels_added'] > 0
            for r in range(world):
                np.testing.assert_array_equal(got[r][0][i][0], want[b[r]:b[r + 1]], err_msg=f'{op} {r2} {s} {b} rank {r}')
                assert got[r][0][i][1] == stats
            i += 1
    if world == 2:
        eng, em, vols, sets, counts = case(ORTHO)
        want = morph_ref(vols[1], ('open', 2))
        assert got[0][1][0] == (0, 20) and got[1][1][0] == (20, 40)
        np.testing.assert_array_equal(np.concatenate([got[0][1][1], got[1][1][1]]), want)
        for r in (0, 1):
            assert got[r][1][2] == {1: _stats(vols[1], want, ('open', 2))}
            assert got[r][1][3] == {**counts, 1: len(np.unique(want[want != 0]))}
            np.testing.assert_array_equal(got[r][1][4][1], measure_ref(want))
        np.testing.assert_array_equal(np.asarray(ZarrV2Group(path, mode='r')[NAMES[1]]), want)


# ------------------------------------------------------------------------------------------------------ infer_volume
MORPHS = [('open', 1), ('close', 1.5, (2, 1, 1))]


def _stats(before, after, morph):
    op, r2, sampling = MO.check(morph)
    return dict(op=op, r2=r2, sampling=sampling, voxels_removed=int(((before != 0) & (after == 0)).sum()),
                voxels_added=int(((before == 0) & (after != 0)).sum()))


def _wanted(vols, morph, repair=False):
    key = (id(vols[1]), morph, repair)
    if key not in _CACHE:
        want = morph_ref(vols[1], morph)
        stats = _stats(vols[1], want, morph)
        assert stats['voxels_removed'] + stats['voxels_added'] > 0, "the operation should change the volume"
        n = len(np.unique(want[want != 0])) if stats['op'] in ('erode', 'open') else None    # None: the counts stay
        if repair:                                              # split_objects=26 and fill_holes=True behind it
            want, split, _ = split_ref(want, 26, min_size=KW['min_size'], min_span=KW['min_span'])
            n = split['objects_out']
            want = fill_ref(want)[0]
        _CACHE[key] = (want, stats, n)
    return _CACHE[key]


def _assert_morphed(res, vols, counts, morph, repair=False):
    want, stats, n = _wanted(vols, morph, repair)
    np.testing.assert_array_equal(_np(res['volumes'][1]), want)
    np.testing.assert_array_equal(_np(res['volumes'][2]), vols[2])          # a stuff class stays as it is
    assert res['morph'] == {1: stats}
    assert dict(res['instances']) == (counts if n is None else {**counts, 1: n})
    if 'objects' in res:
        for c in (1, 2):
            np.testing.assert_array_equal(res['objects'][c], measure_ref(_np(res['volumes'][c])))
    if 'pyramid' in res:
        from empanada_amd.inference import pyramid as pyr
        np.testing.assert_array_equal(_np(res['pyramid'][1][0]), _np(pyr.build(res['volumes'][1], [(2, 2, 2)])[0]))
    for c, ds in res['datasets'].items():
        if ds is not None:
            np.testing.assert_array_equal(np.asarray(ds[...]), _np(res['volumes'][c]))


@pytest.mark.parametrize('morph', MORPHS, ids=['open', 'close'])
def test_infer_volume_plain_path_with_a_store(tmp_path, case, morph):
    eng, vol, vols, sets, counts = case(ORTHO)
    res = _run(eng, vol, tmp_path / 's.zarr', axes=ORTHO, morph=morph, measure=True, pyramid=1, compressor='zlib')
    _assert_morphed(res, vols, counts, morph)
    assert 'split' not in res and 'filled' not in res
    # with split_objects and fill_holes: they see the morphed volume, in that order
    both = _run(eng, vol, None, axes=ORTHO, morph=morph, split_objects=26, fill_holes=True, measure=True)
    _assert_morphed(both, vols, counts, morph, repair=True)
    assert 'split' in both and 'filled' in both
    # off: the parent's keys and bytes
    off = _run(eng, vol, tmp_path / 'n.zarr', axes=ORTHO, morph=None)
    assert sorted(off) == ['datasets', 'instances', 'volumes', 'z_range'] and dict(off['instances']) == counts
    for c in (1, 2):
        assert _np(off['volumes'][c]).tobytes() == vols[c].tobytes()


@pytest.mark.parametrize('morph', MORPHS, ids=['open', 'close'])
def test_infer_volume_stack_mode_and_windows(tmp_path, case, morph):
    eng, vol, vols, _, counts = case(('xy',))
    _assert_morphed(_run(eng, vol, None, axes=('xy',), morph=morph, measure=True), vols, counts, morph)
    kw = dict(axes=('xy',), batch_pixels=4 * 96 * 96, window_slices=8)      # 4 slices per model call, windows of 8
    win = _run(eng, vol, tmp_path / 'w.zarr', morph=morph, **kw)
    assert win['windows']['xy'] > 1
    _assert_morphed(win, vols, counts, morph)


def test_infer_volume_pipeline(tmp_path, case):
    from empanada_amd.inference.pipeline import VolumePipeline
    eng, vol, vols, sets, counts = case(ORTHO)
    pipe = VolumePipeline(eng, tune=False, graph=True, overlap=True, batch_pixels=1 << 22)
    try:
        for morph in MORPHS:
            res = _run(eng, vol, tmp_path / f'{morph[0]}.zarr', axes=ORTHO, morph=morph, measure=True, pipeline=pipe)
            _assert_morphed(res, vols, counts, morph)
        off = _run(eng, vol, None, axes=ORTHO, pipeline=pipe)
        assert 'morph' not in off and dict(off['instances']) == counts
        assert _np(off['volumes'][1]).tobytes() == vols[1].tobytes()
    finally:
        pipe.close()


def test_infer_volume_rejects_a_bad_morph_before_any_work(case):
    eng, vol, _, _, _ = case(ORTHO)
    for bad in (('open', 0), ('thin', 1), ('open', 1, (0, 1, 1)), 'open'):
        with pytest.raises(ValueError, match='morph'):
            _run(eng, vol, None, axes=ORTHO, morph=bad)
