"""GPU: _hip.label_grow equals the level-by-level flood of separate_ref.py and separation.separate_volume equals
separate_ref (scipy's transform and labelling, the flood, plan) -- bit for bit -- over tile borders, z-blocks, halos and
ranks, and infer_volume(separate=) repairs the volumes after morph and before split_objects, on every path."""
import os
import queue
import time

import numpy as np
import pytest
import torch

from empanada_amd import separation as SP
from empanada_amd import synthetic as SY
from separate_ref import (ball, dumbbell, grow_ref, random_case, separate_ref, serpentine_flat, serpentine_tall)
from test_components_host import split_ref
from test_holes_host import fill_ref
from test_measure_host import measure_ref
from test_morph_host import morph_ref
from test_pyramid_gpu import KW, NAMES, ORTHO, SHAPE, _dev, _engine, _free_port, _np, _run, case  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

TILE = (8, 8, 64)
SHAPES = [(1, 1, 1), (1, 1, 130), (5, 13, 70), (9, 17, 130), (19, 9, 67), tuple(t + 1 for t in TILE)]
_CACHE = {}


def _grow(lab, seeds, **kw):
    from empanada_amd import _hip
    dev = _dev(lab)
    g = _hip.label_grow(dev, _dev(seeds), **kw)
    own = g.owners()
    assert own.dtype == torch.uint32 and own.is_cuda and tuple(own.shape) == lab.shape
    np.testing.assert_array_equal(_np(dev), lab)                # the input is not written
    return _np(own), g


def _want(name, make):
    if name not in _CACHE:
        lab, seeds = make()
        _CACHE[name] = (lab, seeds, grow_ref(lab, seeds)[0])
    return _CACHE[name]


# ------------------------------------------------------------------------------------------------------ random volumes
@pytest.mark.parametrize('dtype', [np.uint8, np.uint32], ids=['u8', 'u32'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_label_grow_equals_the_checker(shape, dtype):
    for seed, n_labels in ((0, 3), (1, 4)):
        for density in (0.0, 'one', 0.05):
            for big in ((False, True) if dtype == np.uint32 else (False,)):
                lab, seeds = random_case(shape, seed, n_labels, density=density, dtype=dtype, big=big)
                if seed == 1 and big:                           # solid objects: paths across many tiles
                    lab[:] = np.where(lab != 0, lab.max(), 0)
                info = {}
                got, g = _grow(lab, seeds, info=info)
                np.testing.assert_array_equal(got, grow_ref(lab, seeds)[0], err_msg=f'{seed} {density} {big}')
                assert info['blocks'] == 1 and info['rounds'] == 1 and info['sweeps'] == g.sweeps
                assert info['work_bytes'] >= 8 * lab.size
                if not lab.any():
                    assert info['active_tiles'] == 0 and g.sweeps == 0


def test_int32_bits_are_taken_as_they_are():
    from empanada_amd import _hip
    lab, seeds = random_case((5, 13, 70), 3, density=0.02, big=True)
    g = _hip.label_grow(torch.from_numpy(lab.view(np.int32)).cuda(), torch.from_numpy(seeds.view(np.int32)).cuda())
    want = grow_ref(lab, seeds)[0]
    assert want.max() == 2 ** 32 - 1 and (want >= 2 ** 31).any()
    np.testing.assert_array_equal(_np(g.owners()), want)


# ------------------------------------------------------------------------------------------------------ probes
@pytest.mark.parametrize('dtype', [np.uint8, np.uint32], ids=['u8', 'u32'])
def test_probes(dtype):
    # two seeds equidistant from a voxel: the larger wins; a seed on background is ignored; labels are not crossed;
    # labelled voxels that no seed reaches have owner 0
    lab = np.zeros((3, 3, 140), dtype)
    seeds = np.zeros((3, 3, 140), np.uint32)
    lab[1, 1, :129] = 3
    lab[1, 1, 129:135] = 4                                       # touches label 3
    lab[1, 1, 137:] = 3                                          # the same label, but no path
    seeds[1, 1, 0], seeds[1, 1, 128], seeds[1, 1, 130], seeds[0, 0, 5] = 7, 9, 2, 5
    got, _ = _grow(lab, seeds)
    assert got[1, 1].tolist() == [7] * 64 + [9] * 65 + [2] * 6 + [0] * 5
    assert not got[0].any() and not got[2].any() and not got[1, 0].any()
    seeds[1, 1, 0], seeds[1, 1, 128] = 9, 7
    assert _grow(lab, seeds)[0][1, 1, :129].tolist() == [9] * 65 + [7] * 64
    # all zero, and seeds alone
    zero = np.zeros((3, 9, 70), dtype)
    got, g = _grow(zero, seeds[:, :, :70].repeat(3, axis=1))
    assert not got.any() and g.sweeps == 0
    solid = np.full((9, 9, 65), 2, dtype)
    none = np.zeros(solid.shape, np.uint32)
    assert not _grow(solid, none)[0].any()
    none[8, 8, 64] = 2 ** 32 - 1
    assert (_grow(solid, none)[0] == 2 ** 32 - 1).all()


def test_empty_and_refusals():
    from empanada_amd import _hip
    empty = torch.zeros((0, 5, 7), dtype=torch.uint8, device='cuda')
    info = {}
    g = _hip.label_grow(empty, torch.zeros((0, 5, 7), dtype=torch.uint32, device='cuda'), info=info)
    assert tuple(g.owners().shape) == (0, 5, 7) and g.sweeps == 0 and info['blocks'] == 0 and g.ends() is None
    assert tuple(g.paint([0], dtype=torch.uint8).shape) == (0, 5, 7)
    lab = torch.ones((4, 6, 8), dtype=torch.uint8, device='cuda')
    seeds = torch.zeros((4, 6, 8), dtype=torch.int32, device='cuda').view(torch.uint32)
    for bad, match in (((lab.permute(0, 2, 1), seeds), 'contiguous|expected'), ((lab[:, :, ::2], seeds[:, :, ::2]), 'contiguous'),
                       ((lab.float(), seeds), 'dtype'), ((lab, seeds.view(torch.int32).float()), 'dtype'),
                       ((lab, seeds.view(torch.int32).long()), 'dtype'), ((lab.cpu(), seeds), 'GPU'),
                       ((lab, seeds.cpu()), 'GPU'), ((lab, seeds[:3]), 'expected'), ((lab[0], seeds[0]), r'\(D, H, W\)'),
                       ((_np(lab), seeds), 'tensor')):
        with pytest.raises(ValueError, match=match):
            _hip.label_grow(*bad)
    state = torch.zeros((6, 8), dtype=torch.int64, device='cuda')
    for kw, match in ((dict(block_voxels=0), 'block_voxels'), (dict(block_voxels=2 ** 31), 'block_voxels'),
                      (dict(block_voxels=47), 'single slice'), (dict(max_sweeps=0), 'max_sweeps'),
                      (dict(max_sweeps=1.5), 'max_sweeps'), (dict(below=lab[0]), 'below'),
                      (dict(below=(lab[0], state.int())), 'dtype'), (dict(above=(lab[0, :3], state)), 'expected'),
                      (dict(above=(lab[0].int(), state)), 'dtype')):
        with pytest.raises(ValueError, match=match):
            _hip.label_grow(lab, seeds, **kw)


# ------------------------------------------------------------------------------------------------------ serpentines
@pytest.mark.parametrize('which', ['flat', 'tall'])
def test_a_serpentine_undivided_and_in_blocks(which):
    lab, seeds, want = _want(which, serpentine_flat if which == 'flat' else serpentine_tall)
    D, H, W = lab.shape
    info = {}
    got, g = _grow(lab, seeds, info=info)
    np.testing.assert_array_equal(got, want)
    assert info['rounds'] == 1 and 1 < info['sweeps_needed'] <= info['sweeps'] and info['active_tiles'] > 0
    if which == 'flat':
        assert int((got == 1).sum()) == 102 and int((got == 2).sum()) == 102
    for per in (1, 2, 5):
        info = {}
        got, _ = _grow(lab, seeds, block_voxels=per * H * W + 3, info=info)
        np.testing.assert_array_equal(got, want, err_msg=f'blocks of {per}')
        assert info['blocks'] == -(-D // per)
        if which == 'tall' or per == 1:                         # the flat one lies in slice 1: one block holds it all
            assert info['rounds'] > 1
    from empanada_amd import _hip
    with pytest.raises(RuntimeError, match='max_sweeps'):
        _hip.label_grow(_dev(lab), _dev(seeds), max_sweeps=1)


# ------------------------------------------------------------------------------------------------------ halos
def _halved(lab, seeds, z):
    """the volume cut at z into two label_grow calls that exchange end slices until nothing changes"""
    from empanada_amd import _hip
    a = _hip.label_grow(_dev(lab[:z]), _dev(seeds[:z]))
    b = _hip.label_grow(_dev(lab[z:]), _dev(seeds[z:]))
    rounds = 0
    while True:
        rounds += 1
        fell = a.resume(above=b.ends()[0])
        fell = b.resume(below=a.ends()[1]) or fell
        if not fell:
            return np.concatenate([_np(a.owners()), _np(b.owners())]), rounds


def test_every_z_cut_with_its_halo_slices_equals_the_whole():
    def make():
        rng = np.random.default_rng(5)
        lab = np.zeros((11, 10, 70), np.uint32)
        ball(lab, (5, 5, 20), 5, 3)
        ball(lab, (5, 4, 50), 4, 3)
        lab[4:7, 4:6, 20:50] = 3
        lab[:, 8:, :] = np.where(rng.random((11, 2, 70)) < 0.7, 9, 0)
        seeds = np.where(rng.random(lab.shape) < 0.004, rng.integers(1, 9, lab.shape), 0).astype(np.uint32)
        return lab, seeds
    lab, seeds, want = _want('cut', make)
    assert len(np.unique(want)) > 4 and ((want == 0) & (lab != 0)).any()
    for z in range(1, lab.shape[0]):
        np.testing.assert_array_equal(_halved(lab, seeds, z)[0], want, err_msg=f'cut at {z}')
    lab, seeds, want = _want('tall', serpentine_tall)
    for z in (1, 8, 17):
        got, rounds = _halved(lab, seeds, z)
        np.testing.assert_array_equal(got, want, err_msg=f'cut at {z}')
        assert rounds > 2


# ------------------------------------------------------------------------------------------------------ paint
def test_paint():
    from empanada_amd import _hip
    lab, seeds = random_case((9, 9, 65), 4, density=0.01, big=True)
    seeds = np.where(seeds != 0, np.arange(seeds.size).reshape(seeds.shape) % 6 + 1, 0).astype(np.uint32)
    owner = grow_ref(lab, seeds)[0]
    assert ((owner == 0) & (lab != 0)).any() and len(np.unique(owner)) == 7
    lut = np.asarray([99, 11, 12, 2 ** 32 - 1, 14, 2 ** 31, 16], np.int64)
    want = np.where(owner != 0, lut[owner], lab).astype(np.uint32)
    dev = _dev(lab)
    g = _hip.label_grow(dev, _dev(seeds))
    fresh = g.paint(lut)
    assert fresh.dtype == torch.uint32 and fresh.data_ptr() != dev.data_ptr()
    np.testing.assert_array_equal(_np(fresh), want)
    np.testing.assert_array_equal(_np(dev), lab)
    other = torch.full(lab.shape, 5, dtype=torch.int32, device='cuda')
    assert g.paint(torch.from_numpy(lut), out=other) is other
    np.testing.assert_array_equal(other.cpu().numpy().view(np.uint32), want)
    # uint8 out: a value that does not fit is refused and nothing is written
    small = np.asarray([0, 1, 2, 3, 4, 5, 255], np.int64)
    lab8 = np.where(lab != 0, lab % 200 + 1, 0).astype(np.uint8)
    dev8 = _dev(lab8)
    g8 = _hip.label_grow(dev8, _dev(seeds))
    own8 = grow_ref(lab8, seeds)[0]
    out8 = torch.full(lab.shape, 77, dtype=torch.uint8, device='cuda')
    with pytest.raises(ValueError, match='cannot hold'):
        g8.paint(lut, out=out8)
    with pytest.raises(ValueError, match='cannot hold'):
        g8.paint(np.asarray([0, 1, 2, 3, 4, 5, 256]), out=dev8)
    with pytest.raises(ValueError, match='cannot hold'):
        g.paint(small, dtype=torch.uint8)                       # the slab's own labels do not fit
    assert (out8 == 77).all()
    np.testing.assert_array_equal(_np(dev8), lab8)
    np.testing.assert_array_equal(_np(g8.paint(small, out=out8)), np.where(own8 != 0, small[own8], lab8))
    np.testing.assert_array_equal(_np(g8.paint(small, dtype=torch.uint32)), np.where(own8 != 0, small[own8], lab8))
    # in place
    assert g8.paint(small, out=dev8) is dev8
    np.testing.assert_array_equal(_np(dev8), np.where(own8 != 0, small[own8], lab8))
    assert g.paint(lut, out=dev) is dev
    np.testing.assert_array_equal(_np(dev), want)
    # other refusals
    for kw, match in ((dict(lut=lut[:6]), 'largest seed id'), (dict(lut=lut.astype(np.float32)), 'integers'),
                      (dict(lut=lut, dtype=torch.float32), 'dtype'), (dict(lut=lut, out=other[:4]), 'expected'),
                      (dict(lut=lut, out=other, dtype=torch.uint8), 'together'),
                      (dict(lut=lut, out=g.state.view(torch.int32)[:, :, :65]), 'contiguous'),
                      (dict(lut=-lut), 'cannot hold')):
        with pytest.raises(ValueError, match=match):
            g.paint(**kw)
    np.testing.assert_array_equal(_np(g.owners()), owner)


# ------------------------------------------------------------------------------------------------------ separate_volume
def _three_balls(dtype=np.uint32):
    vol = np.zeros((15, 15, 52), dtype)
    for x in (8, 25, 42):
        ball(vol, (7, 7, x), 6, 9)
    vol[6:9, 6:9, 8:43] = 9
    return vol


def _two_dumbbells(dtype=np.uint32):
    """different labels, lying side by side along y and touching: the first one bites into the second"""
    a = dumbbell(dtype, label=5)
    b = dumbbell(dtype, label=200)
    vol = np.zeros((17, 28, 41), dtype)
    vol[:, 11:][b != 0] = 200
    vol[:, :17][a != 0] = 5
    return vol


def _crumb(dtype=np.uint32):
    """a dumbbell and, under the same label, a far thin sliver that the erosion removes: no core of its own"""
    vol = np.concatenate([dumbbell(dtype), np.zeros((4, 17, 41), dtype)])
    vol[19, 2:15, 3:30] = 5
    return vol


CASES = {'dumbbell r2=4': (dumbbell, 4, 1, (1, 1, 1)), 'dumbbell r2=9': (dumbbell, 9, 1, (1, 1, 1)),
         'dumbbell u8': (lambda: dumbbell(np.uint8), 9, 1, (1, 1, 1)),
         'three balls': (_three_balls, 9, 1, (1, 1, 1)), 'two dumbbells': (_two_dumbbells, 9, 1, (1, 1, 1)),
         'small second core': (lambda: dumbbell(second_r=4), 9, 30, (1, 1, 1)),
         'small second core counts': (lambda: dumbbell(second_r=4), 9, 1, (1, 1, 1)),
         'crumb': (_crumb, 9, 1, (1, 1, 1)), 'sampling': (lambda: dumbbell(r=7, neck=3), 16, 1, (3, 1, 1))}


def _case(name):
    if ('sep', name) not in _CACHE:
        make, r2, min_core, sampling = CASES[name]
        vol = make()
        _CACHE['sep', name] = (vol, r2, min_core, sampling) + separate_ref(vol, r2, min_core, sampling)[:2]
    return _CACHE['sep', name]


@pytest.mark.parametrize('name', list(CASES))
def test_separate_volume_equals_the_checker(name):
    vol, r2, min_core, sampling, want, stats = _case(name)
    dev = _dev(vol)
    out, got = SP.separate_volume(dev, vol.shape, r2, min_core, sampling)
    assert out is dev
    np.testing.assert_array_equal(_np(dev), want)
    sweeps = got.pop('sweeps')
    assert got == stats
    changes = name not in ('dumbbell r2=4', 'small second core')
    assert (stats['pieces_added'] > 0) == changes and (sweeps > 0) == changes and (want != vol).any() == changes
    if name == 'three balls':
        assert stats['pieces_added'] == 2
    if name == 'two dumbbells':
        assert stats['objects_separated'] == 2 and sorted(np.unique(want).tolist()) == [0, 5, 200, 201, 202]
    if name == 'crumb':
        assert (want[19][vol[19] != 0] == 5).all() and (want[19] == vol[19]).all()


def test_separate_volume_refuses_labels_that_a_uint8_slab_cannot_hold():
    vol = dumbbell(np.uint8, label=255)
    dev = _dev(vol)
    with pytest.raises(ValueError, match='would pass 255'):
        SP.separate_volume(dev, vol.shape, 9)
    np.testing.assert_array_equal(_np(dev), vol)
    vol = dumbbell(np.uint32, label=2 ** 32 - 1)
    dev = _dev(vol)
    with pytest.raises(ValueError, match='would pass'):
        SP.separate_volume(dev, vol.shape, 9)
    np.testing.assert_array_equal(_np(dev), vol)
    vol = dumbbell(np.uint32, label=2 ** 32 - 2)
    want = separate_ref(vol, 9)[0]
    assert want.max() == 2 ** 32 - 1
    np.testing.assert_array_equal(_np(SP.separate_volume(_dev(vol), vol.shape, 9)[0]), want)


def test_without_a_candidate_no_growth_is_launched(monkeypatch):
    from empanada_amd import _hip
    monkeypatch.setattr(_hip, 'label_grow', lambda *a, **k: pytest.fail("label_grow was called"))
    vol = dumbbell()
    dev = _dev(vol)
    ptr = dev.data_ptr()
    out, stats = SP.separate_volume(dev, vol.shape, 4)
    assert out is dev and out.data_ptr() == ptr and stats['sweeps'] == 0 and stats['pieces_added'] == 0
    np.testing.assert_array_equal(_np(dev), vol)
    zero = _dev(np.zeros((3, 4, 5), np.uint32))
    assert SP.separate_volume(zero, (3, 4, 5), 1)[1]['objects_in'] == 0


# ------------------------------------------------------------------------------------------------------ ranks
RANK_BOUNDS = [(0, 8, 17), (0, 3, 17), (0, 16, 17), (0, 0, 17), (0, 17, 17)]
TALL_BOUNDS = [(0, 16, 33), (0, 5, 33), (0, 33, 33)]


def _rank(rank, world, port, q, infer):
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        out = []
        vol = dumbbell()
        for b in RANK_BOUNDS:
            new, stats = SP.separate_volume(_dev(vol[b[rank]:b[rank + 1]]), vol.shape, 9, group=dist.group.WORLD,
                                            z_base=b[rank])
            out.append((_np(new), stats))
        lab, seeds = serpentine_tall()
        for b in TALL_BOUNDS:
            g = SP.grow_volume(_dev(lab[b[rank]:b[rank + 1]]), _dev(seeds[b[rank]:b[rank + 1]]), dist.group.WORLD)
            out.append((_np(g.owners()), None))
        res = None
        if infer is not None:
            eng, em = _engine(), SY.em_volume(SHAPE, seed=3)
            r = _run(eng, em, None, axes=ORTHO, group=dist.group.WORLD, separate=infer, measure=True)
            res = (tuple(r['z_range']), _np(r['volumes'][1]), r['separated'], dict(r['instances']), r['objects'])
        q.put((rank, out, res))
    finally:
        dist.destroy_process_group()


def test_two_ranks(case):
    """every rank's slab is its part of the single-rank result and the stats are the same on both ranks; one split leaves
    a rank empty.  Also infer_volume(separate=) over two ranks."""
    import torch.multiprocessing as mp
    eng, em, vols, sets, counts = case(ORTHO)
    separate = _pick(vols)
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank, args=(r, 2, port, q, separate)) for r in range(2)]
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
    vol = dumbbell()
    want, stats, _ = separate_ref(vol, 9)
    i = 0
    for b in RANK_BOUNDS:
        for r in (0, 1):
            np.testing.assert_array_equal(got[r][0][i][0], want[b[r]:b[r + 1]], err_msg=f'{b} rank {r}')
            assert {k: v for k, v in got[r][0][i][1].items() if k != 'sweeps'} == stats
        assert got[0][0][i][1] == got[1][0][i][1] and got[0][0][i][1]['sweeps'] > 0
        i += 1
    lab, seeds, owner = _want('tall', serpentine_tall)
    for b in TALL_BOUNDS:
        for r in (0, 1):
            np.testing.assert_array_equal(got[r][0][i][0], owner[b[r]:b[r + 1]], err_msg=f'{b} rank {r}')
        i += 1
    want, stats = _wanted(vols, separate)[:2]
    assert got[0][1][0] == (0, 20) and got[1][1][0] == (20, 40)
    np.testing.assert_array_equal(np.concatenate([got[0][1][1], got[1][1][1]]), want)
    for r in (0, 1):
        assert {k: v for k, v in got[r][1][2][1].items() if k != 'sweeps'} == stats
        assert got[r][1][3] == {**counts, 1: counts[1] + stats['pieces_added']}
        np.testing.assert_array_equal(got[r][1][4][1], measure_ref(want))
    assert got[0][1][2] == got[1][1][2]


# ------------------------------------------------------------------------------------------------------ infer_volume
def _wanted(vols, separate, before=None):
    """(volume, stats, objects) that separate_ref makes of the plain call's thing volume -- `before`: a morph first"""
    key = ('infer', id(vols[1]), separate, before)
    if key not in _CACHE:
        r2, min_core, sampling = SP.check(separate)
        start = vols[1] if before is None else morph_ref(vols[1], before)
        want, stats, _ = separate_ref(start, r2, min_core, sampling)
        _CACHE[key] = (want, stats, len(np.unique(want[want != 0])))
    return _CACHE[key]


def _pick(vols, before=None):
    """the first of a few radii at which the checker separates something in the plain call's thing volume"""
    for r in (2, 1.5, 1, 3, 4, 5):
        if _wanted(vols, (r, 1), before)[1]['pieces_added'] > 0:
            return (r, 1)
    pytest.fail("the synthetic volume holds no touching objects at any of the radii tried")


def _assert_separated(res, vols, counts, separate):
    want, stats, n = _wanted(vols, separate)
    changes = stats['pieces_added'] > 0
    np.testing.assert_array_equal(_np(res['volumes'][1]), want)
    np.testing.assert_array_equal(_np(res['volumes'][2]), vols[2])          # a stuff class stays as it is
    assert list(res['separated']) == [1]
    got = dict(res['separated'][1])
    assert (got.pop('sweeps') > 0) == changes and got == stats
    assert dict(res['instances']) == {**counts, 1: counts[1] + stats['pieces_added']}
    assert n == len(np.unique(vols[1][vols[1] != 0])) + stats['pieces_added']
    if 'objects' in res:
        for c in (1, 2):
            np.testing.assert_array_equal(res['objects'][c], measure_ref(_np(res['volumes'][c])))
    for c, ds in res['datasets'].items():
        if ds is not None:
            np.testing.assert_array_equal(np.asarray(ds[...]), _np(res['volumes'][c]))


THICK = (1.5, 3, (2, 1, 1))


@pytest.mark.parametrize('which', ['picked', 'thick'])
def test_infer_volume_plain_path_with_a_store(tmp_path, case, which):
    eng, vol, vols, sets, counts = case(ORTHO)
    separate = _pick(vols) if which == 'picked' else THICK
    res = _run(eng, vol, tmp_path / 's.zarr', axes=ORTHO, separate=separate, measure=True, compressor='zlib')
    _assert_separated(res, vols, counts, separate)
    assert 'split' not in res and 'filled' not in res and 'morph' not in res
    # off: the parent's keys and bytes
    off = _run(eng, vol, tmp_path / 'n.zarr', axes=ORTHO, separate=None)
    assert sorted(off) == ['datasets', 'instances', 'volumes', 'z_range'] and dict(off['instances']) == counts
    for c in (1, 2):
        assert _np(off['volumes'][c]).tobytes() == vols[c].tobytes()


def test_infer_volume_order_morph_separate_split_fill(case):
    eng, vol, vols, sets, counts = case(ORTHO)
    morph = ('open', 1)
    separate = _pick(vols, before=morph)
    sep, stats, _ = _wanted(vols, separate, before=morph)
    # the smallest piece that the separation made: a min_size just above it makes split_objects erase that piece
    made = np.unique(sep[sep != morph_ref(vols[1], morph)])
    sizes = {int(l): int((sep == l).sum()) for l in made}
    smallest = min(sizes.values())
    if smallest < KW['min_size']:
        kw, base = {}, vols[1]
    else:
        kw = dict(min_size=smallest + 1)
        base = _np(_run(eng, vol, None, axes=ORTHO, **kw)['volumes'][1])
    min_size = kw.get('min_size', KW['min_size'])
    r2, min_core, sampling = SP.check(separate)
    morphed = morph_ref(base, morph)
    sep, stats, _ = separate_ref(morphed, r2, min_core, sampling)
    new_sizes = [int((sep == l).sum()) for l in np.unique(sep[sep != morphed])]
    assert new_sizes and min(new_sizes) < min_size, "a piece that separate made should fall below min_size"
    want, split, _ = split_ref(sep, 6, min_size=min_size, min_span=KW['min_span'])
    assert split['pieces_removed'] > 0
    want = fill_ref(want)[0]
    res = _run(eng, vol, None, axes=ORTHO, morph=morph, separate=separate, split_objects=6, fill_holes=True, measure=True,
               **kw)
    np.testing.assert_array_equal(_np(res['volumes'][1]), want)
    assert {k: v for k, v in res['separated'][1].items() if k != 'sweeps'} == stats
    assert res['split'][1] == split and res['instances'][1] == split['objects_out'] and 'filled' in res and 'morph' in res
    np.testing.assert_array_equal(res['objects'][1], measure_ref(want))
    # split alone, without the separation, keeps the voxels of that piece: the order is what erased them
    alone = split_ref(morphed, 6, min_size=min_size, min_span=KW['min_span'])[0]
    assert int((alone != 0).sum()) > int((split_ref(sep, 6, min_size=min_size, min_span=KW['min_span'])[0] != 0).sum())


def test_infer_volume_stack_mode_and_windows(tmp_path, case):
    eng, vol, vols, _, counts = case(('xy',))
    separate = _pick(vols)
    _assert_separated(_run(eng, vol, None, axes=('xy',), separate=separate, measure=True), vols, counts, separate)
    kw = dict(axes=('xy',), batch_pixels=4 * 96 * 96, window_slices=8)      # 4 slices per model call, windows of 8
    win = _run(eng, vol, tmp_path / 'w.zarr', separate=separate, **kw)
    assert win['windows']['xy'] > 1
    _assert_separated(win, vols, counts, separate)


def test_infer_volume_pipeline(tmp_path, case):
    from empanada_amd.inference.pipeline import VolumePipeline
    eng, vol, vols, sets, counts = case(ORTHO)
    pipe = VolumePipeline(eng, tune=False, graph=True, overlap=True, batch_pixels=1 << 22)
    try:
        for i, separate in enumerate((_pick(vols), THICK)):
            res = _run(eng, vol, tmp_path / f'{i}.zarr', axes=ORTHO, separate=separate, measure=True, pipeline=pipe)
            _assert_separated(res, vols, counts, separate)
        off = _run(eng, vol, None, axes=ORTHO, pipeline=pipe)
        assert 'separated' not in off and dict(off['instances']) == counts
        assert _np(off['volumes'][1]).tobytes() == vols[1].tobytes()
    finally:
        pipe.close()


def test_infer_volume_rejects_a_bad_separate_before_any_work(case):
    eng, vol, _, _, _ = case(ORTHO)
    before = torch.cuda.memory_allocated()
    for bad in (0, (2, 0), (2, 1, (0, 1, 1)), 'two', (2, 1, (1, 1, 1), 5)):
        with pytest.raises(ValueError, match='separate'):
            _run(eng, vol, None, axes=ORTHO, separate=bad)
    assert torch.cuda.memory_allocated() == before
