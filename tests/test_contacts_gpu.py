"""GPU: contact sites between labelled objects -- emp_label_contacts_* (csrc/emp_label_contacts.hip) through
_hip.label_contacts, contacts.volume_contacts and infer_volume(..., contacts=).  The checker is tests/contacts_ref.py's
`contact_table`, a numpy restatement of the definition in include/emp_hip.h (E9) that shares nothing with the kernel and
that tests/test_contacts_host.py checks against scipy's edt.  Every column is an integer and is compared bit for bit.
The engine and volume of the infer_volume cases are those of tests/test_pyramid_gpu.py."""
import itertools
import os
import queue
import sys
import time

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contacts_ref as ref  # noqa: E402

from empanada_amd import synthetic as SY  # noqa: E402
from test_contacts_host import assert_hand_case, hand_cases  # noqa: E402
from test_pyramid_gpu import KW, NAMES, ORTHO, SHAPE, _dev, _engine, _free_port, _np, _run, case  # noqa: E402,F401 (fixture)

pytestmark = pytest.mark.gpu

N_COL = 10
SHAPES = [(1, 1, 1), (3, 5, 7), (9, 10, 70), (17, 9, 130), (8, 8, 64), (16, 16, 128)]
RADII = [(1, (1, 1, 1)), (2, (1, 1, 1)), (3, (1, 1, 1)), (9, (1, 1, 1)), (24, (1, 1, 1)), (9, (3, 1, 1)), (16, (3, 1, 1)),
         (9, (2, 1, 3)), (16, (2, 1, 3))]
BIG = (0x80000000, 0xFFFFFFFF)
_CACHE = {}


def _contacts(A, B=None, r2=1, sampling=(1, 1, 1), below=None, above=None, **kw):
    from empanada_amd import _hip
    dev = lambda t: None if t is None else _dev(t)
    got = _hip.label_contacts(dev(A), dev(B), r2, sampling, below=dev(below), above=dev(above), **kw)
    assert got.dtype == torch.int64 and got.is_cuda and got.dim() == 2 and got.shape[1] == N_COL
    return got.cpu().numpy()


def _operands(shape, density, mode, seed):
    """(A, B or None) of a dtype mode: ids of a few dozen, in 32 bits with 0x80000000 and 0xFFFFFFFF among them"""
    u32 = lambda s: ref.random_labels(shape, density, 30, s, np.uint32, special=BIG)
    u8 = lambda s: ref.random_labels(shape, density, 40, s, np.uint8)
    if mode == 'u8':
        return u8(seed), None
    if mode == 'u32':
        return u32(seed), None
    if mode == 'i32':
        return u32(seed).view(np.int32), None
    if mode == 'u32|u8':
        return u32(seed), u8(seed + 1)
    if mode == 'u8|i32':
        return u8(seed), u32(seed + 1).view(np.int32)
    return u32(seed), u32(seed + 1)


MODES = ['u8', 'u32', 'i32', 'u32|u8', 'u8|i32', 'u32|u32']


# ------------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize('density', [0.05, 0.5])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_kernel_equals_the_restatement(shape, density):
    # every dtype mode meets every radius: half of the pairs at this density, the other half at the other one
    for seed, ((i, mode), (j, (r2, sampling))) in enumerate(itertools.product(enumerate(MODES), enumerate(RADII))):
        if (i + j) % 2 != (density > 0.1):
            continue
        A, B = _operands(shape, density, mode, seed)
        want = ref.contact_table(A, B, r2, sampling, z_base=seed % 3)
        got = _contacts(A, B, r2, sampling, z_base=seed % 3)
        np.testing.assert_array_equal(got, want, err_msg=f'{mode} {shape} r2 {r2} {sampling}')


def test_ids_above_2_31_sort_as_unsigned():
    A, _ = _operands((9, 10, 70), 0.5, 'i32', 5)
    got = _contacts(A, None, 3)
    assert (got[:, 0] >= 2 ** 31).any() and (got[:, 1] == 0xFFFFFFFF).any()
    keys = [(a << 32) | b for a, b in got[:, :2].tolist()]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)


@pytest.mark.parametrize('offset', [1, 3])
def test_unaligned_slab(offset):
    """the slabs and the halo stacks are views at an element offset: the kernels read element by element, same table"""
    from empanada_amd import _hip
    for mode in ('u8', 'u32', 'u32|u8'):
        tall_a, tall_b = _operands((13, 9, 70), 0.3, mode, 7)
        r2 = 5
        pieces = {}
        for name, arr in (('a', tall_a), ('b', tall_b)):
            if arr is None:
                continue
            tdt = torch.uint8 if arr.dtype == np.uint8 else torch.int32
            flat = torch.zeros((arr.size + 8,), dtype=tdt, device='cuda')
            flat[offset:offset + arr.size] = _dev(arr).view(tdt).ravel()
            v = flat[offset:offset + arr.size].view(arr.shape)
            pieces[name] = v.view(torch.uint32) if arr.dtype == np.uint32 else v
        a = pieces['a']
        b = pieces.get('b')
        src = a if b is None else b
        assert a.data_ptr() % (4 * a.element_size()) != 0
        got = _hip.label_contacts(a[2:11], None if b is None else b[2:11], r2, below=src[0:2], above=src[11:13], z_base=2)
        np.testing.assert_array_equal(got.cpu().numpy(), ref.restrict_to_slab(tall_a, tall_b, 2, 11, r2), err_msg=mode)


def test_cases_counted_by_hand():
    for name, A, B, r2, sampling, want in hand_cases():
        assert_hand_case(name, _contacts(A, B, r2, sampling), want)
    t = _contacts(ref.distinct_block(), None, 3)
    assert len(t) == 316 and int((t[:, 0] == 14).sum()) == 26 and (t[:, 2] == 1).all()
    t = _contacts(ref.two_cubes(0), None, 1, z_base=10)
    assert t[0, 4:7].tolist() == [4 * 10 + 6, 6, 8]


@pytest.mark.parametrize('r2', [3, 9])
def test_crowded_every_voxel_its_own_label(r2):
    """up to 26 and 118 partners per voxel: far more than the register cache of the walk holds, so a pair is lost or
    emitted twice unless the first occurrence is decided exactly"""
    from empanada_amd import _hip
    vol = ref.crowded((5, 5, 70))
    want = ref.contact_table(vol, None, r2)
    assert (want[:, 2] == 1).all() and np.bincount(want[:, 0]).max() == (26 if r2 == 3 else 118)
    info = {}
    got = _hip.label_contacts(_dev(vol), None, r2, info=info).cpu().numpy()
    np.testing.assert_array_equal(got, want)
    assert info['records'] == len(want) and info['tiles'] == 2 and info['blocks'] == 1
    # against a copy with other ids: every voxel also meets the label at its own place
    other = (vol + np.uint32(100000)).astype(np.uint32)
    np.testing.assert_array_equal(_contacts(vol, other, r2), ref.contact_table(vol, other, r2))


def test_objects_across_tile_borders():
    shape = (20, 20, 140)
    for axis, at in ((0, 8), (1, 8), (2, 64), (0, 16), (2, 128)):
        vol = ref.slabs_on_border(axis, at, shape)
        t = _contacts(vol, None, 1)
        np.testing.assert_array_equal(t, ref.contact_table(vol, None, 1))
        face = vol.size // shape[axis]
        assert t[:, :4].tolist() == [[1, 2, face, 1], [2, 1, face, 1]] and t[0, 7 + axis] == face
        far = ref.slabs_on_border(axis, at, shape, gap=3)                   # three empty voxels: distance 4 across the border
        assert _contacts(far, None, 15).shape == (0, N_COL)
        t = _contacts(far, None, 16)
        np.testing.assert_array_equal(t, ref.contact_table(far, None, 16))
        assert t[:, :4].tolist() == [[1, 2, face, 16], [2, 1, face, 16]] and (t[:, 7:] == 0).all()
        wide = ref.slabs_on_border(axis, at, shape, gap=4)                  # a gap of four: distance 5, out of reach
        for r2 in (16, 24):
            assert ref.contact_table(wide, None, r2).shape == (0, N_COL) and _contacts(wide, None, r2).shape == (0, N_COL)
        info = {}
        from empanada_amd import _hip
        _hip.label_contacts(_dev(far), None, 16, info=info)
        assert 0 < info['tiles'] < 27 and info['records'] == 2 * face


# ------------------------------------------------------------------------------------------------------ blocks and halos
def _tall():
    """(25, 9, 130) labels and, per radius, the table of the whole volume: computed once, never modified"""
    if 'tall' not in _CACHE:
        vol = ref.random_labels((25, 9, 130), 0.3, 30, 21, np.uint32, special=BIG)
        other = ref.random_labels((25, 9, 130), 0.3, 40, 22, np.uint8)
        _CACHE['tall'] = (vol, other)
    return _CACHE['tall']


@pytest.mark.parametrize('r2', [1, 16])
def test_blocks_equal_the_whole(r2):
    from empanada_amd import _hip
    vol, other = _tall()
    A, B = vol[4:21], other[4:21]                                           # (17, 9, 130)
    per = 9 * 130
    for Bv in (None, B):
        want = ref.contact_table(A, Bv, r2, z_base=4)
        for block, n_blocks in ((9 * per, 2), (6 * per, 3), (per, 17)):
            info = {}
            got = _hip.label_contacts(_dev(A), None if Bv is None else _dev(Bv), r2, z_base=4, block_voxels=block, info=info)
            assert info['blocks'] == n_blocks
            np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=f'{n_blocks} blocks')
        assert torch.equal(got, _hip.label_contacts(_dev(A), None if Bv is None else _dev(Bv), r2, z_base=4, block_voxels=per))
    with pytest.raises(ValueError, match='single slice'):
        _hip.label_contacts(_dev(A), block_voxels=per - 1)


@pytest.mark.parametrize('r2', [1, 16])
def test_halo_stacks_cut_from_a_taller_volume(r2):
    """below / above stand for B outside the slab: the table equals the taller volume's restricted to the slab's voxels;
    at the volume's ends the stacks are shorter than the halo, or absent"""
    vol, other = _tall()
    h = 1 if r2 == 1 else 4
    for z0, z1 in ((4, 21), (0, 9), (2, 12), (16, 25), (20, 23)):
        for tall_b in (None, other):
            src = vol if tall_b is None else tall_b
            lo, hi = src[max(z0 - h, 0):z0], src[z1:z1 + h]
            got = _contacts(vol[z0:z1], None if tall_b is None else tall_b[z0:z1], r2, below=lo if len(lo) else None,
                            above=hi if len(hi) else None, z_base=z0)
            np.testing.assert_array_equal(got, ref.restrict_to_slab(vol, tall_b, z0, z1, r2), err_msg=f'{z0}:{z1}')
    blind = _contacts(vol[4:21], None, r2, z_base=4)                        # the data tell a halo from none
    assert (blind.shape != ref.restrict_to_slab(vol, None, 4, 21, r2).shape
            or (blind != ref.restrict_to_slab(vol, None, 4, 21, r2)).any())


def test_two_runs_are_bit_identical():
    from empanada_amd import _hip
    vol, other = _tall()
    a, b = _dev(vol), _dev(other)
    for args in ((a, None, 24), (a, b, 9)):
        assert torch.equal(_hip.label_contacts(*args), _hip.label_contacts(*args))


def test_empty_and_degenerate_inputs():
    from empanada_amd import _hip
    for shape in ((0, 4, 4), (3, 0, 4), (3, 4, 0)):
        for tdt in (torch.uint8, torch.int32):
            got = _hip.label_contacts(torch.zeros(shape, dtype=tdt, device='cuda'))
            assert tuple(got.shape) == (0, N_COL) and got.dtype == torch.int64 and got.is_cuda
    zero = np.zeros((9, 10, 70), np.uint32)
    one = np.full((9, 10, 70), 7, np.uint32)
    info = {}
    assert _hip.label_contacts(_dev(zero), None, 24, info=info).shape == (0, N_COL)
    assert info == dict(blocks=1, tiles=0, records=0, work_bytes=info['work_bytes'])
    assert _contacts(one, None, 24).shape == (0, N_COL)                     # one label: no partner
    assert _contacts(one, zero, 24).shape == (0, N_COL) and _contacts(zero, one, 24).shape == (0, N_COL)
    t = _contacts(one, one.astype(np.uint8), 1)                             # two volumes: the same id is a partner
    assert t.tolist() == [[7, 7, 6300, 0, 6300 * 4, 6300 * 9 // 2, 6300 * 69 // 2,
                           2 * 8 * 700, 2 * 9 * 630, 2 * 69 * 90]]


def test_symmetry_of_the_same_volume_case():
    vol, _ = _tall()
    t = _contacts(vol, None, 8)
    rows = {(a, b): r for a, b, *r in t.tolist()}
    assert len(rows) > 100
    for (a, b), r in rows.items():
        back = rows[(b, a)]
        assert r[1] == back[1] and r[5:] == back[5:]


def test_volume_contacts(tmp_path):
    from empanada_amd import contacts as C
    from empanada_amd.zarr_utils import ZarrV2Group
    vol, other = _tall()
    g = ZarrV2Group(str(tmp_path / 'gt.zarr'))
    ds = g.create_dataset('lab', shape=vol.shape, dtype=np.uint32, chunks=(1, None, None))
    ds.write_slab(0, vol)
    ds8 = g.create_dataset('other', shape=other.shape, dtype=np.uint8, chunks=(1, None, None))
    ds8.write_slab(0, other)
    for r, sampling in ((1, (1, 1, 1)), (3, (1, 1, 1)), (3, (3, 1, 1))):
        r2 = r * r
        want = ref.contact_table(vol, None, r2, sampling)
        want2 = ref.contact_table(vol, other, r2, sampling)
        for slab_rows in (1, 5, None):
            for source in (vol, ds, _dev(vol)):
                got = C.volume_contacts(source, r=r, sampling=sampling, slab_rows=slab_rows)
                assert isinstance(got, np.ndarray) and got.dtype == np.int64
                np.testing.assert_array_equal(got, want, err_msg=f'{type(source).__name__} slab_rows {slab_rows}')
            for sa, sb in ((vol, other), (ds, ds8), (vol.astype(np.int64), _dev(other))):
                got = C.volume_contacts(sa, sb, r=r, sampling=sampling, slab_rows=slab_rows)
                np.testing.assert_array_equal(got, want2, err_msg=f'two volumes, slab_rows {slab_rows}')
    assert C.volume_contacts(np.zeros((3, 4, 5), np.uint8), r=2).shape == (0, N_COL)
    for bad in (0, True, 2.0):
        with pytest.raises(ValueError, match='slab_rows'):
            C.volume_contacts(vol, r=1, slab_rows=bad)
    with pytest.raises(ValueError):
        C.volume_contacts(vol, other[1:], r=1)
    with pytest.raises(ValueError):
        C.volume_contacts(vol, r=5)


# ------------------------------------------------------------------------------------------------------ infer_volume
PLAIN_KEYS = ['datasets', 'instances', 'volumes', 'z_range']
PAIRS = [(1, 1), (1, 2), (2, 1)]
R2 = 6


def _assert_contacts(res, vols=None, pairs=PAIRS, r2=R2, sampling=(1, 1, 1)):
    """res['contacts'][(ca, cb)] is the checker's table of the (gathered) volumes"""
    vols = {c: _np(v) for c, v in res['volumes'].items()} if vols is None else vols
    assert sorted(res['contacts']) == sorted(pairs) and res['contact_params'] == {'r2': r2, 'sampling': sampling}
    for ca, cb in pairs:
        table = res['contacts'][(ca, cb)]
        assert isinstance(table, np.ndarray) and table.dtype == np.int64
        want = ref.contact_table(vols[ca], None if ca == cb else vols[cb], r2, sampling)
        np.testing.assert_array_equal(table, want, err_msg=f'classes {ca}, {cb}')


def test_infer_volume_plain_path_with_a_store(tmp_path, case):
    from empanada_amd import contacts as C
    from empanada_amd.zarr_utils import ZarrV2Group
    eng, vol, vols, sets, counts = case(ORTHO)
    path = tmp_path / 'c.zarr'
    res = _run(eng, vol, path, axes=ORTHO, contacts=2.5, measure=True)
    _assert_contacts(res)
    assert dict(res['instances']) == counts
    assert len(res['contacts'][(1, 2)]) > 0 and len(res['contacts'][(2, 1)]) == len(res['contacts'][(1, 2)])
    assert (res['contacts'][(1, 2)][:, 1] == 1).all() and (res['contacts'][(2, 1)][:, 0] == 1).all()
    g = ZarrV2Group(str(path), mode='r')
    names = {(1, 1): 'mito_mito_contacts', (1, 2): 'mito_er_contacts', (2, 1): 'er_mito_contacts'}
    for c in (1, 2):
        np.testing.assert_array_equal(_np(res['volumes'][c]), vols[c])
        np.testing.assert_array_equal(np.asarray(res['datasets'][c]), sets[c])
    for p in PAIRS:
        ds = res['contact_datasets'][p]
        assert ds.path == os.path.join(str(path), names[p]) and names[p] in g
        assert ds.dtype == np.int64 and ds.shape == res['contacts'][p].shape
        np.testing.assert_array_equal(np.asarray(g[names[p]]).reshape(-1, N_COL), res['contacts'][p])
    attrs = g.attrs
    assert attrs['contacts'] == {'columns': list(C.COLUMNS), 'r2': R2, 'sampling': [1, 1, 1],
                                 'pairs': [[1, 1], [1, 2], [2, 1]]}
    assert sorted(attrs) == ['contacts', 'objects']                         # what was there survives
    # contacts=None: the parent's keys and the parent's datasets, nothing else
    plain = _run(eng, vol, tmp_path / 'n.zarr', axes=ORTHO)
    assert sorted(plain) == PLAIN_KEYS
    assert sorted(os.listdir(str(tmp_path / 'n.zarr'))) == ['.zgroup', 'er_pred', 'mito_pred']
    # without a store, with a sampling and chosen pairs
    bare = _run(eng, vol, None, axes=ORTHO, contacts=(3, (3, 1, 1), [(2, 1)]))
    _assert_contacts(bare, pairs=[(2, 1)], r2=9, sampling=(3, 1, 1))
    assert sorted(bare) == sorted(PLAIN_KEYS + ['contacts', 'contact_params'])
    with pytest.raises(ValueError, match='class 3'):
        _run(eng, vol, None, axes=ORTHO, contacts=(1, (1, 1, 1), [(1, 3)]))
    with pytest.raises(ValueError, match='more than 4'):
        _run(eng, vol, None, axes=ORTHO, contacts=5)


def test_infer_volume_stack_mode_and_windows(tmp_path, case):
    eng, vol, vols, _, counts = case(('xy',))
    res = _run(eng, vol, None, axes=('xy',), contacts=2.5)
    _assert_contacts(res)
    assert dict(res['instances']) == counts
    np.testing.assert_array_equal(_np(res['volumes'][1]), vols[1])
    kw = dict(axes=('xy',), batch_pixels=4 * 96 * 96, window_slices=8)      # 4 slices per model call, windows of 8
    win = _run(eng, vol, tmp_path / 'w.zarr', contacts=2.5, **kw)
    assert win['windows']['xy'] > 1
    _assert_contacts(win)
    np.testing.assert_array_equal(np.asarray(win['contact_datasets'][(1, 2)]).reshape(-1, N_COL), win['contacts'][(1, 2)])
    assert sorted(_run(eng, vol, None, **kw)) == sorted(PLAIN_KEYS + ['windows', 'head_bytes'])


def test_infer_volume_pipeline(tmp_path, case):
    from empanada_amd.inference.pipeline import VolumePipeline
    eng, vol, vols, sets, counts = case(ORTHO)
    pipe = VolumePipeline(eng, tune=False, graph=True, overlap=True, batch_pixels=1 << 22)
    try:
        res = _run(eng, vol, tmp_path / 'a.zarr', axes=ORTHO, contacts=2.5, pipeline=pipe)
        _assert_contacts(res)
        assert dict(res['instances']) == counts
        for c in (1, 2):
            np.testing.assert_array_equal(_np(res['volumes'][c]), vols[c])
        for p in PAIRS:
            np.testing.assert_array_equal(np.asarray(res['contact_datasets'][p]).reshape(-1, N_COL), res['contacts'][p])
        plain = _run(eng, vol, tmp_path / 'b.zarr', axes=ORTHO, pipeline=pipe)
        assert sorted(plain) == sorted(PLAIN_KEYS + ['pipeline'])
        assert sorted(os.listdir(str(tmp_path / 'b.zarr'))) == ['.zgroup', 'er_pred', 'mito_pred']
    finally:
        pipe.close()


def test_a_class_without_objects(tmp_path):
    """the step infer_volume applies to its result, on volumes of which one is empty: its pairs have (0, 10) tables, which
    the store holds as zero-row arrays; a store that cannot is recorded as None"""
    from empanada_amd.inference import driver
    from empanada_amd.zarr_utils import ZarrV2Group
    full = np.zeros((4, 6, 9), np.uint8)
    full[1:3, 2:5, 3:8] = 1
    things = np.zeros((4, 6, 9), np.uint32)
    things[1:3, 0:2, 3:5] = 1001
    things[0, 2:4, 4:6] = 1002                                              # sqrt(2) from 1001
    vols = {1: torch.zeros((4, 6, 9), dtype=torch.int32, device='cuda').view(torch.uint32), 2: _dev(full), 3: _dev(things)}
    pairs = [(1, 1), (1, 2), (2, 1), (3, 2), (3, 3)]

    def run(out):
        return driver._contacted({'volumes': vols, 'z_range': (3, 7)}, (2, (1, 1, 1), pairs), {1: 'mito', 2: 'er', 3: 'ld'},
                                 out, None)

    res = run(ZarrV2Group(str(tmp_path / 'z.zarr')))
    for p in ((1, 1), (1, 2), (2, 1)):
        assert res['contacts'][p].shape == (0, N_COL) and res['contacts'][p].dtype == np.int64
        ds = res['contact_datasets'][p]
        assert ds is not None and ds.shape == (0, N_COL) and ds.dtype == np.int64
    np.testing.assert_array_equal(res['contacts'][(3, 2)], ref.contact_table(things, full, 2, z_base=3))
    np.testing.assert_array_equal(res['contacts'][(3, 3)], ref.contact_table(things, None, 2, z_base=3))
    assert len(res['contacts'][(3, 2)]) == 2 and len(res['contacts'][(3, 3)]) == 2
    np.testing.assert_array_equal(np.asarray(res['contact_datasets'][(3, 2)]), res['contacts'][(3, 2)])

    class NoEmpty(ZarrV2Group):
        def create_dataset(self, name, shape, **kw):
            if 0 in tuple(shape):
                raise ValueError("no zero-length axes here")
            return super().create_dataset(name, shape=shape, **kw)

    res = run(NoEmpty(str(tmp_path / 'y.zarr')))
    assert res['contact_datasets'][(1, 2)] is None and res['contact_datasets'][(3, 3)] is not None
    assert sorted(os.listdir(str(tmp_path / 'y.zarr'))) == ['.zattrs', '.zgroup', 'ld_er_contacts', 'ld_ld_contacts']


# ----------------------------------------------------------------------------------------------- two ranks over gloo
def _rank(rank, world, port, path, q):
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        eng, vol = _engine(), SY.em_volume(SHAPE, seed=3)
        res = _run(eng, vol, path, axes=ORTHO, group=dist.group.WORLD, contacts=(4, (2, 1, 1)))
        q.put((rank, tuple(res['z_range']), res['contacts'], res['contact_params'], dict(res['instances']),
               {p: np.asarray(a).reshape(-1, N_COL) for p, a in res['contact_datasets'].items()}))
    finally:
        dist.destroy_process_group()


def test_infer_volume_two_ranks(tmp_path, case):
    import torch.multiprocessing as mp
    from empanada_amd.zarr_utils import ZarrV2Group
    eng, vol, vols, sets, counts = case(ORTHO)
    want = {(ca, cb): ref.contact_table(vols[ca], None if ca == cb else vols[cb], 16, (2, 1, 1)) for ca, cb in PAIRS}
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
        assert got[r][2] == {'r2': 16, 'sampling': (2, 1, 1)} and got[r][3] == counts
        for p in PAIRS:
            np.testing.assert_array_equal(got[r][1][p], want[p], err_msg=f'rank {r} classes {p}')
            np.testing.assert_array_equal(got[r][4][p], want[p], err_msg=f'rank {r} dataset of classes {p}')
    for c in (1, 2):
        np.testing.assert_array_equal(np.asarray(g[NAMES[c]]), sets[c])
    np.testing.assert_array_equal(np.asarray(g['mito_er_contacts']).reshape(-1, N_COL), want[(1, 2)])
    assert g.attrs['contacts']['r2'] == 16 and g.attrs['contacts']['sampling'] == [2, 1, 1]
