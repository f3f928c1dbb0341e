"""CPU: the checker of the hole filling (include/emp_hip.h, E4) against cases counted by hand and against
scipy.ndimage.binary_fill_holes, the host logic of empanada_amd.holes (plan, merge_blocks) against the checker, and the
argument errors of infer_volume(fill_holes=) and _hip.label_holes, which come before any GPU work."""
import itertools

import numpy as np
import pytest
import torch
from scipy import ndimage

from empanada_amd import holes as HO

N_COL = 10
NO_LABEL = 2 ** 32
SIX = ndimage.generate_binary_structure(3, 1)
_STEPS = [(0, -1), (0, 1), (1, -1), (1, 1), (2, -1), (2, 1)]


# ------------------------------------------------------------------------------------------------------ the checker
def holes_ref(vol, below=None, above=None, z_base=0):
    """(D, H, W) unsigned labels -> the (n, 10) int64 cavity table of the definition: 6-connected components of the zero
    voxels (scipy.ndimage.label), numbered by first voxel; wall labels from the six shifts of the volume, the slices
    below / above standing for z = -1 and z = D; (2^32, 0) for a cavity that touches an x or y border"""
    vol = np.asarray(vol)
    D, H, W = vol.shape
    if vol.size == 0:
        return np.zeros((0, N_COL), np.int64)
    comp, n = ndimage.label(vol == 0, structure=SIX)
    if n == 0:
        return np.zeros((0, N_COL), np.int64)
    flat = np.arange(vol.size, dtype=np.int64).reshape(vol.shape)
    zero = comp > 0
    first = np.full(n + 1, np.iinfo(np.int64).max, np.int64)
    np.minimum.at(first, comp[zero], flat[zero])
    order = np.argsort(first[1:], kind='stable')
    rank = np.empty(n + 1, np.int64)
    rank[0] = -1
    rank[1 + order] = np.arange(n)
    k = rank[comp]                                             # -1 on labelled voxels
    t = np.zeros((n, N_COL), np.int64)
    t[:, 0] = np.bincount(k[zero], minlength=n)
    t[:, 1] = first[1:][order] + z_base * H * W
    idx = np.nonzero(zero)
    for a in range(3):
        lo = np.full(n, np.iinfo(np.int64).max, np.int64)
        hi = np.zeros(n, np.int64)
        np.minimum.at(lo, k[zero], idx[a])
        np.maximum.at(hi, k[zero], idx[a] + 1)
        t[:, 2 + a], t[:, 5 + a] = lo + (z_base if a == 0 else 0), hi + (z_base if a == 0 else 0)
    # one slice of padding on every side: the neighbour slices along z, nothing (0) elsewhere
    wide = np.zeros((D + 2, H + 2, W + 2), np.int64)
    wide[1:-1, 1:-1, 1:-1] = vol.astype(np.int64) & 0xffffffff
    if below is not None:
        wide[0, 1:-1, 1:-1] = np.asarray(below).astype(np.int64) & 0xffffffff
    if above is not None:
        wide[-1, 1:-1, 1:-1] = np.asarray(above).astype(np.int64) & 0xffffffff
    t[:, 8], t[:, 9] = NO_LABEL, 0
    for axis, step in _STEPS:
        sl = [slice(1, -1)] * 3
        sl[axis] = slice(1 + step, (step - 1) or None)
        nb = wide[tuple(sl)]
        hit = zero & (nb != 0)
        np.minimum.at(t[:, 8], k[hit], nb[hit])
        np.maximum.at(t[:, 9], k[hit], nb[hit])
    border = (t[:, 3] == 0) | (t[:, 4] == 0) | (t[:, 6] == H) | (t[:, 7] == W)
    t[border, 8], t[border, 9] = NO_LABEL, 0
    return t


def components_of(vol):
    """the cavity index of every voxel (-1 on labelled voxels), numbered as holes_ref numbers its rows"""
    comp, n = ndimage.label(np.asarray(vol) == 0, structure=SIX)
    flat = np.arange(comp.size, dtype=np.int64).reshape(comp.shape)
    first = np.full(n + 1, np.iinfo(np.int64).max, np.int64)
    np.minimum.at(first, comp.ravel(), flat.ravel())
    rank = np.empty(n + 1, np.int64)
    rank[0] = -1
    rank[1 + np.argsort(first[1:], kind='stable')] = np.arange(n)
    return rank[comp]


def plan_ref(t, shape, max_voxels=None):
    """(lut int64, stats) from the definition, row by row"""
    lut = np.zeros(len(t), np.int64)
    s = dict(cavities=0, filled=0, voxels_filled=0, shared=0, too_large=0)
    for i, r in enumerate(t):
        if min(r[2:5]) == 0 or any(r[5 + a] == shape[a] for a in range(3)):
            continue
        s['cavities'] += 1
        if r[8] != r[9]:
            s['shared'] += 1
        elif max_voxels is not None and r[0] > max_voxels:
            s['too_large'] += 1
        else:
            lut[i] = r[8]
            s['filled'] += 1
            s['voxels_filled'] += int(r[0])
    return lut, s


def fill_ref(vol, max_voxels=None):
    """(filled volume, stats, table) of the checker"""
    vol = np.asarray(vol)
    t = holes_ref(vol)
    lut, s = plan_ref(t, vol.shape, max_voxels)
    out = vol.copy()
    if len(t):
        k = components_of(vol)
        paint = np.append(lut, 0)[k]                           # k = -1 reads the appended 0
        mask = paint != 0
        vals = paint[mask].astype(np.uint32)
        out[mask] = vals.view(np.int32) if out.dtype == np.int32 else vals.astype(out.dtype)
    return out, s, t


def planted_volume(shape, dtype=np.uint32, seed=0, punch=0.1, labels=None, cell=4):
    """a coarse random grid of few labels and some background cells (objects that touch: shared cavities, background
    cells walled by one label or by several) with random voxels punched and small boxes carved out: closed, open,
    shared and diagonal-leak cavities of one voxel and of many"""
    rng = np.random.default_rng(seed)
    top = int(np.iinfo(dtype).max)
    labs = np.array([0] + (list(labels) if labels else [int(x) for x in rng.integers(1, min(top, 250) + 1, size=3)]) * 2)
    v = labs[rng.integers(0, len(labs), size=[-(-n // cell) for n in shape])]
    for a, n in enumerate(shape):
        v = np.repeat(v, cell, axis=a).take(np.arange(n), axis=a)
    v = v.astype(np.uint32).astype(dtype) if np.dtype(dtype) != np.int32 else v.astype(np.uint32).view(np.int32)
    v[rng.random(shape) < punch] = 0
    for _ in range(6):                                         # cavities of more than one voxel, row and slice
        lo = [int(rng.integers(0, n)) for n in shape]
        v[lo[0]:lo[0] + int(rng.integers(1, 4)), lo[1]:lo[1] + int(rng.integers(1, 4)), lo[2]:lo[2] + int(rng.integers(1, 5))] = 0
    return np.ascontiguousarray(v)


def separate_boxes(seed, punch=0.2):
    """solid boxes a voxel or more apart, none inside another, with random voxels punched out"""
    rng = np.random.default_rng(seed)
    v = np.zeros((12, 14, 16), np.uint32)
    v[1:6, 1:7, 1:8] = 3
    v[1:6, 8:13, 1:8] = 9
    v[7:11, 1:13, 1:8] = 4
    v[0:12, 0:14, 9:16] = 70000                                # reaches the border: cavities opened through every face
    v[rng.random(v.shape) < punch] = 0
    return v


# ------------------------------------------------------------------------------------------------------ the checker's own checks
def test_the_checker_on_cases_counted_by_hand():
    v = np.zeros((5, 5, 5), np.uint32)
    v[1:4, 1:4, 1:4] = 5
    v[2, 2, 2] = 0
    t = holes_ref(v)
    assert t.tolist() == [[98, 0, 0, 0, 0, 5, 5, 5, NO_LABEL, 0], [1, 62, 2, 2, 2, 3, 3, 3, 5, 5]]
    out, s, _ = fill_ref(v)
    assert out[2, 2, 2] == 5 and (out != v).sum() == 1
    assert s == dict(cavities=1, filled=1, voxels_filled=1, shared=0, too_large=0)
    # an edge leak keeps the cavity closed; a face leak opens it
    v[1, 1, 2] = 0                                            # touches (2, 2, 2) across an edge only
    assert len(holes_ref(v)) == 2 and fill_ref(v)[0][2, 2, 2] == 5 and fill_ref(v)[0][1, 1, 2] == 0
    v[1, 2, 2] = 0                                            # shares a face with it and with the outside
    assert len(holes_ref(v)) == 1 and fill_ref(v)[1]['cavities'] == 0
    # two labels on the wall: shared, left; z_base moves first and z
    w = np.zeros((3, 3, 5), np.uint8)
    w[:, :, :2], w[:, :, 3:] = 7, 8
    w[:, :, 2] = 1
    w[1, 1, 2] = 0
    t = holes_ref(w, z_base=10)
    assert t.tolist() == [[1, 10 * 15 + 22, 11, 1, 2, 12, 2, 3, 1, 8]]
    w[1, 1, 1] = 0
    assert holes_ref(w).tolist() == [[2, 21, 1, 1, 1, 2, 2, 3, 1, 8]] and fill_ref(w)[1]['shared'] == 1
    # a neighbour slice enters the wall labels; a diagonal one does not
    u = np.full((1, 3, 3), 4, np.uint8)
    u[0, 1, 1] = 0
    above = np.zeros((3, 3), np.uint8)
    above[0, 0], above[1, 1] = 200, 9
    assert holes_ref(u, above=above)[0, 8:].tolist() == [4, 9] and holes_ref(u)[0, 8:].tolist() == [4, 4]


@pytest.mark.parametrize('seed', range(4))
def test_the_checker_equals_binary_fill_holes_where_nothing_is_nested(seed):
    v = separate_boxes(seed)
    want = v.copy()
    for L in np.unique(v[v > 0]):
        want[ndimage.binary_fill_holes(v == L) & (v == 0)] = L
    got, s, _ = fill_ref(v)
    np.testing.assert_array_equal(got, want)
    assert s['filled'] > 3 and s['shared'] == 0 and s['voxels_filled'] == int((want != v).sum())


# ------------------------------------------------------------------------------------------------------ plan
def _row(voxels, box, lab_min, lab_max, first=0):
    return [voxels, first] + list(box) + [lab_min, lab_max]


def test_plan_boundaries():
    shape = (6, 7, 8)
    inner = (1, 1, 1, 5, 6, 7)                                 # the largest closed box
    t = np.array([_row(4, inner, 9, 9), _row(5, inner, 9, 9), _row(3, inner, 2, 9), _row(2, inner, 2 ** 32 - 1, 2 ** 32 - 1)])
    lut, s = HO.plan(t, shape, max_voxels=4)
    assert lut.dtype == np.uint32 and lut.tolist() == [9, 0, 0, 2 ** 32 - 1]
    assert s == dict(cavities=4, filled=2, voxels_filled=6, shared=1, too_large=1)
    lut, s = HO.plan(t, shape)
    assert lut.tolist() == [9, 9, 0, 2 ** 32 - 1] and s == dict(cavities=4, filled=3, voxels_filled=11, shared=1, too_large=0)
    for a in range(3):                                         # each of the six faces opens it
        for box in (inner[:a] + (0,) + inner[a + 1:], inner[:3 + a] + (shape[a],) + inner[4 + a:]):
            lut, s = HO.plan(np.array([_row(1, box, 9, 9)]), shape)
            assert lut.tolist() == [0] and s == dict(cavities=0, filled=0, voxels_filled=0, shared=0, too_large=0), box
    lut, s = HO.plan(np.zeros((0, N_COL), np.int64), shape)
    assert lut.shape == (0,) and s['cavities'] == 0
    for bad in (0, -1, True, False, 2.0, 'all'):
        with pytest.raises(ValueError, match='max_voxels'):
            HO.plan(t, shape, max_voxels=bad)
    with pytest.raises(ValueError, match='closed cavity without a wall'):
        HO.plan(np.array([_row(1, inner, NO_LABEL, 0)]), shape)


@pytest.mark.parametrize('seed', [0, 2, 3])
def test_plan_equals_the_definition_on_random_volumes(seed):
    v = planted_volume((9, 11, 13), np.uint32, seed, labels=[3, 2 ** 31, 2 ** 32 - 1, 77])
    t = holes_ref(v)
    for cap in (None, 1, 2, 5):
        lut, s = HO.plan(t, v.shape, cap)
        want_lut, want_s = plan_ref(t, v.shape, cap)
        assert lut.astype(np.int64).tolist() == want_lut.tolist() and s == want_s
    assert HO.plan(t, v.shape)[1]['cavities'] > 0


# ------------------------------------------------------------------------------------------------------ merge_blocks
def _block_tables(v, cuts):
    """the tables of the z-blocks [cuts[i], cuts[i + 1]) with their true neighbour slices, and the seams' id pairs"""
    from empanada_amd.components import seam_pairs
    tables, ids, base = [], [], 0
    for z0, z1 in zip(cuts[:-1], cuts[1:]):
        part = v[z0:z1]
        tables.append(holes_ref(part, below=v[z0 - 1] if z0 else None, above=v[z1] if z1 < len(v) else None, z_base=z0))
        ids.append(np.where(part == 0, components_of(part) + 1 + base, 0))
        base += len(tables[-1])
    seams = [seam_pairs(v[z - 1] == 0, ids[i][-1], v[z] == 0, ids[i + 1][0], 6) for i, z in enumerate(cuts[1:-1])]
    return tables, seams, ids


def test_every_z_partition_merges_to_the_table_of_the_whole():
    v = planted_volume((6, 9, 11), np.uint32, 5)
    whole = holes_ref(v)
    assert len(whole) > 8 and (whole[:, 9] > 0).any() and (whole[:, 5] - whole[:, 2] > 1).any()
    k = components_of(v)
    D = v.shape[0]
    for r in range(D):
        for inner in itertools.combinations(range(1, D), r):
            cuts = (0,) + inner + (D,)
            tables, seams, ids = _block_tables(v, cuts)
            got, index = HO.merge_blocks(tables, seams, return_index=True)
            np.testing.assert_array_equal(got, whole, err_msg=str(cuts))
            prov = np.concatenate(ids)                         # every voxel's provisional id maps to its cavity
            np.testing.assert_array_equal(np.where(prov > 0, index[np.maximum(prov, 1) - 1], -1), k)
    merged = HO.merge_blocks([torch.from_numpy(t) for t in tables], seams)
    assert isinstance(merged, torch.Tensor) and merged.numpy().tolist() == whole.tolist()
    assert HO.merge_blocks([], []).shape == (0, N_COL)
    with pytest.raises(ValueError, match='seam ids'):
        HO.merge_blocks(tables, [np.array([[1, 10 ** 6]])])


def test_columns():
    assert HO.COLUMNS == ('voxels', 'first', 'z0', 'y0', 'x0', 'z1', 'y1', 'x1', 'lab_min', 'lab_max')
    assert HO.NO_LABEL == NO_LABEL


# ------------------------------------------------------------------------------------------------------ argument errors
def test_argument_errors_come_before_any_gpu_work():
    from empanada_amd import _hip
    from empanada_amd.inference.driver import _check_fill, infer_volume
    assert _check_fill(None) == (False, None) and _check_fill(True) == (True, None) and _check_fill(7) == (True, 7)
    assert _check_fill(np.int64(3)) == (True, 3)
    for bad in (False, 0, -3, 2.5, 'yes', np.bool_(True), (1,)):
        with pytest.raises(ValueError, match='fill_holes'):
            _check_fill(bad)
        with pytest.raises(ValueError, match='fill_holes'):    # no engine, no volume: nothing was touched before it
            infer_volume(None, None, norms=None, labels=[1], fill_holes=bad)
    cpu = torch.zeros((2, 3, 4), dtype=torch.uint8)
    for kw, msg in ((dict(z_base=-1), 'z_base'), (dict(z_base=True), 'z_base'), (dict(block_voxels=0), 'block_voxels'),
                    (dict(block_voxels=2 ** 31), 'block_voxels'), (dict(), 'on the GPU')):
        with pytest.raises(ValueError, match=msg):
            _hip.label_holes(cpu, **kw)
    with pytest.raises(ValueError, match='on the GPU'):
        _hip.label_holes(np.zeros((2, 3, 4), np.uint8))
