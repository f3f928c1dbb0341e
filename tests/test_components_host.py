"""CPU: 3D connected components (include/emp_hip.h, E3) -- the checker the GPU tests compare the kernel with, and the
host logic of empanada_amd/components.py on O(#components) tables.

`components_ref` restates the definition with scipy.ndimage.label, one call per distinct label with the structuring
element of the connectivity, the pieces ordered by their first flat index; it shares nothing with the kernel.  It is
itself checked against cases counted by hand.  Every comparison is bit for bit."""
import itertools

import numpy as np
import pytest
import torch
from scipy import ndimage

from empanada_amd import components as CP

N_COL = 9
CONNECTIVITIES = (6, 18, 26)


def components_ref(lab, connectivity, z_base=0):
    """(table (n, 9) int64, comp (D, H, W) int64: the component index of every voxel, -1 = background)"""
    lab = np.asarray(lab)
    if lab.dtype == np.int32:
        lab = lab.view(np.uint32)
    D, H, W = lab.shape
    structure = ndimage.generate_binary_structure(3, {6: 1, 18: 2, 26: 3}[connectivity])
    flat = np.arange(lab.size, dtype=np.int64).reshape(lab.shape)
    rows, pieces = [], []
    for v in np.unique(lab):
        if v == 0:
            continue
        cc, n = ndimage.label(lab == v, structure=structure)
        for k, box in enumerate(ndimage.find_objects(cc), start=1):
            mask = cc[box] == k
            first = int(flat[box][mask].min())
            rows.append([int(v), int(mask.sum()), first + z_base * H * W, box[0].start + z_base, box[1].start,
                         box[2].start, box[0].stop + z_base, box[1].stop, box[2].stop])
            pieces.append((first, box, mask))
    table = np.array(rows, dtype=np.int64).reshape(-1, N_COL)
    order = np.argsort(table[:, 2], kind='stable')
    comp = np.full(lab.shape, -1, np.int64)
    for k, i in enumerate(order):
        _, box, mask = pieces[i]
        comp[box][mask] = k
    return table[order], comp


def split_ref(lab, connectivity, min_size=None, min_span=None, z_base=0):
    """the repaired volume and the stats: `plan` over the restatement's table, painted with numpy"""
    lab = np.asarray(lab)
    table, comp = components_ref(lab, connectivity, z_base)
    lut, stats = CP.plan(table, min_size, min_span)
    out = np.where(comp >= 0, np.append(lut, 0)[comp], 0).astype(np.uint32)
    return out, stats, table


def random_labels(shape, n_labels, density, seed, dtype=np.uint32, values=None):
    rng = np.random.default_rng(seed)
    values = np.arange(1, n_labels + 1) if values is None else np.asarray(values)
    lab = values[rng.integers(0, len(values), size=shape)].astype(dtype)
    lab[rng.random(shape) >= density] = 0
    return lab


# ------------------------------------------------------------------------------------------- the restatement itself
def test_restatement_against_cases_counted_by_hand():
    face = np.zeros((2, 2, 2), np.uint8)
    face[0, 0, 0] = face[1, 0, 0] = 3
    edge = np.zeros((2, 2, 2), np.uint8)
    edge[0, 0, 0] = edge[0, 1, 1] = 3
    corner = np.zeros((2, 2, 2), np.uint8)
    corner[0, 0, 0] = corner[1, 1, 1] = 3
    counts = {c: [len(components_ref(v, c)[0]) for v in (face, edge, corner)] for c in CONNECTIVITIES}
    assert counts == {6: [1, 2, 2], 18: [1, 1, 2], 26: [1, 1, 1]}
    table, comp = components_ref(corner, 26, z_base=5)
    assert table.tolist() == [[3, 2, 5 * 4 + 0, 5, 0, 0, 7, 2, 2]]
    table, comp = components_ref(corner, 6, z_base=1)
    assert table.tolist() == [[3, 1, 4, 1, 0, 0, 2, 1, 1], [3, 1, 11, 2, 1, 1, 3, 2, 2]]
    assert comp[0, 0, 0] == 0 and comp[1, 1, 1] == 1 and (comp == -1).sum() == 6
    # two labels side by side never join; order is by first voxel, not by label
    two = np.array([[[9, 9, 4, 4, 0, 9]]], np.uint32)
    table, comp = components_ref(two, 26)
    assert table.tolist() == [[9, 2, 0, 0, 0, 0, 1, 1, 2], [4, 2, 2, 0, 0, 2, 1, 1, 4], [9, 1, 5, 0, 0, 5, 1, 1, 6]]
    assert comp.ravel().tolist() == [0, 0, 1, 1, -1, 2]
    z, y, x = np.indices((8, 8, 8))
    checker = ((z + y + x) % 2 == 0).astype(np.uint8)
    assert [len(components_ref(checker, c)[0]) for c in CONNECTIVITIES] == [256, 1, 1]
    assert components_ref(np.zeros((2, 3, 4), np.uint8), 18)[0].shape == (0, N_COL)
    assert components_ref(np.array([[[-1]]], np.int32), 6)[0][0, 0] == 2 ** 32 - 1


# ------------------------------------------------------------------------------------------------------------- plan
def _row(label, voxels, first, box=(0, 0, 0, 9, 9, 9)):
    return [label, voxels, first, *box]


def test_plan_orders_by_voxels_then_first():
    table = np.array([_row(7, 10, 0), _row(2, 5, 3), _row(7, 30, 8), _row(7, 10, 20), _row(2, 5, 1 + 40)], np.int64)
    lut, stats = CP.plan(table)
    # label 2: rows 1 (first 3) and 4 (first 41) tie on voxels -> row 1 keeps 2, row 4 is the first new label;
    # label 7: row 2 (30 voxels) keeps 7, then rows 0 and 3 tie on 10 voxels -> first 0 before first 20
    assert lut.dtype == np.uint32 and lut.tolist() == [9, 2, 7, 10, 8]
    assert stats == dict(objects_in=2, objects_split=2, pieces_added=3, pieces_removed=0, objects_out=5)
    lut, stats = CP.plan(table[[2, 1]])
    assert lut.tolist() == [7, 2] and stats == dict(objects_in=2, objects_split=0, pieces_added=0, pieces_removed=0,
                                                    objects_out=2)
    lut, stats = CP.plan(np.zeros((0, N_COL), np.int64), 5, 5)
    assert lut.shape == (0,) and stats['objects_out'] == 0 and stats['objects_in'] == 0


def test_plan_filter_boundaries():
    box = (2, 3, 4, 6, 7, 8)                                          # spans 4, 4, 4
    for voxels, keeps in ((500, True), (499, False)):
        lut, stats = CP.plan(np.array([_row(3, voxels, 0, box)], np.int64), min_size=500)
        assert bool(lut[0]) == keeps and stats['pieces_removed'] == (0 if keeps else 1)
    for axis in range(3):
        for span, keeps in ((4, True), (3, False)):
            b = list(box)
            b[3 + axis] = b[axis] + span
            lut, stats = CP.plan(np.array([_row(3, 1000, 0, tuple(b))], np.int64), min_span=4)
            assert bool(lut[0]) == keeps, (axis, span)
            assert stats['objects_out'] == int(keeps)
    # the first piece is judged on its own too: it goes, the second survives and gets the new label
    table = np.array([_row(3, 1000, 0, (0, 0, 0, 1, 9, 9)), _row(3, 600, 5), _row(3, 40, 9)], np.int64)
    lut, stats = CP.plan(table, min_size=500, min_span=4)
    assert lut.tolist() == [0, 4, 0]
    assert stats == dict(objects_in=1, objects_split=1, pieces_added=1, pieces_removed=2, objects_out=1)
    # new labels go to survivors only: dense above the old maximum
    table = np.array([_row(1, 90, 0), _row(1, 10, 1), _row(1, 80, 2), _row(5, 70, 3), _row(5, 9, 4), _row(5, 60, 5)],
                     np.int64)
    lut, stats = CP.plan(table, min_size=50)
    assert lut.tolist() == [1, 0, 6, 5, 0, 7]
    assert stats == dict(objects_in=2, objects_split=2, pieces_added=2, pieces_removed=2, objects_out=4)


def test_plan_a_label_whose_pieces_all_vanish_and_overflow():
    table = np.array([_row(4, 3, 0), _row(4, 2, 9), _row(6, 100, 20)], np.int64)
    lut, stats = CP.plan(table, min_size=50)
    assert lut.tolist() == [0, 0, 6]
    assert stats == dict(objects_in=2, objects_split=1, pieces_added=0, pieces_removed=2, objects_out=1)
    top = 2 ** 32 - 1
    ok = np.array([_row(top - 1, 9, 0), _row(top - 1, 8, 5)], np.int64)
    assert CP.plan(ok)[0].tolist() == [top - 1, top]
    with pytest.raises(ValueError, match='would pass'):
        CP.plan(np.array([_row(top, 9, 0), _row(top, 8, 5)], np.int64))
    assert CP.plan(np.array([_row(top, 9, 0), _row(top, 8, 5)], np.int64), min_size=9)[0].tolist() == [top, 0]
    with pytest.raises(ValueError):
        CP.plan(np.array([_row(0, 9, 0)], np.int64))


# ------------------------------------------------------------------------------------- merge_blocks and seam_pairs
def test_seam_pairs_shifts_by_hand():
    lab_a = torch.tensor([[5, 0, 0], [0, 0, 0], [0, 0, 7]], dtype=torch.int32)
    ids_a = torch.tensor([[1, 0, 0], [0, 0, 0], [0, 0, 2]], dtype=torch.int32)
    lab_b = torch.tensor([[0, 0, 0], [5, 5, 0], [0, 0, 9]], dtype=torch.int32)
    ids_b = torch.tensor([[0, 0, 0], [3, 3, 0], [0, 0, 4]], dtype=torch.int32)
    # a[0, 0] meets b[1, 0] by an edge (18) and b[1, 1] by a corner (26); 7 over 9 never joins
    assert CP.seam_pairs(lab_a, ids_a, lab_b, ids_b, 6).tolist() == []
    assert CP.seam_pairs(lab_a, ids_a, lab_b, ids_b, 18).tolist() == [[1, 3]]
    assert CP.seam_pairs(lab_a, ids_a, lab_b * torch.tensor([0, 1, 1]), ids_b, 18).tolist() == []
    assert CP.seam_pairs(lab_a, ids_a, lab_b * torch.tensor([0, 1, 1]), ids_b, 26).tolist() == [[1, 3]]
    got = CP.seam_pairs(lab_a.numpy(), ids_a.numpy(), lab_a.numpy(), (ids_a + 4).numpy(), 6)
    assert isinstance(got, np.ndarray) and got.tolist() == [[1, 5], [2, 6]]
    with pytest.raises(ValueError):
        CP.seam_pairs(lab_a, ids_a, lab_b, ids_b, 8)


@pytest.mark.parametrize('connectivity', CONNECTIVITIES)
def test_every_z_partition_gives_the_table_of_the_whole(connectivity):
    lab = random_labels((6, 7, 9), 3, 0.45, seed=connectivity)
    whole, comp_whole = components_ref(lab, connectivity, z_base=2)
    assert len(whole) > 8
    for cuts in itertools.chain.from_iterable(itertools.combinations(range(1, 6), k) for k in range(6)):
        bounds = [0, *cuts, 6]
        tables, ids, base = [], [], 0
        for z0, z1 in zip(bounds[:-1], bounds[1:]):
            t, comp = components_ref(lab[z0:z1], connectivity, z_base=2 + z0)
            tables.append(torch.from_numpy(t))
            ids.append(np.where(comp >= 0, comp + base + 1, 0))
            base += len(t)
        seams = [CP.seam_pairs(torch.from_numpy(lab[z - 1].astype(np.int64)), torch.from_numpy(ids[k][-1]),
                               torch.from_numpy(lab[z].astype(np.int64)), torch.from_numpy(ids[k + 1][0]), connectivity)
                 for k, z in enumerate(cuts)]
        merged, index = CP.merge_blocks(tables, seams, return_index=True)
        assert isinstance(merged, torch.Tensor) and merged.dtype == torch.int64
        np.testing.assert_array_equal(merged.numpy(), whole, err_msg=str(cuts))
        prov = np.concatenate([i.reshape(-1) for i in ids]).reshape(lab.shape)
        np.testing.assert_array_equal(np.where(prov > 0, np.append(index.numpy(), -1)[prov - 1], -1), comp_whole)
    assert CP.merge_blocks([], []).shape == (0, N_COL)
    assert isinstance(CP.merge_blocks([whole], []), np.ndarray)
    with pytest.raises(ValueError, match='different labels'):
        two = np.array([_row(1, 1, 0), _row(2, 1, 1)], np.int64)
        CP.merge_blocks([two], [np.array([[1, 2]])])


# ------------------------------------------------------------------------------------------------ argument errors
def test_check_split():
    from empanada_amd.inference.driver import _check_split
    assert _check_split(None) is None
    assert [_check_split(c) for c in (6, 18, np.int64(26))] == [6, 18, 26]
    for bad in (True, False, 0, 8, 27, '26', 26.0, (26,)):
        with pytest.raises(ValueError, match='split_objects'):
            _check_split(bad)


def test_infer_volume_refuses_a_bad_switch_before_any_work():
    from empanada_amd.inference.driver import infer_volume
    with pytest.raises(ValueError, match='split_objects'):
        infer_volume(None, None, norms=None, labels=[1], split_objects=4)


def test_hip_argument_errors_come_before_any_gpu_work():
    from empanada_amd import _hip
    for name, n_args in (('emp_label_components_work_bytes', 1), ('emp_label_components', 14),
                         ('emp_label_components_paint', 16)):
        assert len(_hip.SIGNATURES[name][1]) == n_args
    ok = torch.zeros((2, 3, 4), dtype=torch.uint8)
    for c in (0, 4, 8, True, '26', None):
        with pytest.raises(ValueError, match='connectivity'):
            _hip.label_components(ok, c)
    for dt in (torch.int64, torch.float32, torch.int16):
        with pytest.raises(ValueError, match='dtype'):
            _hip.label_components(torch.zeros((2, 3, 4), dtype=dt))
    with pytest.raises(ValueError, match='contiguous'):
        _hip.label_components(torch.zeros((2, 3, 8), dtype=torch.uint8)[:, :, ::2])
    with pytest.raises(ValueError, match=r'\(D, H, W\)'):
        _hip.label_components(torch.zeros((3, 4), dtype=torch.uint8))
    with pytest.raises(ValueError, match='single slice'):
        _hip.label_components(ok, block_voxels=11)
    for bad in (0, -1, 2 ** 31, 1.5, True):
        with pytest.raises(ValueError, match='block_voxels'):
            _hip.label_components(ok, block_voxels=bad)
    with pytest.raises(ValueError, match='z_base'):
        _hip.label_components(ok, z_base=-1)
    with pytest.raises(ValueError, match='is on cpu'):
        _hip.label_components(ok)
    with pytest.raises(ValueError):
        _hip.label_components(np.zeros((2, 3, 4), np.uint8))
