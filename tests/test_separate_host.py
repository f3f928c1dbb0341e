"""Host: the CPU checkers of separate_ref.py are themselves checked -- the level-by-level flood against scipy's shortest
paths and against the 64-bit min-relaxation in random order -- then separation.check and separation.plan on every form
of their arguments, the dumbbell counted with scipy, and the argument errors that come before any GPU work."""
import numpy as np
import pytest
import torch
from scipy import ndimage

from empanada_amd import separation as SP
from separate_ref import (INF, cores_ref, dumbbell, erode_ref, grow_brute, grow_ref, grow_relax, random_case, separate_ref,
                          serpentine_flat, serpentine_tall)


# ------------------------------------------------------------------------------------------------------ the checker
@pytest.mark.parametrize('shape', [(1, 1, 1), (1, 1, 6), (2, 3, 4), (4, 5, 6), (6, 6, 6)], ids=lambda s: 'x'.join(map(str, s)))
def test_grow_ref_equals_shortest_paths_and_the_relaxation(shape):
    rng = np.random.default_rng(11)
    ties = reached = 0
    for seed in range(6):
        for density in (0.0, 'one', 0.05, 0.3):
            for big in (False, True):
                lab, seeds = random_case(shape, seed, n_labels=3 + seed % 2, density=density, big=big)
                if seed % 3 == 0:                               # solid objects: long paths and many ties
                    lab[:] = np.where(lab != 0, 3, 0) if seed else 3
                owner, dist = grow_ref(lab, seeds)
                o2, d2 = grow_brute(lab, seeds)
                np.testing.assert_array_equal(dist, d2)
                np.testing.assert_array_equal(owner, o2)
                o3, d3 = grow_relax(lab, seeds, rng)
                np.testing.assert_array_equal(dist, d3)
                np.testing.assert_array_equal(owner, o3)
                assert ((owner != 0) == (dist != INF)).all() and not owner[lab == 0].any()
                held = (seeds != 0) & (lab != 0)
                np.testing.assert_array_equal(owner[held], seeds[held])
                reached += int((dist != INF).sum() - held.sum())
    assert reached > 0 or np.prod(shape) < 6


def test_grow_ref_by_hand():
    # two seeds equidistant from a voxel: the larger wins; a seed on background is ignored; no crossing of labels
    lab = np.asarray([[[3, 3, 3, 3, 3, 0, 4, 4, 0, 3]]], np.uint32)
    seeds = np.asarray([[[7, 0, 0, 0, 9, 5, 0, 2, 0, 0]]], np.uint32)
    owner, dist = grow_ref(lab, seeds)
    assert owner[0, 0].tolist() == [7, 7, 9, 9, 9, 0, 2, 2, 0, 0]
    assert dist[0, 0].tolist() == [0, 1, 2, 1, 0, INF, 1, 0, INF, INF]
    seeds[0, 0, 0] = 2 ** 32 - 1
    assert grow_ref(lab, seeds)[0][0, 0].tolist() == [2 ** 32 - 1, 2 ** 32 - 1, 2 ** 32 - 1, 9, 9, 0, 2, 2, 0, 0]
    # the path must stay inside the label: around a wall of another label
    lab = np.asarray([[[1, 1, 1], [1, 2, 1], [1, 2, 1]]], np.uint32)
    seeds = np.zeros_like(lab)
    seeds[0, 2, 0] = 6
    assert grow_ref(lab, seeds)[1][0].tolist() == [[2, 3, 4], [1, INF, 5], [0, INF, 6]]


def test_the_serpentines():
    lab, seeds = serpentine_flat()
    assert lab.shape == (3, 9, 40) and int((lab != 0).sum()) == 204
    owner, dist = grow_ref(lab, seeds)
    assert int(dist[lab != 0].max()) == 101 and int((owner == 1).sum()) == 102 and int((owner == 2).sum()) == 102
    lab, seeds = serpentine_tall()
    n = int((lab != 0).sum())
    owner, dist = grow_ref(lab, seeds)
    assert lab.shape == (33, 9, 70) and int(dist[lab != 0].max()) == (n - 1) // 2
    assert int((owner == 1).sum()) + int((owner == 2).sum()) == n and abs(int((owner == 1).sum()) - n / 2) <= 1


# ------------------------------------------------------------------------------------------------------ check
def test_check_accepts():
    assert SP.check(None) is None
    assert SP.check(3) == (9, 1, (1, 1, 1)) and SP.check(3.0) == (9, 1, (1, 1, 1))
    assert SP.check(np.float32(1.5)) == (2, 1, (1, 1, 1))
    assert SP.check(2 ** 0.5) == (2, 1, (1, 1, 1)) and SP.check(3 ** 0.5) == (3, 1, (1, 1, 1))
    assert SP.check((3, 20)) == (9, 20, (1, 1, 1)) and SP.check([2, np.int64(4)]) == (4, 4, (1, 1, 1))
    assert SP.check((3, 1, (3, 1, 1))) == (9, 1, (3, 1, 1)) and SP.check((3, 2, [2, 16, 1])) == (9, 2, (2, 16, 1))
    assert SP.check(255.99) == (65530, 1, (1, 1, 1))
    from empanada_amd import morphology as MO
    for r in (1, 1.5, 2, 7.3, 100):
        for s in ((1, 1, 1), (3, 1, 1)):
            if r >= min(s):
                assert SP.check((r, 1, s))[0::2] == MO.check(('erode', r, s))[1:]


@pytest.mark.parametrize('bad', [0, -1, 0.5, True, '3', float('nan'), float('inf'), 256.5, (3,), (3, 1, (1, 1, 1), 4), (3, 0),
                                 (3, 1.0), (3, True), (3, None), (3, 1, (1, 1)), (3, 1, (0, 1, 1)), (3, 1, (1, 17, 1)),
                                 (3, 1, 1), (2, 1, (3, 3, 3)), ('open', 3), {'r': 3}, (None, 1)],
                         ids=lambda b: repr(b).replace(' ', ''))
def test_check_rejects(bad):
    with pytest.raises(ValueError, match='separate'):
        SP.check(bad)


def test_infer_volume_checks_separate_before_any_work():
    import inspect
    from empanada_amd.inference import driver
    assert driver._check_separate(None) is None and driver._check_separate((3, 2)) == (9, 2, (1, 1, 1))
    with pytest.raises(ValueError, match='separate'):
        driver._check_separate((3, 0))
    assert inspect.signature(driver.infer_volume).parameters['separate'].default is None


# ------------------------------------------------------------------------------------------------------ plan
def test_plan_orders_by_voxels_then_seed_id_and_takes_the_top_of_the_class():
    #          label seed voxels
    pieces = [(5, 1, 10), (5, 2, 30), (5, 3, 30), (2, 4, 7), (2, 5, 7), (9, 6, 1), (9, 7, 2)]
    lut, stats = SP.plan(pieces, 40)
    # label 2 first: seed 4 keeps (tie on voxels: the smaller seed id), seed 5 -> 41; label 5: seed 2 keeps, 3 -> 42,
    # 1 -> 43; label 9: seed 7 keeps, 6 -> 44
    assert lut.dtype == np.uint32 and lut.tolist() == [0, 43, 5, 42, 2, 41, 44, 9]
    assert stats == dict(objects_separated=3, pieces_added=4, voxels_moved=7 + 30 + 10 + 1)
    # the top is the class's, not the table's
    assert SP.plan(pieces, 1000)[0].tolist() == [0, 1003, 5, 1002, 2, 1001, 1004, 9]
    # the order of the rows does not matter
    assert SP.plan(pieces[::-1], 40)[0].tolist() == lut.tolist()
    assert SP.plan(np.asarray(pieces), 40)[0].tolist() == lut.tolist()


def test_plan_zero_candidates_and_errors():
    lut, stats = SP.plan(np.zeros((0, 3), np.int64), 17)
    assert lut.tolist() == [0] and stats == dict(objects_separated=0, pieces_added=0, voxels_moved=0)
    assert SP.plan([], 0)[0].tolist() == [0]
    two = [(7, 1, 4), (7, 2, 5)]
    assert SP.plan(two, 2 ** 32 - 2)[0].tolist() == [0, 2 ** 32 - 1, 7]
    with pytest.raises(ValueError, match='would pass'):
        SP.plan(two, 2 ** 32 - 1)
    assert SP.plan(two, 254, 255)[0].tolist() == [0, 255, 7]
    with pytest.raises(ValueError, match='would pass 255'):
        SP.plan(two, 255, 255)
    with pytest.raises(ValueError, match='seed ids'):
        SP.plan([(7, 1, 4), (7, 3, 5)], 9)
    with pytest.raises(ValueError, match='seed ids'):
        SP.plan([(7, 1, 4), (7, 1, 5)], 9)
    with pytest.raises(ValueError, match='labels outside'):
        SP.plan(two, 6)
    with pytest.raises(ValueError, match='labels outside'):
        SP.plan([(0, 1, 4)], 6)
    for top in (-1, 2 ** 32, 1.5, True, None):
        with pytest.raises(ValueError, match='top'):
            SP.plan(two, top)


# ------------------------------------------------------------------------------------------------------ the dumbbell
def test_the_dumbbell_counted_with_scipy():
    vol = dumbbell()
    assert vol.shape == (17, 17, 41) and int((vol != 0).sum()) == 2017
    # r2 = 4: the neck of radius 2 survives as a line, one core, nothing changes
    rows, _ = cores_ref(erode_ref(vol, 4))
    assert len(rows) == 1
    new, stats, _ = separate_ref(vol, 4)
    np.testing.assert_array_equal(new, vol)
    assert stats == dict(r2=4, min_core=1, sampling=(1, 1, 1), objects_in=1, objects_separated=0, pieces_added=0,
                         voxels_moved=0)
    # r2 = 9: the neck is gone and the balls' cores remain
    mask = vol != 0
    assert ndimage.label(ndimage.distance_transform_edt(mask) ** 2 > 9.5, ndimage.generate_binary_structure(3, 1))[1] == 2
    rows, _ = cores_ref(erode_ref(vol, 9))
    assert len(rows) == 2 and rows[0, 1] == rows[1, 1] and rows[0, 2] < rows[1, 2]
    new, stats, owner = separate_ref(vol, 9)
    assert sorted(np.unique(new).tolist()) == [0, 5, 6]
    np.testing.assert_array_equal(new != 0, mask)               # no voxel lost or added
    assert int((owner == 1).sum()) == 1002 and int((owner == 2).sum()) == 1015
    assert int((new == 5).sum()) == 1015 and int((new == 6).sum()) == 1002   # the larger piece keeps the label
    x = np.broadcast_to(np.arange(41), vol.shape)
    assert x[owner == 1].max() == 19 and x[owner == 2].min() == 20   # the midplane x = 20 goes to the larger seed id
    assert stats == dict(r2=9, min_core=1, sampling=(1, 1, 1), objects_in=1, objects_separated=1, pieces_added=1,
                         voxels_moved=1002)
    # a second core below min_core: untouched
    small = dumbbell(second_r=4)
    rows, _ = cores_ref(erode_ref(small, 9))
    assert len(rows) == 2 and rows[:, 1].min() < 30 <= rows[:, 1].max()
    np.testing.assert_array_equal(separate_ref(small, 9, min_core=30)[0], small)
    assert separate_ref(small, 9, min_core=1)[1]['pieces_added'] == 1


# ------------------------------------------------------------------------------------------------------ _hip without a GPU
def test_argument_errors_are_raised_without_a_gpu():
    from empanada_amd import _hip
    cpu = torch.zeros((3, 4, 5), dtype=torch.uint8)
    seeds = torch.zeros((3, 4, 5), dtype=torch.int32)
    with pytest.raises(ValueError, match='GPU'):
        _hip.label_grow(cpu, seeds)
    with pytest.raises(ValueError, match='tensor'):
        _hip.label_grow(np.zeros((3, 4, 5), np.uint8), seeds)
    with pytest.raises(ValueError, match='dtype'):
        _hip.label_grow(cpu.float(), seeds)
    with pytest.raises(ValueError, match='contiguous'):
        _hip.label_grow(cpu.permute(2, 1, 0), seeds)
