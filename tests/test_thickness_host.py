"""CPU: the local thickness (include/emp_hip.h, E10) without a GPU -- the two restatements of tests/thickness_ref.py agree
with each other, closed forms, the cap is no clamp, and the host side of empanada_amd/thickness.py: check, halo_slices,
merge_tables, derive, histogram, and the argument errors of _hip.label_thickness and infer_volume(thickness=)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import thickness_ref as ref  # noqa: E402

from empanada_amd import thickness as TH  # noqa: E402
from test_holes_host import planted_volume  # noqa: E402
from test_morph_host import SAMPLINGS, blobs  # noqa: E402

CAPS = [2, 10, 65535]


# ------------------------------------------------------------------------------------------------------ the checkers
@pytest.mark.parametrize('sampling', SAMPLINGS, ids=str)
@pytest.mark.parametrize('shape', [(13, 21, 37), (6, 9, 1)], ids=lambda s: 'x'.join(map(str, s)))
def test_fast_checker_equals_brute_force(shape, sampling):
    for make in (blobs, planted_volume):
        lab = make(shape, np.uint32, seed=3)
        for cap in CAPS:
            fast, d_fast = ref.thickness_fast(lab, cap, sampling)
            brute, d_brute = ref.thickness_brute(lab, cap, sampling)
            np.testing.assert_array_equal(d_fast, d_brute)
            np.testing.assert_array_equal(fast, brute, err_msg=f'{make.__name__} cap {cap}')
            assert ((fast > 0) == (lab != 0)).all() and (fast >= d_fast).all() and fast.max() <= cap


def test_closed_forms():
    full = np.full((5, 6, 7), 9, np.uint8)
    for cap in (1, 10, 65535):
        assert (ref.thickness_fast(full, cap)[0] == cap).all()
    for k in (0, 1, 3):
        plate = np.zeros((2 * k + 5, 9, 11), np.uint32)
        plate[2:2 * k + 3] = 4                                  # 2 k + 1 slices that span y and x
        t2 = ref.thickness_fast(plate)[0]
        assert (t2[2:2 * k + 3] == (k + 1) ** 2).all() and (t2[:2] == 0).all() and (t2[2 * k + 3:] == 0).all()
        t2 = ref.thickness_fast(plate, sampling=(3, 1, 1))[0]
        assert (t2[2:2 * k + 3] == 9 * (k + 1) ** 2).all()
    one = np.zeros((3, 3, 3), np.uint8)
    one[1, 1, 1] = 1
    assert ref.thickness_fast(one)[0].sum() == 1
    line = np.zeros((5, 5, 9), np.uint8)
    line[2, 2, :] = 3                                           # one voxel wide: the diameter reads 2
    assert (ref.thickness_fast(line)[0][2, 2] == 1).all()
    # two touching boxes of different labels, 7 and 3 thick: neither takes the other's radius
    two = np.zeros((9, 12, 14), np.uint32)
    two[1:8, 1:11, 1:8] = 5
    two[1:4, 1:11, 8:13] = 6
    t2 = ref.thickness_fast(two)[0]
    assert t2[two == 5].max() == 16 and t2[two == 6].max() == 4
    alone = ref.thickness_fast(np.where(two == 6, two, 0))[0]
    np.testing.assert_array_equal(t2[two == 6], alone[two == 6])


def test_the_cap_is_not_a_clamp():
    lab = ref.dumbbell()
    free, d2 = ref.thickness_fast(lab, 65535)
    assert (d2 == 65535).sum() == 0 and free.max() >= 121
    for cap in (10, 50):
        capped, d2c = ref.thickness_fast(lab, cap)
        clamp = np.minimum(free, cap)
        assert (capped <= clamp).all() and (capped != clamp).any() and (d2c == cap).sum() > 0
    roomy, d2r = ref.thickness_fast(lab, 1024)
    assert (d2r == 1024).sum() == 0
    np.testing.assert_array_equal(roomy, free)                  # nothing reached the cap: the uncapped result


def test_table_ref_counts_every_labelled_voxel_once():
    lab = blobs((13, 21, 37), np.uint32, seed=1).view(np.int32)
    t2 = ref.thickness_fast(lab, 10)[0]
    table = ref.table_ref(lab, t2)
    assert table[:, 2].sum() == (lab != 0).sum() and (table[:, 0] >= 2 ** 31).any()
    keys = [(a << 32) | b for a, b in table[:, :2].tolist()]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)


# ------------------------------------------------------------------------------------------------------ thickness.py
def test_check_accepts():
    assert TH.COLUMNS == ('label', 't2', 'voxels')
    assert TH.check(None) is None
    assert TH.check(True) == (32.0, 1024, (1, 1, 1))
    assert TH.check(1) == (1.0, 1, (1, 1, 1))
    assert TH.check(math.sqrt(10)) == (math.sqrt(10), 10, (1, 1, 1))
    assert TH.check((2.5, (3, 1, 2))) == (2.5, 6, (3, 1, 2))
    assert TH.check([255.9, [1, 1, 1]])[1] == 65484
    assert TH.check(math.sqrt(65535))[1] == 65535


@pytest.mark.parametrize('bad', [False, 0, 0.5, -1, 256, float('nan'), float('inf'), 'big', (3,), (3, (1, 1)),
                                 (3, (0, 1, 1)), (3, (1, 17, 1)), (3, (1.0, 1, 1)), (3, (1, 1, 1), 1), (True, (1, 1, 1))])
def test_check_rejects(bad):
    with pytest.raises(ValueError):
        TH.check(bad)


def test_halo_slices():
    assert TH.halo_slices(1) == 0 and TH.halo_slices(2) == 2 and TH.halo_slices(10) == 6 and TH.halo_slices(1024) == 62
    assert TH.halo_slices(1025) == 64 and TH.halo_slices(26, (3, 1, 1)) == 2 and TH.halo_slices(10, (1, 2, 1)) == 6
    assert TH.halo_slices(65535) == 510


HAND = np.array([[7, 4, 3], [2, 1, 5], [7, 1, 1], [2 ** 31 + 1, 9, 2], [2, 9, 1], [7, 4, 2]], np.int64)


def test_merge_tables_order_and_sums():
    want = [[2, 1, 5], [2, 9, 1], [7, 1, 1], [7, 4, 5], [2 ** 31 + 1, 9, 2]]
    assert TH.merge_tables([HAND]).tolist() == want
    assert TH.merge_tables([HAND[:2], HAND[2:]]).tolist() == want
    got = TH.merge_tables([torch.from_numpy(HAND[:3]), HAND[3:]])
    assert isinstance(got, torch.Tensor) and got.dtype == torch.int64 and got.tolist() == want
    assert TH.merge_tables([HAND, HAND])[:, 2].tolist() == [10, 2, 2, 10, 4]
    for none in ([], [np.zeros((0, 3), np.int64)]):
        assert TH.merge_tables(none).shape == (0, 3)
    assert TH.gather_tables(HAND).tolist() == want              # no process group: sorted


def test_derive_and_histogram():
    d = TH.derive(HAND, unit=2.0)
    assert d['label'].tolist() == [2, 7, 2 ** 31 + 1] and d['voxels'].tolist() == [6, 6, 2]
    for i, values in enumerate(([1] * 5 + [9], [1] + [4] * 5, [9, 9])):
        diam = 2.0 * np.sqrt(np.asarray(values, np.float64)) * 2.0
        for key, fn in (('mean', np.mean), ('std', np.std), ('min', np.min), ('median', np.median), ('max', np.max)):
            assert d[key][i] == pytest.approx(fn(diam), rel=1e-12), (key, i)
    even = TH.derive(np.array([[1, 1, 2], [1, 4, 2]]))          # the two middle values differ: their mean
    assert even['median'].tolist() == [3.0]
    h = TH.histogram(HAND, [0, 2, 4, 6])
    assert h['label'].tolist() == [2, 7, 2 ** 31 + 1]
    assert h['counts'].tolist() == [[0, 5, 1], [0, 1, 5], [0, 0, 2]]     # diameters 2, 4 and 6: 6 is the last right edge
    assert TH.histogram(HAND, [0, 2])['counts'].tolist() == [[5], [1], [0]]
    assert TH.histogram(HAND, [0, 1.9])['counts'].tolist() == [[0], [0], [0]]
    assert TH.histogram(HAND, [0, 5], unit=0.5)['counts'].tolist() == [[6], [6], [2]]
    empty = TH.derive(np.zeros((0, 3), np.int64))
    assert all(len(v) == 0 for v in empty.values())
    for bad in ([1], [2, 1], [0, float('nan')]):
        with pytest.raises(ValueError):
            TH.histogram(HAND, bad)
    with pytest.raises(ValueError):
        TH.derive(HAND, unit=0)


def test_infer_volume_checks_thickness_before_any_work():
    from empanada_amd.inference.driver import _check_thickness, infer_volume
    assert _check_thickness(None) is None and _check_thickness(True) == (32.0, 1024, (1, 1, 1))
    for bad, match in ((0.5, 'r_cap'), (300, 'cap'), ((3, (1, 1)), 'sampling'), ('x', 'r_cap')):
        with pytest.raises(ValueError, match=match):
            _check_thickness(bad)

    class Engine:                                               # nothing of it is reached
        thing_list = [1]

    with pytest.raises(ValueError, match='r_cap'):
        infer_volume(Engine(), np.zeros((4, 4, 4), np.uint8), norms=None, labels=[1], thickness=-2)


def test_argument_errors_are_raised_without_a_gpu():
    from empanada_amd import _hip
    ok = torch.zeros((4, 5, 6), dtype=torch.uint8)
    for kw in (dict(cap=0), dict(cap=65536), dict(cap=2.0), dict(cap=True), dict(sampling=(1, 1)),
               dict(sampling=(0, 1, 1)), dict(sampling=(1, 1, 17)), dict(sampling=(1.0, 1, 1)), dict(block_voxels=0),
               dict(block_voxels=2 ** 31), dict(block_voxels=1.5)):
        with pytest.raises(ValueError):
            _hip.label_thickness(ok, **kw)
    for slab in (ok, ok.numpy(), None, torch.zeros((4, 5, 6), dtype=torch.int64), torch.zeros((0, 5, 6), dtype=torch.uint8)):
        if isinstance(slab, torch.Tensor) and slab.is_cuda:
            continue
        with pytest.raises(ValueError):                         # a CPU tensor, whatever else is right about it
            _hip.label_thickness(slab)
    # the library refuses what the wrapper would never pass, before any launch
    lib = _hip.load()
    assert lib.emp_label_thick_work_bytes(4, 5, 6, 0, 0) > 0
    assert lib.emp_label_thick_work_bytes(4, 5, 6, 2, 3) > lib.emp_label_thick_work_bytes(4, 5, 6, 0, 0)
    assert lib.emp_label_thick_work_bytes(-1, 5, 6, 0, 0) == -1 and lib.emp_label_thick_work_bytes(4, 0, 6, 0, 0) == -1
    assert lib.emp_label_thick_work_bytes(2 ** 20, 2 ** 6, 2 ** 5, 0, 0) == -1
    assert lib.emp_label_thick_work_bytes(4, 5, 6, -1, 0) == -1
    assert lib.emp_label_thick_edt(None, 2, 4, 5, 6, None, 0, None, 0, 1, 1, 1, 10, None, 0, None) == -1
    assert b'uint8' in lib.emp_last_error()
    assert lib.emp_label_thick_edt(None, 1, 4, 5, 6, None, 0, None, 0, 1, 1, 1, 0, None, 0, None) == -1
    assert b'cap' in lib.emp_last_error()
    assert lib.emp_label_thick_edt(None, 1, 4, 5, 6, None, 0, None, 0, 1, 1, 1, 10, None, 0, None) == -1
    assert b'null' in lib.emp_last_error()
    assert lib.emp_label_thick_lists(4, 5, 6, 0, 0, 10, None, 0, None, None) == -1
    assert lib.emp_label_thick_resolve(4, 5, 6, 0, 0, 1, 1, 0, 10, None, 0, None, None) == -1
    assert b'sampling' in lib.emp_last_error()
    assert lib.emp_label_thick_resolve(4, 5, 6, 0, 0, 1, 1, 1, 10, None, 0, None, None) == -1
