"""CPU: the skeleton checker itself (tests/skeleton_ref.py) on the counted cases of the definition, skeletons.check /
derive / write_obj, the refusals of the wrappers, and the argument validation of the E8 entry points without a GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
from scipy import ndimage

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import skeleton_ref as ref  # noqa: E402

from empanada_amd import _hip, skeletons  # noqa: E402


def _ends_junctions(S):
    g = ref.graph(S)
    return int((g['degree'] == 1).sum()), int((g['degree'] >= 3).sum()), g


# ---------------------------------------------------------------------------------------------- the checker
def test_checker_bar():
    L = ref.bar()
    assert int(L.sum()) == 1666
    S, iterations, deleted = ref.thin(L)
    assert int((S != 0).sum()) == 25 and iterations == 5 and deleted == 1666 - 25
    ends, junctions, g = _ends_junctions(S)
    assert (ends, junctions) == (2, 0)
    v = g['vertices']
    assert len(np.unique(v[:, 0])) == 1 and len(np.unique(v[:, 1])) == 1          # one straight line along x
    assert np.array_equal(np.sort(v[:, 2]), np.arange(v[:, 2].min(), v[:, 2].min() + 25))
    assert ref.topology(S) == ref.topology(L)


def test_checker_ball():
    L = ref.ball()
    assert int(L.sum()) == 2109
    S, iterations, _ = ref.thin(L)
    assert int((S != 0).sum()) == 1 and iterations == 9
    assert ref.topology(S) == ref.topology(L)


def test_checker_torus():
    L = ref.torus()
    assert int(L.sum()) == 1348
    S, _, _ = ref.thin(L)
    g = ref.graph(S)
    assert len(g['vertices']) == 44 and np.all(g['degree'] == 2)                  # a ring: no end point
    assert ndimage.label(S != 0, structure=np.ones((3, 3, 3)))[1] == 1
    assert ref.topology(S) == ref.topology(L)


def test_checker_touching_and_subset():
    L = ref.touching()
    S, _, _ = ref.thin(L)
    assert int((S == 1).sum()) == 1 and int((S == 2).sum()) == 1
    assert np.all((S == 0) | (S == L))
    N = ref.noise((12, 14, 30), 5)
    T, _, _ = ref.thin(N)
    assert np.all((T == 0) | (T == N)) and ref.topology(T) == ref.topology(N)


def test_checker_predicates():
    assert ref.classify(0) == 0                                                   # an isolated voxel stays
    assert ref.classify(1 << 12) == 1                                             # the end of a curve is simple
    assert ref.classify((1 << 12) | (1 << 13)) == 2                               # a curve's inner voxel is an isthmus
    assert ref.classify(0x3ffffff) == 0                                           # an interior voxel


def test_checker_graph_by_hand():
    S = np.zeros((2, 3, 4), dtype=np.uint32)
    S[0, 0, 0] = S[0, 1, 1] = S[1, 1, 2] = 7                                      # a diagonal chain
    S[0, 2, 3] = 9                                                                # 26-adjacent to label 7, alone
    g = ref.graph(S, z_base=3)
    assert g['vertices'].tolist() == [[3, 0, 0], [3, 1, 1], [4, 1, 2], [3, 2, 3]]
    assert g['degree'].tolist() == [1, 2, 1, 0]
    assert g['edges'].tolist() == [[0, 1], [1, 2]]
    assert g['objects'].tolist() == [[7, 0, 3, 0, 2, 0, 2, 0], [9, 3, 4, 2, 2, 1, 0, 0]]


# ---------------------------------------------------------------------------------------------- skeletons.check
def test_check_accepts():
    assert skeletons.check(None) is None
    assert skeletons.check(True) == (64.0, 4096, (1, 1, 1))
    assert skeletons.check(10) == (10.0, 100, (1, 1, 1))
    assert skeletons.check(2.5) == (2.5, 6, (1, 1, 1))
    assert skeletons.check((3, (2, 1, 1))) == (3.0, 9, (2, 1, 1))
    assert skeletons.check([255.9, [16, 16, 16]])[1] == 65484
    assert skeletons.check(np.sqrt(65535.0) + 1e-7)[1] == 65535


@pytest.mark.parametrize('bad', [False, 0, -1, 0.5, 256, 1e9, float('nan'), float('inf'), 'yes', (3,), (3, (1, 1)),
                                 (3, (0, 1, 1)), (3, (1, 1, 17)), (3, (1.0, 1, 1)), (True, (1, 1, 1)), (3, 1, 1),
                                 {'r_cap': 3}, (3, None)])
def test_check_refuses(bad):
    with pytest.raises(ValueError):
        skeletons.check(bad)


# ---------------------------------------------------------------------------------------------- derive, write_obj
def _hand_made():
    # object 4: an L of four vertices with a unit step, a face diagonal and a space diagonal; object 6: one vertex
    vertices = np.array([[0, 0, 0], [0, 0, 1], [0, 1, 2], [1, 2, 3], [5, 5, 5]], np.int32)
    edges = np.array([[0, 1], [1, 2], [2, 3]], np.int32)
    return {'vertices': vertices, 'degree': np.array([1, 2, 2, 1, 0], np.int32),
            'radius2': np.array([1, 4, 9, 16, 25], np.int32), 'edges': edges,
            'objects': np.array([[4, 0, 4, 0, 3, 0, 2, 0], [6, 4, 5, 3, 3, 1, 0, 0]], np.int64)}


def test_derive_by_hand():
    d = skeletons.derive(_hand_made())
    assert d['label'].tolist() == [4, 6]
    assert d['length'] == pytest.approx([1 + np.sqrt(2) + np.sqrt(3), 0.0], rel=1e-15)
    assert d['ends'].tolist() == [2, 0] and d['junctions'].tolist() == [0, 0] and d['isolated'].tolist() == [0, 1]
    assert d['mean_radius'] == pytest.approx([2.5, 5.0]) and d['max_radius'] == pytest.approx([4.0, 5.0])
    d = skeletons.derive(_hand_made(), spacing=(3, 2, 1))
    assert d['length'] == pytest.approx([1 + np.sqrt(4 + 1) + np.sqrt(9 + 4 + 1), 0.0], rel=1e-15)
    empty = {'vertices': np.zeros((0, 3), np.int32), 'degree': np.zeros(0, np.int32), 'radius2': np.zeros(0, np.int32),
             'edges': np.zeros((0, 2), np.int32), 'objects': np.zeros((0, 8), np.int64)}
    assert len(skeletons.derive(empty)['length']) == 0
    with pytest.raises(ValueError):
        skeletons.derive(_hand_made(), spacing=(1, 0, 1))
    broken = _hand_made()
    broken['edges'] = np.array([[0, 9]], np.int32)
    with pytest.raises(ValueError):
        skeletons.derive(broken)


def test_derive_of_the_checkers_bar():
    S, _, _ = ref.thin(ref.bar())
    g = ref.graph(S)
    g['radius2'] = np.ones(len(g['vertices']), np.int32)
    d = skeletons.derive(g)
    assert d['length'].tolist() == [24.0] and d['ends'].tolist() == [2]


def test_object_skeleton_and_write_obj(tmp_path):
    s = _hand_made()
    v, deg, r2, e = skeletons.object_skeleton(s, 6)
    assert v.tolist() == [[5, 5, 5]] and deg.tolist() == [0] and r2.tolist() == [25] and e.shape == (0, 2)
    with pytest.raises(KeyError):
        skeletons.object_skeleton(s, 5)
    skeletons.write_obj(tmp_path / 'all.obj', s)
    lines = (tmp_path / 'all.obj').read_text().splitlines()
    assert lines[1:6] == ['v 0 0 0', 'v 1 0 0', 'v 2 1 0', 'v 3 2 1', 'v 5 5 5']     # x y z
    assert lines[6:] == ['o 4', 'l 1 2', 'l 2 3', 'l 3 4', 'o 6']
    skeletons.write_obj(tmp_path / 'one.obj', s, label=4)
    lines = (tmp_path / 'one.obj').read_text().splitlines()
    assert [l for l in lines if l[0] == 'l'] == ['l 1 2', 'l 2 3', 'l 3 4'] and sum(l[0] == 'v' for l in lines) == 4


# ---------------------------------------------------------------------------------------------- refusals, no GPU
def test_wrappers_refuse_before_any_gpu_work():
    cpu = torch.zeros((2, 3, 4), dtype=torch.uint8)
    for f in (_hip.label_thin, _hip.label_graph, _hip.LabelThin):
        with pytest.raises(ValueError):
            f(cpu)
        with pytest.raises(ValueError):
            f(np.zeros((2, 3, 4), np.uint8))
    with pytest.raises(ValueError):
        _hip.skel_classify(torch.zeros((4,), dtype=torch.int32))
    with pytest.raises(ValueError):
        _hip.graph_finish((cpu, cpu), (cpu, cpu), (3, 4))
    with pytest.raises(ValueError):
        _hip.graph_finish(None, None, (3, 4))


def test_abi_argument_validation_without_gpu():
    """the error paths return before any launch"""
    lib = _hip.load()
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.addressof(buf)
    assert lib.emp_label_thin_work_bytes(8, 8, 64) > 0
    assert lib.emp_label_thin_work_bytes(1 << 20, 1 << 10, 1 << 10) == -1
    assert lib.emp_label_thin_work_bytes(1, 0, 4) == -1
    wb = lib.emp_label_thin_work_bytes(4, 4, 4)
    assert lib.emp_skel_classify(None, 4, None, None) == -1 and b'null' in lib.emp_last_error()
    assert lib.emp_skel_classify(None, -1, None, None) == -1
    assert lib.emp_skel_classify(None, 0, None, None) == 0
    assert lib.emp_label_thin_init(p, 2, 4, 4, 4, p, p, wb, None) == -1 and b'uint8' in lib.emp_last_error()
    assert lib.emp_label_thin_init(p, 1, 4, 0, 4, p, p, wb, None) == -1
    assert lib.emp_label_thin_init(p, 1, 1 << 20, 1 << 10, 1 << 10, p, p, wb, None) == -1
    assert b'2^31' in lib.emp_last_error()
    assert lib.emp_label_thin_init(p, 1, 4, 4, 4, p, p, wb - 1, None) == -1 and b'workspace' in lib.emp_last_error()
    assert lib.emp_label_thin_init(None, 1, 4, 4, 4, p, p, wb, None) == -1
    assert lib.emp_label_thin_init(p + 2, 4, 4, 4, 4, p, p, wb, None) == -1 and b'misaligned' in lib.emp_last_error()
    assert lib.emp_label_thin_init(None, 1, 0, 4, 4, None, None, 0, None) == 0          # D == 0 is a no-op
    assert lib.emp_label_thin_mark(p, 1, 4, 4, 4, p, p, None, None, None, p, wb, 1, 0, None) == -1
    assert b'halo' in lib.emp_last_error()
    assert lib.emp_label_thin_mark(p, 1, 4, 4, 4, p, None, None, None, None, p, wb, 1, 4, None) == -1
    assert lib.emp_label_thin_mark(p, 1, 4, 4, 4, p, None, None, None, None, p, wb, 2, 0, None) == -1
    assert lib.emp_label_thin_mark(p, 1, 4, 4, 4, p, None, None, None, None, p, wb - 1, 1, 0, None) == -1
    assert lib.emp_label_thin_mark(p, 1, 0, 4, 4, None, None, None, None, None, None, 0, 0, 0, None) == 0
    assert lib.emp_label_thin_pass(p, 1, 4, 4, 4, p, None, None, None, None, p, wb, 1, 8, 0, None) == -1
    assert b'subfield' in lib.emp_last_error()
    assert lib.emp_label_thin_pass(p, 1, 4, 4, 4, p, None, None, None, None, p, wb, 1, 0, -1, None) == -1
    assert lib.emp_label_thin_pass(p, 1, 4, 4, 4, None, None, None, None, None, p, wb, 1, 0, 0, None) == -1
    assert lib.emp_label_thin_pass(p, 1, 4, 4, 4, p, None, None, p, None, p, wb, 1, 0, 0, None) == -1
    assert lib.emp_label_thin_pass(p, 1, 0, 4, 4, None, None, None, None, None, None, 0, 0, 0, 0, None) == 0
    assert lib.emp_label_thin_paint(p, p, 1, 16, p + 4096, 2, None) == -1
    assert lib.emp_label_thin_paint(p, p + 4096, 1, 16, p + 4100, 1, None) == -1 and b'overlaps' in lib.emp_last_error()
    assert lib.emp_label_thin_paint(p, p + 4096, 1, 16, p + 8, 1, None) == -1 and b'state' in lib.emp_last_error()
    assert lib.emp_label_thin_paint(None, None, 1, 0, None, 1, None) == 0
    assert lib.emp_label_graph_count_work_bytes(16) > 0
    assert lib.emp_label_graph_count(p, 1, 1 << 10, 1 << 10, 1 << 10, None, None, p, 1 << 16, p, None) == -1
    assert b'2^26' in lib.emp_last_error()
    assert lib.emp_label_graph_count(p, 1, 4, 4, 4, None, None, p, 8, p, None) == -1
    assert lib.emp_label_graph_count(p, 3, 4, 4, 4, None, None, p, 1 << 16, p, None) == -1
    assert lib.emp_label_graph_emit(p, 1, 4, 4, 4, None, None, 1 << 40, p, 1, 0, p, p, p, p, None) == -1
    assert b'2^32' in lib.emp_last_error()
    assert lib.emp_label_graph_emit(p, 1, 4, 4, 4, None, None, 0, p, 65, 0, p, p, p, p, None) == -1
    assert lib.emp_label_graph_emit(p, 1, 4, 4, 4, None, None, 0, p, 1, 0, None, None, None, None, None) == -1
    assert lib.emp_label_graph_emit(p, 1, 4, 4, 4, None, None, 0, p, 0, 0, None, None, None, None, None) == 0
    assert lib.emp_label_graph_index(p, p, 1 << 31, p, p, 0, 4, 4, p, 1 << 16, p, p, p, 4, p, None) == -1
    assert lib.emp_label_graph_index(p, p, 4, p, p, 0, 0, 4, p, 1 << 16, p, p, p, 4, p, None) == -1
    assert lib.emp_label_graph_index(p, p, 4, p, p, 0, 4, 4, p, 8, p, p, p, 4, p, None) == -1
    assert lib.emp_label_graph_index(p, p, 4, p, p, 0, 4, 4, p, 1 << 16, p, p, p, 4, None, None) == -1
