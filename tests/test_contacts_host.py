"""CPU: the contact checker itself (tests/contacts_ref.py) against scipy's edt object by object and on the cases of the
definition counted by hand, contacts.check / merge_tables / derive / partners, the ball table, and the refusals of
_hip.label_contacts and of the E9 entry points without a GPU."""
import ctypes
import itertools
import os
import sys

import numpy as np
import pytest
import torch
from scipy import ndimage

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contacts_ref as ref  # noqa: E402

from empanada_amd import _hip, contacts as C  # noqa: E402

N_COL = 10


# ---------------------------------------------------------------------------------------------- the checker
def per_pair_table(A, B, r2, sampling):
    """the table stated per pair with scipy: the contact voxels of (a, b) are A == a where the squared distance to the
    nearest voxel of b in B, an exact integer after rounding, is at most r2"""
    same = B is None
    Bv = A if same else B
    rows = []
    for b in np.unique(Bv[Bv != 0]):
        d2 = np.rint(ndimage.distance_transform_edt(Bv != b, sampling=sampling) ** 2).astype(np.int64)
        pad = np.pad(Bv, 1)
        for a in np.unique(A[A != 0]):
            if same and a == b:
                continue
            m = (A == a) & (d2 <= r2)
            if not m.any():
                continue
            z, y, x = np.nonzero(m)
            faces = []
            for axis, step in enumerate(((1, 0, 0), (0, 1, 0), (0, 0, 1))):
                n = 0
                if sampling[axis] ** 2 <= r2:
                    for s in (-1, 1):
                        n += int((pad[z + 1 + s * step[0], y + 1 + s * step[1], x + 1 + s * step[2]] == b).sum())
                faces.append(n)
            rows.append([int(a), int(b), len(z), int(d2[m].min()), int(z.sum()), int(y.sum()), int(x.sum())] + faces)
    rows.sort()
    return np.asarray(rows, np.int64).reshape(-1, N_COL)


@pytest.mark.parametrize('sampling', [(1, 1, 1), (3, 1, 1), (2, 1, 3)], ids=str)
def test_restatement_equals_the_per_pair_statement(sampling):
    for seed, shape in enumerate(((6, 6, 8), (4, 5, 7), (1, 6, 8), (6, 1, 1))):
        A = ref.random_labels(shape, 0.5, 5, seed)
        B = ref.random_labels(shape, 0.4, 4, seed + 100)
        for r2 in (min(sampling) ** 2, 4, 9, 16):
            np.testing.assert_array_equal(ref.contact_table(A, None, r2, sampling), per_pair_table(A, None, r2, sampling),
                                          err_msg=f'same {shape} r2 {r2}')
            np.testing.assert_array_equal(ref.contact_table(A, B, r2, sampling), per_pair_table(A, B, r2, sampling),
                                          err_msg=f'two {shape} r2 {r2}')


def test_ball():
    assert len(ref.ball(24)) == 485 and ref.ball(24)[0] == (0, 0, 0, 0)
    for r2, sampling in ((1, (1, 1, 1)), (24, (1, 1, 1)), (9, (3, 1, 1)), (16, (2, 1, 3)), (6399, (16, 16, 16))):
        got = _hip.contact_ball(r2, sampling)
        assert got.dtype == np.int32
        assert [(d, z, y, x) for z, y, x, d in got.tolist()] == ref.ball(r2, sampling)
    assert len(_hip.contact_ball(1)) == 7 and len(_hip.contact_ball(3)) == 27


# ---------------------------------------------------------------------------------------------- cases counted by hand
def hand_cases():
    """[(name, A, B, r2, sampling, rows as a list or None, check)]: the rows where the definition gives them outright"""
    touch = ref.two_cubes(0)
    gap = ref.two_cubes(2)
    stacked = ref.two_cubes(0, axis=0)
    row = lambda a, b, n, d, f: (a, b, n, d, f)
    return [
        ('touching r2 1', touch, None, 1, (1, 1, 1), [row(1, 2, 4, 1, (0, 0, 4)), row(2, 1, 4, 1, (0, 0, 4))]),
        ('gap 2 r2 8', gap, None, 8, (1, 1, 1), []),
        ('gap 2 r2 9', gap, None, 9, (1, 1, 1), [row(1, 2, 4, 9, (0, 0, 0)), row(2, 1, 4, 9, (0, 0, 0))]),
        ('gap 2 r2 10', gap, None, 10, (1, 1, 1), [row(1, 2, 4, 9, (0, 0, 0)), row(2, 1, 4, 9, (0, 0, 0))]),
        ('stacked pitch 3 r2 8', stacked, None, 8, (3, 1, 1), []),
        ('stacked pitch 3 r2 9', stacked, None, 9, (3, 1, 1), [row(1, 2, 4, 9, (4, 0, 0)), row(2, 1, 4, 9, (4, 0, 0))]),
        ('overlap', np.array([[[0, 5, 0]]], np.uint32), np.array([[[0, 7, 7]]], np.uint32), 1, (1, 1, 1),
         [row(5, 7, 1, 0, (0, 0, 1))]),
    ]


def assert_hand_case(name, table, want):
    assert table.shape == (len(want), N_COL), name
    for got, (a, b, n, d, f) in zip(table.tolist(), want):
        assert got[:4] == [a, b, n, d] and tuple(got[7:]) == f, f'{name}: {got}'


def test_cases_counted_by_hand():
    for name, A, B, r2, sampling, want in hand_cases():
        assert_hand_case(name, ref.contact_table(A, B, r2, sampling), want)
    t = ref.contact_table(ref.distinct_block(), None, 3)
    assert len(t) == 316 and int((t[:, 0] == 14).sum()) == 26 and (t[:, 2] == 1).all()
    # the centroid of the touching cubes' contact site: the face layer of cube 1 at x = 2
    t = ref.contact_table(ref.two_cubes(0), None, 1, z_base=10)
    assert t[0, 4:7].tolist() == [4 * 10 + 6, 6, 8]


def test_symmetry_of_the_same_volume_case():
    A = ref.random_labels((7, 6, 9), 0.5, 6, 3)
    t = ref.contact_table(A, None, 5)
    rows = {(a, b): r for a, b, *r in t.tolist()}
    for (a, b), r in rows.items():
        back = rows[(b, a)]
        assert r[1] == back[1] and r[5:] == back[5:]


# ---------------------------------------------------------------------------------------------- the host module
def test_merge_tables_over_every_z_partition():
    A = ref.random_labels((5, 6, 7), 0.5, 5, 8, special=(0x80000000, 0xFFFFFFFF))
    B = ref.random_labels((5, 6, 7), 0.5, 5, 9)
    for Bv, r2 in ((None, 2), (B, 5)):
        whole = ref.contact_table(A, Bv, r2)
        assert len(whole) > 10 and (whole[:, 0] >= 2 ** 31).any()
        h = C.halo_slices(r2)
        for cuts in itertools.chain.from_iterable(itertools.combinations(range(1, 5), k) for k in range(5)):
            edges = [0, *cuts, 5]
            parts = []
            for z0, z1 in zip(edges[:-1], edges[1:]):
                src = A if Bv is None else Bv
                parts.append(ref.contact_table(A[z0:z1], None if Bv is None else Bv[z0:z1], r2, z_base=z0,
                                               below=src[max(z0 - h, 0):z0], above=src[z1:z1 + h]))
            np.testing.assert_array_equal(C.merge_tables(parts), whole, err_msg=str(cuts))
            got = C.merge_tables([torch.from_numpy(p) for p in parts[::-1]])
            assert isinstance(got, torch.Tensor) and got.dtype == torch.int64
            np.testing.assert_array_equal(got.numpy(), whole, err_msg=str(cuts))
    empty = np.zeros((0, N_COL), np.int64)
    assert C.merge_tables([]).shape == (0, N_COL) and C.merge_tables([empty, empty]).shape == (0, N_COL)
    assert tuple(C.merge_tables([torch.from_numpy(empty)]).shape) == (0, N_COL)
    np.testing.assert_array_equal(C.merge_tables([empty, whole, torch.from_numpy(empty)]).numpy(), whole)
    np.testing.assert_array_equal(C.gather_tables(whole[::-1]), whole)


def test_derive_and_partners():
    t = ref.contact_table(ref.two_cubes(0), None, 1, z_base=10)
    d = C.derive(t, sampling=(3, 1, 2), unit=2.0)
    assert d['a'].tolist() == [1, 2] and d['b'].tolist() == [2, 1] and d['voxels'].tolist() == [4, 4]
    assert d['min_distance'].tolist() == [2.0, 2.0]
    assert d['centroid'].tolist() == [[11.5, 1.5, 2.0], [11.5, 1.5, 3.0]]
    assert d['area'].tolist() == [4 * 3 * 1 * 4.0] * 2                  # four x faces of az * ay each, unit^2
    assert C.derive(torch.from_numpy(t))['area'].tolist() == [4.0, 4.0]
    assert C.derive(np.zeros((0, N_COL), np.int64))['centroid'].shape == (0, 3)
    for bad in ((1, 1), (0, 1, 1), 'abc'):
        with pytest.raises(ValueError):
            C.derive(t, sampling=bad)
    with pytest.raises(ValueError):
        C.derive(t, unit=0)
    p = C.partners(ref.contact_table(ref.distinct_block(), None, 3))
    assert p['a'].tolist() == list(range(1, 28)) and p['partners'][13] == 26 and p['partners'][0] == 7
    assert (p['min_d2'] == 1).all()
    p = C.partners(ref.contact_table(ref.two_cubes(2), None, 10))
    assert p['a'].tolist() == [1, 2] and p['partners'].tolist() == [1, 1] and p['min_d2'].tolist() == [9, 9]
    assert C.partners(np.zeros((0, N_COL), np.int64))['a'].shape == (0,)


def test_check():
    assert C.COLUMNS == ('a', 'b', 'voxels', 'min_d2', 'sum_z', 'sum_y', 'sum_x', 'faces_z', 'faces_y', 'faces_x')
    assert C.check(None) is None
    assert C.check(1) == (1, (1, 1, 1), None)
    assert C.check(2 ** 0.5) == (2, (1, 1, 1), None) and C.check(3 ** 0.5) == (3, (1, 1, 1), None)
    assert C.check(4.9) == (24, (1, 1, 1), None)
    assert C.check((3, (3, 1, 1))) == (9, (3, 1, 1), None)
    assert C.check([4, [2, 1, 3]]) == (16, (2, 1, 3), None)
    assert C.check((2, (1, 1, 1), [(1, 2), [2, 1], (1, 2)])) == (4, (1, 1, 1), [(1, 2), (2, 1)])
    assert C.check((64, (16, 16, 16))) == (4096, (16, 16, 16), None)
    assert C.halo_slices(24) == 4 and C.halo_slices(9, (3, 1, 1)) == 1 and C.halo_slices(8, (3, 1, 1)) == 0
    bad = [0, -1, True, 'r', float('nan'), float('inf'), 0.5,            # below min(pitch)^2
           5, (15, (3, 3, 3)),                                           # a ring above 4
           (2, (3, 3, 3)),                                               # below the smallest pitch
           (1,), (1, (1, 1, 1), [(1, 2)], 4), (1, (1, 1)), (1, (0, 1, 1)), (1, (1, 1, 17)), (1, (1.0, 1, 1)), (1, 'abc'),
           (1, (1, 1, 1), []), (1, (1, 1, 1), 'ab'), (1, (1, 1, 1), [(1,)]), (1, (1, 1, 1), [1, 2]), (1, (1, 1, 1), ['ab'])]
    for value in bad:
        with pytest.raises(ValueError):
            C.check(value)
    with pytest.raises(ValueError, match='point'):
        C.check((2, (3, 3, 3)))
    with pytest.raises(ValueError, match='more than 4'):
        C.check(5)
    with pytest.raises(ValueError, match='contacts:'):
        C.check((1, (1, 1, 17)))


def test_infer_volume_argument_is_checked_before_any_work():
    from empanada_amd.inference import driver
    assert driver._check_contacts(None, [1, 2], [1]) is None
    assert driver._check_contacts(2, [1, 2], [1]) == (4, (1, 1, 1), [(1, 1), (1, 2), (2, 1)])
    assert driver._check_contacts(1, [1, 2, 3], [1, 3])[2] == [(1, 1), (1, 2), (1, 3), (2, 1), (2, 3), (3, 1), (3, 2), (3, 3)]
    assert driver._check_contacts((1, (1, 1, 1), [(2, 1), (1, 2)]), [1, 2], [1])[2] == [(1, 2), (2, 1)]
    with pytest.raises(ValueError, match='class 7'):
        driver._check_contacts((1, (1, 1, 1), [(1, 7)]), [1, 2], [1])
    assert driver.contact_dataset_names([(1, 2)], {1: 'mito', 2: 'er'}) == {(1, 2): 'mito_er_contacts'}


# ---------------------------------------------------------------------------------------------- refusals without a GPU
def test_label_contacts_refuses_before_any_launch():
    a = torch.zeros((4, 5, 6), dtype=torch.int32)
    with pytest.raises(ValueError, match='on the GPU'):
        _hip.label_contacts(a)                                          # a CPU tensor
    with pytest.raises(ValueError, match='on the GPU'):
        _hip.label_contacts(a, a.to(torch.uint8))
    with pytest.raises(ValueError, match='shapes must be equal'):
        _hip.label_contacts(a, torch.zeros((4, 5, 7), dtype=torch.uint8))
    with pytest.raises(ValueError, match='contiguous'):
        _hip.label_contacts(torch.zeros((4, 5, 12), dtype=torch.int32)[:, :, ::2])
    with pytest.raises(ValueError, match='contiguous'):
        _hip.label_contacts(a, torch.zeros((4, 6, 5), dtype=torch.int32).transpose(1, 2))
    for bad in (torch.zeros((5, 6), dtype=torch.int32), torch.zeros((4, 5, 6)), torch.zeros((4, 5, 6), dtype=torch.int64),
                np.zeros((4, 5, 6), np.int32)):
        with pytest.raises(ValueError):
            _hip.label_contacts(bad)
    # halo stacks: too many slices for the ball, another (H, W), another dtype than B's, not a stack
    with pytest.raises(ValueError, match='the ball reaches 1'):
        _hip.label_contacts(a, r2=1, below=torch.zeros((2, 5, 6), dtype=torch.int32))
    with pytest.raises(ValueError, match='the ball reaches 0'):
        _hip.label_contacts(a, r2=8, sampling=(3, 1, 1), above=torch.zeros((1, 5, 6), dtype=torch.int32))
    for kw in (dict(below=torch.zeros((1, 5, 7), dtype=torch.int32)), dict(above=torch.zeros((1, 5, 6), dtype=torch.uint8)),
               dict(below=torch.zeros((5, 6), dtype=torch.int32))):
        with pytest.raises(ValueError, match='below|above'):
            _hip.label_contacts(a, r2=4, **kw)
    with pytest.raises(ValueError, match='dtype'):                     # the stacks follow B, not A
        _hip.label_contacts(a, a.to(torch.uint8), r2=4, below=torch.zeros((1, 5, 6), dtype=torch.int32))
    for kw in (dict(r2=0), dict(r2=25), dict(r2=1.0), dict(r2=True), dict(r2=8, sampling=(3, 3, 3)), dict(sampling=(1, 1)),
               dict(sampling=(1, 0, 1)), dict(z_base=-1), dict(z_base=1.5), dict(block_voxels=0), dict(block_voxels=2 ** 31)):
        with pytest.raises(ValueError):
            _hip.label_contacts(a, **kw)


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    lib = _hip.load()
    buf = (ctypes.c_uint8 * 4096)()
    p = ctypes.addressof(buf)
    geom = lambda **kw: [kw.get(k, v) for k, v in dict(a=p, item_a=4, b=p, item_b=4, D=4, H=5, W=6, below=None, hb=0,
                                                       above=None, ha=0, same=1, az=1, ay=1, ax=1, r2=1, ball=p,
                                                       n_ball=7).items()]
    tail = [p, 1 << 20, p, None]
    for kw, word in ((dict(a=None), 'null'), (dict(item_a=2), 'uint8'), (dict(W=0), 'shape'), (dict(D=1 << 20, H=1 << 10, W=1 << 10), '2^31'),
                     (dict(same=2), 'same'), (dict(b=p + 4), 'same = 1'), (dict(az=0), 'sampling'), (dict(ax=17), 'sampling'),
                     (dict(r2=0), 'point'), (dict(r2=25), 'ring'), (dict(r2=8, az=3, ay=3, ax=3), 'point'),
                     (dict(hb=2, below=p), 'halo'), (dict(ha=1), 'null'), (dict(n_ball=0), 'ball'), (dict(n_ball=730), 'ball'),
                     (dict(ball=None), 'ball'), (dict(a=p + 1, b=p + 1), 'misaligned')):
        assert lib.emp_label_contacts_count(*geom(**kw), *tail) == -1, kw
        assert word.encode() in lib.emp_last_error(), (kw, lib.emp_last_error())
        assert lib.emp_label_contacts_emit(*geom(**kw), p, 1 << 20, 1, 1, p, p, p, None) == -1, kw
    assert lib.emp_label_contacts_count(*geom(), p, 16, p, None) == -1 and b'workspace' in lib.emp_last_error()
    assert lib.emp_label_contacts_count(*geom(), p, 1 << 20, None, None) == -1
    assert lib.emp_label_contacts_emit(*geom(), p, 1 << 20, 2, 1, p, p, p, None) == -1 and b'listed' in lib.emp_last_error()
    assert lib.emp_label_contacts_emit(*geom(), p, 1 << 20, 1, 1 << 31, p, p, p, None) == -1
    assert b'below 2^31' in lib.emp_last_error()
    assert lib.emp_label_contacts_emit(*geom(), p, 1 << 20, 1, 0, None, None, None, None) == 0      # nothing to emit
    assert lib.emp_label_contacts_work_bytes(4, 5, 6) > 0 and lib.emp_label_contacts_work_bytes(1 << 20, 1 << 10, 1 << 10) == -1
    assert lib.emp_label_contacts_work_bytes(-1, 5, 6) == -1 and lib.emp_label_contacts_work_bytes(0, 5, 6) > 0
    assert lib.emp_label_contacts_rows_work_bytes(10) > 0 and lib.emp_label_contacts_rows_work_bytes(1 << 31) == -1
    assert lib.emp_label_contacts_rows(p, 1 << 31, p, 1 << 20, p, None) == -1
    assert lib.emp_label_contacts_rows(p, 10, p, 8, p, None) == -1 and b'workspace' in lib.emp_last_error()
    assert lib.emp_label_contacts_rows(None, 10, p, 1 << 20, p, None) == -1
    assert lib.emp_label_contacts_reduce(p, p, p, p, 10, 5, 6, 0, p, 1 << 20, p, 11, None) == -1
    assert lib.emp_label_contacts_reduce(p, p, p, p, 10, 0, 6, 0, p, 1 << 20, p, 5, None) == -1
    assert lib.emp_label_contacts_reduce(p, p, p, p, 10, 5, 6, -1, p, 1 << 20, p, 5, None) == -1
    assert lib.emp_label_contacts_reduce(p, None, p, p, 10, 5, 6, 0, p, 1 << 20, p, 5, None) == -1
    assert lib.emp_label_contacts_reduce(None, None, None, None, 0, 5, 6, 0, None, 0, None, 0, None) == 0
