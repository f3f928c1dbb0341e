"""CPU: the numpy checker of the surface meshes (mesh_ref.py) against cases counted by hand and against the properties
the definition promises (include/emp_hip.h, E7), and the host helpers of empanada_amd/meshes.py."""
import itertools

import numpy as np
import pytest

from empanada_amd import meshes as MS
from mesh_ref import (corner_number, det_sum, emit_ref, finish_ref, hand_cases, mesh_ref, neighbours_ref, random_volume,
                      taubin_ref)

HAND = hand_cases()
RANDOM = [((5, 7, 9), 0), ((4, 6, 5), 1), ((1, 5, 8), 2), ((6, 1, 7), 3), ((3, 4, 1), 4)]


def _edge_use(quads):
    """undirected edge -> number of quads on it"""
    use = {}
    for q in np.asarray(quads):
        for j in range(4):
            e = tuple(sorted((int(q[j]), int(q[(j + 1) % 4]))))
            use[e] = use.get(e, 0) + 1
    return use


def _corners_with(mesh, n):
    """corners that carry exactly n vertices"""
    _, counts = np.unique(mesh['vertices'], axis=0, return_counts=True)
    return int((counts == n).sum())


# ------------------------------------------------------------------------------------------------------ by hand
def test_one_voxel():
    m = mesh_ref(HAND['one'])
    assert m['vertices'].shape == (8, 3) and m['quads'].shape == (6, 4)
    assert m['vertices'].dtype == np.int32 and m['quads'].dtype == np.int32 and m['objects'].dtype == np.int64
    np.testing.assert_array_equal(m['objects'], [[7, 0, 8, 0, 6]])
    np.testing.assert_array_equal(m['vertices'], [list(p) for p in itertools.product((1, 2), repeat=3)])
    assert det_sum(m['vertices'], m['quads']) == 6
    assert set(_edge_use(m['quads']).values()) == {2}


def test_a_voxel_at_the_origin_gives_two_per_far_face():
    vol = np.zeros((2, 2, 2), np.uint32)
    vol[0, 0, 0] = 1
    m = mesh_ref(vol)
    p = m['vertices'].astype(np.int64)[m['quads']]
    det = lambda a, b, c: np.einsum('ni,ni->n', a, np.cross(b, c))
    per_quad = det(p[:, 0], p[:, 1], p[:, 2]) + det(p[:, 0], p[:, 2], p[:, 3])
    # quads ascend by direction code: -z +z -y +y -x +x
    np.testing.assert_array_equal(per_quad, [0, 2, 0, 2, 0, 2])
    # every quad starts at its lowest corner
    assert (p[:, 0][:, None, :] <= p).all()


def test_two_voxels_sharing_an_edge():
    m = mesh_ref(HAND['edge'])
    assert m['vertices'].shape[0] == 14 and m['quads'].shape[0] == 12 and len(m['objects']) == 1
    use = _edge_use(m['quads'])
    assert sorted(use.values()).count(4) == 1 and set(use.values()) == {2, 4}
    assert det_sum(m['vertices'], m['quads']) == 12


def test_two_voxels_sharing_a_corner():
    m = mesh_ref(HAND['corner'])
    assert m['vertices'].shape[0] == 15 and m['quads'].shape[0] == 12


def test_two_labels_face_to_face():
    m = mesh_ref(HAND['pair'])
    np.testing.assert_array_equal(m['objects'], [[4, 0, 8, 0, 6], [9, 8, 16, 6, 12]])
    assert _corners_with(m, 2) == 4 and _corners_with(m, 1) == 8
    for row in m['objects']:
        assert det_sum(m['vertices'], m['quads'][row[3]:row[4]]) == 6
    # the shared face is there twice, with opposite windings
    a = m['vertices'][m['quads'][5]]          # +x of label 4
    b = m['vertices'][m['quads'][6 + 4]]      # -x of label 9
    np.testing.assert_array_equal(a, b[[0, 3, 2, 1]])


def test_eight_labels_around_one_corner():
    m = mesh_ref(HAND['eight'])
    assert len(m['objects']) == 8 and m['vertices'].shape[0] == 64 and m['quads'].shape[0] == 48
    centre = (m['vertices'] == 1).all(axis=1)
    assert int(centre.sum()) == 8 and _corners_with(m, 8) == 1


def test_voxels_at_the_array_corners():
    vol = HAND['ends']
    m = mesh_ref(vol)
    assert m['vertices'].shape[0] == 16 and m['quads'].shape[0] == 12
    np.testing.assert_array_equal(m['vertices'][0], [0, 0, 0])
    np.testing.assert_array_equal(m['vertices'][-1], vol.shape)
    assert det_sum(m['vertices'], m['quads']) == 12


def test_a_volume_filled_by_one_label():
    vol = HAND['full']
    D, H, W = vol.shape
    m = mesh_ref(vol)
    assert m['quads'].shape[0] == 2 * (D * H + H * W + D * W)
    assert m['vertices'].shape[0] == (D + 1) * (H + 1) * (W + 1) - (D - 1) * (H - 1) * (W - 1)
    assert det_sum(m['vertices'], m['quads']) == 6 * D * H * W


# ------------------------------------------------------------------------------------------------------ properties
def _axis_counts(vol, label):
    """exposed faces of `label` per axis, counted voxel by neighbour"""
    pad = np.pad(vol, 1)
    me = pad == label
    out = []
    for axis in range(3):
        n = 0
        for step in (-1, 1):
            n += int((me & (np.roll(pad, -step, axis) != label))[1:-1, 1:-1, 1:-1].sum())
        out.append(n)
    return out


@pytest.mark.parametrize('shape,seed', RANDOM, ids=lambda v: str(v))
def test_random_volumes(shape, seed):
    vol = random_volume(shape, seed=seed, big=True)
    D, H, W = shape
    m = mesh_ref(vol)
    V, Q, O = m['vertices'], m['quads'], m['objects']
    labels = np.unique(vol[vol != 0])
    np.testing.assert_array_equal(O[:, 0], labels)
    assert O[0, 1] == 0 and O[0, 3] == 0 and O[-1, 2] == len(V) and O[-1, 4] == len(Q)
    np.testing.assert_array_equal(O[1:, 1], O[:-1, 2])
    np.testing.assert_array_equal(O[1:, 3], O[:-1, 4])
    assert (Q >= 0).all()
    # the eight-voxel rule, evaluated corner by corner
    pad = np.pad(vol, 1)
    want = set()
    for z, y, x in itertools.product(range(D + 1), range(H + 1), range(W + 1)):
        cell = pad[z:z + 2, y:y + 2, x:x + 2].ravel()
        for l in set(cell.tolist()) - {0}:
            if (cell != l).any():
                want.add((l, z, y, x))
    got = [(int(l), *map(int, V[i])) for l, v0, v1, _, _ in O for i in range(v0, v1)]
    assert len(got) == len(set(got)) and set(got) == want
    assert got == sorted(got)                                                   # (label, z, y, x) ascending
    for l, v0, v1, q0, q1 in O:
        q = Q[q0:q1]
        assert ((q >= v0) & (q < v1)).all()                                     # an object uses its own vertices
        assert det_sum(V, q) == 6 * int((vol == l).sum())
        # per axis: a quad's normal is the axis along which its corners do not move
        p = V[q]
        axis = (p.max(axis=1) == p.min(axis=1)).argmax(axis=1)
        assert np.bincount(axis, minlength=3).tolist() == _axis_counts(vol, l)
        # closed: every directed edge is matched by its reverse equally often
        directed = {}
        for quad in q:
            for j in range(4):
                e = (int(quad[j]), int(quad[(j + 1) % 4]))
                directed[e] = directed.get(e, 0) + 1
        assert all(directed.get((b, a), 0) == n for (a, b), n in directed.items())


@pytest.mark.parametrize('shape,seed', RANDOM[:3], ids=lambda v: str(v))
def test_every_z_partition_concatenates_to_the_whole(shape, seed):
    vol = random_volume(shape, seed=seed)
    D, H, W = shape
    whole = mesh_ref(vol)
    cuts = [[0, D]] + [[0, z, D] for z in range(0, D + 1)] + [list(range(D + 1))]
    for b in cuts:
        keys, qk, qd = [], [], []
        for z0, z1 in zip(b[:-1], b[1:]):
            k, a, d = emit_ref(vol[z0:z1], below=vol[z0 - 1] if z0 else None, above=vol[z1] if z1 < D else None,
                               z_base=z0, top=z1 == D)
            keys.append(k), qk.append(a), qd.append(d)
        assert len(np.unique(np.concatenate(keys))) == len(np.concatenate(keys)), "a vertex emitted twice"
        got = finish_ref(np.concatenate(keys), np.concatenate(qk), np.concatenate(qd), H, W)
        for k in whole:
            np.testing.assert_array_equal(got[k], whole[k], err_msg=f'{b} {k}')


def test_neighbours_and_smoothing():
    vol = random_volume((4, 5, 6), seed=5)
    m = mesh_ref(vol)
    nbr = neighbours_ref(m['vertices'], m['quads'])
    V = m['vertices'].astype(np.int64)
    step = np.array([(-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)])
    for s in range(6):
        have = nbr[:, s] >= 0
        np.testing.assert_array_equal(V[nbr[have, s]], V[have] + step[s])
    assert ((nbr >= 0).sum(axis=1) >= 3).all()
    # an object's neighbours are its own
    for _, v0, v1, _, _ in m['objects']:
        part = nbr[v0:v1]
        assert ((part == -1) | ((part >= v0) & (part < v1))).all()
    np.testing.assert_array_equal(taubin_ref(m['vertices'], m['quads'], 0), V)
    # one voxel shrinks towards its centre under lambda alone, symmetrically
    one = mesh_ref(hand_cases()['one'])
    p = taubin_ref(one['vertices'], one['quads'], 1, lam=0.5, mu=0.0)
    np.testing.assert_allclose(np.abs(p - 1.5), np.full_like(p, 1 / 3), atol=1e-12)   # 1/2 - lambda / 3
    p10 = taubin_ref(m['vertices'], m['quads'], 10)
    assert np.isfinite(p10).all() and np.abs(p10 - V).max() < 2


# ------------------------------------------------------------------------------------------------------ meshes.py
def test_check():
    assert MS.check(None) is None and MS.check(True) == 0 and MS.check(0) == 0 and MS.check(3) == 3
    assert MS.check(np.int64(4)) == 4
    for bad in (False, -1, 1.5, '3', (1,), np.bool_(True)):
        with pytest.raises(ValueError, match='mesh'):
            MS.check(bad)


def test_triangles():
    q = np.array([[0, 1, 2, 3], [4, 5, 6, 7]], np.int32)
    np.testing.assert_array_equal(MS.triangles(q), [[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7]])
    assert MS.triangles(np.zeros((0, 4), np.int32)).shape == (0, 3)
    with pytest.raises(ValueError):
        MS.triangles(np.zeros((2, 3), np.int32))
    # the split keeps the signed volume
    m = mesh_ref(hand_cases()['edge'])
    p = m['vertices'].astype(np.int64)[MS.triangles(m['quads'])]
    assert int(np.einsum('ni,ni->n', p[:, 0], np.cross(p[:, 1], p[:, 2])).sum()) == 12


def test_object_mesh():
    m = mesh_ref(hand_cases()['pair'])
    v, q = MS.object_mesh(m, 9)
    np.testing.assert_array_equal(v, m['vertices'][8:])
    np.testing.assert_array_equal(q, m['quads'][6:] - 8)
    assert q.min() == 0 and q.max() == 7 and det_sum(v, q) == 6
    with pytest.raises(KeyError):
        MS.object_mesh(m, 5)
    with pytest.raises(KeyError):
        MS.object_mesh(m, 10)


def _read_obj(path):
    v, f, names = [], [], []
    for line in open(path):
        t = line.split()
        if t and t[0] == 'v':
            v.append([float(s) for s in t[1:]])
        elif t and t[0] == 'f':
            f.append([int(s) for s in t[1:]])
        elif t and t[0] == 'o':
            names.append(t[1])
    return np.array(v).reshape(-1, 3), np.array(f, np.int64).reshape(-1, 4), names


def test_write_obj_round_trip(tmp_path):
    vol = random_volume((3, 4, 5), seed=6, big=True)
    m = mesh_ref(vol)
    MS.write_obj(tmp_path / 'all.obj', m)
    v, f, names = _read_obj(tmp_path / 'all.obj')
    np.testing.assert_array_equal(v[:, ::-1], m['vertices'])
    np.testing.assert_array_equal(f[:, [0, 3, 2, 1]] - 1, m['quads'])
    assert names == [str(int(l)) for l in m['objects'][:, 0]]
    # in x y z the faces are counter-clockwise from outside: the signed volume is positive there
    assert det_sum(v.astype(np.int64), f - 1) == 6 * int((vol != 0).sum())
    label = int(m['objects'][1, 0])
    MS.write_obj(tmp_path / 'one.obj', m, label=label)
    v, f, names = _read_obj(tmp_path / 'one.obj')
    ov, oq = MS.object_mesh(m, label)
    np.testing.assert_array_equal(v[:, ::-1], ov)
    np.testing.assert_array_equal(f[:, [0, 3, 2, 1]] - 1, oq)
    assert names == [str(label)] and f.min() == 1
    smooth = dict(m, vertices=taubin_ref(m['vertices'], m['quads'], 2).astype(np.float32))
    MS.write_obj(tmp_path / 's.obj', smooth)
    np.testing.assert_allclose(_read_obj(tmp_path / 's.obj')[0][:, ::-1], smooth['vertices'], rtol=1e-7)


def test_corner_numbers():
    assert corner_number((0, 0, 0), 3, 4) == 0 and corner_number((2, 3, 4), 3, 4) == 2 * 20 + 3 * 5 + 4
