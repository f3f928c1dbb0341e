"""CPU: the shape table's definition (tests/shape_ref.py) against topology that is known by construction, and
empanada_amd.shapes' host side -- Crofton weights, derive, merge, argument checks."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import shape_ref  # noqa: E402
from test_holes_host import planted_volume  # noqa: E402


def _components26(mask):
    from scipy.ndimage import label
    return label(mask, structure=np.ones((3, 3, 3), int))[1]


def _cavities(mask):
    """background components (6-connected) that do not reach the border of the padded volume"""
    from scipy.ndimage import label
    lab, n = label(~np.pad(mask, 1))
    return n - 1


def _shapes():
    ball = shape_ref.ball(6) != 0
    torus = shape_ref.torus(8.0, 3.0, 25) != 0
    shell = shape_ref.ball(8) != 0
    g = np.indices(shell.shape) - shell.shape[0] // 2
    shell &= (g ** 2).sum(0) > 25
    corner = np.zeros((4, 4, 4), bool)
    corner[1, 1, 1] = corner[2, 2, 2] = True
    slab = np.zeros((5, 12, 20), bool)
    slab[1:4, 1:11, 1:19] = True
    slab[:, 4:7, 3:6] = False
    slab[:, 4:7, 12:16] = False
    pierced = torus.copy()                                   # a closed cavity inside the tube
    n = torus.shape[0]
    pierced[n // 2, n // 2, n // 2 + 8] = False
    return {'ball': (ball, 0), 'torus': (torus, 1), 'shell': (shell, 0), 'corner': (corner, 0), 'two-hole slab': (slab, 2),
            'torus with a cavity': (pierced, 1)}


@pytest.mark.parametrize('name', ['ball', 'torus', 'shell', 'corner', 'two-hole slab', 'torus with a cavity'])
def test_reference_euler_number_is_components_minus_tunnels_plus_cavities(name):
    mask, tunnels = _shapes()[name]
    comps, cavs = _components26(mask), _cavities(mask)
    expected = {'ball': (1, 0), 'torus': (1, 0), 'shell': (1, 1), 'corner': (1, 0), 'two-hole slab': (1, 0),
                'torus with a cavity': (1, 1)}[name]
    assert (comps, cavs) == expected                         # the shapes are what their names say
    t = shape_ref.shape_table(mask.astype(np.uint8) * 7)
    assert t.shape == (1, 26) and t[0, 0] == 7 and t[0, 1] == mask.sum()
    assert shape_ref.euler(t)[0] == comps - tunnels + cavs


def test_crofton_weights_are_the_published_constants():
    from empanada_amd.shapes import DIRECTIONS, crofton_weights
    assert [tuple(d) for d in DIRECTIONS] == shape_ref.DIRS
    w = crofton_weights((1, 1, 1))
    assert w.shape == (13,) and w.dtype == np.float64
    n1 = np.abs(np.array(DIRECTIONS)).sum(axis=1)
    np.testing.assert_allclose(w[n1 == 1], 0.0915558, atol=1e-6, rtol=0)
    np.testing.assert_allclose(w[n1 == 2], 0.0739613, atol=1e-6, rtol=0)
    np.testing.assert_allclose(w[n1 == 3], 0.0703913, atol=1e-6, rtol=0)
    assert abs(w.sum() - 1.0) < 1e-12
    a = crofton_weights((3, 1, 1))
    assert abs(a.sum() - 1.0) < 1e-12
    swapped = [DIRECTIONS.index(d) if d in DIRECTIONS else DIRECTIONS.index((-d[0], -d[1], -d[2]))
               for d in ((dz, dx, dy) for dz, dy, dx in DIRECTIONS)]
    np.testing.assert_allclose(a, a[swapped], atol=1e-12, rtol=0)
    assert not np.allclose(a, w)


@pytest.mark.parametrize('r', [6, 12, 20])
def test_derive_gives_the_area_of_a_ball(r):
    from empanada_amd.shapes import derive
    t = shape_ref.shape_table(shape_ref.ball(r, label=3))
    d = derive(t)
    true = 4 * np.pi * r * r
    area = d['surface_area'][0]
    faces = t[0, 19] + t[0, 13] + t[0, 11]
    print(f"r={r}: crofton {area / true:.4f} x, faces {faces / true:.4f} x, sphericity {d['sphericity'][0]:.4f}")
    assert abs(area / true - 1) < 0.03
    assert 1.40 < faces / true < 1.55                        # what the crack area would have said
    assert 0.97 < d['sphericity'][0] < 1.03
    assert d['euler'][0] == 1 and d['tunnels'][0] == 0
    assert d['volume'][0] == t[0, 1]
    np.testing.assert_allclose(d['centroid'][0], [r + 1.0] * 3, atol=1e-9)      # symmetric about its centre voxel
    assert 0.97 < d['elongation'][0] <= 1.0 + 1e-12 and 0.97 < d['flatness'][0] <= 1.0 + 1e-12


def test_derive_anisotropic_ball():
    """a ball of radius 18 sampled at pitch (3, 1, 1): 13 x 37 x 37 voxels"""
    from empanada_amd.shapes import derive
    g = np.indices((15, 41, 41)).astype(np.float64)
    d2 = (3 * (g[0] - 7)) ** 2 + (g[1] - 20) ** 2 + (g[2] - 20) ** 2
    t = shape_ref.shape_table((d2 <= 18 * 18).astype(np.uint8))
    d = derive(t, (3, 1, 1))
    assert abs(d['surface_area'][0] / (4 * np.pi * 18 * 18) - 1) < 0.03
    np.testing.assert_allclose(d['axes'][0], 18.0, rtol=0.03)


@pytest.mark.parametrize('spacing', [(1, 1, 1), (3, 1, 0.5)], ids=str)
def test_derive_axes_of_a_box(spacing):
    from empanada_amd.shapes import derive
    a, b, c = 4, 9, 6
    v = np.zeros((7, 12, 10), np.uint32)
    v[2:2 + a, 1:1 + b, 3:3 + c] = 2 ** 31 + 5
    d = derive(shape_ref.shape_table(v, z_base=11), spacing)
    assert d['label'][0] == 2 ** 31 + 5
    ext = np.array([a, b, c]) * np.array(spacing, float)
    np.testing.assert_allclose(d['axes'][0], np.sqrt(5.0 / 12.0) * np.sort(ext)[::-1], rtol=0, atol=1e-9)
    order = np.argsort(-ext, kind='stable')
    for i, ax in enumerate(order):
        e = np.zeros(3)
        e[ax] = 1
        np.testing.assert_allclose(np.abs(d['axis_vectors'][0, i]), e, atol=1e-9)
    np.testing.assert_allclose(d['centroid'][0], [11 + 2 + (a - 1) / 2, 1 + (b - 1) / 2, 3 + (c - 1) / 2])
    np.testing.assert_allclose(d['elongation'][0], np.sort(ext)[1] / np.sort(ext)[2])
    np.testing.assert_allclose(d['flatness'][0], np.sort(ext)[0] / np.sort(ext)[1])
    np.testing.assert_allclose(d['covariance'][0], np.diag(ext ** 2 / 12.0), atol=1e-9)


def test_derive_exact_for_large_indices():
    """central moments from sums near 2^60 keep their digits: a 2-voxel object far from the origin"""
    from empanada_amd.shapes import COLUMNS, derive
    z, y, x = 2 ** 20 - 2, 2 ** 20 - 1, 2 ** 20 - 1
    t = np.zeros((1, len(COLUMNS)), np.int64)
    t[0, :11] = [1, 2, 2 * z + 1, 2 * y, 2 * x, z * z + (z + 1) ** 2, 2 * y * y, 2 * x * x, (2 * z + 1) * y, (2 * z + 1) * x,
                 2 * y * x]
    d = derive(t)
    np.testing.assert_allclose(d['covariance'][0], np.diag([0.25 + 1 / 12, 1 / 12, 1 / 12]), atol=1e-12)


@pytest.mark.parametrize('dtype', [np.uint8, np.uint32])
def test_merge_of_the_blocks_is_the_whole(dtype):
    from empanada_amd.shapes import merge_tables
    vol = planted_volume((11, 9, 14), dtype, seed=3)
    whole = shape_ref.shape_table(vol, z_base=5)
    cuts = [0, 1, 4, 5, 9, 11]
    parts = [shape_ref.shape_table(vol[a:b], below=vol[a - 1] if a else None, above=vol[b] if b < 11 else None,
                                   z_base=5 + a) for a, b in zip(cuts[:-1], cuts[1:])]
    for order in ([0, 1, 2, 3, 4], [4, 2, 0, 3, 1]):
        got = merge_tables([parts[i] for i in order])
        assert got.dtype == np.int64 and np.array_equal(got, whole)
    assert merge_tables([]).shape == (0, 26)
    # without the neighbour slices the blocks do not add up: the halo is part of the definition
    bare = merge_tables([shape_ref.shape_table(vol[a:b], z_base=5 + a) for a, b in zip(cuts[:-1], cuts[1:])])
    assert not np.array_equal(bare, whole)
    # the identities the table is built to keep
    assert np.array_equal(whole[:, 11], _faces(vol, 2)) and np.array_equal(whole[:, 13], _faces(vol, 1))
    assert np.array_equal(whole[:, 19], _faces(vol, 0))


def _faces(vol, axis):
    """exposed faces normal to `axis` per label, ascending"""
    v = np.pad(vol.astype(np.int64), 1)
    core = v[1:-1, 1:-1, 1:-1]
    n = (np.roll(v, 1, axis)[1:-1, 1:-1, 1:-1] != core).astype(np.int64) + (np.roll(v, -1, axis)[1:-1, 1:-1, 1:-1] != core)
    labels = np.unique(core[core != 0])
    return np.array([n[core == k].sum() for k in labels], np.int64)


def test_argument_errors():
    from empanada_amd.shapes import check, crofton_weights, derive
    assert check(None) is None and check(True) == (1.0, 1.0, 1.0) and check((3, 1, 0.5)) == (3.0, 1.0, 0.5)
    assert check(np.array([2, 1, 1])) == (2.0, 1.0, 1.0)
    for bad in (False, 0, 1, 'abc', (1, 1), (1, 1, 0), (1, -1, 1), (1, 1, float('nan')), (1, 1, float('inf')),
                (True, 1, 1), ('1', 1, 1), [1, 2, 3, 4]):
        with pytest.raises(ValueError, match='shapes must be'):
            check(bad)
    t = np.zeros((0, 26), np.int64)
    d = derive(t)
    assert d['label'].shape == (0,) and d['axes'].shape == (0, 3) and d['axis_vectors'].shape == (0, 3, 3)
    for bad in ((1, 1), (0, 1, 1), 'xyz', None, (1, 1, float('nan'))):
        with pytest.raises(ValueError, match='spacing'):
            derive(t, bad)
        with pytest.raises(ValueError, match='spacing'):
            crofton_weights(bad)
    with pytest.raises(ValueError, match='table'):
        derive(np.zeros((2, 14), np.int64))
    with pytest.raises(ValueError, match='table'):
        derive(np.zeros((2, 26), np.float64))


def test_infer_volume_refuses_a_bad_shapes_argument_before_any_gpu_work():
    from empanada_amd.inference.driver import infer_volume
    with pytest.raises(ValueError, match='shapes must be'):
        infer_volume(None, np.zeros((2, 2, 2), np.uint8), norms=None, labels=[1], shapes=(1, 1))
