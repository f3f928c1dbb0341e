"""Shape descriptors of a labelled volume: a Crofton surface area and sphericity, the Euler number and the inertia
ellipsoid of every label.

The reference stops at the labelled volume; its users run MorphoLibJ's "Analyze Regions 3D" or regionprops on a CPU
afterwards, object by object.  The table is defined in include/emp_hip.h (E11) and read on the device by
_hip.shape_labels (csrc/emp_label_shape.hip), slab by slab, rank by rank: one row of 26 int64 per distinct non-zero
label, ascending by label, the columns being COLUMNS.  Every column after the label is a sum of integers over the
label's voxels, so tables of the z-blocks of a volume -- each taken with its true neighbour slices -- merge into the
table of the whole (`merge_tables`), whatever the partition and the order.  `derive` turns a table into physical
quantities on the host.
"""
import numpy as np
import torch

from .tables import (_labels_to_device, bits, gather_keyed, merge_keyed, volume_device, volume_slabs,
                     volume_table)

__all__ = ['COLUMNS', 'DIRECTIONS', 'merge_tables', 'gather_tables', 'volume_shapes', 'check', 'crofton_weights',
           'derive']

COLUMNS = (('label', 'voxels', 'sum_z', 'sum_y', 'sum_x', 'sum_zz', 'sum_yy', 'sum_xx', 'sum_zy', 'sum_zx', 'sum_yx')
           + tuple(f'cross_{k}' for k in range(13)) + ('corners', 'edges'))
_SUM = list(range(1, len(COLUMNS)))
_CROSS = COLUMNS.index('cross_0')
# direction k of cross_k as (dz, dy, dx): the 13 offsets above (0, 0, 0) in (z, y, x) order (E8's edge codes)
DIRECTIONS = tuple((p // 9 - 1, (p // 3) % 3 - 1, p % 3 - 1) for p in range(14, 27))


def merge_tables(tables):
    """Merge of shape tables ((n, 26) int64 each, of a volume's z-blocks or of the ranks' slabs): one row per distinct
    label, ascending by label, every other column added.  numpy in, numpy out; with any torch tensor among them the
    result is a torch table on that tensor's device.  No tables, or empty ones, give a (0, 26) table."""
    return merge_keyed(tables, len(COLUMNS), [0], _SUM)


def gather_tables(table, group=None):
    """The ranks' tables merged: every rank of `group` passes the table of its own slab and receives the table of all of
    them.  Without an initialised process group the table comes back merged with itself, i.e. sorted."""
    return gather_keyed(table, len(COLUMNS), merge_tables, group)


def volume_shapes(labels, *, slab_rows=None, group=None):
    """The shape table of a label volume (D, H, W) as an (n, 26) int64 numpy array: `labels` is a numpy array, a tensor
    or anything that has a shape and can be sliced along axis 0 (a ZarrV2Array, say).  Every slab of slab_rows slices
    goes to the device and through _hip.shape_labels together with the slices next to it, which stand for what lies
    outside the slab; slab_rows=None takes a device tensor whole and host data in slabs of about 2^27 voxels.  With
    `group` the ranks' tables are merged too -- every rank passes a volume of its own and all receive the merge; ranks
    that hold the z-slabs of ONE volume must hand each slab its neighbour slices themselves (_hip.shape_labels' below /
    above, as infer_volume does) and then call gather_tables."""
    from . import _hip
    _hip.require_gpu()
    if len(labels.shape) != 3:
        raise ValueError(f"volume_shapes: labels must be (D, H, W), got {tuple(labels.shape)}")
    dev, resident = volume_device(labels)
    tables, below = [], None
    for z, z1, _, hi in volume_slabs("volume_shapes", labels.shape, slab_rows, resident, halo=1):
        # one upload covers the slab and the slice above it; the slice below is kept from the slab before
        part = _labels_to_device(labels[z:hi], dev)
        slab = part[:z1 - z]
        above = part[z1 - z] if hi > z1 else None
        if slab.numel():
            tables.append(_hip.shape_labels(slab, below=below, above=above, z_base=z))
        if slab.shape[0]:                   # a copy of one slice, so that the slab itself can go (as int32: same bits)
            below = bits(slab[-1]).clone().view(slab.dtype)
        del part, slab, above
    return volume_table(tables, len(COLUMNS), merge_tables, gather_tables, group, dev)


def _spacing(who, spacing):
    bad = ValueError(f"{who}: spacing must be three positive numbers (sz, sy, sx), got {spacing!r}")
    if isinstance(spacing, (bool, np.bool_, str, bytes)):
        raise bad
    try:
        values = list(spacing)
    except TypeError:
        raise bad from None
    import numbers
    if len(values) != 3 or any(isinstance(v, (bool, np.bool_)) or not isinstance(v, numbers.Real) for v in values):
        raise bad
    values = tuple(float(v) for v in values)
    if not all(np.isfinite(v) and v > 0 for v in values):
        raise bad
    return values


def check(shapes):
    """infer_volume's `shapes` argument -> None or the voxel spacing (sz, sy, sx): None = off, True = (1, 1, 1), or three
    positive numbers; anything else is a ValueError"""
    if shapes is None:
        return None
    if shapes is True:
        return (1.0, 1.0, 1.0)
    try:
        return _spacing("shapes", shapes)
    except ValueError:
        raise ValueError("shapes must be None, True or a voxel spacing (sz, sy, sx) of three positive numbers, got "
                         f"{shapes!r}") from None


def crofton_weights(spacing=(1.0, 1.0, 1.0)):
    """The weights of the 13 lattice directions (DIRECTIONS) in the Crofton estimate of a surface area, for a voxel of
    `spacing` = (sz, sy, sx): the areas of the spherical Voronoi cells of the 26 unit vectors d * spacing / |d * spacing|,
    divided by 4 pi, with the cells of +d and -d added.  13 float64 that sum to 1; for a cubic voxel the constants of
    Ohser and Muecklich, 0.0915558 (axes), 0.0739613 (face diagonals), 0.0703913 (body diagonals)."""
    from scipy.spatial import SphericalVoronoi
    s = np.array(_spacing("crofton_weights", spacing))
    d = np.array(DIRECTIONS, dtype=np.float64) * s
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    areas = SphericalVoronoi(np.concatenate([d, -d]), radius=1.0, center=np.zeros(3)).calculate_areas()
    return (areas[:13] + areas[13:]) / (4.0 * np.pi)


def derive(table, spacing=(1.0, 1.0, 1.0)):
    """Physical quantities of a shape table ((n, 26) int64, numpy or torch) for a voxel of `spacing` = (sz, sy, sx), in
    float64 on the host; no GPU is needed.  Returns a dict of numpy arrays:
        label, voxels   table[:, 0], table[:, 1]
        volume          voxels * v, v = sz * sy * sx
        centroid        (n, 3): (sum_z, sum_y, sum_x) / voxels, in voxel indices
        surface_area    2 * sum_k w_k * cross_k * v / |d_k * spacing|, w = crofton_weights(spacing): the Crofton
                        estimate from the intercepts along 13 directions -- within about 2 % for a digitised ball of 6
                        voxels radius or more, where the count of exposed faces (measurements.derive) is 50 % above
        sphericity      pi^(1/3) * (6 * volume)^(2/3) / surface_area: 1 for a ball, less for anything else
        euler           corners - edges + faces - voxels, faces = 3 * voxels + (cross_8 + cross_2 + cross_0) / 2: the
                        Euler number of the object as a 26-connected set with 6-connected background (int64)
        tunnels         1 - euler (int64).  This is the number of tunnels (loops of a network) only for ONE 26-connected
                        component without cavities, i.e. after split_objects=26 and fill_holes=True; in general euler =
                        components - tunnels + cavities and the three cannot be told apart from it
        covariance      (n, 3, 3), zyx: the central second moments of the voxel centres in physical units, plus
                        spacing^2 / 12 on the diagonal for the voxel's own extent
        axes            (n, 3): the semi-axes sqrt(5 * eigenvalue) of the solid ellipsoid with that covariance, descending
        axis_vectors    (n, 3, 3): axis_vectors[i, j] is the unit vector (z, y, x) of axes[i, j]
        elongation      axes[:, 1] / axes[:, 0]
        flatness        axes[:, 2] / axes[:, 1]
    The second-order sums of the table are exact only below 2^63 (always at 1024^3; in general while the largest index
    squared times the voxels of the label stays below 2^63); an overflow is not detected, here or on the device."""
    if isinstance(table, torch.Tensor):
        table = table.cpu().numpy()
    t = np.asarray(table)
    if t.dtype.kind not in 'iu' or t.ndim != 2 or t.shape[1] != len(COLUMNS):
        raise ValueError(f"derive: expected an (n, {len(COLUMNS)}) integer table, got {t.dtype} {t.shape}")
    t = t.astype(np.int64)
    sp = np.array(_spacing("derive", spacing))
    v = float(sp[0] * sp[1] * sp[2])
    voxels = t[:, 1]
    n = voxels.astype(np.float64)
    cross = t[:, _CROSS:_CROSS + 13]
    length = np.linalg.norm(np.array(DIRECTIONS, dtype=np.float64) * sp, axis=1)
    area = 2.0 * (cross.astype(np.float64) * (crofton_weights(sp) * v / length)).sum(axis=1)
    volume = n * v
    faces = 3 * voxels + (cross[:, 8] + cross[:, 2] + cross[:, 0]) // 2
    euler = t[:, 24] - t[:, 25] + faces - voxels
    with np.errstate(divide='ignore', invalid='ignore'):
        centroid = t[:, 2:5] / n[:, None]
        # central moments from exact integers: n * sum_ab - sum_a * sum_b, formed in Python integers where int64 would overflow
        second = np.empty((len(t), 3, 3), np.float64)
        for (a, b), col in (((0, 0), 5), ((1, 1), 6), ((2, 2), 7), ((0, 1), 8), ((0, 2), 9), ((1, 2), 10)):
            num = _exact_central(voxels, t[:, col], t[:, 2 + a], t[:, 2 + b])
            second[:, a, b] = second[:, b, a] = num / (n * n) * sp[a] * sp[b]
        second[:, [0, 1, 2], [0, 1, 2]] += sp * sp / 12.0
        sphericity = np.pi ** (1.0 / 3.0) * (6.0 * volume) ** (2.0 / 3.0) / area
    lam, vec = np.linalg.eigh(second) if len(t) else (np.zeros((0, 3)), np.zeros((0, 3, 3)))
    lam, vec = lam[:, ::-1], np.swapaxes(vec, 1, 2)[:, ::-1]           # descending; rows are vectors
    axes = np.sqrt(5.0 * np.maximum(lam, 0.0))
    with np.errstate(divide='ignore', invalid='ignore'):
        elongation, flatness = axes[:, 1] / axes[:, 0], axes[:, 2] / axes[:, 1]
    return {'label': t[:, 0].copy(), 'voxels': voxels.copy(), 'volume': volume, 'centroid': centroid,
            'surface_area': area, 'sphericity': sphericity, 'euler': euler, 'tunnels': 1 - euler,
            'covariance': second, 'axes': axes, 'axis_vectors': np.ascontiguousarray(vec),
            'elongation': elongation, 'flatness': flatness}


def _exact_central(n, s_ab, s_a, s_b):
    """n * s_ab - s_a * s_b as float64, exactly rounded: in int64 where that cannot overflow, in Python integers otherwise"""
    big = max((int(np.abs(x).max()) if len(x) else 0) for x in (n, s_ab, s_a, s_b))
    if big < 2 ** 31:
        return (n * s_ab - s_a * s_b).astype(np.float64)
    return np.array([float(int(k) * int(ab) - int(a) * int(b)) for k, ab, a, b in zip(n, s_ab, s_a, s_b)], np.float64)
