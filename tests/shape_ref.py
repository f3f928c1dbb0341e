"""A numpy restatement of the shape table (include/emp_hip.h, E11) that shares nothing with the kernel: no neighbourhood
mask and no ownership masks.  The lattice corners and edges an object touches are listed cell by cell for every voxel,
and the owner of a cell is the first voxel of the label around it, found by sorting; the intercept ends are shifted
comparisons; the moments are np.add.at over the voxels."""
import numpy as np

N_COL = 26
# direction k of cross_k: the 13 offsets above (0, 0, 0) in (z, y, x) order, written out
DIRS = [(0, 0, 1), (0, 1, -1), (0, 1, 0), (0, 1, 1), (1, -1, -1), (1, -1, 0), (1, -1, 1), (1, 0, -1), (1, 0, 0), (1, 0, 1),
        (1, 1, -1), (1, 1, 0), (1, 1, 1)]


def _unsigned(a):
    a = np.asarray(a)
    if a.dtype == np.int32:
        a = a.view(np.uint32)
    return a.astype(np.int64)


def _owned(lab, order, counted, cells, n_labels, rows):
    """per label the cells whose first voxel (smallest `order`) among those of the label that touch it is `counted`.
    lab / order / counted: per voxel; cells: list of per-voxel cell ids"""
    ids = np.concatenate(cells)
    k = len(cells)
    lab_k, order_k, counted_k, rows_k = np.tile(lab, k), np.tile(order, k), np.tile(counted, k), np.tile(rows, k)
    s = np.lexsort((order_k, ids, lab_k))
    first = np.ones(len(s), bool)
    first[1:] = (lab_k[s][1:] != lab_k[s][:-1]) | (ids[s][1:] != ids[s][:-1])
    take = s[first]
    out = np.zeros(n_labels, np.int64)
    np.add.at(out, rows_k[take][counted_k[take]], 1)
    return out


def shape_table(vol, below=None, above=None, z_base=0):
    """(n, 26) int64: the table of E11 for the (D, H, W) block `vol` with its optional neighbour slices"""
    vol = _unsigned(vol)
    D, H, W = vol.shape
    P = np.zeros((D + 2, H + 2, W + 2), np.int64)
    P[1:-1, 1:-1, 1:-1] = vol
    if below is not None:
        P[0, 1:-1, 1:-1] = _unsigned(below)
    if above is not None:
        P[-1, 1:-1, 1:-1] = _unsigned(above)
    labels = np.unique(vol[vol != 0])
    out = np.zeros((len(labels), N_COL), np.int64)
    out[:, 0] = labels
    if not len(labels):
        return out
    # every non-zero voxel of the padded block, the halo slices included: they can own a cell before a voxel of the block
    zz, yy, xx = np.nonzero(P)
    lab = P[zz, yy, xx]
    known = np.isin(lab, labels)                       # a label of the halo alone has no row
    zz, yy, xx, lab = zz[known], yy[known], xx[known], lab[known]
    rows = np.searchsorted(labels, lab)
    core = (zz >= 1) & (zz <= D)
    order = (zz * (H + 2) + yy) * (W + 2) + xx
    cz, cy, cx, cl, cr = zz[core], yy[core], xx[core], lab[core], rows[core]
    gz, gy, gx = cz - 1 + int(z_base), cy - 1, cx - 1
    for col, val in ((1, np.ones_like(gz)), (2, gz), (3, gy), (4, gx), (5, gz * gz), (6, gy * gy), (7, gx * gx),
                     (8, gz * gy), (9, gz * gx), (10, gy * gx)):
        np.add.at(out[:, col], cr, val)
    for k, (dz, dy, dx) in enumerate(DIRS):
        ends = (P[cz + dz, cy + dy, cx + dx] != cl).astype(np.int64) + (P[cz - dz, cy - dy, cx - dx] != cl)
        np.add.at(out[:, 11 + k], cr, ends)
    # lattice points: voxel (z, y, x) of the padded block spans the points (z .. z + 1, y .. y + 1, x .. x + 1)
    ny, nx = H + 3, W + 3
    corners = [((zz + a) * ny + yy + b) * nx + xx + c for a in (0, 1) for b in (0, 1) for c in (0, 1)]
    out[:, 24] = _owned(lab, order, core, corners, len(labels), rows)
    # an edge is its lower end point and its axis
    edges = []
    for axis in range(3):
        for a in (0, 1):
            for b in (0, 1):
                off = [a, b]
                off.insert(axis, 0)
                point = ((zz + off[0]) * ny + yy + off[1]) * nx + xx + off[2]
                edges.append(point * 3 + axis)
    out[:, 25] = _owned(lab, order, core, edges, len(labels), rows)
    return out


def euler(table):
    t = np.asarray(table, np.int64)
    faces = 3 * t[:, 1] + (t[:, 19] + t[:, 13] + t[:, 11]) // 2
    return t[:, 24] - t[:, 25] + faces - t[:, 1]


# ------------------------------------------------------------------------------------------ volumes the tests share
def ball(r, centre=None, label=1, dtype=np.uint32):
    n = 2 * int(np.ceil(r)) + 3
    c = (n - 1) / 2.0 if centre is None else centre
    g = np.indices((n, n, n)).astype(np.float64)
    c = np.broadcast_to(np.asarray(c, np.float64), (3,))
    d2 = sum((g[i] - c[i]) ** 2 for i in range(3))
    return np.where(d2 <= r * r, label, 0).astype(dtype)


def torus(R, r, n, axis=0, label=1, dtype=np.uint32):
    """a solid torus around `axis` through the middle of an n^3 volume"""
    g = np.indices((n, n, n)).astype(np.float64) - (n - 1) / 2.0
    along = g[axis]
    a, b = [g[i] for i in range(3) if i != axis]
    d2 = (np.sqrt(a * a + b * b) - R) ** 2 + along ** 2
    return np.where(d2 <= r * r, label, 0).astype(dtype)


def planted_objects(dtype=np.uint32):
    """(24, 40, 72): a ball, a solid torus and a bar of three labels, apart from each other, without cavities"""
    v = np.zeros((24, 40, 72), dtype)
    b = ball(7, label=5, dtype=dtype)                                   # 17^3
    v[3:20, 2:19, 2:19] = b
    t = torus(7.0, 2.6, 23, axis=0, label=9, dtype=dtype)               # 23^3, the ring in the (y, x) plane
    v[0:23, 14:37, 24:47] = np.maximum(v[0:23, 14:37, 24:47], t)
    v[10:13, 5:8, 50:71] = 200
    return v
