"""numpy checker of the surface meshes (include/emp_hip.h, E7), written from the definition by another route than the
kernels: quads from shifted comparisons of the padded volume, vertices from np.unique over the quads' (label, corner)
pairs -- never from the eight-voxel rule -- and a float64 Taubin smoother over the quad edges."""
import numpy as np

# direction code -> (axis, step) of the face's normal
DIRECTIONS = [(0, -1), (0, 1), (1, -1), (1, 1), (2, -1), (2, 1)]
# direction code -> the four corners of the quad relative to its voxel (z, y, x), the header's table written out
WINDING = np.array([
    [(0, 0, 0), (0, 0, 1), (0, 1, 1), (0, 1, 0)],      # -z: o, o+ex, o+ey+ex, o+ey
    [(1, 0, 0), (1, 1, 0), (1, 1, 1), (1, 0, 1)],      # +z: o, o+ey, o+ey+ex, o+ex
    [(0, 0, 0), (1, 0, 0), (1, 0, 1), (0, 0, 1)],      # -y: o, o+ez, o+ez+ex, o+ex
    [(0, 1, 0), (0, 1, 1), (1, 1, 1), (1, 1, 0)],      # +y: o, o+ex, o+ex+ez, o+ez
    [(0, 0, 0), (0, 1, 0), (1, 1, 0), (1, 0, 0)],      # -x: o, o+ey, o+ez+ey, o+ez
    [(0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)],      # +x: o, o+ez, o+ez+ey, o+ey
], dtype=np.int64)
LAMBDA, MU = 0.5, -0.53


def faces_ref(vol, below=None, above=None):
    """every exposed face of every non-zero voxel of vol (D, H, W): (label uint64, voxel (n, 3) int64, code int64),
    in no particular order.  below / above: (H, W) slices that stand for z = -1 and z = D; all else outside reads 0"""
    vol = np.asarray(vol)
    D, H, W = vol.shape
    pad = np.zeros((D + 2, H + 2, W + 2), np.uint64)
    pad[1:-1, 1:-1, 1:-1] = vol
    if below is not None:
        pad[0, 1:-1, 1:-1] = below
    if above is not None:
        pad[-1, 1:-1, 1:-1] = above
    centre = pad[1:-1, 1:-1, 1:-1]
    labels, voxels, codes = [], [], []
    for code, (axis, step) in enumerate(DIRECTIONS):
        sl = [slice(1, -1)] * 3
        sl[axis] = slice(1 + step, pad.shape[axis] - 1 + step)
        exposed = (centre != 0) & (centre != pad[tuple(sl)])
        at = np.argwhere(exposed)
        labels.append(centre[exposed])
        voxels.append(at)
        codes.append(np.full(len(at), code, np.int64))
    return np.concatenate(labels), np.concatenate(voxels).reshape(-1, 3), np.concatenate(codes)


def corner_number(zyx, H, W):
    zyx = np.asarray(zyx, np.int64)
    return (zyx[..., 0] * (H + 1) + zyx[..., 1]) * (W + 1) + zyx[..., 2]


def emit_ref(vol, below=None, above=None, z_base=0, top=True):
    """what a slab contributes: (keys, qkeys, qdirs) -- keys: the sorted uint64 label << 32 | corner of every vertex on
    a corner plane the slab owns (z_base .. z_base + D - 1, and z_base + D with top); qkeys / qdirs: the slab's quads
    as label << 32 | lowest corner and direction code, in (z, y, x, code) order of the owning voxel.  The halo slices
    are meshed as voxels too (only the faces that their known neighbours decide can touch an owned plane), so that the
    vertices a label of the slab below leaves on the seam plane are there"""
    vol = np.asarray(vol)
    D, H, W = vol.shape
    if D == 0:                                                                  # an empty slab owns nothing
        return np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.int32)
    parts, first = [], 0
    if below is not None:
        parts.append(np.asarray(below)[None])
        first = 1
    parts.append(vol)
    if above is not None:
        parts.append(np.asarray(above)[None])
    ext = np.concatenate(parts)
    lab, vox, code = faces_ref(ext)
    vox = vox + np.array([z_base - first, 0, 0])
    corners = vox[:, None, :] + WINDING[code]                                   # (n, 4, 3)
    pair = (lab[:, None] << np.uint64(32)) | corner_number(corners, H, W).astype(np.uint64)
    owned = (corners[..., 0] >= z_base) & (corners[..., 0] < z_base + D + (1 if top else 0))
    keys = np.unique(pair[owned])
    mine = (vox[:, 0] >= z_base) & (vox[:, 0] < z_base + D)
    lab, vox, code, pair = lab[mine], vox[mine], code[mine], pair[mine]
    order = np.lexsort((code, vox[:, 2], vox[:, 1], vox[:, 0]))
    return keys, pair[order, 0], code[order].astype(np.int32)


def finish_ref(keys, qkeys, qdirs, H, W):
    """the mesh of sorted-or-not keys and quad records in z order: {'vertices', 'quads', 'objects'}"""
    keys = np.sort(np.asarray(keys, np.uint64))
    qkeys = np.asarray(qkeys, np.uint64)
    order = np.argsort(qkeys >> np.uint64(32), kind='stable')
    qkeys, qdirs = qkeys[order], np.asarray(qdirs, np.int64)[order]
    corner = (keys & np.uint64(0xffffffff)).astype(np.int64)
    plane = (H + 1) * (W + 1)
    vertices = np.stack([corner // plane, corner % plane // (W + 1), corner % (W + 1)], axis=1).astype(np.int32)
    o = (qkeys & np.uint64(0xffffffff)).astype(np.int64)
    rel = WINDING[qdirs] - WINDING[qdirs][:, :1]                                 # steps from the lowest corner
    want = ((qkeys >> np.uint64(32)) << np.uint64(32))[:, None] | (o[:, None] + corner_number(rel, H, W)).astype(np.uint64)
    if len(keys):
        idx = np.searchsorted(keys, want)
        found = (idx < len(keys)) & (keys[np.minimum(idx, len(keys) - 1)] == want)
        quads = np.where(found, idx, -1).astype(np.int32).reshape(-1, 4)
    else:
        quads = np.full((len(qkeys), 4), -1, np.int32)
    vlab, qlab = keys >> np.uint64(32), qkeys >> np.uint64(32)
    labels = np.unique(vlab)
    objects = np.stack([labels.astype(np.int64),
                        np.searchsorted(vlab, labels, 'left'), np.searchsorted(vlab, labels, 'right'),
                        np.searchsorted(qlab, labels, 'left'), np.searchsorted(qlab, labels, 'right')], axis=1).astype(np.int64)
    return {'vertices': vertices, 'quads': quads, 'objects': objects.reshape(-1, 5)}


def mesh_ref(vol):
    """the mesh of a whole volume"""
    vol = np.asarray(vol)
    keys, qkeys, qdirs = emit_ref(vol)
    return finish_ref(keys, qkeys, qdirs, vol.shape[1], vol.shape[2])


def neighbours_ref(vertices, quads):
    """(nv, 6) int32: the vertex one lattice step away per direction code over the quad edges, -1 = none"""
    vertices, quads = np.asarray(vertices, np.int64), np.asarray(quads, np.int64)
    nbr = np.full((len(vertices), 6), -1, np.int32)
    for j in range(4):
        a, b = quads[:, j], quads[:, (j + 1) % 4]
        d = vertices[b] - vertices[a]
        assert (np.abs(d).sum(axis=1) == 1).all(), "a quad edge that is no lattice step"
        axis = np.abs(d).argmax(axis=1)
        slot = 2 * axis + (d[np.arange(len(d)), axis] > 0)
        nbr[a, slot] = b
        nbr[b, slot ^ 1] = a
    return nbr


def taubin_ref(vertices, quads, iterations, lam=LAMBDA, mu=MU):
    """float64 Taubin smoothing over the quad edges"""
    p = np.asarray(vertices, np.float64).copy()
    nbr = neighbours_ref(vertices, quads)
    have = nbr >= 0
    n = np.maximum(have.sum(axis=1), 1)[:, None]
    for _ in range(iterations):
        for f in (lam, mu):
            m = np.where(have[:, :, None], p[np.maximum(nbr, 0)], 0.0).sum(axis=1) / n
            p = np.where(have.any(axis=1)[:, None], p + f * (m - p), p)
    return p


def det_sum(vertices, quads):
    """sum over the quads of det[p0, p1, p2] + det[p0, p2, p3]"""
    p = np.asarray(vertices, np.int64)[np.asarray(quads, np.int64)]              # (n, 4, 3)
    det = lambda a, b, c: np.einsum('ni,ni->n', a, np.cross(b, c))
    return int((det(p[:, 0], p[:, 1], p[:, 2]) + det(p[:, 0], p[:, 2], p[:, 3])).sum())


def random_volume(shape, n_labels=5, density=0.3, seed=0, dtype=np.uint32, big=False):
    """n_labels labels at the given density; big: the largest is >= 2^31 (uint32 only)"""
    rng = np.random.default_rng(seed)
    vol = np.where(rng.random(shape) < density, rng.integers(1, n_labels + 1, shape), 0).astype(dtype)
    if big:
        vol[vol == n_labels] = 2 ** 31 + 7
    return vol


def hand_cases():
    """name -> volume (uint32), the cases counted by hand in the tests"""
    one = np.zeros((3, 3, 3), np.uint32)
    one[1, 1, 1] = 7
    edge = np.zeros((3, 4, 4), np.uint32)
    edge[1, 1, 1] = edge[1, 2, 2] = 3
    corner = np.zeros((4, 4, 4), np.uint32)
    corner[1, 1, 1] = corner[2, 2, 2] = 3
    pair = np.zeros((3, 3, 4), np.uint32)
    pair[1, 1, 1], pair[1, 1, 2] = 4, 9
    eight = np.arange(1, 9, dtype=np.uint32).reshape(2, 2, 2)
    ends = np.zeros((3, 4, 5), np.uint32)
    ends[0, 0, 0] = ends[2, 3, 4] = 5
    full = np.full((2, 3, 4), 6, np.uint32)
    return {'one': one, 'edge': edge, 'corner': corner, 'pair': pair, 'eight': eight, 'ends': ends, 'full': full}
