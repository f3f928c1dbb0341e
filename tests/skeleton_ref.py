"""A numpy / scipy checker of the skeleton definition of include/emp_hip.h, E8: the predicates (scipy.ndimage.label on
the 3 x 3 x 3 block -- deliberately another method than the device's bit floods), the thinning schedule run
sequentially, the graph of a sparse label volume in plain numpy, and the topology numbers the thinning preserves."""
import numpy as np
from scipy import ndimage

# offset n of the 26: ascending (dz, dy, dx) from (-1, -1, -1), the centre skipped
OFFSETS = np.array([(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
                    if (dz, dy, dx) != (0, 0, 0)], dtype=np.int64)
UPPER = OFFSETS[13:]                                  # edge codes 0 .. 12
_S26 = np.ones((3, 3, 3), dtype=bool)
_S6 = ndimage.generate_binary_structure(3, 1)
_NORM1 = np.abs(OFFSETS).sum(1)
_cache = {}


def block_of(mask):
    """the 3 x 3 x 3 boolean block of a 26-bit mask, centre clear"""
    b = np.zeros((3, 3, 3), dtype=bool)
    for n in range(26):
        if (int(mask) >> n) & 1:
            b[tuple(OFFSETS[n] + 1)] = True
    return b


def classify(mask):
    """bit 0 simple, bit 1 isthmus"""
    mask = int(mask) & 0x3ffffff
    if mask in _cache:
        return _cache[mask]
    b = block_of(mask)
    c26 = ndimage.label(b, structure=_S26)[1]
    free = np.zeros((3, 3, 3), dtype=bool)
    for n in range(26):
        if _NORM1[n] <= 2 and not b[tuple(OFFSETS[n] + 1)]:
            free[tuple(OFFSETS[n] + 1)] = True
    lab = ndimage.label(free, structure=_S6)[0]
    faces = {int(lab[tuple(OFFSETS[n] + 1)]) for n in range(26) if _NORM1[n] == 1} - {0}
    t6 = len(faces)
    out = (1 if (c26 == 1 and t6 == 1) else 0) | (2 if c26 >= 2 else 0)
    _cache[mask] = out
    return out


def as_u32(vol):
    a = np.asarray(vol)
    if a.dtype == np.int32:
        return a.view(np.uint32)
    return a.astype(np.uint32)


def masks_at(obj, coords):
    """M of the voxels at coords (n, 3) of obj = alive ? label : 0, a (D, H, W) uint32 array"""
    p = np.pad(obj, 1)
    c = coords + 1
    own = p[c[:, 0], c[:, 1], c[:, 2]]
    m = np.zeros(len(coords), dtype=np.int64)
    for n, (dz, dy, dx) in enumerate(OFFSETS):
        m |= (p[c[:, 0] + dz, c[:, 1] + dy, c[:, 2] + dx] == own).astype(np.int64) << n
    return m


def thin(labels, z_base=0, max_iterations=None):
    """(S, iterations, deleted): the definition, run sub-field by sub-field.  max_iterations stops it early."""
    L = as_u32(labels)
    obj = L.copy()
    kept = np.zeros(L.shape, dtype=bool)
    it = total = 0
    if L.size == 0:
        return obj, 0, 0
    zz, yy, xx = np.meshgrid(*(np.arange(s) for s in L.shape), indexing='ij')
    field = (((zz + z_base) & 1) << 2) | ((yy & 1) << 1) | (xx & 1)
    while max_iterations is None or it < max_iterations:
        it += 1
        p = np.pad(obj, 1)
        inner = np.ones(L.shape, dtype=bool)
        for dz, dy, dx in ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)):
            inner &= p[1 + dz:1 + dz + L.shape[0], 1 + dy:1 + dy + L.shape[1], 1 + dx:1 + dx + L.shape[2]] == obj
        marked = (obj != 0) & ~inner
        deleted = 0
        for s in range(8):
            coords = np.argwhere((field == s) & marked & (obj != 0) & ~kept)
            if len(coords) == 0:
                continue
            distinct, inverse = np.unique(masks_at(obj, coords), return_inverse=True)
            cls = np.array([classify(m) for m in distinct])[inverse]
            k = coords[(cls & 2) != 0]
            kept[k[:, 0], k[:, 1], k[:, 2]] = True
            d = coords[cls == 1]
            obj[d[:, 0], d[:, 1], d[:, 2]] = 0
            deleted += len(d)
        total += deleted
        if deleted == 0:
            break
    return obj, it, total


def graph(skel, z_base=0):
    """{'vertices' (nv, 3) int32, 'degree', 'edges' (ne, 2) int32, 'objects' (n, 8) int64} of a sparse label volume"""
    S = as_u32(skel)
    coords = np.argwhere(S != 0)
    lab = S[coords[:, 0], coords[:, 1], coords[:, 2]].astype(np.int64)
    order = np.lexsort((coords[:, 2], coords[:, 1], coords[:, 0], lab))
    coords, lab = coords[order], lab[order]
    H, W = S.shape[1:]
    number = (coords[:, 0] * H + coords[:, 1]) * W + coords[:, 2]
    index = {(int(l), int(v)): i for i, (l, v) in enumerate(zip(lab, number))}
    m = masks_at(S, coords) if len(coords) else np.zeros(0, dtype=np.int64)
    degree = np.array([bin(int(v)).count('1') for v in m], dtype=np.int32)
    edges = []
    for i in range(len(coords)):
        for c in range(13):
            if (int(m[i]) >> (13 + c)) & 1:
                dz, dy, dx = UPPER[c]
                edges.append((i, index[(int(lab[i]), int(number[i] + (dz * H + dy) * W + dx))]))
    edges = np.array(edges, dtype=np.int32).reshape(-1, 2)
    objects = []
    elab = lab[edges[:, 0]]                           # ascending: the vertices were walked in their order
    for l in np.unique(lab):
        v = np.flatnonzero(lab == l)
        d = degree[v]
        objects.append((l, v[0], v[-1] + 1, np.searchsorted(elab, l, 'left'), np.searchsorted(elab, l, 'right'),
                        int((d == 0).sum()), int((d == 1).sum()), int((d >= 3).sum())))
    vertices = coords.astype(np.int32)
    vertices[:, 0] += z_base
    return {'vertices': vertices, 'degree': degree, 'edges': edges,
            'objects': np.array(objects, dtype=np.int64).reshape(-1, 8)}


def topology(vol):
    """{label: (26-components, 6-components of the padded complement)} of a label volume"""
    V = as_u32(vol)
    out = {}
    for l in np.unique(V):
        if l == 0:
            continue
        mask = V == l
        out[int(l)] = (ndimage.label(mask, structure=_S26)[1],
                       ndimage.label(~np.pad(mask, 1), structure=_S6)[1])
    return out


# ---------------------------------------------------------------------------------------------- the cases
def bar():
    v = np.zeros((20, 24, 40), dtype=np.uint8)
    v[6:13, 8:15, 3:37] = 1
    return v


def ball():
    z, y, x = np.ogrid[:20, :24, :40]
    return ((z - 10) ** 2 + (y - 12) ** 2 + (x - 20) ** 2 <= 64).astype(np.uint8)


def torus():
    z, y, x = np.ogrid[:20, :24, :40]
    return (((np.sqrt((y - 12.0) ** 2 + (x - 20.0) ** 2) - 8) ** 2 + (z - 10.0) ** 2) <= 9).astype(np.uint8)


def touching():
    v = np.zeros((20, 24, 40), dtype=np.uint8)
    v[5:12, 8:15, 10:17] = 1                         # two cubes that share a face
    v[5:14, 8:17, 17:26] = 2
    return v


def ypsilon():
    """three arms, three voxels thick, that meet at a tile corner: (8, 8, 64) lies inside the junction"""
    v = np.zeros((17, 18, 130), dtype=np.uint8)
    v[7:10, 7:10, 40:66] = 3
    for i in range(0, 50):
        y = 8 + i // 6
        v[7:10, max(0, y - 1):y + 2, 64 + i:66 + i] = 3
        z = 8 + i // 7
        v[max(0, z - 1):min(17, z + 2), 7 - i // 10:10 - i // 10, 64 + i:66 + i] = 3
    return v


def noise(shape, seed, threshold=0.52, sigma=1.5):
    """seeded smoothed noise, relabelled by 6-connected components: many thin, branching objects next to one another"""
    rng = np.random.default_rng(seed)
    f = ndimage.gaussian_filter(rng.random(shape), sigma, mode='constant', cval=0.5)
    f = (f - f.mean()) / (f.std() + 1e-12)
    lab, n = ndimage.label(f > (threshold - 0.5) * 4)
    return lab.astype(np.uint32)


def in_shape(case, shape):
    """the case cropped or zero-padded to `shape`"""
    out = np.zeros(shape, dtype=case.dtype)
    s = tuple(slice(0, min(a, b)) for a, b in zip(case.shape, shape))
    out[s] = case[s]
    return out
