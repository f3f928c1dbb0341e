"""CPU checkers for the separation of touching objects (include/emp_hip.h, E6): `grow_ref`, the restatement of the
geodesic growth as a synchronous level-by-level flood with numpy shifts; two independent statements of the same thing
to check it against (`grow_brute`: scipy's shortest paths over the same-label 6-graph; `grow_relax`: the 64-bit
min-relaxation in random order); `separate_ref`, the whole repair from scipy and numpy; and the volumes the tests share.
"""
import numpy as np
from scipy import ndimage

NONE = (1 << 64) - 1
INF = np.iinfo(np.int64).max


def _u32(a):
    a = np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.int32 else a.astype(np.uint32)


def shifted(a, axis, step):
    """a moved by `step` (+1 / -1) along `axis`, zeros moving in: out[.., i, ..] = a[.., i - step, ..]"""
    out = np.zeros_like(a)
    src = [slice(None)] * a.ndim
    dst = [slice(None)] * a.ndim
    if step > 0:
        src[axis], dst[axis] = slice(0, a.shape[axis] - 1), slice(1, None)
    else:
        src[axis], dst[axis] = slice(1, None), slice(0, a.shape[axis] - 1)
    out[tuple(dst)] = a[tuple(src)]
    return out


def grow_ref(lab, seeds):
    """(owner uint32, dist int64 with INF = not reached): level k takes every unreached labelled voxel with a face
    neighbour of its own label at level k - 1 and gives it the largest owner among those neighbours"""
    lab, seeds = _u32(lab), _u32(seeds)
    owner = np.where(lab != 0, seeds, 0).astype(np.uint32)
    dist = np.where(owner != 0, 0, INF).astype(np.int64)
    front = owner != 0
    k = 0
    while front.any():
        k += 1
        cand = np.zeros_like(owner)
        for axis in range(3):
            for step in (1, -1):
                ok = shifted(front, axis, step) & (shifted(lab, axis, step) == lab) & (lab != 0) & (dist == INF)
                cand = np.maximum(cand, np.where(ok, shifted(owner, axis, step), 0).astype(np.uint32))
        front = cand != 0
        owner[front] = cand[front]
        dist[front] = k
    return owner, dist


def _graph(lab):
    from scipy.sparse import coo_matrix
    lab = _u32(lab)
    idx = np.arange(lab.size).reshape(lab.shape)
    rows, cols = [], []
    for axis in range(3):
        a = [slice(None)] * 3
        b = [slice(None)] * 3
        a[axis], b[axis] = slice(0, -1), slice(1, None)
        same = (lab[tuple(a)] == lab[tuple(b)]) & (lab[tuple(a)] != 0)
        rows.append(idx[tuple(a)][same])
        cols.append(idx[tuple(b)][same])
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    return coo_matrix((np.ones(len(rows)), (rows, cols)), shape=(lab.size, lab.size)).tocsr()


def grow_brute(lab, seeds):
    """the same from all-pairs shortest paths: g(v) is the smallest path length to a seed voxel, and the owner the
    largest seed id among the seed voxels at exactly that length (every shortest path to a nearest seed descends
    through the levels, and every descending path is one)"""
    from scipy.sparse.csgraph import shortest_path
    lab, seeds = _u32(lab), _u32(seeds)
    seeds = np.where(lab != 0, seeds, 0).astype(np.uint32)
    at = np.flatnonzero(seeds.ravel())
    owner = np.zeros(lab.size, np.uint32)
    dist = np.full(lab.size, INF, np.int64)
    if len(at):
        d = shortest_path(_graph(lab), method='D', directed=False, unweighted=True, indices=at)
        g = d.min(axis=0)
        reached = np.isfinite(g)
        ids = np.where(d == g[None, :], seeds.ravel()[at][:, None], 0).max(axis=0)
        owner[reached] = ids[reached]
        dist[reached] = g[reached].astype(np.int64)
    return owner.reshape(lab.shape), dist.reshape(lab.shape)


def grow_relax(lab, seeds, rng):
    """the same as the fixed point of key(v) = min over same-label face neighbours of key(u) + (1 << 32), keys
    dist << 32 | ~owner with the seeds fixed, started from all-ones and updated one voxel at a time in random order"""
    lab, seeds = _u32(lab), _u32(seeds)
    D, H, W = lab.shape
    key = {}
    for v in np.ndindex(*lab.shape):
        s = int(seeds[v]) if lab[v] else 0
        key[v] = (~s & 0xffffffff) if s else NONE
    todo = [v for v in np.ndindex(*lab.shape) if lab[v] and key[v] == NONE]
    changed = True
    while changed:
        changed = False
        for i in rng.permutation(len(todo)):
            v = todo[i]
            best = key[v]
            for axis in range(3):
                for step in (-1, 1):
                    u = list(v)
                    u[axis] += step
                    u = tuple(u)
                    if 0 <= u[axis] < lab.shape[axis] and lab[u] == lab[v] and key[u] != NONE:
                        best = min(best, key[u] + (1 << 32))
            if best < key[v]:
                key[v], changed = best, True
    owner = np.zeros(lab.shape, np.uint32)
    dist = np.full(lab.shape, INF, np.int64)
    for v, k in key.items():
        if k != NONE:
            owner[v], dist[v] = ~k & 0xffffffff, k >> 32
    return owner, dist


SIX = ndimage.generate_binary_structure(3, 1)


def erode_ref(lab, r2, sampling=(1, 1, 1)):
    lab = _u32(lab)
    out = np.zeros_like(lab)
    for l in np.unique(lab[lab != 0]):
        m = lab == l
        d2 = np.rint(ndimage.distance_transform_edt(m, sampling) ** 2).astype(np.int64)
        out[m & (d2 > r2)] = l
    return out


def cores_ref(eroded):
    """rows (label, voxels, first flat index) of the 6-connected components of every label, ascending by first, and
    the volume of their 1-based row numbers"""
    rows, where = [], []
    for l in np.unique(eroded[eroded != 0]):
        cc, n = ndimage.label(eroded == l, SIX)
        for k in range(1, n + 1):
            m = cc == k
            rows.append((int(l), int(m.sum()), int(np.flatnonzero(m.ravel())[0])))
            where.append(m)
    order = sorted(range(len(rows)), key=lambda i: rows[i][2])
    ids = np.zeros(eroded.shape, np.int64)
    for new, i in enumerate(order):
        ids[where[i]] = new + 1
    return np.asarray([rows[i] for i in order], np.int64).reshape(-1, 3), ids


def separate_ref(lab, r2, min_core=1, sampling=(1, 1, 1), max_label=None):
    """(new volume, stats without 'sweeps', owners): erode per label with scipy's exact transform, label the cores with
    the 6-structure, seed the labels with two or more cores of at least min_core voxels, grow_ref, separation.plan"""
    from empanada_amd import separation as SP
    lab = np.asarray(lab)
    wide = _u32(lab)
    rows, ids = cores_ref(erode_ref(wide, r2, sampling))
    big = rows[:, 1] >= min_core
    labels, counts = np.unique(rows[big, 0], return_counts=True)
    seed = big & np.isin(rows[:, 0], labels[counts >= 2])
    number = np.zeros(len(rows) + 1, np.uint32)
    number[1:][seed] = 1 + np.arange(int(seed.sum()))
    seeds = number[ids]
    owner, _ = grow_ref(wide, seeds)
    present = np.unique(wide[wide != 0])
    n = int(seed.sum())
    sizes = np.bincount(owner.ravel(), minlength=n + 1)[1:n + 1]
    pieces = np.stack([rows[seed, 0], 1 + np.arange(n), sizes], axis=1) if n else np.zeros((0, 3), np.int64)
    top = int(present.max()) if len(present) else 0
    if max_label is None:
        max_label = 255 if lab.dtype == np.uint8 else 2 ** 32 - 1
    lut, stats = SP.plan(pieces, top, max_label)
    new = np.where(owner != 0, lut[owner], wide).astype(lab.dtype if lab.dtype != np.int32 else np.uint32)
    stats = dict(r2=int(r2), min_core=int(min_core), sampling=tuple(sampling), objects_in=len(present), **stats)
    assert stats['voxels_moved'] == int((new != wide).sum())
    return new, stats, owner


# ------------------------------------------------------------------------------------------------------ shared volumes
def ball(vol, centre, r, value):
    z, y, x = np.ogrid[:vol.shape[0], :vol.shape[1], :vol.shape[2]]
    vol[(z - centre[0]) ** 2 + (y - centre[1]) ** 2 + (x - centre[2]) ** 2 <= r * r] = value
    return vol


def dumbbell(dtype=np.uint32, label=5, shape=(17, 17, 41), centres=((8, 8, 8), (8, 8, 32)), r=6, neck=2, second_r=None):
    """two balls joined by a cylinder along x, all under one label"""
    vol = np.zeros(shape, dtype)
    ball(vol, centres[0], r, label)
    ball(vol, centres[1], r if second_r is None else second_r, label)
    z, y, x = np.ogrid[:shape[0], :shape[1], :shape[2]]
    cyl = ((z - centres[0][0]) ** 2 + (y - centres[0][1]) ** 2 <= neck * neck) & (x >= centres[0][2]) & (x <= centres[1][2])
    vol[cyl] = label
    return vol


def path_volume(shape, path, label=7, dtype=np.uint32):
    """a corridor one voxel wide: consecutive voxels of `path` are face neighbours and no others are"""
    vol = np.zeros(shape, dtype)
    assert len(set(path)) == len(path)
    for a, b in zip(path[:-1], path[1:]):
        assert sum(abs(p - q) for p, q in zip(a, b)) == 1
    for v in path:
        vol[v] = label
    seeds = np.zeros(shape, np.uint32)
    seeds[path[0]], seeds[path[-1]] = 1, 2
    return vol, seeds


def serpentine_flat():
    """(3, 9, 40): rows y = 0, 2, .. 8 of slice 1 joined at alternating ends -- 204 voxels, a seed at either end"""
    path = []
    for i, y in enumerate(range(0, 9, 2)):
        xs = range(40) if i % 2 == 0 else range(39, -1, -1)
        path += [(1, y, x) for x in xs]
        if y < 8:
            path.append((1, y + 1, path[-1][2]))
    return path_volume((3, 9, 40), path)


def serpentine_tall():
    """(33, 9, 70): columns along z at y = 3, x = 0, 2, .. 68 joined at alternating ends, then along y to row 8 and back
    along x at z = 32 or 0 -- it crosses every border of the 8 x 8 x 64 tiles and every z-seam many times"""
    path = []
    for i, x in enumerate(range(0, 70, 2)):
        zs = range(33) if i % 2 == 0 else range(32, -1, -1)
        path += [(z, 3, x) for z in zs]
        if x < 68:
            path.append((path[-1][0], 3, x + 1))
    z_end = path[-1][0]
    path += [(z_end, y, 68) for y in range(4, 9)]
    path += [(z_end, 8, x) for x in range(67, 9, -1)]
    return path_volume((33, 9, 70), path)


def random_case(shape, seed, n_labels=3, background=0.2, density=0.05, dtype=np.uint32, big=False):
    """random labels (a few values, `background` zeros) and seeds (`density` of the voxels, background included)"""
    rng = np.random.default_rng(seed)
    values = np.asarray([3, 4, 200, 77][:n_labels], np.uint32)
    if big and dtype != np.uint8:
        values[:2] = (2 ** 31 + 5, 2 ** 32 - 1)
    lab = np.where(rng.random(shape) < background, 0, values[rng.integers(0, n_labels, shape)]).astype(dtype)
    if density == 'one':
        seeds = np.zeros(shape, np.uint32)
        if lab.size:
            seeds.ravel()[int(rng.integers(lab.size))] = 9
    else:
        ids = rng.integers(1, 50, shape).astype(np.uint32)
        if big:
            ids = np.where(ids % 3 == 0, np.uint32(2 ** 32 - 1), np.where(ids % 3 == 1, ids + np.uint32(2 ** 31), ids))
        seeds = np.where(rng.random(shape) < density, ids, 0).astype(np.uint32)
    return lab, seeds
