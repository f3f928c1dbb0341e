"""A numpy restatement of the contact table of include/emp_hip.h, E9, and the builders of the test cases.

`contact_table` follows the definition and nothing of the kernel: the ball is listed in ascending (d2, dz, dy, dx), B is
compared once per offset as a shifted view of a zero-padded copy (nothing lies outside the volume, and 0 is never a
partner), every (voxel, b) pair keeps the d2 of the first offset that shows it, and the rows are sums and minima over
the pairs.  tests/test_contacts_host.py checks it against scipy's edt, object by object, and against cases counted by
hand.
"""
import math

import numpy as np

COLS = 10


def as_u32(x):
    """the labels as uint32, the bits of an int32 taken as they are"""
    x = np.asarray(x)
    if x.dtype == np.int32:
        return x.view(np.uint32)
    return x.astype(np.uint32)


def ball(r2, sampling=(1, 1, 1)):
    """[(d2, dz, dy, dx)] ascending"""
    az, ay, ax = sampling
    root = math.isqrt(r2)
    out = []
    for dz in range(-(root // az), root // az + 1):
        for dy in range(-(root // ay), root // ay + 1):
            for dx in range(-(root // ax), root // ax + 1):
                d2 = (az * dz) ** 2 + (ay * dy) ** 2 + (ax * dx) ** 2
                if d2 <= r2:
                    out.append((d2, dz, dy, dx))
    return sorted(out)


def contact_table(A, B=None, r2=1, sampling=(1, 1, 1), z_base=0, below=None, above=None, same=None):
    """(n, 10) int64: the table of E9 for the slab A against B (None: A itself), B continued by the stacks below / above;
    same=True with a B: the same-volume rule b != a against a B that is A seen through another window"""
    same = B is None if same is None else same
    if B is None:
        B = A
    A = as_u32(A)
    Bv = as_u32(B)
    assert A.shape == Bv.shape and A.ndim == 3
    D, H, W = A.shape
    offsets = ball(r2, sampling)
    hz, hy, hx = (math.isqrt(r2) // a for a in sampling)
    pad = np.zeros((D + 2 * hz, H + 2 * hy, W + 2 * hx), np.uint32)
    pad[hz:hz + D, hy:hy + H, hx:hx + W] = Bv
    if below is not None and len(below):
        lo = as_u32(below)
        assert len(lo) <= hz
        pad[hz - len(lo):hz, hy:hy + H, hx:hx + W] = lo
    if above is not None and len(above):
        hi = as_u32(above)
        assert len(hi) <= hz
        pad[hz + D:hz + D + len(hi), hy:hy + H, hx:hx + W] = hi
    if A.size == 0:
        return np.zeros((0, COLS), np.int64)
    vox = np.arange(A.size, dtype=np.uint64).reshape(A.shape)
    keys = np.zeros(0, np.uint64)           # voxel << 32 | b, unique, with the d2 of the first offset that showed it
    dist = np.zeros(0, np.int64)
    new_k, new_d = [], []

    def compact():
        nonlocal keys, dist, new_k, new_d
        k = np.concatenate([keys] + new_k)
        d = np.concatenate([dist] + new_d)
        order = np.argsort(k, kind='stable')            # earlier offsets stay in front
        k, d = k[order], d[order]
        first = np.ones(len(k), bool)
        first[1:] = k[1:] != k[:-1]
        keys, dist, new_k, new_d = k[first], d[first], [], []

    for i, (d2, dz, dy, dx) in enumerate(offsets):
        L = pad[hz + dz:hz + dz + D, hy + dy:hy + dy + H, hx + dx:hx + dx + W]
        m = (A != 0) & (L != 0)
        if same:
            m &= L != A
        if m.any():
            new_k.append((vox[m] << np.uint64(32)) | L[m].astype(np.uint64))
            new_d.append(np.full(int(m.sum()), d2, np.int64))
        if len(new_k) >= 32 or i == len(offsets) - 1:
            compact()
    if len(keys) == 0:
        return np.zeros((0, COLS), np.int64)
    v = (keys >> np.uint64(32)).astype(np.int64)
    b = (keys & np.uint64(0xffffffff)).astype(np.uint32)
    a = A.reshape(-1)[v]
    z, rem = np.divmod(v, H * W)
    y, x = np.divmod(rem, W)
    faces = np.zeros((len(v), 3), np.int64)
    for axis, (step, pitch) in enumerate(zip(((1, 0, 0), (0, 1, 0), (0, 0, 1)), sampling)):
        if pitch * pitch > r2:
            continue                                    # that neighbour is not in the ball: no ring, no count
        for s in (-1, 1):
            faces[:, axis] += pad[z + hz + s * step[0], y + hy + s * step[1], x + hx + s * step[2]] == b
    pair = (a.astype(np.uint64) << np.uint64(32)) | b.astype(np.uint64)
    rows, inv = np.unique(pair, return_inverse=True)
    inv = inv.reshape(-1)
    out = np.zeros((len(rows), COLS), np.int64)
    out[:, 0] = (rows >> np.uint64(32)).astype(np.int64)
    out[:, 1] = (rows & np.uint64(0xffffffff)).astype(np.int64)
    out[:, 3] = np.iinfo(np.int64).max
    np.add.at(out[:, 2], inv, 1)
    np.minimum.at(out[:, 3], inv, dist)
    np.add.at(out[:, 4], inv, z + z_base)
    np.add.at(out[:, 5], inv, y)
    np.add.at(out[:, 6], inv, x)
    for axis in range(3):
        np.add.at(out[:, 7 + axis], inv, faces[:, axis])
    return out


def restrict_to_slab(volume_a, volume_b, z0, z1, r2, sampling=(1, 1, 1)):
    """the rows that the slab [z0, z1) of A contributes to the table of the whole volume: A outside the slab zeroed (a
    contact voxel belongs to the block that owns it), B whole"""
    A = as_u32(volume_a).copy()
    A[:z0] = 0
    A[z1:] = 0
    return contact_table(A, as_u32(volume_a if volume_b is None else volume_b), r2, sampling, same=volume_b is None)


# ------------------------------------------------------------------------------------------------------------ case builders
def random_labels(shape, density, n_ids, seed, dtype=np.uint32, special=()):
    """labels drawn from n_ids ids (plus `special` ones) on `density` of the voxels, 0 elsewhere"""
    rng = np.random.default_rng(seed)
    ids = np.concatenate([np.arange(1, n_ids + 1, dtype=np.uint64), np.asarray(special, dtype=np.uint64)])
    vol = ids[rng.integers(0, len(ids), size=shape)]
    vol[rng.random(shape) >= density] = 0
    if dtype == np.uint8:
        assert vol.max(initial=0) < 256
        return vol.astype(np.uint8)
    vol = vol.astype(np.uint32)
    return vol.view(np.int32) if dtype == np.int32 else vol


def two_cubes(gap=0, axis=2, labels=(1, 2)):
    """two 2 x 2 x 2 cubes side by side along `axis` with `gap` background voxels between them, one voxel of margin"""
    shape = [4, 4, 4]
    shape[axis] = 6 + gap
    vol = np.zeros(shape, np.uint32)
    sl = [slice(1, 3)] * 3
    sl[axis] = slice(1, 3)
    vol[tuple(sl)] = labels[0]
    sl[axis] = slice(3 + gap, 5 + gap)
    vol[tuple(sl)] = labels[1]
    return vol


def distinct_block():
    """3 x 3 x 3 voxels of 27 distinct labels 1 .. 27 inside a 5 x 5 x 5 volume; the centre label is 14"""
    vol = np.zeros((5, 5, 5), np.uint32)
    vol[1:4, 1:4, 1:4] = np.arange(1, 28, dtype=np.uint32).reshape(3, 3, 3)
    return vol


def crowded(shape=(5, 5, 70)):
    """every voxel its own label"""
    return np.arange(1, int(np.prod(shape)) + 1, dtype=np.uint32).reshape(shape)


def slabs_on_border(axis, at, shape, gap=0):
    """label 1 on one side of index `at` along `axis`, label 2 on the other, `gap` background voxels in between"""
    vol = np.zeros(shape, np.uint32)
    lo = [slice(None)] * 3
    hi = [slice(None)] * 3
    lo[axis] = slice(max(at - 3, 0), at)
    hi[axis] = slice(at + gap, at + gap + 3)
    vol[tuple(lo)] = 1
    vol[tuple(hi)] = 2
    return vol
