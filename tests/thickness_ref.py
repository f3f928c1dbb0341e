"""Checkers for the local thickness (include/emp_hip.h, E10); not a test.  Two restatements of the definition

    T2(p) = max { d2(q) : |p - q|^2 < d2(q) },   d2 = the capped squared distance of emp_label_edt (test_morph_host.edt_ref)

that share nothing with the kernel: `thickness_brute` shifts the mask d2 == u over every offset of the open ball of
squared radius u, for every distinct u; `thickness_fast` asks scipy's exact Euclidean transform for the nearest voxel
with d2 == u and recomputes the weighted squared distance to it in integers.  tests/test_thickness_host.py checks one
against the other.  `table_ref` is the per-object histogram with numpy.unique."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_morph_host import ball, edt_ref, shifted  # noqa: E402


def thickness_brute(lab, cap=65535, sampling=(1, 1, 1)):
    """(T2, d2) by the definition; for small volumes"""
    d2 = edt_ref(lab, sampling, cap).astype(np.int64)
    t2 = np.zeros(d2.shape, np.int64)
    for u in np.unique(d2):
        if u == 0:
            continue
        mask = d2 == u
        covered = mask.copy()
        for dz, dy, dx, _ in ball(int(u) - 1, sampling):        # 0 < |o|^2 <= u - 1
            covered |= shifted(mask, (dz, dy, dx))[0]
        t2[covered] = u                                         # ascending u: the maximum stays
    return t2.astype(np.uint16), d2.astype(np.uint16)


def thickness_fast(lab, cap=65535, sampling=(1, 1, 1)):
    """(T2, d2): per distinct u ascending, the voxels whose nearest voxel with d2 == u lies nearer than sqrt(u)"""
    from scipy.ndimage import distance_transform_edt
    d2 = edt_ref(lab, sampling, cap).astype(np.int64)
    t2 = np.zeros(d2.shape, np.int64)
    if d2.size == 0:
        return t2.astype(np.uint16), d2.astype(np.uint16)
    grid = np.indices(d2.shape).astype(np.int64)
    pitch = np.asarray(sampling, np.int64).reshape(3, 1, 1, 1)
    for u in np.unique(d2):
        if u == 0:
            continue
        _, idx = distance_transform_edt(d2 != u, sampling=[float(a) for a in sampling], return_indices=True)
        sq = (((idx.astype(np.int64) - grid) * pitch) ** 2).sum(axis=0)
        t2[sq < u] = u
    return t2.astype(np.uint16), d2.astype(np.uint16)


def as_u32(lab):
    lab = np.asarray(lab)
    return lab.view(np.uint32) if lab.dtype == np.int32 else lab.astype(np.uint32)


def table_ref(lab, t2):
    """rows (label, t2, voxels) of the labelled voxels, ascending by (label, t2) with the label unsigned"""
    l = as_u32(lab).astype(np.uint64).ravel()
    t = np.asarray(t2).astype(np.uint64).ravel()
    keep = l != 0
    keys, counts = np.unique((l[keep] << np.uint64(32)) | t[keep], return_counts=True)
    out = np.zeros((len(keys), 3), np.int64)
    out[:, 0] = (keys >> np.uint64(32)).astype(np.int64)
    out[:, 1] = (keys & np.uint64(0xffffffff)).astype(np.int64)
    out[:, 2] = counts
    return out


def _paint_ball(v, centre, r, label):
    z, y, x = np.ogrid[:v.shape[0], :v.shape[1], :v.shape[2]]
    v[(z - centre[0]) ** 2 + (y - centre[1]) ** 2 + (x - centre[2]) ** 2 <= r * r] = label
    return v


def dumbbell(dtype=np.uint32):
    """(30, 30, 64): balls of radius 11 and 6 joined by a 5 x 5 bar, and a plate of a second label close to the bar"""
    v = np.zeros((30, 30, 64), dtype)
    v[13:18, 13:18, 14:52] = 7
    _paint_ball(v, (15, 15, 14), 11, 7)
    _paint_ball(v, (15, 15, 52), 6, 7)
    v[20:23, 8:24, 28:40] = 200
    return v


def tube_and_ball(dtype=np.uint32):
    """(20, 19, 150): a tube of radius 3 along x through two x-tile borders, and a ball of radius 8 centred on the
    corner (8, 8, 64) of eight tiles: its centre voxels cover voxels two tiles away in z and in y"""
    v = np.zeros((20, 19, 150), dtype)
    z, y = np.ogrid[:20, :19]
    v[((z - 15) ** 2 + (y - 4) ** 2 <= 9)[:, :, None] & np.ones((1, 1, 150), bool)] = 3
    v[:, :, :20] = 0
    v[:, :, 140:] = 0
    _paint_ball(v, (8, 8, 64), 8, 9)
    return v
