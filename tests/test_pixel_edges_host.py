"""CPU: the two references behind tests/test_pixel_edges_gpu.py (oracle/postprocess.py and the plain-numpy statement
written there) agree on every input of that module -- so that a wrong reference cannot hide a wrong kernel, and so that
the inputs and references are exercised where there is no GPU."""
import numpy as np
import pytest

import test_pixel_edges_gpu as E


def test_median_references_agree():
    for ks, C in E.MEDIAN_SWEEP:
        for D in E.median_depths(ks):
            E.median_refs(E.median_input(C, D, 7, 37), ks, 0.5)
    for C in E.MEDIAN_CLASSES:
        E.median_refs(E.median_input(C, 9, 7, 37), 3, 0.5)
    for C, ks in E.MEDIAN_LARGE_LDS:
        E.median_refs(E.median_input(C, ks + 3, 2, 130), ks, 0.5)
    for hw, C in E.MEDIAN_FEW:
        E.median_refs(E.median_input(C, 5, *hw), 3, 0.5)
    for C in (1, 3):
        x, thr = E.harden_input(C)
        E.median_refs(x, 1, thr)


@pytest.mark.parametrize('C', [1, 2])
def test_median_references_agree_large(C):
    filt, sem = E.median_refs(E.median_input(C, 3, 1, E.MEDIAN_BIG_HW), 3, 0.5)
    assert 0 < sem.mean() < 1 and not np.array_equal(filt[1], E.median_input(C, 3, 1, E.MEDIAN_BIG_HW)[1])


def test_nms_references_agree():
    n = 0
    for h, w in E.CENTERS_TINY:
        for k in E.CENTERS_TINY_K:
            n += sum(len(e) for e in E.centers_refs(E.centers_tiny_map(h, w), 0.1, k))
    for k in (2, 3, 7):
        for h, w in E.CENTERS_BATCH:
            n += sum(len(e) for e in E.centers_refs(E.centers_batch_map(h, w), 0.1, k))
        n += len(E.centers_refs(E.centers_wave_map(), 0.1, k)[0])
        n += len(E.centers_refs(E.centers_row_end_map(), 0.1, k)[0])
    for k in (3, 7):
        for h, w in E.CENTERS_CORNERS:
            n += sum(len(e) for e in E.centers_refs(E.centers_corner_map(h, w), 0.1, k))
    for h, w, thr in E.CENTERS_THR:
        for k in (1, 3):
            n += len(E.centers_refs(E.centers_threshold_map(h, w, thr), thr, k)[0])
    assert n > 1000


def test_fuse_references_agree():
    for H, W, up in E.FUSE_BRANCHES:
        sem, ids = E.fuse_stack(3, H, W, up, 12, 4, 20)
        exp = E.fuse_refs(sem, ids, up, **E.FUSE_KW)
        assert len(np.unique(exp)) > 4
    sem, ids = E.fuse_stack(2, 32, 64, 1, 4000, 4, 21)
    E.fuse_refs(sem, ids, 1, cap=4000, nc=4, thing=[1, 3], div=10000, stuff_area=9, void=0)
    for up in (1, 4):
        sem, ids = E.fuse_stack(3, 16, 24, up, 12, 4, 22)
        E.fuse_refs(sem, ids, up, **E.FUSE_KW)
    for H, W in E.FUSE_EDGE_SHAPES:
        sem, ids = E.fuse_value_edges(H, W)
        E.fuse_refs(sem, ids, 1, cap=5, nc=4, thing=[1, 3], div=1000, stuff_area=6, void=255)
    for H, W in E.FUSE_HIGH_SHAPES:
        sem, ids = E.fuse_stack(2, H, W, 1, 12, 3, 23)
        assert E.fuse_refs(sem, ids, 1, cap=12, nc=3, thing=[2], div=1 << 30, stuff_area=4, void=0).max() > (1 << 31)
    for _, H, W, up, cap in E.FUSE_ABOVE:
        sem, ids = E.fuse_above_cap(H, W, up, cap)
        E.fuse_refs(sem, ids, up, cap=cap, nc=4, thing=[1, 3], div=10000, stuff_area=9, void=255)
