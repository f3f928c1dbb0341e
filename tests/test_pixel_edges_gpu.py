"""GPU: edges and dispatch branches of the per-pixel post-processing kernels (csrc/emp_pixel.hip).

Every result is an integer map or an exact fp32 selection: every comparison is assert_array_equal.  The reference is
oracle/postprocess.py; the median, the NMS and the fusion also have a second, plain-numpy statement in this file, and
the two references must agree on the CPU before a GPU result is looked at (``*_refs`` helpers; the same helpers run
without a GPU from tests/test_pixel_edges_host.py).

Dispatch predicates of emp_pixel.hip and the tests that take each side
----------------------------------------------------------------------
median (launch_median)
  C == 1                   yes: test_median_depth_sweep[*-1], test_median_few_pixels[*-1], test_median_second_grid_trip[1]
                           no : every C > 1 case below
  ks > 1 && C <= MC_CMAX   yes (mc8): test_median_depth_sweep[*-5], test_median_class_counts[2|4|8],
                                      test_median_few_pixels[*-3], test_median_second_grid_trip[2]
                           no  (mc) : test_median_depth_sweep[*-9], test_median_class_counts[9|16],
                                      test_median_few_pixels[*-9]; ks == 1: test_harden_direct[3]
  lds > 64 KiB (opt-in)    yes: test_median_large_lds[8-9] (mc8, 72 KiB), [16-9] (mc, 144 KiB), [14-11] (mc, 154 KiB)
                           no : all other C > 1 cases
  lds > 160 KiB (refusal)  yes: test_median_lds_refusal[15], [16];  no: everything else
  grid-stride second trip  test_median_second_grid_trip (HW > 8192 * 256)
centre NMS (emp_find_centers = sorted list, emp_find_centers_ws = bitmap; both run in every test)
  vec4 (w % 4 == 0)        yes: test_centers_tiny[3x4], [1x260], test_centers_wave_boundary, test_centers_row_end,
                                test_centers_corners[6x8], test_centers_threshold[8x12-*]
                           no : test_centers_tiny[1x1|1x5|5x1|2x3|9x257], test_centers_scalar_batch,
                                test_centers_corners[5x7], test_centers_threshold[7x9-*]
  thr >= 0                 refused otherwise: test_centers_negative_threshold
nearest-centre vote (group_pixels_kernel)
  K == 0 / K <= 20 / K > 20, K > GP_PRUNE_MIN   test_group_many_k (K = 0, 1, 16, 17, 20, 21, 64 in one call)
  8-byte class load vs per-pixel               test_group_class_map_alignment (w = 67: every alignment mod 8)
  patch mostly outside the slice               test_group_small_slices
fusion (emp_fuse_lut / emp_fuse_apply / emp_fuse_panoptic)
  fuse_vec4_ok             yes: test_fuse_branches[16x24u1|16x24u4|16x48u8|8x36u1|12x100u1]
                           no : [16x24u2] (up), [6x10u2|5x7u1] (W % 4), test_fuse_misaligned (pointers)
  use_lds                  yes: all but test_fuse_without_lds; no: test_fuse_without_lds, test_fuse_ids_above_cap[nolds]
  hist kernel              fuse_hist_vec4_kernel: vec4 yes & lds;  fuse_hist_kernel (lds): vec4 no;  (no lds): cap 4000
  output type              uint32 + vec4 -> fuse_apply_multi_kernel, int64 + vec4 -> fuse_apply_vec4_kernel<int64>,
                           not vec4 -> fuse_apply_kernel<uint32|int64>: both types in every fuse test
                           (fuse_apply_vec4_kernel<uint32> needs H*W >= 2^31: not reachable at test size)
  up                       1: per-pixel id loads; 2: scalar kernels; 4, 8: one id per 4 pixels (test_fuse_branches)
  partial FA_U group       [8x36u1] (72 items: item 0 of 4 only), [12x100u1] (300 items, 256 lanes: item 1 partial)
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def hip():
    from empanada_amd import _hip
    _hip.load()
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return _hip


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.cpu().numpy()


# =========================================================================================== 1. median and harden
def median_input(C, D, H, W, seed=0):
    """(D,C,H,W) fp32 probabilities.  Pixel bands (flat index, an eighth of the slice each): [0,b) exactly 0.5 in every
    slice, [b,2b) 0.5 in the even slices, and for C > 1 [2b,3b) with channels 0 and 1 bit-equal and dominant and
    [3b,4b) with the last two channels bit-equal and dominant (an argmax tie must go to the first of them)."""
    rng = np.random.default_rng([seed, C, D, H, W])
    x = rng.random((D, C, H, W), dtype=np.float32)
    f = x.reshape(D, C, H * W)
    b = (H * W) // 8
    if b:
        f[:, :, :b] = 0.5
        f[::2, :, b:2 * b] = 0.5
        if C > 1:
            f[:, 2:, 2 * b:3 * b] *= 0.25
            f[:, 1, 2 * b:3 * b] = f[:, 0, 2 * b:3 * b]
            f[:, :-2, 3 * b:4 * b] *= 0.25
            f[:, -1, 3 * b:4 * b] = f[:, -2, 3 * b:4 * b]
    return x


def _median_oracle(x, ks, thr):
    """oracle/postprocess.MedianQueue over the stack, in emission order, then harden_seg per slice"""
    from oracle import postprocess as OP
    q = OP.MedianQueue(ks)
    outs = []
    for t in range(len(x)):
        q.enqueue({'sem': x[t:t + 1].copy()})
        o = q.get_next(['sem'])
        if o is not None:
            outs.append(o['sem'].copy())
    outs += [o['sem'].copy() for o in q.end()]
    filt = np.concatenate(outs, axis=0)
    sem = np.concatenate([OP.harden_seg(f[None], thr)[0] for f in filt], axis=0)
    return filt, sem.astype(np.uint8)


def _median_plain(x, ks, thr):
    """the recursive median in so many words: the filtered value replaces the raw one, the first and last ks // 2
    slices pass through; C == 1: p >= thr, C > 1: first maximum over the channels"""
    D, C = x.shape[:2]
    m = ks // 2
    out = x.copy()
    for s in range(m, D - m):
        window = np.concatenate([out[s - m:s], x[s:s + m + 1]], axis=0)
        out[s] = np.sort(window, axis=0)[ks // 2]
    if C == 1:
        sem = out[:, 0] >= np.float32(thr)
    else:
        best = out[:, 0].copy()
        sem = np.zeros(best.shape, dtype=np.uint8)
        for c in range(1, C):
            better = out[:, c] > best
            sem[better] = c
            best[better] = out[:, c][better]
    return out, sem.astype(np.uint8)


def median_refs(x, ks, thr):
    filt, sem = _median_oracle(x, ks, thr)
    filt2, sem2 = _median_plain(x, ks, thr)
    np.testing.assert_array_equal(filt, filt2, err_msg='the two median references disagree')
    np.testing.assert_array_equal(sem, sem2, err_msg='the two harden references disagree')
    return filt, sem


def _check_median(hip, x, ks, thr=0.5, what=''):
    filt, sem = median_refs(x, ks, thr)
    g = _dev(x)
    gsem, gfilt = hip.median_harden_stack(g, ks, thr, want_prob=True)
    gsem_only = hip.median_harden_stack(g, ks, thr)
    np.testing.assert_array_equal(_np(gfilt), filt, err_msg=what)
    np.testing.assert_array_equal(_np(gsem), sem, err_msg=what)
    np.testing.assert_array_equal(_np(gsem_only), sem, err_msg=what + ' (want_prob=False)')
    return g, sem


def median_depths(ks):
    m = ks // 2
    return [ks, ks + 1, 2 * m + 4, 2 * m + 5, 2 * m + 8, 2 * m + 9, 2 * m + 16, 2 * m + 17, 2 * m + 27]


MEDIAN_SWEEP = [(ks, C) for ks in (3, 5, 11) for C in (1, 5, 9)]
MEDIAN_CLASSES = [2, 4, 8, 9, 16]
MEDIAN_LARGE_LDS = [(8, 9), (16, 9), (14, 11)]
MEDIAN_FEW = [(hw, C) for hw in ((1, 1), (1, 63), (1, 257)) for C in (1, 3, 9)]
MEDIAN_BIG_HW = 8192 * 256 + 300


@pytest.mark.parametrize('ks,C', MEDIAN_SWEEP, ids=[f'{ks}-{C}' for ks, C in MEDIAN_SWEEP])
def test_median_depth_sweep(hip, ks, C):
    """trip counts of the prefetch pipelines (PF = 8 for C = 1, MC_PF = 4 for C <= 8): one filtered slice, D - 2M a
    multiple of the depth, one more, fewer, three and more trips"""
    for D in median_depths(ks):
        _check_median(hip, median_input(C, D, 7, 37), ks, what=f'D={D}')


@pytest.mark.parametrize('C', MEDIAN_CLASSES)
def test_median_class_counts(hip, C):
    x = median_input(C, 9, 7, 37)
    g, sem = _check_median(hip, x, 3)
    # argmax: thr has no influence for C > 1
    for thr in (0.0, 2.0, -1.0):
        np.testing.assert_array_equal(_np(hip.median_harden_stack(g, 3, thr)), sem, err_msg=f'thr={thr}')


@pytest.mark.parametrize('C,ks', MEDIAN_LARGE_LDS, ids=[f'{C}-{ks}' for C, ks in MEDIAN_LARGE_LDS])
def test_median_large_lds(hip, C, ks):
    """C * ks KiB of LDS per block: 72 (mc8, opt-in), 144 (mc, opt-in), 154 (the largest request the entry accepts)"""
    _check_median(hip, median_input(C, ks + 3, 2, 130), ks)


@pytest.mark.parametrize('C', [15, 16])
def test_median_lds_refusal(hip, C):
    x = median_input(C, 14, 2, 130)
    with pytest.raises(hip.HipError, match='LDS'):
        hip.median_harden_stack(_dev(x), 11, 0.5)
    _check_median(hip, median_input(3, 5, 2, 130), 3)          # the library is still in working order


@pytest.mark.parametrize('hw,C', MEDIAN_FEW, ids=[f'{h}x{w}-{C}' for (h, w), C in MEDIAN_FEW])
def test_median_few_pixels(hip, hw, C):
    _check_median(hip, median_input(C, 5, *hw), 3)


@pytest.mark.parametrize('C', [1, 2])
def test_median_second_grid_trip(hip, C):
    """HW > 8192 blocks x 256 lanes: the first 300 pixels' lanes take a second trip of the grid-stride loop.
    (C = 9 at this size is left out: its two CPU references alone take longer than a test may.)"""
    _check_median(hip, median_input(C, 3, 1, MEDIAN_BIG_HW), 3)


def harden_input(C):
    rng = np.random.default_rng(40 + C)
    x = rng.random((2, C, 5, 53), dtype=np.float32)
    thr = np.float32(0.3)
    if C == 1:
        x[:, 0, 0, 0:30:3] = thr
        x[:, 0, 0, 1:30:3] = np.nextafter(thr, np.float32(1))
        x[:, 0, 0, 2:30:3] = np.nextafter(thr, np.float32(0))
    else:
        x[:, 1, 1] = x[:, 0, 1]                                  # ties between channels: the first wins
        x[:, 2, 2] = x[:, 1, 2]
        x[:, :, 3] = 0.25                                        # all equal
    return x, float(thr)


@pytest.mark.parametrize('C', [1, 3])
def test_harden_direct(hip, C):
    """emp_harden as inference/engines.py and patterns.py call it; equal to the ks = 1 filter"""
    from oracle import postprocess as OP
    x, thr = harden_input(C)
    _, sem = median_refs(x, 1, thr)
    np.testing.assert_array_equal(np.concatenate([OP.harden_seg(x[d:d + 1], thr)[0] for d in range(2)]), sem)
    g = _dev(x)
    D, _, H, W = x.shape
    out = torch.full((D, H, W), 255, dtype=torch.uint8, device='cuda')
    hip.call('emp_harden', g.data_ptr(), D, C, H * W, thr, out.data_ptr(), hip.stream())
    np.testing.assert_array_equal(_np(out), sem)
    np.testing.assert_array_equal(_np(hip.median_harden_stack(g, 1, thr)), sem)


# =========================================================================================== 2. centre NMS
def _centers_oracle(hm, thr, k):
    """oracle.postprocess.find_instance_center; it squeezes its input like the reference does and so cannot take a map
    with a side of 1 -- those go to the same C routine directly"""
    from oracle import postprocess as OP
    h, w = hm.shape
    if h > 1 and w > 1:
        yx = OP.find_instance_center(hm[None, None], thr, k)
    else:
        from oracle._clib import lib
        hm = np.ascontiguousarray(hm, dtype=np.float32)
        out = np.empty((h * w, 2), dtype=np.int64)
        n = lib().emp_oracle_find_centers(hm.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), h, w,
                                          ctypes.c_float(thr), int(k),
                                          out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), h * w)
        yx = out[:n]
    return (yx[:, 0] * w + yx[:, 1]).astype(np.int64)


def _centers_plain(hm, thr, k):
    """brute force: a pixel is a centre when its thresholded value is positive and equals the maximum of the
    thresholded map over rows y - k//2 .. y - k//2 + k - 1 and the same columns (outside the map: -inf)"""
    h, w = hm.shape
    t = np.where(hm > np.float32(thr), hm, np.float32(-1)).astype(np.float32)
    pad = k // 2
    padded = np.full((h + k, w + k), -np.inf, dtype=np.float32)
    padded[pad:pad + h, pad:pad + w] = t
    mx = np.full((h, w), -np.inf, dtype=np.float32)
    for dy in range(k):
        for dx in range(k):
            mx = np.maximum(mx, padded[dy:dy + h, dx:dx + w])
    return np.flatnonzero((t == mx) & (t > 0)).astype(np.int64)


def centers_refs(hm3, thr, k):
    """per slice: flat indices y*w+x in raster order, identical from both references"""
    exp = []
    for hm in hm3:
        a, b = _centers_oracle(hm, thr, k), _centers_plain(hm, thr, k)
        np.testing.assert_array_equal(a, b, err_msg=f'the two NMS references disagree (k={k}, thr={thr})')
        exp.append(a)
    return exp


def _check_centers(hip, hm3, thr, k):
    exp = centers_refs(hm3, thr, k)
    D, h, w = hm3.shape
    g = _dev(hm3)
    idx, cnt = hip.find_centers(g, thr, k, cap=4096)
    idx_ws, cnt_ws = hip.find_centers_ws(g, thr, k, min(h * w, hip.CENTER_LIMIT))
    cnt, cnt_ws, idx, idx_ws = _np(cnt), _np(cnt_ws), _np(idx), _np(idx_ws)
    for d in range(D):
        what = f'slice {d}, k={k}, thr={thr}, {h}x{w}'
        assert cnt[d] == len(exp[d]) and cnt_ws[d] == len(exp[d]), what
        np.testing.assert_array_equal(idx[d, :cnt[d]], exp[d], err_msg=what)
        np.testing.assert_array_equal(idx_ws[d, :cnt_ws[d]], exp[d], err_msg=what + ' (ws)')
    return exp


def heat(shape, seed, scale=1.0):
    rng = np.random.default_rng([seed, *shape])
    return (rng.random(shape, dtype=np.float32) ** 6 * np.float32(scale)).astype(np.float32)


CENTERS_TINY = [(1, 1), (1, 5), (5, 1), (3, 4), (2, 3), (1, 260), (9, 257)]
CENTERS_TINY_K = [1, 2, 3, 15]


def centers_tiny_map(h, w):
    hm = heat((1, h, w), 1)
    if w >= 2:
        hm[0, 0, 0:2] = 0.9                                       # two equal neighbours: both are centres
    return hm


@pytest.mark.parametrize('h,w', CENTERS_TINY, ids=[f'{h}x{w}' for h, w in CENTERS_TINY])
def test_centers_tiny(hip, h, w):
    """images smaller than a wave's span, sides of 1, w < 4; k = 1 (no neighbours), k = CT_MAXK = 15 (225 window
    pixels > 64 lanes) and k larger than the image"""
    for k in CENTERS_TINY_K:
        _check_centers(hip, centers_tiny_map(h, w), 0.1, k)


CENTERS_BATCH = [(9, 7), (17, 129)]


def centers_batch_map(h, w):
    hm = heat((3, h, w), 2, scale=0.9)
    hm[1] = 0
    hm[2, h - 1, w - 1] = 0.95                                    # the very last pixel of the batch
    return hm


@pytest.mark.parametrize('h,w', CENTERS_BATCH, ids=[f'{h}x{w}' for h, w in CENTERS_BATCH])
def test_centers_scalar_batch(hip, h, w):
    """scalar kernel with D = 3 and an odd slice size: slices 1 and 2 start unaligned; slice 1 holds no centre"""
    for k in (2, 3, 7):
        exp = _check_centers(hip, centers_batch_map(h, w), 0.1, k)
        assert len(exp[1]) == 0 and len(exp[0]) > 0 and (h * w - 1) in exp[2]


def centers_wave_map():
    hm = heat((1, 4, 1024), 3, scale=0.5)
    hm[0, 0, 254:259] = 0.8                                       # plateau over the first wave boundary (lane 63 | lane 0)
    hm[0, 0, 1021:1024] = 0.8                                     # plateau up to the row end
    hm[0, 3, 256] = 0.9                                           # lone maximum in lane 0 of the second wave
    return hm


def test_centers_wave_boundary(hip):
    w = 1024
    for k in (2, 3, 7):
        exp = _check_centers(hip, centers_wave_map(), 0.1, k)[0]
        if k == 3:
            assert set(range(254, 259)) | set(range(1021, 1024)) | {3 * w + 256} <= set(exp.tolist())


def centers_row_end_map():
    hm = heat((1, 8, 260), 4, scale=0.5)
    hm[0, 2, 258:260] = 0.8                                       # adjacent in memory, not in the image:
    hm[0, 3, 0:2] = 0.8                                           # two plateaus, each pixel judged by its own window
    return hm


def test_centers_row_end(hip):
    w = 260
    for k in (2, 3, 7):
        exp = _check_centers(hip, centers_row_end_map(), 0.1, k)[0]
        if k == 3:
            assert {2 * w + 258, 2 * w + 259, 3 * w, 3 * w + 1} <= set(exp.tolist())


CENTERS_CORNERS = [(5, 7), (6, 8)]


def centers_corner_map(h, w):
    hm = heat((2, h, w), 5, scale=0.5)
    for d in range(2):
        for y, x in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)):
            hm[d, y, x] = 0.9
    return hm


@pytest.mark.parametrize('h,w', CENTERS_CORNERS, ids=[f'{h}x{w}' for h, w in CENTERS_CORNERS])
def test_centers_corners(hip, h, w):
    for k in (3, 7):
        exp = _check_centers(hip, centers_corner_map(h, w), 0.1, k)
        for e in exp:
            assert {0, w - 1, (h - 1) * w, h * w - 1} <= set(e.tolist())


CENTERS_THR = [(h, w, thr) for (h, w) in ((7, 9), (8, 12)) for thr in (0.1, 0.0)]


def centers_threshold_map(h, w, thr):
    """zeros, negative zeros and negatives, with isolated planted values around the threshold"""
    rng = np.random.default_rng([6, h, w])
    thr = np.float32(thr)
    hm = np.where(rng.random((h, w)) < 0.5, np.float32(0.0), -rng.random((h, w), dtype=np.float32)).astype(np.float32)
    hm[rng.random((h, w)) < 0.2] = np.float32(-0.0)
    planted = [thr, np.nextafter(thr, np.float32(np.inf)), np.nextafter(thr, np.float32(-np.inf)), np.float32(0.0),
               np.float32(-0.0), np.float32(-0.25), np.float32(0.5), np.nextafter(thr, np.float32(np.inf))]
    spots = [(y, x) for y in (1, 5) for x in range(1, w, 2)][:len(planted)]
    for (y, x), v in zip(spots, planted):
        hm[y, x] = v
    hm[3, 0:2] = thr                                              # a pair exactly at the threshold: strict >
    hm[3, 4:6] = np.nextafter(thr, np.float32(np.inf))            # a pair just above it: both centres
    return hm[None]


@pytest.mark.parametrize('h,w,thr', CENTERS_THR, ids=[f'{h}x{w}-{thr}' for h, w, thr in CENTERS_THR])
def test_centers_threshold(hip, h, w, thr):
    hm = centers_threshold_map(h, w, thr)
    for k in (1, 3):
        exp = _check_centers(hip, hm, thr, k)[0]
        assert {3 * w + 4, 3 * w + 5} <= set(exp.tolist()) and not {3 * w, 3 * w + 1} & set(exp.tolist())


def test_centers_negative_threshold(hip):
    """the in-register shortcut is proven for thr >= 0 only: both entries and both wrappers refuse a negative one"""
    g = _dev(heat((1, 8, 12), 7))
    with pytest.raises(hip.HipError, match='must be >= 0'):
        hip.find_centers(g, -0.1, 3, cap=64)
    with pytest.raises(hip.HipError, match='must be >= 0'):
        hip.find_centers_ws(g, -0.1, 3, 96)
    idx = torch.zeros((1, 96), dtype=torch.int32, device='cuda')
    cnt = torch.zeros((1,), dtype=torch.int32, device='cuda')
    work = torch.zeros((hip.query('emp_find_centers_work_elems', 1, 8, 12, 96),), dtype=torch.int32, device='cuda')
    with pytest.raises(hip.HipError, match=r'emp_find_centers failed.*must be >= 0'):
        hip.call('emp_find_centers', g.data_ptr(), 1, 8, 12, -0.1, 3, 96, idx.data_ptr(), cnt.data_ptr(), hip.stream())
    with pytest.raises(hip.HipError, match=r'emp_find_centers_ws failed.*must be >= 0'):
        hip.call('emp_find_centers_ws', g.data_ptr(), 1, 8, 12, -0.1, 3, 96, work.data_ptr(), idx.data_ptr(),
                 cnt.data_ptr(), hip.stream())
    _check_centers(hip, heat((1, 8, 12), 7), 0.0, 3)             # thr = 0 is accepted


# =========================================================================================== 3. nearest-centre vote
def group_stack(h, w, counts, cap, step, seed):
    """per-slice centre lists (D, cap) with h*w - 1 past each slice's count, counts, offsets (D,2,h,w): integer-valued
    (exact ties), fractional noise on the upper half (near ties), rows 5..7 farther than 1e5 from every centre"""
    rng = np.random.default_rng([seed, h, w, step])
    D = len(counts)
    idx = np.full((D, cap), h * w - 1, dtype=np.int32)
    ctrs = []
    for d, K in enumerate(counts):
        ctr = np.stack([rng.integers(0, h, K), rng.integers(0, w, K)], axis=1).astype(np.int64).reshape(K, 2)
        idx[d, :K] = ctr[:, 0] * w + ctr[:, 1]
        ctrs.append(ctr)
    off = rng.integers(-12, 13, (D, 2, h, w)).astype(np.float32) * step
    off[:, :, : h // 2] += rng.normal(0, 1e-3, (D, 2, h // 2, w)).astype(np.float32)
    if h > 8:
        off[:, :, 5:8] += np.float32(3e5)
    return idx, np.asarray(counts, dtype=np.int32), ctrs, off


def group_oracle(ctrs, off, step):
    from oracle import postprocess as OP
    D, _, h, w = off.shape
    exp = np.zeros((D, h, w), dtype=np.int64)
    for d, ctr in enumerate(ctrs):
        if len(ctr):
            exp[d] = OP.group_pixels(ctr, off[d:d + 1], step=step)[0]
    return exp


GROUP_COUNTS = [0, 1, 16, 17, 20, 21, 64]


@pytest.mark.parametrize('step', [1, 4])
def test_group_many_k(hip, step):
    """one call whose slices sit on every side of the per-slice switches: K = 0, K <= GP_PRUNE_MIN = 16 < K,
    K <= 20 < K (1e5 ceiling, id 0 for far pixels), K = cap"""
    idx, cnt, ctrs, off = group_stack(40, 100, GROUP_COUNTS, 64, step, 11)
    exp = group_oracle(ctrs, off, step)
    assert (exp[5, 5:8] == 0).all() and (exp[4, 5:8] > 0).all()     # K = 21 keeps 0 beyond 1e5, K = 20 does not
    ids = hip.group_pixels(_dev(idx), _dev(cnt), _dev(off), step)
    np.testing.assert_array_equal(_np(ids).astype(np.int64), exp)


@pytest.mark.parametrize('step', [1, 4])
def test_group_class_map_alignment(hip, step):
    """w = 67, D = 3: rows and slices of the class map start at every alignment mod 8; slice 1 has no thing pixel"""
    h, w = 19, 67
    idx, cnt, ctrs, off = group_stack(h, w, [17, 21, 64], 64, step, 12)
    rng = np.random.default_rng(13)
    sem = np.repeat(np.repeat(rng.integers(0, 4, (3, h // 3 + 1, w // 9 + 1)), 3, 1), 9, 2)[:, :h, :w]
    sprinkle = rng.random((3, h, w)) < 0.15
    sem = np.where(sprinkle, rng.integers(0, 4, (3, h, w)), sem).astype(np.uint8)
    sem[1] = np.where(np.isin(sem[1], [1, 3]), sem[1] - 1, sem[1])
    thing = np.isin(sem, [1, 3])
    assert not thing[1].any() and thing[0].any() and thing[2].any()
    exp = group_oracle(ctrs, off, step) * thing
    ids = hip.group_pixels(_dev(idx), _dev(cnt), _dev(off), step, sem=_dev(sem), thing_list=[1, 3])
    np.testing.assert_array_equal(_np(ids).astype(np.int64), exp)


GROUP_SMALL = [(1, 1), (3, 5), (15, 63), (17, 65)]


@pytest.mark.parametrize('h,w', GROUP_SMALL, ids=[f'{h}x{w}' for h, w in GROUP_SMALL])
def test_group_small_slices(hip, h, w):
    """slices smaller than (or one pixel past) a block's 16 x 64 patch, K = 3 and K = 25 in one call"""
    for step in (1, 4):
        idx, cnt, ctrs, off = group_stack(h, w, [3, 25], 25, step, 14)
        ids = hip.group_pixels(_dev(idx), _dev(cnt), _dev(off), step)
        np.testing.assert_array_equal(_np(ids).astype(np.int64), group_oracle(ctrs, off, step), err_msg=f'step {step}')


# =========================================================================================== 4. fusion
def _fuse_plain(cls, ids, cap, nc, thing, div, stuff_area, void):
    """cls (H,W) classes < nc, ids (H,W) in 0..cap: np.bincount per (id, class), then a loop over the ids"""
    is_thing = np.isin(cls, thing)
    ins = np.where(is_thing, ids, 0)
    counts = np.bincount((ins * nc + cls).ravel(), minlength=(cap + 1) * nc).reshape(cap + 1, nc)
    pan = np.full(cls.shape, void, dtype=np.int64)
    next_id = {}
    for i in range(1, cap + 1):
        if counts[i].sum() == 0:
            continue                                              # no thing pixel: the id consumes no number
        c = int(np.argmax(counts[i]))                             # first maximum: ties go to the smaller class
        next_id[c] = next_id.get(c, 0) + 1
        pan[ins == i] = c * div + next_id[c]
    for c in range(nc):
        if c not in thing and counts[0, c] > 0 and counts[0, c] >= stuff_area:
            pan[(cls == c)] = c * div
    return pan


def fuse_refs(sem, ids, up, cap, nc, thing, div, stuff_area, void):
    """sem (D,H,W) raw class bytes, ids (D,H/up,W/up) -> (D,H,W) int64 labels, identical from both references.
    Per the ABI a class >= nc counts as nc - 1 and an id > cap as 0 before either reference sees them."""
    from oracle import postprocess as OP
    out = []
    for d in range(len(sem)):
        cls = np.minimum(sem[d].astype(np.int64), nc - 1)
        full = np.repeat(np.repeat(ids[d].astype(np.int64), up, 0), up, 1)
        full = np.where(full <= cap, full, 0)
        if up == 1:
            a = OP.merge_semantic_and_instance(cls[None], (full * np.isin(cls, thing))[None], div, thing, stuff_area,
                                               void)[0]
        else:
            a = OP.get_panoptic_seg(cls[None], full[None, None].astype(np.float32), div, thing, stuff_area, void)[0]
        b = _fuse_plain(cls, full, cap, nc, thing, div, stuff_area, void)
        np.testing.assert_array_equal(a, b, err_msg=f'the two fusion references disagree (slice {d})')
        out.append(a)
    return np.stack(out)


def _mask(thing):
    m = 0
    for t in thing:
        m |= 1 << int(t)
    return m


def _fuse_gpu(hip, form, sem, ids, up, cap, nc, thing, div, stuff_area, void, dtype):
    """form 'wrapper': _hip.fuse_panoptic; 'two': emp_fuse_lut + emp_fuse_apply on a workspace of exactly
    emp_fuse_work_elems; 'one': the single emp_fuse_panoptic entry"""
    if form == 'wrapper':
        return hip.fuse_panoptic(sem, ids, cap, nc, thing, div, stuff_area, void, up=up, out_dtype=dtype)
    D, H, W = sem.shape
    work = torch.empty((hip.query('emp_fuse_work_elems', D, cap, nc),), dtype=torch.int32, device='cuda')
    pan = torch.empty((D, H, W), dtype=dtype, device='cuda')
    p32 = pan.data_ptr() if dtype == torch.uint32 else None
    p64 = pan.data_ptr() if dtype == torch.int64 else None
    head = (sem.data_ptr(), ids.data_ptr(), D, H, W, up, cap, nc, _mask(thing), div)
    if form == 'two':
        hip.call('emp_fuse_lut', *head, stuff_area, work.data_ptr(), hip.stream())
        hip.call('emp_fuse_apply', *head, void, work.data_ptr(), p32, p64, hip.stream())
    else:
        hip.call('emp_fuse_panoptic', *head, stuff_area, void, work.data_ptr(), p32, p64, hip.stream())
    return pan


def _check_fuse(hip, sem, ids, up, cap, nc, thing, div, stuff_area, void, forms=('wrapper', 'two', 'one'),
                sem_dev=None, ids_dev=None):
    exp = fuse_refs(sem, ids, up, cap, nc, thing, div, stuff_area, void)
    s = _dev(sem) if sem_dev is None else sem_dev
    i = _dev(ids.astype(np.int16)) if ids_dev is None else ids_dev
    for dtype in (torch.uint32, torch.int64):
        for form in forms:
            pan = _fuse_gpu(hip, form, s, i, up, cap, nc, thing, div, stuff_area, void, dtype)
            got = _np(pan).astype(np.int64)
            assert got.min() >= 0, 'labels are zero-extended'
            np.testing.assert_array_equal(got, exp, err_msg=f'{form}, {dtype}')
    return exp


def fuse_stack(D, H, W, up, cap, nc, seed):
    """blocky class and id maps, different in every slice, with single pixels that break the 4-pixel uniformity"""
    rng = np.random.default_rng([seed, D, H, W, up])
    h, w = H // up, W // up
    sem = np.repeat(np.repeat(rng.integers(0, nc, (D, H // 3 + 1, W // 5 + 1)), 3, 1), 5, 2)[:, :H, :W]
    sem = np.where(rng.random((D, H, W)) < 0.1, rng.integers(0, nc, (D, H, W)), sem).astype(np.uint8)
    ids = np.repeat(np.repeat(rng.integers(0, cap + 1, (D, h // 2 + 1, w // 3 + 1)), 2, 1), 3, 2)[:, :h, :w]
    ids = np.where(rng.random((D, h, w)) < 0.1, rng.integers(0, cap + 1, (D, h, w)), ids).astype(np.int64)
    return sem, ids


FUSE_BRANCHES = [(16, 24, 1), (16, 24, 2), (16, 24, 4), (16, 48, 8), (6, 10, 2), (5, 7, 1), (8, 36, 1), (12, 100, 1)]
FUSE_KW = dict(cap=12, nc=4, thing=[1, 3], div=1000, stuff_area=9, void=0)


@pytest.mark.parametrize('H,W,up', FUSE_BRANCHES, ids=[f'{H}x{W}u{up}' for H, W, up in FUSE_BRANCHES])
def test_fuse_branches(hip, H, W, up):
    """every kernel of the two passes (see the table above), D = 3 with other classes and ids in every slice, all
    three call forms and both output types"""
    sem, ids = fuse_stack(3, H, W, up, 12, 4, 20)
    _check_fuse(hip, sem, ids, up, **FUSE_KW)


def test_fuse_without_lds(hip):
    """(cap + 1) * nc * 4 B = 64 KiB > 48 KiB: the histogram pass adds to the global bins directly"""
    sem, ids = fuse_stack(2, 32, 64, 1, 4000, 4, 21)
    _check_fuse(hip, sem, ids, 1, cap=4000, nc=4, thing=[1, 3], div=10000, stuff_area=9, void=0)


@pytest.mark.parametrize('up', [1, 4])
def test_fuse_misaligned(hip, up):
    """contiguous operands whose storage offset breaks the 4- and 8-byte alignment: scalar kernels, same labels"""
    D, H, W = 3, 16, 24
    sem, ids = fuse_stack(D, H, W, up, 12, 4, 22)
    n, m = sem.size, ids.size
    sem_buf = torch.zeros((n + 16,), dtype=torch.uint8, device='cuda')
    ids_buf = torch.zeros((m + 16,), dtype=torch.int16, device='cuda')
    sem_dev = sem_buf[1:1 + n].view(D, H, W)
    ids_dev = ids_buf[1:1 + m].view(D, H // up, W // up)
    sem_dev.copy_(_dev(sem))
    ids_dev.copy_(_dev(ids.astype(np.int16)))
    assert sem_dev.is_contiguous() and ids_dev.is_contiguous()
    assert sem_dev.data_ptr() % 4 == 1 and ids_dev.data_ptr() % 8 == 2
    exp = _check_fuse(hip, sem, ids, up, sem_dev=sem_dev, ids_dev=ids_dev, **FUSE_KW)
    # and with one operand misaligned at a time
    _check_fuse(hip, sem, ids, up, sem_dev=sem_dev, forms=('two',), **FUSE_KW)
    _check_fuse(hip, sem, ids, up, ids_dev=ids_dev, forms=('two',), **FUSE_KW)
    np.testing.assert_array_equal(_check_fuse(hip, sem, ids, up, forms=('two',), **FUSE_KW), exp)


FUSE_EDGE_SHAPES = [(8, 16), (9, 14)]


def fuse_value_edges(H, W):
    """classes 0, 2 stuff, 1, 3 things, stuff_area 6.  Laid out along the flat pixel order:
    id 1: 4 pixels of class 1 and 4 of class 3 (tie -> class 1);  id 2: only on class-0 pixels (consumes no number);
    id 3: class 1 (second instance of class 1);  id 4: class byte 7 (counts as 3);  class 0: exactly 6 pixels (kept);
    class 2: exactly 5 pixels (void);  the rest: class 1 with id 0 (void) or id 5"""
    sem = np.full(H * W, 1, dtype=np.uint8)
    ids = np.zeros(H * W, dtype=np.int64)
    ids[H * W // 2:] = 5
    p = 0

    def put(n, c, i):
        nonlocal p
        sem[p:p + n] = c
        ids[p:p + n] = i
        p += n
    put(4, 1, 1), put(4, 3, 1), put(3, 0, 2), put(7, 1, 3), put(5, 7, 4), put(3, 0, 0), put(2, 2, 4), put(3, 2, 0)
    return sem.reshape(1, H, W), ids.reshape(1, H, W)


@pytest.mark.parametrize('H,W', FUSE_EDGE_SHAPES, ids=[f'{H}x{W}' for H, W in FUSE_EDGE_SHAPES])
def test_fuse_value_edges(hip, H, W):
    sem, ids = fuse_value_edges(H, W)
    kw = dict(cap=5, nc=4, thing=[1, 3], div=1000, stuff_area=6, void=255)
    exp = _check_fuse(hip, sem, ids, 1, **kw).ravel()
    # what the layout is there to show, stated on the reference
    assert (exp[0:8] == 1001).all() and (exp[11:18] == 1002).all() and (exp[18:23] == 3001).all()
    assert (exp[8:11] == 0).all() and (exp[23:26] == 0).all()           # class 0: area 6 == stuff_area
    assert (exp[26:31] == 255).all() and exp[31] == 255 and exp[-1] == 1003


FUSE_HIGH_SHAPES = [(16, 24), (5, 7)]


@pytest.mark.parametrize('H,W', FUSE_HIGH_SHAPES, ids=[f'{H}x{W}' for H, W in FUSE_HIGH_SHAPES])
def test_fuse_high_labels(hip, H, W):
    """labels >= 2^31 (class 2 x 2^30): the uint32 map holds them, the int64 map holds them zero-extended"""
    sem, ids = fuse_stack(2, H, W, 1, 12, 3, 23)
    exp = _check_fuse(hip, sem, ids, 1, cap=12, nc=3, thing=[2], div=1 << 30, stuff_area=4, void=0)
    assert exp.max() > (1 << 31)


FUSE_ABOVE = [('vec4', 16, 24, 1, 12), ('up2', 16, 24, 2, 12), ('up4', 16, 24, 4, 12), ('nolds', 32, 64, 1, 4000)]


def fuse_above_cap(H, W, up, cap):
    sem, ids = fuse_stack(2, H, W, up, cap, 4, 24)
    ids[0, 1:4, :] = cap + 1                                      # thing and stuff pixels of slice 0 alike
    ids[0, -1, ::2] = cap + 1
    return sem, ids


@pytest.mark.parametrize('name,H,W,up,cap', FUSE_ABOVE, ids=[c[0] for c in FUSE_ABOVE])
def test_fuse_ids_above_cap(hip, name, H, W, up, cap):
    """an id of cap + 1 counts as 0 in both passes; slice 1 (whose tables follow slice 0's) is untouched.  Only
    cap + 1 is used: it would index the LDS stuff bins or slice 1's tables, inside the workspace of the two-call form.
    The void label is not 0: entry 0 of slice 1's label table, which such an id would read, is."""
    sem, ids = fuse_above_cap(H, W, up, cap)
    assert np.isin(sem[0][np.repeat(np.repeat(ids[0], up, 0), up, 1) == cap + 1], [1, 3]).any()
    _check_fuse(hip, sem, ids, up, cap=cap, nc=4, thing=[1, 3], div=10000, stuff_area=9, void=255, forms=('two',))
