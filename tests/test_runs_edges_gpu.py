"""GPU: edges and dispatch branches of the run, range and track kernels (csrc/emp_runs.hip, emp_ranges.hip,
emp_tracks.hip).

Everything here is integer work: every comparison is exact equality.  Each kernel is compared with a plain numpy /
pure-Python statement of the operation written in this file (a row scan, a flood fill, a dense coverage count, a painted
array) and with the existing oracle (oracle/rle_seg.py, oracle/rle_ops.py, oracle/tracks.py); the two must agree on the
CPU before a GPU result is looked at (``*_refs`` helpers; tests/test_runs_edges_host.py runs the same helpers without a
GPU).  Where the oracle follows the reference into undefined territory (malformed ranges, join_ranges of one list) only
the plain statement of the include/emp_hip.h contract is used at the raw entry point, and the oracle through the
array_utils wrapper on well-formed input.

Dispatch predicates and the tests that take each side
-----------------------------------------------------
row_runs_kernel<4|1>      W % 4 == 0 and 16-byte base: test_row_runs[W % 4 == 0]; W % 4 != 0: the other widths;
                          base 4 bytes off: the `unaligned` pass of test_row_runs (same data, scalar kernel)
  chunks of 64 / 256 px   below, at and above 1, 2 and 4 chunks (ROW_WIDTHS), runs aimed at each chunk border
  second grid trip        test_row_runs_second_grid_trip (69 000 rows > 65 536 waves)
scan_sums                 test_scan_edges: 524 288 (256 block sums) and 524 289 (257: second pass of the loop)
label kernels             hash pass on/off: plain classes, cc classes, classes >= 32 with a partial and the full mask;
                          second grid trip: test_label_second_grid_trip (1 126 400 runs > 1 048 576 threads)
fills (one wave per run)  second grid trip: test_fill_u32_many_runs (40 000 runs > 32 768 waves)
pair intersections        second grid trip: test_pair_intersections_many (530 000 pairs > 524 288 threads)
box_pairs                 nb = 1, 256, 257, 600 (one block, exactly one, two, three per box a)
"""
import collections
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

POS_BITS = 40
POS_MASK = (1 << POS_BITS) - 1


@pytest.fixture(scope='module')
def hip():
    from empanada_amd import _hip
    _hip.load()
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return _hip


def _dev(a, dtype=None):
    a = np.ascontiguousarray(a if dtype is None else np.asarray(a).astype(dtype))
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a).cuda()


def _np(t):
    return t.cpu().numpy()


def _np_u32(t):
    return _np(t.view(torch.int32) if t.dtype == torch.uint32 else t).view(np.uint32)


def _np_u64(t):
    return _np(t).view(np.uint64)


def _full(n, dtype, value=-7):
    return torch.full((max(int(n), 1),), value, dtype=dtype, device='cuda')


# =========================================================================================== 1. row runs
ROW_WIDTHS = [1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257, 260, 511, 512, 513, 516, 1028]
ROW_DH = (2, 3)
ROW_BIG = [(3, 23000, 5), (3, 23000, 8)]


def row_patterns(W, D=2, H=3):
    """name -> (D, H, W) uint32 stack.  Chunk borders of both vector widths (64 pixels for the scalar kernel, 256 for
    the 4-wide one) at one, two and four chunks are hit in different rows of the border patterns."""
    shape = (D, H, W)
    x = np.arange(W)
    rows = np.arange(D * H).reshape(D, H, 1)
    out = {}
    out['zero'] = np.zeros(shape, np.uint32)
    out['full'] = np.full(shape, 7, np.uint32)                     # one run per row; rows must not join
    out['v0v0'] = np.where((x + rows) % 2 == 0, 5, 0).astype(np.uint32)
    out['v1v2'] = np.where((x + rows) % 2 == 0, 5, 6).astype(np.uint32)
    borders = [64, 256, 128, 512, 192, 768]                        # one per row
    diff = np.zeros(shape, np.uint32)
    same = np.zeros(shape, np.uint32)
    span = np.zeros(shape, np.uint32)
    for r, c in enumerate(borders[:D * H]):
        d, y = divmod(r, H)
        diff[d, y, max(c - 5, 0):c] = 11                           # ends on a chunk's last pixel ...
        diff[d, y, c:c + 3] = 12                                   # ... and another value starts on the next one
        same[d, y, max(c - 5, 0):c + 3] = 13                       # one value across the border
        c0 = 64 if r % 2 == 0 else 256
        span[d, y, max(c0 - 1, 0):2 * c0 + 1] = 14                 # a run over three chunks
    out['border_diff'], out['border_same'], out['span3'] = diff, same, span
    hi = np.array([0x80000000, 0x80000000, 0xffffffff, 0, 0xffffffff, 0x80000000, 0x7fffffff], np.uint32)
    out['high'] = np.broadcast_to(hi[(x + rows) % len(hi)], shape).copy()
    join = np.zeros(shape, np.uint32)
    join[:, :, 0] = 9
    join[:, :, -1] = 9                                             # last pixel of a row == first of the next
    out['row_join'] = join
    rng = np.random.default_rng([W, 3])
    out['random'] = (rng.integers(0, 3, shape) * rng.integers(1, 3, shape)).astype(np.uint32)
    return out


def runs_scan(pan):
    """the plain statement: walk every row left to right; a run is a maximal span of one non-zero value.
    -> (row_counts int32 (D*H), r_start int32 (y*W + x0 inside the slice), r_len int32, r_val uint32), raster order"""
    D, H, W = pan.shape
    counts, st, ln, val = [], [], [], []
    for d in range(D):
        for y in range(H):
            row = pan[d, y].tolist()
            x = c = 0
            while x < W:
                v = row[x]
                if v == 0:
                    x += 1
                    continue
                x1 = x + 1
                while x1 < W and row[x1] == v:
                    x1 += 1
                st.append(y * W + x)
                ln.append(x1 - x)
                val.append(v)
                c += 1
                x = x1
            counts.append(c)
    return (np.array(counts, np.int32).reshape(-1), np.array(st, np.int32).reshape(-1),
            np.array(ln, np.int32).reshape(-1), np.array(val, np.uint32).reshape(-1))


def runs_oracle(pan):
    """the same table from oracle/tracks.lift_yz (the RLE along x of a dense labelling).  Its keys carry value - 1 in
    24 bits, so the values go in as their rank among the distinct values (runs depend on equality and zero only)."""
    from oracle import tracks as OT
    D, H, W = pan.shape
    lut = np.unique(np.concatenate([[0], pan.reshape(-1)])).astype(np.uint32)
    rank = np.searchsorted(lut, pan).astype(np.int64)
    key, ln = OT.lift_yz(rank, W)
    pos = (key & np.uint64(POS_MASK)).astype(np.int64)
    row, x = pos // W, pos % W
    val = lut[(key >> np.uint64(POS_BITS)).astype(np.int64) + 1]
    counts = np.bincount(row, minlength=D * H).astype(np.int32)
    return counts, ((row % H) * W + x).astype(np.int32), ln.astype(np.int32), val.astype(np.uint32)


def runs_numpy(pan):
    """vectorised form for the large stacks: a run starts where a non-zero pixel differs from the one before it"""
    D, H, W = pan.shape
    rows = pan.reshape(D * H, W)
    prev = np.zeros_like(rows)
    prev[:, 1:] = rows[:, :-1]
    nxt = np.zeros_like(rows)
    nxt[:, :-1] = rows[:, 1:]
    r, xs = np.nonzero((rows != 0) & (rows != prev))
    _, xe = np.nonzero((rows != 0) & (rows != nxt))
    counts = np.bincount(r, minlength=D * H).astype(np.int32)
    return counts, ((r % H) * W + xs).astype(np.int32), (xe + 1 - xs).astype(np.int32), rows[r, xs].astype(np.uint32)


def _same_tables(a, b, what):
    for u, v, name in zip(a, b, ('row_counts', 'r_start', 'r_len', 'r_val')):
        assert u.dtype == v.dtype and u.shape == v.shape, f'{what}: {name} {u.dtype}{u.shape} vs {v.dtype}{v.shape}'
        np.testing.assert_array_equal(u, v, err_msg=f'{what}: {name}')


def runs_refs(pan):
    a, b = runs_scan(pan), runs_oracle(pan)
    _same_tables(a, b, 'the two row-run references disagree')
    return a


def row_big_stack(D, H, W):
    """(stack, closed form).  Row r = d * H + y: empty when r % 5 == 0, else the run [0, 2) with value 1 + r % 1000 and
    the run [W - 1, W) with value 2000 + r % 7."""
    r = np.arange(D * H)
    live = r % 5 != 0
    pan = np.zeros((D * H, W), np.uint32)
    pan[live, 0] = pan[live, 1] = (1 + r % 1000)[live]
    pan[live, W - 1] = (2000 + r % 7)[live]
    rr = r[live]
    y = rr % H
    st = np.stack([y * W, y * W + W - 1], axis=1).reshape(-1).astype(np.int32)
    ln = np.tile(np.array([2, 1], np.int32), len(rr))
    val = np.stack([1 + rr % 1000, 2000 + rr % 7], axis=1).reshape(-1).astype(np.uint32)
    return pan.reshape(D, H, W), ((live * 2).astype(np.int32), st, ln, val)


def _gpu_runs_raw(hip, pan_t, D, H, W):
    """emp_runs_count -> scan -> emp_runs_extract on a (D, H, W) device stack, with sentinels behind the outputs"""
    n_rows = D * H
    rows = _full(n_rows + 1, torch.int32)
    hip.call('emp_runs_count', pan_t.data_ptr(), D, H, W, rows.data_ptr(), hip.stream())
    assert int(rows[n_rows]) == -7, 'emp_runs_count wrote past row_counts'
    offs = hip.exclusive_scan_i32(rows[:n_rows])
    n = int(offs[-1])
    st, ln, val = _full(n + 1, torch.int32), _full(n + 1, torch.int32), _full(n + 1, torch.int32)
    hip.call('emp_runs_extract', pan_t.data_ptr(), D, H, W, offs.data_ptr(), st.data_ptr(), ln.data_ptr(),
             val.data_ptr(), hip.stream())
    for t in (st, ln, val):
        assert int(t[n]) == -7, 'emp_runs_extract wrote past the run table'
    return _np(rows[:n_rows]), _np(st[:n]), _np(ln[:n]), _np_u32(val[:n])


def _check_runs(hip, pan, exp, what, wrapper=True):
    D, H, W = pan.shape
    t = _dev(pan)
    assert t.data_ptr() % 16 == 0
    _same_tables(_gpu_runs_raw(hip, t, D, H, W), exp, what + ' (raw)')
    # the same data 4 bytes off 16-byte alignment: the scalar kernel whatever W is
    buf = torch.zeros((pan.size + 8,), dtype=torch.int32, device='cuda')
    buf[1:1 + pan.size] = t.reshape(-1)
    off = buf[1:1 + pan.size].view(D, H, W)
    assert off.data_ptr() % 16 == 4 and off.is_contiguous()
    _same_tables(_gpu_runs_raw(hip, off, D, H, W), exp, what + ' (unaligned)')
    if wrapper:
        for src, tag in ((t, 'extract_runs'), (off, 'extract_runs, unaligned')):
            tab = hip.extract_runs(src.view(torch.uint32), 1000, [])
            assert tab.n_runs == len(exp[1])
            got = (_np(tab.row_offsets[1:] - tab.row_offsets[:-1]), _np(tab.r_start), _np(tab.r_len), _np_u32(tab.r_val))
            _same_tables(got, exp, f'{what} ({tag})')


@pytest.mark.parametrize('W', ROW_WIDTHS)
def test_row_runs(hip, W):
    for name, pan in row_patterns(W, *ROW_DH).items():
        _check_runs(hip, pan, runs_refs(pan), f'W={W} {name}')


@pytest.mark.parametrize('shape', ROW_BIG, ids=lambda s: 'x'.join(map(str, s)))
def test_row_runs_second_grid_trip(hip, shape):
    pan, exp = row_big_stack(*shape)
    _same_tables(runs_numpy(pan), exp, 'closed form')
    _check_runs(hip, pan, exp, f'{shape}', wrapper=False)


def test_row_runs_no_slices(hip):
    """D = 0: nothing is launched and nothing written"""
    pan = torch.zeros((16,), dtype=torch.int32, device='cuda')
    rows, offs = _full(4, torch.int32), torch.zeros((1,), dtype=torch.int32, device='cuda')
    out = [_full(4, torch.int32) for _ in range(3)]
    hip.call('emp_runs_count', pan.data_ptr(), 0, 3, 8, rows.data_ptr(), hip.stream())
    hip.call('emp_runs_extract', pan.data_ptr(), 0, 3, 8, offs.data_ptr(), *[o.data_ptr() for o in out], hip.stream())
    for t in [rows] + out:
        assert (_np(t) == -7).all()
    assert _np(hip.exclusive_scan_i32(rows[:0])).tolist() == [0]


# =========================================================================================== 2. components
def _run_rows(counts):
    return np.repeat(np.arange(len(counts)), counts)


def label_plain(pan, div, cc_classes):
    """the emp_hip.h contract by flood fill: a class in cc_classes (0..31 only: the mask has 32 bits) is split into
    8-connected components of equal value, labelled class * div + k in raster order of the first pixel, per slice and
    class; every other value is one component per (slice, value) and keeps its value.  Components are numbered over the
    stack in the order of their first pixel."""
    D, H, W = pan.shape
    cc = {int(c) for c in cc_classes if 0 <= int(c) < 32}
    comp_img = -np.ones(pan.shape, np.int64)
    c_slice, c_val, c_label, c_area, c_box = [], [], [], [], []
    for d in range(D):
        img = pan[d].astype(np.int64)
        rank = collections.Counter()
        for y in range(H):
            for x in range(W):
                v = int(img[y, x])
                if v == 0 or comp_img[d, y, x] >= 0:
                    continue
                k = len(c_slice)
                cls = v // div
                if cls in cc:
                    comp_img[d, y, x] = k
                    stack, ys, xs = [(y, x)], [], []
                    while stack:
                        py, px = stack.pop()
                        ys.append(py)
                        xs.append(px)
                        for qy in (py - 1, py, py + 1):
                            for qx in (px - 1, px, px + 1):
                                if 0 <= qy < H and 0 <= qx < W and comp_img[d, qy, qx] < 0 and img[qy, qx] == v:
                                    comp_img[d, qy, qx] = k
                                    stack.append((qy, qx))
                    rank[cls] += 1
                    label = cls * div + rank[cls]
                else:
                    m = img == v
                    comp_img[d][m] = k
                    ys, xs = np.nonzero(m)
                    label = v
                c_slice.append(d)
                c_val.append(v)
                c_label.append(label)
                c_area.append(len(ys))
                c_box.append((min(ys), min(xs), max(ys) + 1, max(xs) + 1))
    counts, st, ln, val = runs_scan(pan)
    row = _run_rows(counts)
    r_comp = comp_img[row // H, st // W, st % W].astype(np.int32) if len(st) else np.zeros(0, np.int32)
    n_comp = len(c_slice)
    c_first = np.full(n_comp, -1, np.int32)
    for i in range(len(r_comp) - 1, -1, -1):
        c_first[r_comp[i]] = i
    return dict(counts=counts, r_start=st, r_len=ln, r_val=val, r_comp=r_comp, n_comp=n_comp, comp_img=comp_img,
                c_slice=np.array(c_slice, np.int32).reshape(-1), c_val=np.array(c_val, np.int64).reshape(-1),
                c_label=np.array(c_label, np.int64).reshape(-1), c_area=np.array(c_area, np.int64).reshape(-1),
                c_box=np.array(c_box, np.int32).reshape(-1, 4), c_first=c_first)


def _encode(idx):
    """sorted flat indices -> [(start, length)] of the maximal contiguous spans, in so many words"""
    out = []
    for i in idx:
        if out and out[-1][0] + out[-1][1] == i:
            out[-1][1] += 1
        else:
            out.append([int(i), 1])
    return out


def _segs_plain(T, pan, div):
    """the rle_seg dicts of every slice from the flood-fill table: {class: {label: (box, [(start, length)])}}"""
    D = pan.shape[0]
    segs = [collections.defaultdict(dict) for _ in range(D)]
    for k in range(T['n_comp']):
        d = int(T['c_slice'][k])
        idx = np.flatnonzero(T['comp_img'][d].reshape(-1) == k)
        segs[d][int(T['c_val'][k]) // div][int(T['c_label'][k])] = (tuple(int(b) for b in T['c_box'][k]), _encode(idx))
    return [dict(s) for s in segs]


def _segs_from(rle_seg):
    return {int(c): {int(l): (tuple(int(b) for b in a['box']),
                              [[int(s), int(r)] for s, r in zip(a['starts'], a['runs'])])
                     for l, a in attrs.items()} for c, attrs in rle_seg.items() if len(attrs)}


def label_refs(pan, div, cc_classes):
    """flood-fill table, after oracle/rle_seg.pan_seg_to_rle_seg has agreed with it slice by slice"""
    from oracle import rle_seg as ORS
    T = label_plain(pan, div, cc_classes)
    things = [int(c) for c in cc_classes if 0 <= int(c) < 32]
    plain = _segs_plain(T, pan, div)
    for d in range(pan.shape[0]):
        img = pan[d].astype(np.int64)
        classes = sorted(set((img[img > 0] // div).tolist()))
        got = _segs_from(ORS.pan_seg_to_rle_seg(img, classes, div, things, force_connected=True))
        assert got == plain[d], f'the two component references disagree in slice {d}'
    T['segs'] = plain
    return T


def cc_mask_of(cc_classes):
    m = 0
    for c in cc_classes:
        if 0 <= int(c) < 32:
            m |= 1 << int(c)
    return m


_LABEL_COLS = ('r_comp', 'c_slice', 'c_label', 'c_area', 'c_box', 'c_first')


def _gpu_label_raw(hip, T, D, H, W, div, mask):
    n = len(T['r_start'])
    offs = _dev(np.concatenate([[0], np.cumsum(T['counts'])]).astype(np.int32))
    st, ln, val = _dev(T['r_start']), _dev(T['r_len']), _dev(T['r_val'])
    if n == 0:
        st = ln = val = _full(1, torch.int32)
    work = _full(hip.query('emp_runs_label_work_elems', n), torch.int32)
    r_comp, c_slice, c_first = _full(n + 1, torch.int32), _full(n + 1, torch.int32), _full(n + 1, torch.int32)
    c_label, c_area = _full(n + 1, torch.int64), _full(n + 1, torch.int64)
    c_box = _full(4 * (n + 1), torch.int32)
    ncomp = _full(1, torch.int32)
    hip.call('emp_runs_label', st.data_ptr(), ln.data_ptr(), val.data_ptr(), offs.data_ptr(), n, D, H, W, int(div),
             int(mask), work.data_ptr(), r_comp.data_ptr(), c_slice.data_ptr(), c_label.data_ptr(), c_area.data_ptr(),
             c_box.data_ptr(), c_first.data_ptr(), ncomp.data_ptr(), hip.stream())
    nc = int(ncomp[0])
    assert 0 <= nc <= n
    for t in (r_comp, c_slice, c_first, c_label, c_area):
        assert int(t[n]) == -7, 'emp_runs_label wrote past an output'
    return dict(n_comp=nc, r_comp=_np(r_comp[:n]), c_slice=_np(c_slice[:nc]), c_label=_np(c_label[:nc]),
                c_area=_np(c_area[:nc]), c_box=_np(c_box[:4 * nc]).reshape(-1, 4), c_first=_np(c_first[:nc]))


def _same_labels(got, T, what):
    assert got['n_comp'] == T['n_comp'], f"{what}: n_comp {got['n_comp']} != {T['n_comp']}"
    for c in _LABEL_COLS:
        assert got[c].dtype == T[c].dtype, f'{what}: {c} dtype'
        np.testing.assert_array_equal(got[c], T[c], err_msg=f'{what}: {c}')


def _check_label(hip, pan, div, cc_classes, what, mask=None, segs=True):
    D, H, W = pan.shape
    T = label_refs(pan, div, cc_classes)
    _same_labels(_gpu_label_raw(hip, T, D, H, W, div, cc_mask_of(cc_classes) if mask is None else mask), T,
                 what + ' (raw)')
    if mask is not None:
        return T
    from empanada_amd.inference import rle
    things = [int(c) for c in cc_classes]
    tab = hip.extract_runs(_dev(pan).view(torch.uint32), div, things)
    assert tab.n_runs == len(T['r_start'])
    _same_labels(dict(n_comp=tab.n_comp, **{c: _np(getattr(tab, c)) for c in _LABEL_COLS}), T, what + ' (extract_runs)')
    if segs:
        classes = sorted(set((pan[pan > 0].astype(np.int64) // div).tolist()))
        got, _ = rle.stack_to_rle_segs(_dev(pan).view(torch.uint32), classes, div, things, force_connected=True)
        assert [_segs_from(g) for g in got] == T['segs'], what + ' (stack_to_rle_segs)'
    return T


def _spiral(H, W):
    """one-pixel-wide rectangular spiral, arms two pixels apart (never 8-adjacent except along the path)"""
    img = np.zeros((H, W), bool)
    y0, x0, y1, x1 = 0, 0, H - 1, W - 1
    while y1 - y0 >= 2 and x1 - x0 >= 2:
        img[y0, x0:x1 + 1] = True
        img[y0:y1 + 1, x1] = True
        img[y1, x0 + 2:x1 + 1] = True
        img[y0 + 2:y1 + 1, x0 + 2] = True
        y0, x0, y1, x1 = y0 + 2, x0 + 2, y1 - 2, x1 - 2
    return img


def label_cases():
    """name -> (stack (D, H, W) uint32, label_divisor, cc classes)"""
    A, B, P = 1005, 1006, 3007                      # classes 1, 1 and 3 at divisor 1000; 3 is never a cc class here
    cases = {}
    yy, xx = np.mgrid[0:9, 0:12]
    cases['checker_one'] = (np.where((yy + xx) % 2 == 0, A, 0)[None], 1000, [1])
    cases['checker_two'] = (np.where((yy + xx) % 2 == 0, A, B)[None], 1000, [1])
    s = np.zeros((2, 10, 10), np.int64)
    s[0][np.arange(10), np.arange(10)] = A          # staircase down-right
    s[1][np.arange(10), 9 - np.arange(10)] = A      # staircase down-left
    s[1, 0, 0:3] = A
    s[1, 2, 0:2] = A
    cases['stairs'] = (s, 1000, [1])
    e = np.zeros((4, 3, 8), np.int64)
    e[0, 0, 1] = e[0, 1, 0] = A                     # diagonal contact only, at x = 0 ...
    e[1, 0, 0] = e[1, 1, 1] = A
    e[2, 0, 6] = e[2, 1, 7] = A                     # ... and at x = W - 1
    e[3, 0, 7] = e[3, 1, 6] = A
    e[:, 2, 3] = B
    cases['diag_at_ends'] = (e, 1000, [1])
    w = np.zeros((2, 3, 9), np.int64)
    w[0, 0, 6:9] = w[0, 1, 0:2] = A                 # ends at W - 1 above a run that starts at 0: no wrap
    w[1, 1, 5:9] = w[1, 2, 0:4] = A
    cases['no_wrap'] = (w, 1000, [1])
    c = np.zeros((4, 12, 21), np.int64)
    c[0, :, ::2] = A
    c[0, :11, :] = np.where(c[0, :11, :] > 0, A, 0)
    c[0, 11, :] = A                                 # comb: the teeth join on the last row
    c[1, :, 0] = c[1, :, 20] = c[1, 11, :] = A      # U
    c[1, :8, 10] = B
    c[2][_spiral(12, 21)] = A
    c[3][_spiral(12, 21)[::-1]] = A                 # the spiral upside down: it joins from below
    c[2, 11, 18] = A
    cases['comb_u_spiral'] = (c, 1000, [1])
    for i, dens in enumerate((0.4, 0.55, 0.7)):
        rng = np.random.default_rng([5, i])
        r = np.where(rng.random((2, 40, 70)) < dens, A, 0)
        r[1] = np.where(r[1] > 0, np.where(rng.random((40, 70)) < 0.5, A, B), 0)
        cases[f'random_{dens}'] = (r, 1000, [1])
    a = np.zeros((1, 6, 10), np.int64)
    a[0, 1:5, 1:5] = A
    a[0, 1:5, 5:9] = B                              # two values of one class side by side
    cases['adjacent_values'] = (a, 1000, [1])
    g = np.zeros((4, 6, 9), np.int64)
    g[0, 1, 2:5] = g[0, 3, 2:5] = g[0, 4, 3:6] = A  # rows 0, 2 and 5 empty; slice 1 empty
    g[2, 0, :] = g[2, 5, :] = A
    g[3, 2, 4] = P
    cases['empty_rows'] = (g, 1000, [1])
    t = np.zeros((3, 4, 8), np.int64)
    t[0, 3, :] = t[1, 0, :] = A                     # last row of slice 0, first row of slice 1: two components
    t[1, 3, 4:] = t[2, 0, :4] = 2004
    t[2, 2, :] = A
    cases['across_slices'] = (t, 1000, [1, 2])
    o = np.zeros((2, 5, 20), np.int64)
    o[0, ::2, ::2] = 5                              # 30 separate pixels of class 1 at divisor 4: labels run past it
    o[1, 0, ::2] = 6
    o[1, 2, ::2] = 9                                # class 2
    cases['past_divisor'] = (o, 4, [1, 2])
    p = np.zeros((2, 8, 12), np.int64)
    p[0, ::3, ::4] = P
    p[0, 7, 11] = P
    p[1, 2, 3] = p[1, 6, 9] = P                     # one value scattered: one component per slice
    p[1, 4, 4:8] = A
    cases['plain_scattered'] = (p, 1000, [1])
    m = np.zeros(2 * 40 * 70, np.int64)
    m[:5000] = 1 + np.random.default_rng(9).permutation(5000)
    cases['plain_5000_values'] = (m.reshape(2, 40, 70), 10000, [3])
    h = np.zeros((2, 6, 10), np.int64)
    h[0, 1, 1:4] = h[0, 4, 6:9] = 0x80000005
    h[0, 2, 5] = 0xffffffff
    h[1, 0, :] = 0xfffffffe
    h[1, 3, 2] = h[1, 5, 7] = 0x80000005
    cases['plain_high_values'] = (h, 1000, [1])
    q = h.copy()
    cases['cc_high_values'] = (q, 1 << 30, [2, 3])  # 0x80000005 is class 2, 0xfffffffe class 3: split into components
    return {k: (np.ascontiguousarray(v[0]).astype(np.uint32), v[1], v[2]) for k, v in cases.items()}


LABEL_CASES = label_cases()


@pytest.mark.parametrize('name', list(LABEL_CASES))
def test_label(hip, name):
    pan, div, cc = LABEL_CASES[name]
    T = _check_label(hip, pan, div, cc, name)
    if name in ('checker_one', 'checker_two'):
        assert T['n_comp'] == {'checker_one': 1, 'checker_two': 2}[name]
    if name == 'past_divisor':
        assert T['c_label'].max() == 1 * 4 + 30 and T['n_comp'] == 50


def high_class_stack():
    """class 33 (divisor 10: values 330..339) next to cc class 1 and plain class 2"""
    s = np.zeros((2, 6, 12), np.uint32)
    s[0, 0, 0:3] = s[0, 2, 5:8] = s[0, 5, 9:12] = 335       # three separate blobs of one value of class 33
    s[0, 3, 0:2] = 337
    s[0, 1, 4:6] = s[0, 4, 4:6] = 15                        # class 1: two components
    s[0, 0, 8] = s[0, 3, 10] = 25                           # class 2
    s[1, 1, 1] = s[1, 4, 8] = 335
    s[1, 2, 3:5] = 15
    return s, 10


@pytest.mark.parametrize('mask', [0b010, 0xffffffff], ids=['partial_mask', 'full_mask'])
def test_label_class_32_and_up_raw(hip, mask):
    """a class of 32 or more is grouped by value whatever the mask says: one component per (slice, value).  With the
    full mask the value-grouping pass used to be skipped and every such run became its own component."""
    pan, div = high_class_stack()
    cc = [c for c in range(32) if (mask >> c) & 1]
    T = _check_label(hip, pan, div, cc, f'mask {mask:#x}', mask=mask)
    k = np.flatnonzero((T['c_val'] == 335) & (T['c_slice'] == 0))
    assert len(k) == 1 and T['c_area'][k[0]] == 9 and T['c_box'][k[0]].tolist() == [0, 0, 6, 12]


def test_label_class_32_and_up_refused(hip):
    """a connected-component class outside 0..31 does not fit the 32-bit mask (it used to be dropped silently, and
    the class grouped by value): extract_runs and stack_to_rle_segs refuse it"""
    from empanada_amd.inference import rle
    pan, div = high_class_stack()
    t = _dev(pan).view(torch.uint32)
    for bad in (33, 32, -1):
        with pytest.raises(ValueError, match='0..31'):
            hip.extract_runs(t, div, [1, bad])
    with pytest.raises(ValueError, match='0..31'):
        rle.stack_to_rle_segs(t, [1, 2, 33], div, [1, 33], force_connected=True)
    segs, _ = rle.stack_to_rle_segs(t, [1, 2, 33], div, [1, 33], force_connected=False)     # no cc class: accepted
    assert sorted(segs[0][33]) == [335, 337]


def test_label_second_grid_trip(hip):
    """vertical stripes: 1 126 400 runs (> 256 * 4096 threads) in 1 024 components with closed-form columns"""
    H, W = 1100, 2048
    pan = np.zeros((1, H, W), np.uint32)
    pan[0, :, ::2] = 1001
    y, k = np.divmod(np.arange(H * 1024), 1024)
    T = dict(counts=np.full(H, 1024, np.int32), r_start=(y * W + 2 * k).astype(np.int32),
             r_len=np.ones(H * 1024, np.int32), r_val=np.full(H * 1024, 1001, np.uint32))
    _same_tables(runs_numpy(pan), (T['counts'], T['r_start'], T['r_len'], T['r_val']), 'closed form')
    c = np.arange(1024)
    exp = dict(n_comp=1024, r_comp=k.astype(np.int32), c_slice=np.zeros(1024, np.int32), c_label=1001 + c,
               c_area=np.full(1024, H, np.int64), c_first=c.astype(np.int32),
               c_box=np.stack([0 * c, 2 * c, 0 * c + H, 2 * c + 1], axis=1).astype(np.int32))
    _same_labels(_gpu_label_raw(hip, T, 1, H, W, 1000, 0b10), exp, 'stripes (raw)')
    tab = hip.extract_runs(_dev(pan).view(torch.uint32), 1000, [1])
    assert tab.n_runs == H * 1024
    _same_labels(dict(n_comp=tab.n_comp, **{c_: _np(getattr(tab, c_)) for c_ in _LABEL_COLS}), exp, 'stripes')


def test_label_no_runs(hip):
    T = label_refs(np.zeros((2, 3, 4), np.uint32), 1000, [1])
    assert _gpu_label_raw(hip, T, 2, 3, 4, 1000, 2)['n_comp'] == 0
    assert hip.extract_runs(_dev(np.zeros((2, 3, 4), np.uint32)).view(torch.uint32), 1000, [1]).n_comp == 0


# =========================================================================================== 3. overlaps
def overlap_cases():
    A, B, C = 1005, 1006, 2005
    cases = {}
    one = np.zeros((1, 4, 10), np.int64)
    one[0, 1, 2:7] = A
    cases['single_slice'] = one
    rng = np.random.default_rng(11)
    r = (rng.integers(0, 3, (1, 12, 30)) * rng.integers(1000, 1003, (1, 12, 30)))
    cases['identical'] = np.concatenate([r, r])
    sh = np.zeros((1, 12, 30), np.int64)
    sh[0, :, 1:] = r[0, :, :-1]
    cases['shifted'] = np.concatenate([r, sh, r])
    t = np.zeros((2, 3, 12), np.int64)
    t[0, 0, 2:5] = t[1, 0, 5:8] = A                  # b0 == a1: no common pixel
    t[0, 1, 5:8] = t[1, 1, 2:5] = A                  # b1 == a0
    t[0, 2, 0:4] = t[1, 2, 3:12] = A                 # one common pixel
    cases['touching'] = t
    k = np.zeros((2, 2, 10), np.int64)
    k[0, 0, 2:8] = A
    k[1, 0, 2:8] = C                                 # same span, another class
    k[0, 1, 2:8] = A
    k[1, 1, 2:8] = B                                 # same span, same class, another value
    cases['other_class'] = k
    cases['empty_middle'] = np.concatenate([r, np.zeros_like(r), r])
    return {n: v.astype(np.uint32) for n, v in cases.items()}


OVERLAP_CASES = overlap_cases()


def overlap_plain(pan, div, T):
    """per pair of runs in consecutive slices, same row, same class: the number of common pixels, counted pixel by
    pixel -> Counter of (comp_a, comp_b, pixels)"""
    D, H, W = pan.shape
    run_img = -np.ones((D, H * W), np.int64)
    row = _run_rows(T['counts'])
    for i, (s, l) in enumerate(zip(T['r_start'], T['r_len'])):
        run_img[row[i] // H, s:s + l] = i
    cls = pan.reshape(D, H * W).astype(np.int64) // div
    out = collections.Counter()
    for d in range(D - 1):
        both = (run_img[d] >= 0) & (run_img[d + 1] >= 0) & (cls[d] == cls[d + 1])
        pairs = collections.Counter(zip(run_img[d][both].tolist(), run_img[d + 1][both].tolist()))
        for (ra, rb), n in pairs.items():
            out[(int(T['r_comp'][ra]), int(T['r_comp'][rb]), n)] += 1
    return out


def reduce_plain(trip):
    acc = collections.defaultdict(int)
    for a, b, n in trip:
        acc[(int(a), int(b))] += int(n)
    return np.array([[a, b, n] for (a, b), n in sorted(acc.items())], np.int64).reshape(-1, 3)


def overlap_refs(pan, div, cc):
    """run-pair triplets by pixel count; their sum per component pair must be oracle/rle_ops.rle_intersection of the
    two components' run lists, and zero for every pair of one class that has no triplet"""
    from oracle import rle_ops as ORO
    T = label_refs(pan, div, cc)
    trip = overlap_plain(pan, div, T)
    red = {(a, b): n for a, b, n in reduce_plain([t for t, m in trip.items() for _ in range(m)]).tolist()}
    runs_of = [np.flatnonzero(T['r_comp'] == k) for k in range(T['n_comp'])]
    for a in range(T['n_comp']):
        for b in range(T['n_comp']):
            if T['c_slice'][b] != T['c_slice'][a] + 1 or T['c_val'][a] // div != T['c_val'][b] // div:
                assert (a, b) not in red
                continue
            ia, ib = runs_of[a], runs_of[b]
            n = ORO.rle_intersection(T['r_start'][ia].astype(np.int64), T['r_len'][ia].astype(np.int64),
                                     T['r_start'][ib].astype(np.int64), T['r_len'][ib].astype(np.int64))
            assert n == red.get((a, b), 0), 'the two overlap references disagree'
    return T, trip


def _gpu_overlap_raw(hip, T, D, H, W, div, cap):
    n = len(T['r_start'])
    offs = _dev(np.concatenate([[0], np.cumsum(T['counts'])]).astype(np.int32))
    cols = [_dev(T[c]) if n else _full(1, torch.int32) for c in ('r_start', 'r_len', 'r_comp', 'r_val')]
    out = _full(3 * (cap + 1), torch.int32)
    cnt = _full(1, torch.int32)
    hip.call('emp_runs_overlap_next', *[c.data_ptr() for c in cols], offs.data_ptr(), n, D, H, W, int(div),
             out.data_ptr() if cap else None, cap, cnt.data_ptr(), hip.stream())
    assert (_np(out[3 * cap:]) == -7).all(), 'emp_runs_overlap_next wrote past cap'
    return int(cnt[0]), _np(out[:3 * cap]).reshape(-1, 3)


@pytest.mark.parametrize('name', list(OVERLAP_CASES))
def test_overlap_next(hip, name):
    pan, div, cc = OVERLAP_CASES[name], 1000, [1]
    D, H, W = pan.shape
    T, trip = overlap_refs(pan, div, cc)
    true = sum(trip.values())
    if name in ('single_slice', 'other_class'):
        assert true == (0 if name == 'single_slice' else 1)
    if name == 'touching':
        assert sorted(trip) == [(1, 2, 1)]           # the pairs that only touch give nothing, not a zero-pixel triplet
    n, rows = _gpu_overlap_raw(hip, T, D, H, W, div, true + 8)
    assert n == true
    got = collections.Counter(map(tuple, rows[:n].tolist()))
    assert got == trip and all(t[2] > 0 for t in got)
    for cap in sorted({0, true // 2}):
        n, rows = _gpu_overlap_raw(hip, T, D, H, W, div, cap)
        assert n == true, 'n_out must hold the true count'
        first = collections.Counter(map(tuple, rows[:min(cap, true)].tolist()))
        assert not first - trip, 'rows below cap must come from the true multiset'
    tab = hip.extract_runs(_dev(pan).view(torch.uint32), div, cc)
    red = _np(hip.overlap_next(tab, div)).astype(np.int64).reshape(-1, 3)
    np.testing.assert_array_equal(red, reduce_plain([t for t, m in trip.items() for _ in range(m)]))


def reduce_inputs():
    rng = np.random.default_rng(13)
    same = np.stack([np.full(5000, 70000), np.full(5000, 3), rng.integers(1, 50, 5000)], axis=1)
    distinct = np.stack([rng.permutation(5000) // 7, rng.permutation(5000), rng.integers(1, 50, 5000)], axis=1)
    mixed = np.stack([rng.integers(0, 40, 5000), rng.integers(0, 40, 5000), rng.integers(1, 50, 5000)], axis=1)
    return {'all_equal': same, 'all_distinct': distinct, 'one': np.array([[4, 2, 9]]), 'mixed': mixed}


REDUCE_INPUTS = reduce_inputs()


def reduce_refs(trip):
    from oracle import tracks as OT
    a, b = reduce_plain(trip), OT.reduce_triplets(trip)
    np.testing.assert_array_equal(a, b, err_msg='the two reduce references disagree')
    return a


@pytest.mark.parametrize('name', list(REDUCE_INPUTS))
def test_triplets_reduce(hip, name):
    trip = REDUCE_INPUTS[name]
    exp = reduce_refs(trip)
    assert len(exp) == {'all_equal': 1, 'all_distinct': 5000, 'one': 1}.get(name, len(exp))
    got = _np(hip.reduce_triplets(_dev(trip, np.int32))).astype(np.int64)
    np.testing.assert_array_equal(got, exp)


def test_workspace_one_byte_short(hip):
    """emp_triplets_reduce, emp_vote_ranges and emp_track_sort refuse a workspace one byte short, before any launch"""
    n = 100
    buf = _full(1 << 16, torch.int64)
    out = _full(4 * n, torch.int64)
    cnt = _full(1, torch.int32)
    wb = hip.query('emp_triplets_reduce_work_bytes', n)
    work = torch.empty((wb,), dtype=torch.uint8, device='cuda')
    with pytest.raises(hip.HipError, match='workspace too small'):
        hip.call('emp_triplets_reduce', buf.data_ptr(), n, work.data_ptr(), wb - 1, out.data_ptr(), cnt.data_ptr(),
                 hip.stream())
    wb = hip.query('emp_vote_work_bytes', n)
    work = torch.empty((wb,), dtype=torch.uint8, device='cuda')
    with pytest.raises(hip.HipError, match='workspace too small'):
        hip.call('emp_vote_ranges', buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), n, 4, 1, work.data_ptr(), wb - 1,
                 out.data_ptr(), cnt.data_ptr(), hip.stream())
    wb = hip.query('emp_track_sort_work_bytes', n)
    work = torch.empty((wb,), dtype=torch.uint8, device='cuda')
    with pytest.raises(hip.HipError, match='workspace too small'):
        hip.call('emp_track_sort', buf.data_ptr(), buf.data_ptr(), n, 1, work.data_ptr(), wb - 1, out.data_ptr(),
                 out.data_ptr(), out.data_ptr(), cnt.data_ptr(), hip.stream())
    assert (_np(out) == -7).all() and int(cnt[0]) == -7


# =========================================================================================== 4. scan and sort
SCAN_N = [0, 1, 2047, 2048, 2049, 524288, 524289]


def scan_input(n):
    return np.random.default_rng([17, n]).integers(-3, 4, n).astype(np.int32)


def scan_refs(x):
    exp = np.concatenate([[0], np.cumsum(x.astype(np.int64))])
    if len(x) <= 2049:
        acc, plain = 0, [0]
        for v in x.tolist():
            acc += v
            plain.append(acc)
        assert plain == exp.tolist()
    assert np.abs(exp).max(initial=0) < 2 ** 31
    return exp.astype(np.int32)


@pytest.mark.parametrize('n', SCAN_N)
def test_scan_edges(hip, n):
    x = scan_input(n)
    exp = scan_refs(x)
    got = _np(hip.exclusive_scan_i32(_dev(x) if n else torch.zeros((0,), dtype=torch.int32, device='cuda')))
    assert got.shape == (n + 1,)
    np.testing.assert_array_equal(got, exp)


def sort_input(n=3000, seed=19):
    """keys = instance << 40 | position with few distinct instances and few distinct positions: many ties in each
    field; every fourth key has bit 63 set"""
    rng = np.random.default_rng(seed)
    inst = rng.integers(0, 12, n).astype(np.uint64)
    inst[::4] |= np.uint64(1 << 23)
    pos = rng.integers(0, 40, n).astype(np.uint64) * np.uint64((1 << 39) // 40)
    return (inst << np.uint64(POS_BITS)) | pos


def sort_refs(keys, b0, b1):
    """stable order by the bit field [b0, b1): numpy's stable argsort against a decorated Python sort"""
    field = (keys >> np.uint64(b0)) & np.uint64((1 << (b1 - b0)) - 1) if b1 - b0 < 64 else keys
    order = np.argsort(field, kind='stable')
    plain = [i for _, i in sorted((int(f), i) for i, f in enumerate(field.tolist()))]
    assert order.tolist() == plain
    return order


@pytest.mark.parametrize('bits', [(40, 64), (0, 40), (0, 64), (63, 64)], ids=lambda b: f'{b[0]}-{b[1]}')
def test_sort_bit_ranges(hip, bits):
    keys = sort_input()
    order = sort_refs(keys, *bits)
    ko, vo = hip.sort_u64_i32(_dev(keys), _dev(np.arange(len(keys), dtype=np.int32)), *bits)
    np.testing.assert_array_equal(_np(vo), order.astype(np.int32))
    np.testing.assert_array_equal(_np_u64(ko), keys[order])


def test_sort_tiny_and_workspace(hip):
    k = np.array([(1 << 63) | 5], np.uint64)
    ko, vo = hip.sort_u64_i32(_dev(k), _dev(np.array([42], np.int32)))
    assert _np_u64(ko).tolist() == k.tolist() and _np(vo).tolist() == [42]
    e64, e32 = torch.zeros((0,), dtype=torch.int64, device='cuda'), torch.zeros((0,), dtype=torch.int32, device='cuda')
    ko, vo = hip.sort_u64_i32(e64, e32)
    assert ko.numel() == 0 and vo.numel() == 0
    # the smallest workspace the sort accepts, by bisection (calls that are refused launch nothing; accepted ones are
    # ordinary sorts inside a buffer of the full advertised size); one byte less is refused and writes nothing
    n = 3000
    keys = sort_input(n)
    kin, vin = _dev(keys), _dev(np.arange(n, dtype=np.int32))
    full = hip.query('emp_sort_work_bytes', n)
    work = torch.empty((full,), dtype=torch.uint8, device='cuda')

    def run(wb, kout, vout):
        hip.call('emp_sort_u64_i32', kin.data_ptr(), kout.data_ptr(), vin.data_ptr(), vout.data_ptr(), n, 0, 64,
                 work.data_ptr(), wb, hip.stream())

    def accepted(wb):
        try:
            run(wb, _full(n, torch.int64), _full(n, torch.int32))
            return True
        except hip.HipError as e:
            assert 'workspace too small' in str(e)
            return False

    assert accepted(full)
    lo, hi = 0, full                               # lo refused (or 0), hi accepted
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if accepted(mid):
            hi = mid
        else:
            lo = mid
    kout, vout = _full(n, torch.int64), _full(n, torch.int32)
    if hi > 1:
        with pytest.raises(hip.HipError, match='workspace too small'):
            run(hi - 1, kout, vout)
        assert (_np(kout) == -7).all() and (_np(vout) == -7).all()
    run(hi, kout, vout)
    np.testing.assert_array_equal(_np_u64(kout), np.sort(keys))


# =========================================================================================== 5. vote ranges
VOTE_SPAN = 4096


def vote_plain(starts, ends, grp, n_groups, thr, base=0):
    """coverage count over a dense array per group: the maximal intervals where at least thr ranges cover a position
    -> (out_ranges (m, 2) int64 sorted by (group, start), out_off (n_groups + 1) int32); only the groups that occur
    are walked"""
    out, per = [], collections.Counter()
    for g in sorted(set(grp.tolist())):
        cov = np.zeros(VOTE_SPAN + 1, np.int64)
        for s, e, gg in zip(starts.tolist(), ends.tolist(), grp.tolist()):
            if gg == g:
                cov[s - base:e - base] += 1
        ok = np.concatenate([[0], (cov >= thr).astype(np.int8), [0]])
        d = np.diff(ok)
        for s, e in zip(np.flatnonzero(d == 1), np.flatnonzero(d == -1)):
            out.append((int(s) + base, int(e) + base))
            per[g] += 1
    off = np.zeros(n_groups + 1, np.int64)
    for g, c in per.items():
        off[g + 1:] += c
    return np.array(out, np.int64).reshape(-1, 2), off.astype(np.int32)


def vote_cases():
    """name -> (starts, ends, groups, n_groups, base)"""
    def pack(rows, n_groups, base=0):
        a = np.array(rows, np.int64).reshape(-1, 3)
        return a[:, 0] + base, a[:, 1] + base, a[:, 2].astype(np.int32), n_groups, base
    cases = {}
    rows = [(10, 20, 1), (20, 30, 1), (30, 31, 1),                     # touching: merge at threshold 1
            (100, 200, 1), (120, 180, 1), (120, 180, 1), (150, 160, 1),    # nested and duplicated
            (300, 300, 1), (305, 305, 1), (310, 320, 1), (315, 315, 1),    # empty ranges
            (0, 5, 4), (3, 9, 4), (4, 4096, 4), (4000, 4096, 4),
            (50, 60, 6), (55, 65, 6), (58, 70, 6), (70, 80, 6)]
    cases['mixed'] = pack(rows, 9)                                     # groups 0, 2, 3, 5, 7, 8 have no ranges
    rng = np.random.default_rng(23)
    s = rng.integers(0, 4000, 600)
    rnd = np.stack([s, s + rng.integers(0, 90, 600), rng.integers(0, 5, 600) * 2 + 1], axis=1)
    cases['random'] = pack(rnd, 12)
    cases['no_ranges'] = pack([], 5)
    cases['top_group'] = pack([(5, 50, (1 << 22) - 2), (40, 90, (1 << 22) - 2), (7, 9, 3), (8, 12, 3)], (1 << 22) - 1)
    cases['near_2_40'] = pack(rows, 9, base=(1 << 40) - VOTE_SPAN - 1)         # the largest end is 2^40 - 1
    return cases


VOTE_CASES = vote_cases()
VOTE_THR = [1, 2, 3, 700]


def vote_lists():
    """well-formed input for the array_utils wrapper: lists of ranges, each sorted and disjoint"""
    rng = np.random.default_rng(29)
    lists = []
    for _ in range(4):
        cuts = np.sort(rng.choice(3000, 60, replace=False))
        lists.append(np.stack([cuts[0::2], cuts[1::2]], axis=1).astype(np.int64))
    return lists


def vote_lists_refs(lists, thr):
    """oracle/rle_ops.vote_by_ranges against the coverage count, on well-formed input"""
    from oracle import rle_ops as ORO
    cat = np.concatenate(lists)
    plain, _ = vote_plain(cat[:, 0], cat[:, 1], np.zeros(len(cat), np.int32), 1, thr)
    got = np.asarray(ORO.vote_by_ranges(lists, thr), np.int64).reshape(-1, 2)
    np.testing.assert_array_equal(got, plain, err_msg='the two voting references disagree')
    return plain


@pytest.mark.parametrize('name', list(VOTE_CASES))
def test_vote_ranges_raw(hip, name):
    starts, ends, grp, n_groups, base = VOTE_CASES[name]
    n = len(starts)
    for thr in VOTE_THR:
        exp, exp_off = vote_plain(starts, ends, grp, n_groups, thr, base)
        if thr == 700:
            assert len(exp) == 0
        wb = hip.query('emp_vote_work_bytes', n)
        work = torch.empty((wb,), dtype=torch.uint8, device='cuda')
        out = _full(2 * (n + 1), torch.int64)
        off = _full(n_groups + 2, torch.int32)
        args = [_dev(a) if n else _full(1, torch.int64) for a in (starts, ends, grp)]
        hip.call('emp_vote_ranges', *[a.data_ptr() for a in args], n, n_groups, thr, work.data_ptr(), wb,
                 out.data_ptr(), off.data_ptr(), hip.stream())
        assert int(off[n_groups + 1]) == -7
        got_off = _np(off[:n_groups + 1])
        np.testing.assert_array_equal(got_off, exp_off, err_msg=f'{name} thr={thr}: out_off')
        m = int(got_off[-1])
        np.testing.assert_array_equal(_np(out[:2 * m]).reshape(-1, 2), exp, err_msg=f'{name} thr={thr}: out_ranges')
        assert (_np(out[2 * n:]) == -7).all()


@pytest.mark.parametrize('thr', [2, 3])
def test_vote_by_ranges_wrapper(hip, thr):
    from empanada_amd import array_utils as AU
    lists = vote_lists()
    exp = vote_lists_refs(lists, thr)
    np.testing.assert_array_equal(np.asarray(AU.vote_by_ranges(lists, thr), np.int64).reshape(-1, 2), exp)


# =========================================================================================== 6. pair intersections
def pair_instances():
    """12 instances (CSR over int64 starts / lengths), sorted disjoint runs below 600: instance 3 has no runs, 4 and 5
    share their starts, 6 and 7 touch each other everywhere, 8 touches itself (runs that end where the next starts)"""
    rng = np.random.default_rng(31)
    inst = []
    for i in range(12):
        cuts = np.sort(rng.choice(600, 40, replace=False))
        inst.append([(int(a), int(b - a)) for a, b in zip(cuts[0::2], cuts[1::2])])
    inst[3] = []
    inst[5] = [(s, (l + 1) // 2) for s, l in inst[4]]
    inst[6] = [(s, 5) for s in range(0, 600, 10)]
    inst[7] = [(s + 5, 5) for s in range(0, 600, 10)]
    inst[8] = [(s, 4) for s in range(100, 200, 4)]
    starts = np.array([s for r in inst for s, _ in r], np.int64)
    lens = np.array([l for r in inst for _, l in r], np.int64)
    off = np.concatenate([[0], np.cumsum([len(r) for r in inst])]).astype(np.int64)
    return starts, lens, off


def pair_table_refs(starts, lens, off):
    """(12, 12) intersections: dense boolean arrays against oracle/rle_ops.rle_intersection"""
    from oracle import rle_ops as ORO
    k = len(off) - 1
    dense = np.zeros((k, 600 + 64), bool)
    for i in range(k):
        for s, l in zip(starts[off[i]:off[i + 1]], lens[off[i]:off[i + 1]]):
            dense[i, s:s + l] = True
    table = np.zeros((k, k), np.int64)
    for a in range(k):
        for b in range(k):
            table[a, b] = (dense[a] & dense[b]).sum()
            sa, sb = slice(off[a], off[a + 1]), slice(off[b], off[b + 1])
            assert table[a, b] == ORO.rle_intersection(starts[sa], lens[sa], starts[sb], lens[sb]), \
                f'the two intersection references disagree at ({a}, {b})'
    return table


PAIRS_MANY = 530000


def test_pair_intersections(hip):
    starts, lens, off = pair_instances()
    table = pair_table_refs(starts, lens, off)
    assert table[3].sum() == 0 and table[6, 7] == 0 and table[8, 8] == 100 and table[4, 5] > 0
    pairs = np.stack(np.mgrid[0:12, 0:12], axis=-1).reshape(-1, 2).astype(np.int32)
    got = _np(hip.rle_pair_intersections(_dev(starts), _dev(lens), _dev(off), _dev(pairs)))
    np.testing.assert_array_equal(got.reshape(12, 12), table)


def test_pair_intersections_many(hip):
    """530 000 pairs (> 8192 blocks x 64 threads) over the 144 distinct ones"""
    starts, lens, off = pair_instances()
    table = pair_table_refs(starts, lens, off)
    pairs = np.random.default_rng(37).integers(0, 12, (PAIRS_MANY, 2)).astype(np.int32)
    got = _np(hip.rle_pair_intersections(_dev(starts), _dev(lens), _dev(off), _dev(pairs)))
    np.testing.assert_array_equal(got, table[pairs[:, 0], pairs[:, 1]])


# =========================================================================================== 7. fills
def fill_plain(vol, starts, lens, order, ids):
    """paint instance by instance in `order`, later over earlier; id 0 paints nothing; runs are cut at the ends"""
    out = vol.copy()
    n = len(out)
    for k in np.unique(order):
        if ids[k] == 0:
            continue
        for s, l in zip(starts[order == k].tolist(), lens[order == k].tolist()):
            out[max(s, 0):max(min(s + l, n), 0)] = ids[k]
    return out


def fill_case_small():
    """(n_vox, starts, lens, order, ids)"""
    n = 5000
    rows = [(90, 30, 0), (95, 10, 2), (100, 1, 4), (100, 5, 3), (98, 4, 1),      # 0 < 2 < 4 over voxel 100; 1, 3, 5: id 0
            (80, 60, 5),                                                          # id 0 on top of everything: no shadow
            (-5, 10, 0), (n - 3, 10, 2), (-20, 10, 4), (n, 4, 4), (n + 7, 3, 2),  # cut at 0 and at n_vox, or outside
            (300, 0, 2), (301, 0, 0),                                             # zero length
            (400, 1, 6), (500, 64, 6), (600, 65, 6), (700, 1000, 6), (1200, 700, 0), (1699, 2, 2)]
    a = np.array(rows, np.int64)
    ids = np.array([7, 0, 0x7fffffff, 0, 9, 0, 1234567], np.uint32)
    return n, a[:, 0].copy(), a[:, 1].copy(), a[:, 2].astype(np.int32), ids


def fill_case_many():
    """40 000 runs (> 8192 blocks x 4 waves), each overlapping the next, 50 instances with some ids 0"""
    i = np.arange(40000, dtype=np.int64)
    ids = np.random.default_rng(41).integers(1, 2 ** 31, 50).astype(np.uint32)
    ids[::7] = 0
    return 200000, 5 * i - 2, 1 + i % 9, ((i * 7) % 50).astype(np.int32), ids


def fill_refs(n, starts, lens, order, ids, vol=None):
    """the painted array, against oracle/rle_ops.numpy_fill_instances where the input is what it takes (runs inside
    the volume, no id 0; painting in dict order = ascending instance order)"""
    from oracle import rle_ops as ORO
    vol = np.zeros(n, np.uint32) if vol is None else vol
    exp = fill_plain(vol, starts, lens, order, ids)
    keep = (starts >= 0) & (starts + lens <= n) & (ids[order] != 0)
    inst = {}
    for k in np.unique(order[keep]):
        sel = keep & (order == k)
        inst[(int(k), int(ids[k]))] = {'starts': starts[sel], 'runs': lens[sel]}
    # the oracle paints the dict KEY: instances that share an id would collapse, so paint the order and map it
    by_order = ORO.numpy_fill_instances(np.full(n, -1, np.int64), {k: a for (k, _), a in inst.items()})
    cut = fill_plain(vol, starts[keep], lens[keep], order[keep], ids)
    np.testing.assert_array_equal(np.where(by_order >= 0, ids[np.maximum(by_order, 0)], vol), cut,
                                  err_msg='the two fill references disagree')
    return exp


def _gpu_fill(hip, vol, starts, lens, order, ids):
    t = _dev(vol)
    args = (_dev(starts), _dev(lens), _dev(order), _dev(ids))
    hip.fill_runs_u32(t.view(torch.uint32), args[0], args[1], args[2], args[3].view(torch.uint32))
    return t, args


def test_fill_u32_edges(hip):
    n, starts, lens, order, ids = fill_case_small()
    exp = fill_refs(n, starts, lens, order, ids)
    assert exp[100] == 9 and exp[97] == 0x7fffffff and exp[92] == 7 and exp[0] == 7 and exp[n - 1] == 0x7fffffff
    t, args = _gpu_fill(hip, np.zeros(n, np.uint32), starts, lens, order, ids)
    np.testing.assert_array_equal(_np_u32(t), exp)
    hip.fill_runs_u32(t.view(torch.uint32), args[0], args[1], args[2], args[3].view(torch.uint32))
    np.testing.assert_array_equal(_np_u32(t), exp, err_msg='the same call twice')
    # earlier labels below 2^31: kept outside the runs, replaced inside them
    old = np.random.default_rng(43).integers(0, 2 ** 31, n).astype(np.uint32)
    old[100] = old[4999] = 0x7fffffff
    exp = fill_refs(n, starts, lens, order, ids, vol=old)
    covered = exp != old
    assert covered.any() and (exp[2500:4900] == old[2500:4900]).all()
    t, _ = _gpu_fill(hip, old, starts, lens, order, ids)
    np.testing.assert_array_equal(_np_u32(t), exp)


def test_fill_u32_many_runs(hip):
    n, starts, lens, order, ids = fill_case_many()
    exp = fill_refs(n, starts, lens, order, ids)
    t, _ = _gpu_fill(hip, np.zeros(n, np.uint32), starts, lens, order, ids)
    np.testing.assert_array_equal(_np_u32(t), exp)


def test_fill_u32_wrapper(hip):
    """array_utils.numpy_fill_instances on well-formed input, against the oracle of the same name"""
    from empanada_amd import array_utils as AU
    from oracle import rle_ops as ORO
    inst = {1007: {'starts': np.array([5, 40, 100]), 'runs': np.array([10, 3, 65])},
            2001: {'starts': np.array([12, 120]), 'runs': np.array([30, 64])},
            1003: {'starts': np.array([0, 41]), 'runs': np.array([1, 1])}}
    exp = ORO.numpy_fill_instances(np.zeros((10, 30), np.uint32), inst)
    got = AU.numpy_fill_instances(np.zeros((10, 30), np.uint32), inst)
    np.testing.assert_array_equal(got, exp)


class _FakeTracker:
    def __init__(self, instances):
        self.instances = instances


def test_fill_u32_refusals(hip):
    """an id of 2^31 or more, or such a value already in the volume, would make emp_fill_runs_u32 read `ids` out of
    bounds (bit 31 is its tag): every caller that takes them from outside raises ValueError on the host, first"""
    import types
    from empanada_amd import array_utils as AU
    from empanada_amd import consensus as CO
    from empanada_amd.inference import patterns, rle, sharded, tiled
    run = {'box': (0, 0, 1, 4), 'starts': np.array([2]), 'runs': np.array([3])}
    good = {1: {5: dict(run)}}
    for bad_id in (1 << 31, (1 << 32) - 1, (1 << 32) + 5, -1):
        bad = {1: {5: dict(run), bad_id: dict(run)}}
        with pytest.raises(ValueError, match='2\\^31'):
            hip.fill_ids_to_dev([3, bad_id])
        with pytest.raises(ValueError, match='2\\^31'):
            rle.rle_seg_to_pan_seg(bad, (4, 8))
        out = torch.full((4, 8), 3, dtype=torch.int32, device='cuda')
        with pytest.raises(ValueError, match='2\\^31'):
            tiled._paint(bad, (4, 8), out.view(torch.uint32))
        with pytest.raises(ValueError, match='2\\^31'):
            patterns.fill_volume_device((1, 4, 8), [_FakeTracker(bad[1])])
        with pytest.raises(ValueError, match='2\\^31'):
            AU.numpy_fill_instances(np.zeros((4, 8), np.uint32), bad[1])
    assert rle.rle_seg_to_pan_seg(good, (4, 8)).reshape(-1).tolist()[:6] == [0, 0, 5, 5, 5, 0]
    assert _np_u32(patterns.fill_volume_device((1, 4, 8), [_FakeTracker(good[1])])).reshape(-1)[2:5].tolist() == [5] * 3
    with pytest.raises(ValueError, match='2\\^31'):
        AU.numpy_fill_instances(np.full((4, 8), 1 << 31, np.uint32), good[1])
    # ConsensusResult.paint: ids from the caller, and a volume from the caller
    res = CO.ConsensusResult(np.zeros((2, 6)), np.array([3, 3]), _dev(np.array([[2, 5], [9, 12]], np.int64)), [0, 1, 2])
    vol = torch.zeros((32,), dtype=torch.int32, device='cuda')
    with pytest.raises(ValueError, match='2\\^31'):
        res.paint(vol.view(torch.uint32), 0, ids=[7, 1 << 31])
    assert _np(vol).sum() == 0
    vol[20] = -5                                     # 0xfffffffb as uint32
    with pytest.raises(ValueError, match='2\\^31'):
        res.paint(vol.view(torch.uint32), 0)
    vol[20] = 0x7fffffff
    res.paint(vol.view(torch.uint32), 0, ids=[7, 8])
    assert _np(vol)[[2, 4, 5, 9, 11, 20]].tolist() == [7, 7, 0, 8, 8, 0x7fffffff]
    # sharded.plane_volume: labels of the plane's instances
    pt = types.SimpleNamespace(axis='xy', shape3d=(1, 4, 8), n_runs=1, n_inst=1, alive=np.array([True]),
                               inst_cls=np.array([2]), inst_label=np.array([(2 << 30) + 1]),
                               st=_dev(np.array([2], np.int64)), ln=_dev(np.array([3], np.int64)),
                               offsets=lambda: _dev(np.array([0, 1], np.int64)))
    with pytest.raises(ValueError, match='2\\^31'):
        sharded.plane_volume(pt, [2], [2])
    pt.inst_label = np.array([77])
    vols, _, _ = sharded.plane_volume(pt, [2], [2])
    assert _np(vols[2].view(torch.int32)).reshape(-1)[1:6].tolist() == [0, 77, 77, 77, 0]


def fill_u8_case():
    n = 3000
    rows = [(-5, 10), (n - 3, 10), (n, 4), (-20, 10), (300, 0), (400, 1), (500, 64), (600, 65), (700, 1000)]
    a = np.array(rows, np.int64)
    return n, a[:, 0].copy(), a[:, 1].copy()


def fill_u8_plain(vol, starts, lens, value):
    out = vol.copy()
    for s, l in zip(starts.tolist(), lens.tolist()):
        out[max(s, 0):max(min(s + l, len(out)), 0)] = value
    return out


@pytest.mark.parametrize('value', [0, 255])
def test_fill_u8(hip, value):
    n, starts, lens = fill_u8_case()
    old = np.random.default_rng(47).integers(1, 255, n).astype(np.uint8)
    exp = fill_u8_plain(old, starts, lens, value)
    assert (exp == value).sum() == 5 + 3 + 1 + 64 + 65 + 1000
    t = _dev(old)
    hip.fill_runs_u8(t, _dev(starts), _dev(lens), value)
    np.testing.assert_array_equal(_np(t), exp)


def table_stack():
    """(4, 6, 9) stack with cc class 1 and plain class 3, an empty slice, runs at both ends of rows"""
    s = np.zeros((4, 6, 9), np.uint32)
    s[0, 0, 0:3] = s[0, 1, 2:9] = 1005
    s[0, 4, 7:9] = s[0, 5, 0:2] = 1006
    s[1, 2, :] = 3007
    s[1, 4, 4] = 1005
    s[3, 0, 0] = s[3, 5, 8] = 3007
    s[3, 3, 1:8] = 1005
    return s


def table_paint_plain(T, value, shape, n_slices, slice0):
    """run i paints value[r_comp[i]] at slice c_slice - slice0; value 0 and slices outside the slab are skipped"""
    D, H, W = shape
    vol = np.full((n_slices, H * W), 99, np.uint32)
    for s, l, c in zip(T['r_start'], T['r_len'], T['r_comp']):
        sl = T['c_slice'][c] - slice0
        if value[c] != 0 and 0 <= sl < n_slices:
            vol[sl, s:s + l] = value[c]
    return vol.reshape(n_slices, H, W)


@pytest.mark.parametrize('slab', [(0, 4), (1, 2), (3, 1), (2, 5)], ids=lambda s: f'slice0={s[0]}-n={s[1]}')
def test_fill_table_u32(hip, slab):
    slice0, n_slices = slab
    pan = table_stack()
    T = label_refs(pan, 1000, [1])
    value = (np.arange(T['n_comp']) * 3 + 0x7ffffff0).astype(np.uint32)
    value[1] = 0
    exp = table_paint_plain(T, value, pan.shape, n_slices, slice0)
    tab = hip.extract_runs(_dev(pan).view(torch.uint32), 1000, [1])
    vol = torch.full((n_slices, 6, 9), 99, dtype=torch.int32, device='cuda')
    hip.fill_table_u32(vol.view(torch.uint32), tab, _dev(value), slice0)
    np.testing.assert_array_equal(_np_u32(vol), exp)


def scatter_plain(T, value, Z, Y, Xl):
    vol = np.zeros((Z * Y, Xl), np.uint32)
    for s, l, c in zip(T['r_start'], T['r_len'], T['r_comp']):
        if value[c] != 0:
            vol[s:s + l, T['c_slice'][c]] = value[c]
    return vol.reshape(Z, Y, Xl)


def yz_stack(Xl, Z=5, Y=6):
    rng = np.random.default_rng([53, Xl])
    return (rng.integers(0, 3, (Xl, Z, Y)) * rng.integers(1001, 1004, (Xl, Z, Y))).astype(np.uint32)


@pytest.mark.parametrize('Xl', [1, 7])
def test_scatter_yz_u32(hip, Xl):
    Z, Y = 5, 6
    pan = yz_stack(Xl)
    T = label_refs(pan, 1000, [1])
    value = (np.arange(T['n_comp']) % 5).astype(np.uint32)            # every fifth component is dropped
    exp = scatter_plain(T, value, Z, Y, Xl)
    tab = hip.extract_runs(_dev(pan).view(torch.uint32), 1000, [1])
    vol = torch.zeros((Z, Y, Xl), dtype=torch.int32, device='cuda')
    dv = _dev(value)
    hip.call('emp_scatter_yz_u32', vol.data_ptr(), Z, Y, Xl, tab.r_start.data_ptr(), tab.r_len.data_ptr(),
             tab.r_comp.data_ptr(), tab.c_slice.data_ptr(), dv.data_ptr(), tab.n_runs, hip.stream())
    np.testing.assert_array_equal(_np_u32(vol), exp)


# =========================================================================================== 8. box pairs, rle
def boxes_input(n, nd, seed):
    """touching, inverted and negative boxes among random ones"""
    rng = np.random.default_rng([59, n, nd, seed])
    lo = rng.integers(-20, 20, (n, nd))
    b = np.concatenate([lo, lo + rng.integers(-3, 12, (n, nd))], axis=1).astype(np.int32)    # some inverted / empty
    if n >= 4:
        b[1, :nd], b[1, nd:] = b[0, nd:], b[0, nd:] + 5                # touches box 0 in every dimension
        b[2] = b[0]
        b[3, :nd], b[3, nd:] = b[0, nd:] - 1, b[0, nd:] + 4            # one cell in common with box 0 (if 0 is not empty)
    return b


def box_pairs_plain(a, b, src_a=None, src_b=None, upper_only=False):
    nd = a.shape[1] // 2
    out = set()
    for i in range(len(a)):
        for j in range(len(b)):
            if upper_only and j <= i:
                continue
            if src_a is not None and src_b is not None and src_a[i] == src_b[j]:
                continue
            if all(min(a[i, k + nd], b[j, k + nd]) - max(a[i, k], b[j, k]) > 0 for k in range(nd)):
                out.add((i, j))
    return out


def box_pairs_refs(a, b):
    from oracle import rle_ops as ORO
    plain = box_pairs_plain(a, b)
    r, c, _, _ = ORO.box_pairs(a, b)
    assert set(zip(r.tolist(), c.tolist())) == plain, 'the two box references disagree'
    return plain


BOX_NB = [1, 256, 257, 600]


def _pairs_set(t):
    rows = _np(t).tolist()
    s = set(map(tuple, rows))
    assert len(s) == len(rows), 'a pair was reported twice'
    return s


@pytest.mark.parametrize('nd', [2, 3])
@pytest.mark.parametrize('nb', BOX_NB)
def test_box_pairs(hip, nb, nd):
    a, b = boxes_input(5, nd, 0), boxes_input(nb, nd, 1)
    b[:min(nb, 5)] = a[:min(nb, 5)]
    exp = box_pairs_refs(a, b)
    assert nb == 1 or len(exp) > 3
    assert _pairs_set(hip.box_pairs(_dev(a), _dev(b))) == exp
    sa, sb = np.arange(5, dtype=np.int32) % 2, np.arange(nb, dtype=np.int32) % 3
    assert _pairs_set(hip.box_pairs(_dev(a), _dev(b), _dev(sa), _dev(sb))) == box_pairs_plain(a, b, sa, sb)
    assert _pairs_set(hip.box_pairs(_dev(b), upper_only=True)) == box_pairs_plain(b, b, upper_only=True)
    assert _pairs_set(hip.box_pairs(_dev(b), src_a=_dev(sb), upper_only=True)) == box_pairs_plain(b, b, sb, sb, True)
    # only one of the two source arrays: no filtering
    assert _pairs_set(hip.box_pairs(_dev(a), _dev(b), src_a=_dev(sa))) == exp


def test_box_pairs_empty_and_cap(hip):
    a = boxes_input(6, 2, 2)
    e = torch.zeros((0, 4), dtype=torch.int32, device='cuda')
    assert hip.box_pairs(_dev(a), e).shape[0] == 0 and hip.box_pairs(e, _dev(a)).shape[0] == 0
    b = boxes_input(300, 2, 3)
    exp = box_pairs_refs(a, b)
    true = len(exp)
    assert true > 20
    da, db = _dev(a), _dev(b)
    for cap in (0, 7, true, true + 3):
        out = _full(2 * (cap + 1), torch.int32)
        cnt = _full(1, torch.int32)
        hip.call('emp_box_pairs', da.data_ptr(), 6, db.data_ptr(), 300, 2, None, None, 0,
                 out.data_ptr() if cap else None, cap, cnt.data_ptr(), hip.stream())
        assert int(cnt[0]) == true, 'n_out must hold the true count'
        rows = _pairs_set(out[:2 * min(cap, true)].reshape(-1, 2))
        assert rows <= exp and len(rows) == min(cap, true)
        assert (_np(out[2 * cap:]) == -7).all(), 'emp_box_pairs wrote past cap'


def rle_case():
    starts = np.array([5, 40, 40, 200, 300, 500, 501, 900], np.int64)
    runs = np.array([3, 0, 64, 65, 0, 1, 1, 130], np.int64)
    return starts, runs


def rle_decode_refs(starts, runs):
    from oracle import rle_ops as ORO
    plain = [s + i for s, r in zip(starts.tolist(), runs.tolist()) for i in range(r)]
    np.testing.assert_array_equal(ORO.rle_decode(starts, runs), plain)
    return np.array(plain, np.int64)


def rle_encode_refs(idx):
    from oracle import rle_ops as ORO
    plain = np.array(_encode(idx.tolist()), np.int64).reshape(-1, 2)
    s, r = ORO.rle_encode(idx)
    np.testing.assert_array_equal(np.stack([s, r], axis=1), plain)
    return plain[:, 0], plain[:, 1]


def test_rle_decode_encode(hip):
    starts, runs = rle_case()
    idx = rle_decode_refs(starts, runs)
    got = hip.rle_decode(_dev(starts), _dev(runs))
    np.testing.assert_array_equal(_np(got), idx)
    es, er = rle_encode_refs(idx)                                   # 500 and 501 join; the empty runs vanish
    assert er.tolist() == [3, 64, 65, 2, 130]
    gs, gr = hip.rle_encode(got)
    np.testing.assert_array_equal(_np(gs), es)
    np.testing.assert_array_equal(_np(gr), er)
    gs, gr = hip.rle_encode(torch.zeros((0,), dtype=torch.int64, device='cuda'))
    assert gs.numel() == 0 and gr.numel() == 0
    assert hip.rle_decode(_dev(np.array([7, 9], np.int64)), _dev(np.zeros(2, np.int64))).numel() == 0


# =========================================================================================== 9. tracks
def lift_stack():
    """(3, 4, 8) stack, cc class 1 (values 1005, 1006), built for the run-merging rules of the lifts"""
    s = np.zeros((3, 4, 8), np.uint32)
    s[0, 0, 1:3] = 1005
    s[0, 0, 3:6] = 1006                 # two components side by side: one run when they are one instance
    s[0, 1, 5:8] = 1005
    s[0, 2, 0:2] = 1005                 # ends at the row's end, goes on at the next row's start: one run
    s[0, 2, 4:7] = 1006                 # last run of slice 0 ends at flat index 23 ...
    s[1, 2, 7] = 1006                   # ... where the first run of slice 1 starts: never one run
    s[1, 3, 0:8] = 1006
    s[2, 0, 0:8] = 1005
    s[2, 3, 6:8] = 1005
    return s


def lift_plain(axis, T, comp_inst, H, W, Y, X, slice0, inst_base, tile=None):
    """per (instance, slice): the instance's pixels of that slice, sorted, cut into maximal spans of consecutive flat 2D
    indices; the START of each span is moved into the volume (xy, xz) or image (tile) frame and the length kept.
    Output in the order (slice, 2D start)."""
    rows = []
    D = T['comp_img'].shape[0]
    for d in range(D):
        inst_img = np.where(T['comp_img'][d] >= 0, comp_inst[np.maximum(T['comp_img'][d], 0)], -1).reshape(-1)
        spans = []
        for inst in sorted(set(inst_img[inst_img >= 0].tolist())):
            spans += [(s, l, inst) for s, l in _encode(np.flatnonzero(inst_img == inst).tolist())]
        for s, l, inst in sorted(spans):
            g = d + slice0
            if tile is not None:
                tw, y0, x0 = tile
                st = (s // tw + y0) * X + s % tw + x0
            elif axis == 0:
                st = s + g * Y * X
            else:
                st = (s // W) * Y * X + g * X + s % W
            rows.append((((inst_base + inst) << POS_BITS) | st, l))
    a = np.array(rows, dtype=object).reshape(-1, 2)
    return a[:, 0].astype(np.uint64), a[:, 1].astype(np.int64)


def lift_insts(n_comp):
    """name -> comp_inst (int32 per component)"""
    one_each = np.arange(n_comp, dtype=np.int32)
    return {'none': np.full(n_comp, -1, np.int32), 'one_each': one_each,
            'all_one': np.zeros(n_comp, np.int32), 'pairs': (one_each // 2).astype(np.int32),
            'some_dropped': np.where(one_each % 3 == 1, -1, one_each % 2).astype(np.int32)}


LIFT_GEOM = [(0, 0, 0), (0, 5, (1 << 24) - 16), (1, 0, 0), (1, 3, (1 << 24) - 16)]       # (axis, slice0, inst_base)


def lift_refs(axis, T, comp_inst, H, W, Y, X, slice0, inst_base):
    from oracle import tracks as OT
    a = lift_plain(axis, T, comp_inst, H, W, Y, X, slice0, inst_base)
    b = OT.lift_xy_xz(axis, T['r_start'], T['r_len'], T['r_comp'], T['c_slice'], comp_inst, H, W, Y, X, slice0, inst_base)
    np.testing.assert_array_equal(a[0], b[0], err_msg='the two lift references disagree (keys)')
    np.testing.assert_array_equal(a[1], b[1], err_msg='the two lift references disagree (lengths)')
    return a


def tile_refs(T, comp_inst, tw, X, y0, x0, inst_base):
    from oracle import tracks as OT
    a = lift_plain(2, T, comp_inst, 0, tw, 0, X, 0, inst_base, tile=(tw, y0, x0))
    b = OT.lift_tile(T['r_start'], T['r_len'], T['r_comp'], T['c_slice'], comp_inst, tw, X, y0, x0, inst_base)
    np.testing.assert_array_equal(a[0], b[0], err_msg='the two tile-lift references disagree (keys)')
    np.testing.assert_array_equal(a[1], b[1], err_msg='the two tile-lift references disagree (lengths)')
    return a


def _table_dev(T):
    return [_dev(T[c]) for c in ('r_start', 'r_len', 'r_comp', 'c_slice')]


def _gpu_lift(hip, name, T, comp_inst, *geom):
    n = len(T['r_start'])
    cols = _table_dev(T)
    ci = _dev(comp_inst)
    work = _full(hip.query('emp_track_work_elems', n), torch.int32)
    key, ln, cnt = _full(n + 1, torch.int64), _full(n + 1, torch.int64), _full(1, torch.int32)
    tail = (work.data_ptr(), key.data_ptr(), ln.data_ptr(), cnt.data_ptr(), hip.stream())
    if name == 'emp_track_lift':
        axis, rest = geom[0], geom[1:]
        hip.call(name, axis, *[c.data_ptr() for c in cols], ci.data_ptr(), n, *rest, *tail)
    else:
        hip.call(name, *[c.data_ptr() for c in cols], ci.data_ptr(), n, *geom, *tail)
    m = int(cnt[0])
    assert 0 <= m <= n and int(key[n]) == -7 and int(ln[n]) == -7
    return _np_u64(key[:m]), _np(ln[:m])


@pytest.mark.parametrize('geom', LIFT_GEOM, ids=lambda g: f'axis{g[0]}-slice0={g[1]}-base={g[2]}')
def test_track_lift(hip, geom):
    axis, slice0, inst_base = geom
    pan = lift_stack()
    D, H, W = pan.shape
    Y, X = (H, W) if axis == 0 else (D + slice0 + 2, W)
    T = label_refs(pan, 1000, [1])
    for name, comp_inst in lift_insts(T['n_comp']).items():
        ek, el = lift_refs(axis, T, comp_inst, H, W, Y, X, slice0, inst_base)
        if name == 'none':
            assert len(ek) == 0
        if name == 'all_one':
            # 0: [1, 6) merged pair, [13, 18) across the row end, [20, 23); 1: [23, 32) apart from slice 0's last run
            assert el.tolist() == [5, 5, 3, 9, 8, 2]
        gk, gl = _gpu_lift(hip, 'emp_track_lift', T, comp_inst, axis, H, W, Y, X, slice0, inst_base)
        np.testing.assert_array_equal(gk, ek, err_msg=f'{name}: keys')
        np.testing.assert_array_equal(gl, el, err_msg=f'{name}: lengths')


TILE_GEOM = [(8, 8, 0, 0, 0), (8, 21, 0, 13, 0), (8, 30, 5, 9, (1 << 24) - 16)]          # (tw, X, y0, x0, inst_base)


@pytest.mark.parametrize('geom', TILE_GEOM, ids=lambda g: 'tw{}-X{}-y{}-x{}-base{}'.format(*g))
def test_tile_lift(hip, geom):
    tw, X, y0, x0, inst_base = geom
    pan = lift_stack()
    T = label_refs(pan, 1000, [1])
    for name, comp_inst in lift_insts(T['n_comp']).items():
        ek, el = tile_refs(T, comp_inst, tw, X, y0, x0, inst_base)
        if name == 'all_one':
            assert el.tolist() == [5, 5, 3, 9, 8, 2]      # the run wrapped inside the tile keeps its length of 5
        gk, gl = _gpu_lift(hip, 'emp_tile_lift', T, comp_inst, tw, X, y0, x0, inst_base)
        np.testing.assert_array_equal(gk, ek, err_msg=f'{name}: keys')
        np.testing.assert_array_equal(gl, el, err_msg=f'{name}: lengths')


YZ_GEOM = [(1, 5, 4), (7, 7, 0), (3, 8, 5), (3, 8, 0)]                                    # (Xl, X, x0)


def yz_volume(Xl, Z=4, Y=5):
    """(Z, Y, Xl) instance + 1, with rows that are one value from end to end"""
    rng = np.random.default_rng([61, Xl])
    v = rng.integers(0, 4, (Z, Y, Xl)).astype(np.uint32)
    v[1, 1:4, :] = 2
    v[2, :, :] = 3
    return v


def yz_refs(vol, X, x0, inst_base):
    """after the touch-merge: per instance the sorted flat (z, y, x) indices of its voxels, cut into maximal spans;
    against oracle/tracks.lift_yz + sort_runs"""
    from oracle import tracks as OT
    Z, Y, Xl = vol.shape
    rows = []
    zy, x = np.divmod(np.arange(Z * Y * Xl), Xl)
    flat3 = zy * X + x0 + x
    for v in sorted(set(vol[vol > 0].tolist())):
        idx = np.sort(flat3[vol.reshape(-1) == v])
        rows += [(((inst_base + v - 1) << POS_BITS) | s, l) for s, l in _encode(idx.tolist())]
    a = np.array(sorted(rows), dtype=object).reshape(-1, 2)
    before = OT.lift_yz(vol, X, x0, inst_base)
    after = OT.sort_runs(*before, merge_touching=True)
    np.testing.assert_array_equal(a[:, 0].astype(np.uint64), after[0], err_msg='the two yz references disagree')
    np.testing.assert_array_equal(a[:, 1].astype(np.int64), after[1], err_msg='the two yz references disagree')
    return before, after


def _gpu_track_sort(hip, key, ln, merge, want_key=True, want_st=True):
    n = len(key)
    wb = hip.query('emp_track_sort_work_bytes', n)
    work = torch.empty((wb,), dtype=torch.uint8, device='cuda')
    ok, ost, ol, cnt = _full(n + 1, torch.int64), _full(n + 1, torch.int64), _full(n + 1, torch.int64), _full(1, torch.int32)
    dk, dl = _dev(key), _dev(ln)
    hip.call('emp_track_sort', dk.data_ptr() if n else None, dl.data_ptr() if n else None, n, int(merge),
             work.data_ptr(), wb, ok.data_ptr() if want_key else None, ost.data_ptr() if want_st else None,
             ol.data_ptr(), cnt.data_ptr(), hip.stream())
    m = int(cnt[0])
    assert 0 <= m <= n and int(ol[n]) == -7
    if not want_key:
        assert (_np(ok) == -7).all()
    if not want_st:
        assert (_np(ost) == -7).all()
    return _np_u64(ok[:m]), _np(ost[:m]), _np(ol[:m])


@pytest.mark.parametrize('geom', YZ_GEOM, ids=lambda g: 'Xl{}-X{}-x{}'.format(*g))
def test_track_lift_yz(hip, geom):
    Xl, X, x0 = geom
    inst_base = 1000
    vol = yz_volume(Xl)
    Z, Y, _ = vol.shape
    (bk, bl), (ak, al) = yz_refs(vol, X, x0, inst_base)
    counts, st, ln, val = runs_refs(vol)
    offs = _dev(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32))
    n = len(st)
    key, out_len = _full(n + 1, torch.int64), _full(n + 1, torch.int64)
    cols = [_dev(st), _dev(ln), _dev(val)]
    hip.call('emp_track_lift_yz', offs.data_ptr(), *[c.data_ptr() for c in cols], Z * Y, n, Xl, X, x0, inst_base,
             key.data_ptr(), out_len.data_ptr(), hip.stream())
    assert int(key[n]) == -7
    np.testing.assert_array_equal(_np_u64(key[:n]), bk)
    np.testing.assert_array_equal(_np(out_len[:n]), bl)
    gk, gs, gl = _gpu_track_sort(hip, _np_u64(key[:n]), _np(out_len[:n]), True)
    np.testing.assert_array_equal(gk, ak)
    np.testing.assert_array_equal(gl, al)
    np.testing.assert_array_equal(gs, (ak & np.uint64(POS_MASK)).astype(np.int64))


def sort_chain_input():
    """shuffled runs: per instance chains of 1, 2, 65 and 300 touching runs, apart from each other; instance k ends
    where instance k + 1 starts (never one run); two runs of one instance with the same start"""
    rows = []
    for inst, base in ((3, 0), (4, 10000), (9, 20000)):
        pos = base
        for chain in (1, 2, 65, 300):
            pos += 7
            for i in range(chain):
                ln = 1 + (i + inst) % 5
                rows.append((inst, pos, ln))
                pos += ln
    end3 = max(p + l for i, p, l in rows if i == 3)
    rows.append((4, end3, 6))                       # instance 4 starts where instance 3 ends
    rows.append((9, 50000, 0))
    rows.append((9, 50000, 4))                      # equal keys: a zero-length run first (stable), they join
    a = np.array(rows, np.int64)
    perm = np.random.default_rng(67).permutation(len(a))
    perm = np.concatenate([perm[perm != len(a) - 1], [len(a) - 1]])       # the zero-length twin stays ahead
    a = a[perm]
    return ((a[:, 0].astype(np.uint64) << np.uint64(POS_BITS)) | a[:, 1].astype(np.uint64)), a[:, 2].copy()


def sort_chain_refs(key, ln, merge):
    """sorted by key (stable); with merge: a run that starts where the previous run of its instance ends joins it"""
    from oracle import tracks as OT
    order = sorted(range(len(key)), key=lambda i: int(key[i]))
    rows = []
    for i in order:
        k, l = int(key[i]), int(ln[i])
        if merge and rows and rows[-1][0] >> POS_BITS == k >> POS_BITS and rows[-1][0] + rows[-1][1] == k:
            rows[-1][1] += l
        else:
            rows.append([k, l])
    a = np.array(rows, dtype=object).reshape(-1, 2)
    ok, ol = OT.sort_runs(key, ln, merge_touching=merge)
    np.testing.assert_array_equal(a[:, 0].astype(np.uint64), ok, err_msg='the two sort references disagree')
    np.testing.assert_array_equal(a[:, 1].astype(np.int64), ol, err_msg='the two sort references disagree')
    return ok, ol


@pytest.mark.parametrize('merge', [False, True], ids=['plain', 'merge_touching'])
def test_track_sort(hip, merge):
    key, ln = sort_chain_input()
    ek, el = sort_chain_refs(key, ln, merge)
    if merge:
        assert len(ek) == 3 * 4 + 1 + 1
    for want_key, want_st in ((True, True), (False, True), (True, False)):
        gk, gs, gl = _gpu_track_sort(hip, key, ln, merge, want_key, want_st)
        m = len(ek) if merge else len(key)
        if want_key:
            np.testing.assert_array_equal(gk[:m], ek)
        if want_st:
            np.testing.assert_array_equal(gs[:m], (ek & np.uint64(POS_MASK)).astype(np.int64))
        np.testing.assert_array_equal(gl[:m], el)
    k1 = np.array([(5 << POS_BITS) | 77], np.uint64)
    gk, gs, gl = _gpu_track_sort(hip, k1, np.array([4], np.int64), merge)
    assert (gk.tolist(), gs.tolist(), gl.tolist()) == (k1.tolist(), [77], [4])
    gk, _, _ = _gpu_track_sort(hip, np.zeros(0, np.uint64), np.zeros(0, np.int64), merge)
    assert len(gk) == 0


def test_track_offsets_expand(hip):
    from oracle import tracks as OT
    inst = np.array([2, 2, 2, 5, 6, 6, 9], np.uint64)                   # 0, 1, 3, 4, 7, 8, 10, 11 have no runs
    keys = (inst << np.uint64(POS_BITS)) | np.arange(7, dtype=np.uint64)
    for k, n_inst in ((keys, 12), (keys[:0], 4), (keys, 1)):
        exp = OT.offsets(k, n_inst)
        plain = [sum(1 for i in (k >> np.uint64(POS_BITS)).tolist() if i < j) for j in range(n_inst + 1)]
        assert exp.tolist() == plain
        off = _full(n_inst + 2, torch.int64)
        dk = _dev(k)
        hip.call('emp_track_offsets', dk.data_ptr() if len(k) else None, len(k), n_inst, off.data_ptr(), hip.stream())
        assert int(off[n_inst + 1]) == -7
        np.testing.assert_array_equal(_np(off[:n_inst + 1]), exp)
    off = OT.offsets(keys, 12)
    val = (np.arange(12) * 11 - 5).astype(np.int32)
    for o, v in ((off, val), (np.array([0, 7], np.int64), np.array([-3], np.int32))):
        exp = OT.expand(o, v, 7)
        assert exp.tolist() == [int(v[max(j for j in range(len(v)) if o[j] <= i)]) for i in range(7)]
        out = _full(8, torch.int32)
        do, dv = _dev(o), _dev(v)
        hip.call('emp_track_expand', do.data_ptr(), dv.data_ptr(), len(v), 7, out.data_ptr(), hip.stream())
        assert int(out[7]) == -7
        np.testing.assert_array_equal(_np(out[:7]), exp)


def clip_input():
    """runs around the interval [100, 200) (and [100, 100)): (instance, start, length)"""
    rows = [(1, 90, 10),        # ends exactly at lo: dropped
            (1, 95, 6),         # one voxel inside
            (2, 199, 5),        # starts at hi - 1
            (2, 200, 5),        # starts at hi: dropped
            (3, 50, 500),       # across the whole interval
            (3, 150, 0),        # zero length: dropped
            (4, 100, 100), (4, 120, 1), (5, 10, 3), (5, 300, 3)]
    a = np.array(rows, np.int64)
    return ((a[:, 0].astype(np.uint64) << np.uint64(POS_BITS)) | a[:, 1].astype(np.uint64)), a[:, 2].copy()


def clip_refs(key, ln, lo, hi):
    from oracle import tracks as OT
    rows = []
    for k, l in zip(key.tolist(), ln.tolist()):
        s = k & POS_MASK
        vox = [p for p in range(s, s + l) if lo <= p < hi]
        if vox:
            rows.append(((k & ~POS_MASK) | vox[0], len(vox)))
    a = np.array(rows, dtype=object).reshape(-1, 2)
    ok, ol = OT.clip(key, ln, lo, hi)
    np.testing.assert_array_equal(a[:, 0].astype(np.uint64), ok, err_msg='the two clip references disagree')
    np.testing.assert_array_equal(a[:, 1].astype(np.int64), ol, err_msg='the two clip references disagree')
    return ok, ol


CLIP_INTERVALS = [(100, 200), (100, 100), (0, 1 << 39), (96, 97)]


@pytest.mark.parametrize('interval', CLIP_INTERVALS, ids=lambda i: f'{i[0]}-{i[1]}')
def test_track_clip(hip, interval):
    lo, hi = interval
    key, ln = clip_input()
    ek, el = clip_refs(key, ln, lo, hi)
    if interval == (100, 200):
        assert el.tolist() == [1, 1, 100, 100, 1]
    if lo == hi:
        assert len(ek) == 0
    n = len(key)
    work = _full(hip.query('emp_track_work_elems', n), torch.int32)
    ok, ol, cnt = _full(n + 1, torch.int64), _full(n + 1, torch.int64), _full(1, torch.int32)
    dk, dl = _dev(key), _dev(ln)
    hip.call('emp_track_clip', dk.data_ptr(), dl.data_ptr(), n, lo, hi, work.data_ptr(), ok.data_ptr(),
             ol.data_ptr(), cnt.data_ptr(), hip.stream())
    m = int(cnt[0])
    assert m == len(ek) and int(ok[n]) == -7
    np.testing.assert_array_equal(_np_u64(ok[:m]), ek)
    np.testing.assert_array_equal(_np(ol[:m]), el)


# n = 0 with null data, work and output pointers: (entry point, arguments; COUNT stands for the count pointer)
COUNT = object()
NO_INPUT_CALLS = {
    'track_lift_xy': ('emp_track_lift', (0, None, None, None, None, None, 0, 5, 7, 5, 7, 0, 0, None, None, None, COUNT)),
    'track_lift_xz': ('emp_track_lift', (1, None, None, None, None, None, 0, 4, 7, 5, 7, 2, 9, None, None, None, COUNT)),
    'tile_lift': ('emp_tile_lift', (None, None, None, None, None, 0, 4, 9, 2, 3, 0, None, None, None, COUNT)),
    'track_clip': ('emp_track_clip', (None, None, 0, 100, 200, None, None, None, COUNT)),
    'triplets_reduce': ('emp_triplets_reduce', (None, 0, None, 0, None, COUNT)),
    'rle_encode': ('emp_rle_encode', (None, 0, None, None, None, COUNT)),
}


@pytest.mark.parametrize('name', list(NO_INPUT_CALLS))
def test_compaction_no_input(hip, name):
    """the shared early-out of the flags -> scan -> emit entry points: nothing to compact is valid without any data,
    work or output pointer; the count is zeroed on the stream and nothing next to it is written"""
    fn, args = NO_INPUT_CALLS[name]
    cnt = _full(3, torch.int32)                                     # sentinel, count, sentinel
    ptr = cnt.data_ptr() + 4
    hip.call(fn, *[ptr if a is COUNT else a for a in args], hip.stream())
    assert _np(cnt).tolist() == [-7, 0, -7]
