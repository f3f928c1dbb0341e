"""GPU: the sparse overlap table of two label arrays (csrc/emp_overlaps.hip behind _hip.label_overlaps) against

    np.unique(np.stack([g, p], 1), axis=0, return_counts=True)   with (0, 0) dropped.

Integer work: pairs and counts must be equal, in the same order.  The shapes are small and aimed at where a kernel made
of ballots, a carried last pair and a scan breaks:

ov_spans_kernel<.., 4 | 1>  equal element offsets mod 4 of the two bases: wide loads, the lane grid shifted per row
                            (every W with W % 4 != 0 exercises shifts 0..3 and the voxel-by-voxel groups at both row
                            ends); different offsets (`skewed`): one voxel per lane
  wave steps of 256 / 64    W below, at and above 64, 128, 256; spans carried over a step, ending on a step's last
                            voxel, filling the row
  scan                      rows without spans between rows with; R = 5000 (three scan blocks of 2048)
  sort + reduce             keys at the ends of uint32 on either side; a pair repeated in every row (segments of 16
                            spans, partial sums added by atomics); one count past 2^31 (and the wrapper's row blocks)
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

WIDTHS = (1, 2, 63, 64, 65, 127, 128, 129, 257, 1000)
ROWS = (1, 3, 70)


@pytest.fixture(scope='module')
def hip():
    from empanada_amd import _hip
    _hip.load()
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return _hip


def np_table(g, p):
    st = np.stack([np.asarray(g).reshape(-1).astype(np.int64), np.asarray(p).reshape(-1).astype(np.int64)], 1)
    pairs, counts = np.unique(st, axis=0, return_counts=True)
    keep = (pairs != 0).any(axis=1)
    return pairs[keep], counts[keep].astype(np.int64)


def _dev(a, offset=0):
    """numpy uint8 / uint32 labels on the device; offset: elements the data sits past a fresh allocation's base"""
    a = np.ascontiguousarray(a)
    flat = a.reshape(-1)
    if a.dtype == np.uint32:
        flat = flat.view(np.int32)
    buf = torch.zeros((flat.size + offset,), dtype=torch.from_numpy(flat[:0]).dtype, device='cuda')
    buf[offset:] = torch.from_numpy(flat).cuda()
    t = buf[offset:].view(a.shape)
    return t.view(torch.uint32) if a.dtype == np.uint32 else t


def _check(hip, g, p, **kw):
    pairs, counts = hip.label_overlaps(_dev(g, kw.get('og', 0)), _dev(p, kw.get('op', 0)))
    assert pairs.dtype == torch.int64 and counts.dtype == torch.int64 and pairs.is_cuda and counts.is_cuda
    ref_p, ref_c = np_table(g, p)
    np.testing.assert_array_equal(pairs.cpu().numpy(), ref_p)
    np.testing.assert_array_equal(counts.cpu().numpy(), ref_c)
    return ref_p, ref_c


def piecewise(rng, R, W, n_labels, zero=0.3):
    """rows of constant pieces of random length 1..40, a share `zero` of them background; row 1 is one piece, row 2
    has pieces that end exactly on the multiples of 64"""
    out = np.zeros((R, W), dtype=np.uint32)
    for r in range(R):
        x = 0
        while x < W:
            n = int(rng.integers(1, 41))
            if r % 5 == 1:
                n = W
            elif r % 5 == 2:
                n = 64 - x % 64
            v = 0 if (rng.random() < zero and r % 5 != 1) else int(rng.integers(1, n_labels + 1))
            out[r, x:x + n] = v
            x += n
    return out


@pytest.mark.parametrize('W', WIDTHS)
def test_table_equals_numpy(hip, W):
    rng = np.random.default_rng(W)
    for R in ROWS:
        g = piecewise(rng, R, W, 6)
        p = piecewise(rng, R, W, 5)
        if R > 1:
            p[1] = 3                                       # with g[1] constant too: one span that is the whole row
        _check(hip, g, p)
        _check(hip, g, p, og=1, op=1)                      # both bases one element off: the shifted wide path
        _check(hip, g, p, og=2)                            # bases at different offsets: one voxel per lane


@pytest.mark.parametrize('W', (1, 64, 65, 257, 1000))
def test_a_new_span_at_every_voxel(hip, W):
    x = np.arange(W, dtype=np.uint32)
    for R in (1, 3):
        alt = np.broadcast_to(1 + x % 2, (R, W)).copy()
        const = np.full((R, W), 7, dtype=np.uint32)
        for g, p in ((alt, const), (const, alt), (alt, np.zeros_like(alt)),
                     (alt, 1 + (x[None] + 1 + np.arange(R, dtype=np.uint32)[:, None]) % 2),     # both, out of phase
                     (np.broadcast_to(1 + (x // 2) % 2, (R, W)).copy(),                        # each side every second
                      np.broadcast_to(1 + ((x + 1) // 2) % 2, (R, W)).copy())):                 # voxel, shifted by one
            _, counts = _check(hip, g, p.astype(np.uint32))
            assert counts.sum() == R * W                   # W spans per row went in


def test_nothing_to_count(hip):
    for shape in ((3, 70), (1, 1), (5, 64, 64)):
        z = torch.zeros(shape, dtype=torch.int32, device='cuda')
        pairs, counts = hip.label_overlaps(z, z.clone())
        assert tuple(pairs.shape) == (0, 2) and tuple(counts.shape) == (0,) and pairs.dtype == torch.int64
    for shape in ((0, 64), (4, 0), (0,), (2, 0, 8)):
        z = torch.zeros(shape, dtype=torch.uint8, device='cuda')
        pairs, counts = hip.label_overlaps(z, z.clone())
        assert tuple(pairs.shape) == (0, 2) and tuple(counts.shape) == (0,) and counts.dtype == torch.int64


def test_empty_rows_between_full_ones(hip):
    rng = np.random.default_rng(1)
    g = piecewise(rng, 40, 130, 4)
    p = piecewise(rng, 40, 130, 4)
    for r in (0, 3, 4, 5, 17, 38, 39):
        g[r] = 0
        p[r] = 0
    g[20] = 0                                              # a row with spans on one side only
    _check(hip, g, p)


def test_rows_across_scan_blocks(hip):
    rng = np.random.default_rng(2)
    g = rng.integers(0, 3, size=(5000, 8)).astype(np.uint32)
    p = rng.integers(0, 3, size=(5000, 8)).astype(np.uint32)
    g[2040:2056] = 0
    p[2040:2056] = 0                                       # no spans around the first block border
    _check(hip, g, p)
    _check(hip, g.reshape(10, 500, 8), p.reshape(10, 500, 8))      # leading axes are rows all the same


def test_labels_at_the_ends_of_uint32(hip):
    vals = np.array([0, 1, 2 ** 31, 2 ** 32 - 1, 2 ** 31 - 1], dtype=np.uint32)
    rng = np.random.default_rng(3)
    g = vals[rng.integers(0, len(vals), size=(9, 131))]
    p = vals[rng.integers(0, len(vals), size=(9, 131))]
    ref_p, _ = _check(hip, g, p)
    assert len(ref_p) == 24                                # every pair but (0, 0) occurs
    assert ref_p.min() == 0 and ref_p.max() == 2 ** 32 - 1 and [2 ** 32 - 1, 2 ** 32 - 1] in ref_p.tolist()
    key = [int(a) * 2 ** 32 + int(b) for a, b in ref_p]
    assert all(a < b for a, b in zip(key[:-1], key[1:]))   # ascending as unsigned numbers


def test_few_pairs_in_every_row(hip):
    """the reduce path: 3000 rows x 3 spans of the same three pairs -- segments of 16 sorted spans that lie inside one
    pair, start one and straddle two"""
    g = np.zeros((3000, 96), dtype=np.uint32)
    p = np.zeros_like(g)
    g[:, 0:40] = 5
    p[:, 30:70] = 9
    g[:, 80:96] = 5
    ref_p, ref_c = _check(hip, g, p)
    assert ref_p.tolist() == [[0, 9], [5, 0], [5, 9]] and ref_c.tolist() == [30 * 3000, 46 * 3000, 10 * 3000]
    first = hip.label_overlaps(_dev(g), _dev(p))
    again = hip.label_overlaps(_dev(g), _dev(p))
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])


def test_a_count_past_int32_and_row_blocks(hip):
    """2^31 + 4096 voxels of uint8 with one non-zero pair: the wrapper cuts the rows into two calls (one call counts at
    most 2^31 - 1 spans), each call sums 4096-voxel spans in int64, and the merged count is past 2^31"""
    R, W = 2 ** 19 + 1, 4096
    need = 2 * R * W + (1 << 30)
    if torch.cuda.mem_get_info()[0] < need:
        pytest.skip(f"needs {need >> 20} MiB of free device memory")
    assert R * W == 2 ** 31 + 4096 and R * W > hip.OVERLAP_MAX_VOXELS
    g = torch.full((R, W), 3, dtype=torch.uint8, device='cuda')
    p = torch.full((R, W), 5, dtype=torch.uint8, device='cuda')
    pairs, counts = hip.label_overlaps(g, p)
    assert pairs.tolist() == [[3, 5]] and counts.tolist() == [2 ** 31 + 4096]
    del g, p


def test_every_dtype_combination(hip):
    rng = np.random.default_rng(4)
    g8 = (piecewise(rng, 33, 203, 200) % 256).astype(np.uint8)
    p8 = (piecewise(rng, 33, 203, 200) % 256).astype(np.uint8)
    ref_p, ref_c = np_table(g8, p8)
    for gd in (np.uint8, np.uint32):
        for pd in (np.uint8, np.uint32):
            for og, op in ((0, 0), (3, 3), (0, 1)):
                pairs, counts = hip.label_overlaps(_dev(g8.astype(gd), og), _dev(p8.astype(pd), op))
                np.testing.assert_array_equal(pairs.cpu().numpy(), ref_p, err_msg=f'{gd} {pd} {og} {op}')
                np.testing.assert_array_equal(counts.cpu().numpy(), ref_c, err_msg=f'{gd} {pd} {og} {op}')
    # int32 is read as uint32, and a side stream serves as well as the current one
    gi = torch.from_numpy(g8.astype(np.int32)).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    pairs, counts = hip.label_overlaps(gi, _dev(p8), stream=side)
    side.synchronize()
    np.testing.assert_array_equal(pairs.cpu().numpy(), ref_p)
    np.testing.assert_array_equal(counts.cpu().numpy(), ref_c)


def test_bad_operands_raise_before_any_launch(hip):
    g = torch.ones((6, 40), dtype=torch.int32, device='cuda')
    p = torch.ones((6, 40), dtype=torch.uint8, device='cuda')
    bad = [(g[:, ::2], p[:, ::2]),                         # not contiguous
           (g.t(), p.t()),
           (g.cpu(), p),                                   # host tensors
           (g, p.cpu()),
           (g.cpu().numpy(), p),
           (g, p[:5]),                                     # shapes differ
           (g.reshape(40, 6), p),
           (g.long(), p),                                  # dtypes the kernel does not read
           (g, p.to(torch.int16)),
           (g.float(), p)]
    for a, b in bad:
        with pytest.raises((hip.HipError, ValueError)):
            hip.label_overlaps(a, b)
    torch.cuda.synchronize()
    pairs, counts = hip.label_overlaps(g, p)
    assert pairs.tolist() == [[1, 1]] and counts.tolist() == [240]
