"""The Python mirror of the tiled convolution's plan (tests/conv_plan_ref.py) against the host queries the library
exports -- emp_conv_k_slab, emp_conv_k_slab_cin, emp_conv_k_slab_geom, emp_conv_splitk_plan -- on a seeded sweep of the
dispatch space, and the plans tests/test_conv_branches_gpu.py expects of its launches.  The same for the batched GEMM
(gemm_route against emp_conv_k_slab and emp_conv_stream_eligible at batch > 1) with the launches of
tests/test_wino_branches_gpu.py and tests/test_gemm_branches_gpu.py, and the Winograd tile tables of
empanada_amd._hip.wino_tiles, which must partition the output pixels.  No GPU needed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_plan_ref as ref  # noqa: E402

DRAWS = 24000
COUTS_AT_THE_RULES = [60, 63, 64, 65, 68, 72, 124, 127, 128, 129, 132, 136, 188, 191, 192, 193, 196, 200, 252, 256, 260,
                      320, 324, 384, 448, 449, 452, 508, 511, 512, 513, 516, 576, 580, 640, 1024]


@pytest.fixture(scope='module')
def lib():
    from empanada_amd import _hip
    return _hip.load()


def _draws():
    """(M, Cout, Cin, batch, res): half of the M at a multiple of 128 minus one, plus nothing or plus one, the multiple
    itself log-uniform so that the 256-tile, 512-block and 128-tile (split-K) thresholds all see both sides; half of
    the Cout from the values around 64, 128 and 512 and their residues mod 128"""
    rng = np.random.default_rng(20240607)
    out = []
    for i in range(DRAWS):
        t = int(round(2.0 ** rng.uniform(0, 12.5)))            # pixel tiles, 1 .. 5 793
        if i % 2:
            M = max(1, t * 128 + int(rng.integers(-1, 2)))
        else:
            M = max(1, t * 128 - int(rng.integers(0, 128)))
        Cout = int(rng.choice(COUTS_AT_THE_RULES)) if rng.random() < 0.5 else int(rng.integers(1, 1100))
        Cin = 16 * int(rng.integers(1, 80))
        batch = 1 if rng.random() < 0.6 else int(rng.integers(2, 40))
        out.append((M, Cout, Cin, batch, bool(rng.integers(0, 2))))
    return out


def test_sweep_covers_both_sides_of_every_rule():
    """the sweep is only worth its equalities if the draws reach every outcome of the mirror"""
    seen = set()
    for M, Cout, Cin, batch, res in _draws():
        p = ref.conv_plan(M, Cout, Cin, batch, res)
        seen.add((p.narrow, p.respf, p.slab, Cin % 32 == 0, p.blocks > 512))
        seen.add(('m', M % 128))
        seen.add(('k', ref.splitk_plan(M, Cout, Cin, 3, 3) > 1))
    for narrow in (False, True):
        assert (narrow, True, 32, True, True) in seen           # prefetch keeps slab 32 above 512 blocks
        assert (narrow, False, 16, True, True) in seen
        assert (narrow, False, 32, True, False) in seen
        assert (narrow, False, 16, False, False) in seen        # slab 16 by Cin alone
    assert {('m', 127), ('m', 0), ('m', 1), ('k', True), ('k', False)} <= seen


def test_slab_mirror_equals_the_queries(lib):
    bad = []
    for M, Cout, Cin, batch, res in _draws():
        if ref.conv_plan(M, Cout, Cin, batch, res).slab != lib.emp_conv_k_slab_cin(M, Cout, batch, int(res), Cin):
            bad.append(('cin', M, Cout, Cin, batch, res))
        if ref.conv_plan(M, Cout, 32, batch, res).slab != lib.emp_conv_k_slab(M, Cout, batch, int(res)):
            bad.append(('plain', M, Cout, batch, res))
    assert not bad, f"{len(bad)} mismatches, first: {bad[:5]}"


def test_splitk_mirror_equals_the_query(lib):
    rng = np.random.default_rng(7)
    bad = []
    for M, Cout, Cin, _, _ in _draws():
        KH, KW = int(rng.integers(1, 8)), int(rng.integers(1, 8))
        if ref.splitk_plan(M, Cout, Cin, KH, KW) != lib.emp_conv_splitk_plan(M, Cout, Cin, KH, KW):
            bad.append((M, Cout, Cin, KH, KW))
    assert not bad, f"{len(bad)} mismatches, first: {bad[:5]}"


@pytest.mark.parametrize('name', sorted(ref.CONV_CASES))
def test_branch_cases_reach_their_plan(lib, name):
    """every launch of tests/test_conv_branches_gpu.py resolves, by its shape alone, to the variant of the tiled kernel
    it is there for, and none of them is a shape of the weight-stationary or the persistent kernel"""
    c = ref.CONV_CASES[name]
    OH, OW = ref.out_size(c)
    M = c.N * OH * OW
    has_res = c.res is not None
    p = ref.conv_plan(M, c.Cout, c.Cin, 1, c.res == 'plain')
    assert (p.narrow, p.respf, p.slab) == (c.narrow, c.respf, c.slab)
    q = ref.conv_plan(M, c.Cout, c.Cin, 1, has_res)             # what the queries are told: a residual, prefetchable
    assert lib.emp_conv_k_slab_cin(M, c.Cout, 1, int(has_res), c.Cin) == q.slab
    assert lib.emp_conv_k_slab_geom(M, c.Cout, int(has_res), c.Cin, c.KH, c.KW, c.stride, c.pad, 1) == q.slab
    if c.res == 'odd':
        assert (q.slab, c.slab) == (32, 16)                     # the queries' has_residual means a PREFETCHABLE residual
    else:
        assert q.slab == c.slab
    assert lib.emp_conv_stream_eligible(1, M, c.Cin, c.Cout, c.KH, c.KW, c.stride, c.pad, 1, int(has_res), 0) == 0
    assert lib.emp_conv1x1_ws_kind_for(M, c.Cin, c.Cout, c.KH, c.KW, c.stride, c.pad, 1, int(has_res)) == 0


GEMM_DRAWS = 6000


def _gemm_draws():
    """(batch, M, K, N) of batched GEMMs: the batch counts of the tests (3 and the 16 / 25 / 36 Winograd positions); M
    log-uniform around a multiple of 128 up to 131 072 rows, so that the 256-block, 512-block, 2 048-tile and
    262 144-row thresholds all see both sides; half of the N and most of the K from the values the rules name"""
    rng = np.random.default_rng(20240911)
    out = []
    for i in range(GEMM_DRAWS):
        batch = int(rng.choice([3, 16, 25, 36]))
        t = int(round(2.0 ** rng.uniform(0, 10)))
        M = max(1, t * 128 + (int(rng.integers(-1, 2)) if i % 2 else -int(rng.integers(0, 128))))
        N = int(rng.choice([64, 128, 256, 384] + COUTS_AT_THE_RULES)) if rng.random() < 0.6 else int(rng.integers(1, 700))
        K = int(rng.choice([32, 64, 128, 256])) if rng.random() < 0.8 else 32 * int(rng.integers(1, 20))
        out.append((batch, M, K, N))
    return out


def test_gemm_sweep_covers_every_route():
    seen = set()
    for batch, M, K, N in _gemm_draws():
        r = ref.gemm_route(batch, M, K, N)
        seen.add((r.route, r.narrow, r.slab))
        if N % 128 == 0 and not r.narrow and r.slab == 16 and r.route != 'ws':
            seen.add(('tiles', r.blocks >= ref.STREAM_MIN_TILES))
    assert {('ws', False, 16), ('ws', True, 16), ('stream', False, 16), ('tiled', False, 16), ('tiled', False, 32),
            ('tiled', True, 16), ('tiled', True, 32), ('tiles', False), ('tiles', True)} <= seen


def test_gemm_mirror_equals_the_queries(lib):
    """the slab of gemm_route is emp_conv_k_slab at that batch; its 'stream' is the batch > 1 arm of
    emp_conv_stream_eligible, which also answers 0 for what the weight-stationary kernel takes"""
    bad = []
    for batch, M, K, N in _gemm_draws():
        r = ref.gemm_route(batch, M, K, N)
        if r.slab != lib.emp_conv_k_slab(M, N, batch, 0):
            bad.append(('slab', batch, M, K, N))
        if int(r.route == 'stream') != lib.emp_conv_stream_eligible(batch, M, K, N, 1, 1, 1, 0, 0, 0, 0):
            bad.append(('stream', batch, M, K, N))
    assert not bad, f"{len(bad)} mismatches, first: {bad[:5]}"


def test_gemm_cases_reach_their_route(lib):
    """the direct launches of tests/test_gemm_branches_gpu.py, and what the table's comments promise of them"""
    for (batch, M, K, N), want in ref.GEMM_CASES.items():
        r = ref.gemm_route(batch, M, K, N)
        assert (r.route, r.narrow, r.slab) == want, (batch, M, K, N)
        assert lib.emp_conv_k_slab(M, N, batch, 0) == r.slab
        assert lib.emp_conv_stream_eligible(batch, M, K, N, 1, 1, 1, 0, 0, 0, 0) == 0
        assert M % 128 != 0                                       # a partial last row tile in every entry
    G = ref.gemm_route
    assert G(16, 1100, 32, 256).blocks == 288 and G(36, 1030, 64, 256).blocks == 648 < ref.STREAM_MIN_TILES
    assert 200 % 128 == 72 and 38 % 4 != 0 and G(3, 5000, 32, 384).blocks == 3 * 40 * 3 and 96 // 32 == 3


@pytest.mark.parametrize('name', sorted(ref.WINO_CASES))
def test_wino_cases_reach_their_route(lib, name):
    """every launch of tests/test_wino_branches_gpu.py: the tile counts, the plan of the three-call path's GEMM at
    m = 2, 3, 4 (always the tiled kernel), and the width of the fused F(2x2) loader"""
    from empanada_amd import _hip
    c = ref.WINO_CASES[name]
    for m, T, plan in zip(ref.WINO_M, c.T, c.plans):
        batch = (m + 2) ** 2
        assert len(_hip.wino_tiles(c.N, c.H, c.W, c.dil, m)) == ref.wino_tile_count(c.N, c.H, c.W, c.dil, m) == T
        r = ref.gemm_route(batch, T, c.Cin, c.Cout)
        assert (r.route, r.narrow, r.slab) == ('tiled',) + plan
        assert lib.emp_conv_k_slab(T, c.Cout, batch, 0) == r.slab
        assert lib.emp_conv_stream_eligible(batch, T, c.Cin, c.Cout, 1, 1, 1, 0, 0, 0, 0) == 0
        assert batch * T < ref.WS_MIN_ROWS
        assert lib.emp_wino4_fused_eligible(T, c.Cin, c.Cout, 1) == 0
    assert ref.wino_route(c.Cout) == (c.fused_narrow, 32)


def test_wino_cases_geometry():
    """what the table's comments promise of the shapes"""
    C = ref.WINO_CASES
    plans = {p for c in C.values() for p in c.plans}
    assert plans == {(False, 16), (False, 32), (True, 16), (True, 32)}
    assert {ref.wino_route(c.Cout)[0] for c in C.values()} == {False, True}
    assert 128 - C['Q'].Cout % 128 == 56 and ref.cdiv(C['R'].Cout, 64) == 3 and 3 * 64 - C['R'].Cout == 60
    s = C['S']
    assert s.dil > max(s.H, s.W) and s.T == (s.N * s.H * s.W,) * 3    # one tile per pixel: no tap but the centre is inside
    assert (C['T1'].H, C['T1'].W, C['T1'].Cout) == (1, 1, 4) and C['C1'].W == 1
    assert all(t > 2 * 128 for t in C['P'].T + C['Q'].T + C['R'].T)   # more than two tile rows, fused loader included


WINO_TILE_SHAPES = [(1, 1, 1, 1), (2, 3, 5, 7), (1, 5, 7, 6), (1, 2, 9, 3), (1, 13, 1, 2), (2, 33, 35, 12), (1, 17, 19, 18)]


@pytest.mark.parametrize('m', ref.WINO_M)
@pytest.mark.parametrize('shape', WINO_TILE_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_wino_tiles_partition_the_output(shape, m):
    """wino_tiles(N, H, W, dil, m): every output pixel in exactly one tile, no covered pixel at a negative coordinate, the
    table typed and ordered as the kernels read it -- images smaller than a tile, single rows and columns, dil >= H, W"""
    from empanada_amd import _hip
    N, H, W, dil = shape
    tiles = _hip.wino_tiles(N, H, W, dil, m)
    assert tiles.dtype == np.int32 and tiles.ndim == 2 and tiles.shape[1] == 3 and tiles.flags['C_CONTIGUOUS']
    assert len(tiles) == ref.wino_tile_count(N, H, W, dil, m)
    assert tiles[:, 0].min() == 0 and tiles[:, 0].max() == N - 1 and np.all(np.diff(tiles[:, 0]) >= 0)
    seen = np.zeros((N, H, W), dtype=np.int32)
    for a in range(m):
        for b in range(m):
            yy, xx = tiles[:, 1] + dil + a * dil, tiles[:, 2] + dil + b * dil
            assert yy.min() >= 0 and xx.min() >= 0
            ok = (yy < H) & (xx < W)
            np.add.at(seen, (tiles[ok, 0], yy[ok], xx[ok]), 1)
    assert np.all(seen == 1)
    # a tile's first output pixel is inside the image: no tile is all mask
    assert np.all(tiles[:, 1] + dil < H) and np.all(tiles[:, 2] + dil < W)


def test_branch_cases_geometry():
    """what the table's comments promise of the shapes"""
    C = ref.CONV_CASES
    m = {k: C[k].N * ref.out_size(C[k])[0] * ref.out_size(C[k])[1] for k in C}
    assert ref.conv_plan(m['C'], 256).blocks == 514 and ref.conv_plan(m['M'], 256).blocks == 516
    per_image = m['D'] // 2
    assert per_image % 128 != 0                                  # a tile of case D holds rows of both images
    assert C['B'].Cout % 128 > 64 and 128 - C['B'].Cout % 128 == 56
    assert all(m[k] % 128 for k in 'DHJK') and m['M'] % 128 == 1   # partial last pixel tiles; M: a single row
    h = C['H']
    assert ref.out_size(h) == (h.H, h.W) and h.dil >= max(h.H, h.W)   # off-centre taps are a whole image away
