"""The Python mirror of the tiled convolution's plan (tests/conv_plan_ref.py) against the host queries the library
exports -- emp_conv_k_slab, emp_conv_k_slab_cin, emp_conv_k_slab_geom, emp_conv_splitk_plan -- on a seeded sweep of the
dispatch space, and the plans tests/test_conv_branches_gpu.py expects of its launches.  No GPU needed."""
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
