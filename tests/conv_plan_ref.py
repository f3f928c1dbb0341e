"""Python restatement of the tile / K-slab selection of the tiled fp32 convolution (cg_plan and emp_conv_splitk_plan in
empanada_amd/csrc/emp_conv.hip).  The library exports the K-slab and the split count but no query for the tile width
or the residual prefetch, so the tests that aim at one variant of conv_igemm_f32_kernel state the plan they expect
through this mirror; tests/test_conv_plan_host.py keeps the mirror honest against the exported queries.  The second half
restates which kernel emp_gemm_nt_batched hands a batched launch to (weight-stationary, persistent stream or tiled) and
holds the launches of the Winograd and batched-GEMM branch tests."""
from collections import namedtuple

BM = 128                   # CG_BM: output pixels per block tile

ConvPlan = namedtuple('ConvPlan', 'narrow respf slab tiles_m tiles_n blocks')


def cdiv(a, b):
    return -(-a // b)


def conv_plan(M, Cout, Cin=32, batch=1, res=False):
    """res: the launch has a residual the kernel may prefetch (16-byte aligned, pixel stride a multiple of 4)"""
    wide = cdiv(M, BM) * cdiv(Cout, 128) * batch
    narrow = Cout <= 64 or (Cout % 128 != 0 and Cout % 128 <= 64 and Cout < 512) or wide < 256
    tn = cdiv(Cout, 64 if narrow else 128)
    blocks = cdiv(M, BM) * tn * batch
    respf = bool(res) and Cout % (64 if narrow else 128) == 0
    slab = 16 if blocks > 512 else 32
    if respf:
        slab = 32
    if Cin % 32:
        slab = 16
        respf = False
    return ConvPlan(narrow, respf, slab, cdiv(M, BM), tn, blocks)


ConvCase = namedtuple('ConvCase', 'N H W Cin Cout KH KW stride pad dil res narrow respf slab')

# The launches of tests/test_conv_branches_gpu.py and the variant of the tiled kernel each is meant to reach.
# res: None, 'plain' (a contiguous NHWC residual) or 'odd' (channels [1, 1 + Cout) of a Cout + 3 wide NHWC buffer:
# neither 16-byte aligned nor a pixel stride that is a multiple of 4, so it cannot be prefetched).
CONV_CASES = {
    # wide tiles, slab 16 by Cin: the tap changes on every slab
    'A': ConvCase(1, 128, 129, 16, 256, 3, 3, 1, 1, 1, None, False, False, 16),
    # wide, slab 16, tap change every third slab (the ring depth), 56 couts past Cout in the last tile, dilated
    'B': ConvCase(1, 128, 129, 48, 200, 3, 3, 1, 2, 2, None, False, False, 16),
    # wide, slab 16 by block count (514 blocks), even filter
    'C': ConvCase(1, 257, 514, 32, 256, 2, 2, 2, 0, 1, None, False, False, 16),
    # wide, slab 32, stride 2; 8 372 pixels per image = 65 tiles + 52 rows: a tile straddles the two images
    'D': ConvCase(2, 183, 181, 32, 256, 3, 3, 2, 1, 1, None, False, False, 32),
    # wide, residual prefetch, slab 32, tap gather
    'E': ConvCase(1, 128, 129, 32, 256, 3, 3, 1, 1, 1, 'plain', False, True, 32),
    # wide, residual prefetch, three cout tiles, three slabs
    'F': ConvCase(1, 128, 129, 96, 384, 1, 1, 1, 0, 1, 'plain', False, True, 32),
    # wide, a residual that cannot be prefetched (Cout % 128 != 0)
    'G': ConvCase(1, 128, 129, 32, 200, 1, 1, 1, 0, 1, 'plain', False, False, 32),
    # wide, slab 32, every off-centre tap outside the image (zero page only)
    'H': ConvCase(3, 75, 74, 32, 256, 3, 3, 1, 80, 80, None, False, False, 32),
    # narrow, slab 16, tap gather
    'I': ConvCase(4, 129, 128, 16, 64, 3, 3, 1, 1, 1, None, True, False, 16),
    # rectangular filters
    'J': ConvCase(1, 20, 23, 32, 40, 1, 7, 1, 0, 1, None, True, False, 32),
    'Jt': ConvCase(1, 20, 23, 32, 40, 7, 1, 1, 0, 1, None, True, False, 32),
    # the largest filter, stride 3
    'K': ConvCase(2, 30, 31, 32, 72, 7, 7, 3, 3, 1, 'plain', True, False, 32),
    # narrow, slab 16, residual read in the generic epilogue
    'L': ConvCase(4, 129, 128, 16, 64, 1, 1, 1, 0, 1, 'plain', True, False, 16),
    # wide, 516 blocks, residual not prefetchable by alignment: the launch sums in the no-residual plan's slab
    'M': ConvCase(1, 1, 32897, 32, 256, 1, 1, 1, 0, 1, 'odd', False, False, 16),
}


def out_size(c):
    OH = (c.H + 2 * c.pad - c.dil * (c.KH - 1) - 1) // c.stride + 1
    OW = (c.W + 2 * c.pad - c.dil * (c.KW - 1) - 1) // c.stride + 1
    return OH, OW


def splitk_plan(M, Cout, Cin, KH, KW):
    if M <= 0 or Cout <= 0 or Cin % 32 or Cout % 4:
        return 1
    p = conv_plan(M, Cout, Cin)
    tiles = p.tiles_m * p.tiles_n
    if tiles > 128:
        return 1
    S = KH * KW * (Cin // 32)
    k = min(256 // tiles, S // 4, 32)
    return k if k >= 2 else 1


# ---------------------------------------------------------------------------------------------------------------------
# emp_gemm_nt_batched (batch > 1: the Winograd position GEMMs) and the fused F(2x2) loader emp_wino_gemm_fused

WS_MIN_ROWS = 262144       # PW_MIN_ROWS_PLAN of emp_conv1x1.hip: batch x M rows from which the weight-stationary kernel takes a GEMM
WS_TILE_ROWS = 32          # PW_ROWS: it takes no entry shorter than one of its row tiles
STREAM_MIN_TILES = 2048    # CS_MIN_TOTAL of emp_conv.hip

GemmRoute = namedtuple('GemmRoute', 'route narrow slab blocks')


def gemm_route(batch, M, K, N):
    """which kernel emp_gemm_nt_batched gives a (batch, M, K) x (batch, N, K)^T launch with a 16-byte aligned C, and the
    plan it sums in: cg_plan at batch > 1, emp_gemm_ws_eligible, then the batch > 1 arm of emp_conv_stream_eligible.  A C
    that is not 16-byte aligned is 'tiled' whatever this says, in the same plan."""
    assert batch > 1 and K % 32 == 0
    p = conv_plan(M, N, 32, batch)
    ws = K in (64, 128) and N in (64, 128) and p.slab == 16 and M >= WS_TILE_ROWS and batch * M >= WS_MIN_ROWS
    stream = (not ws and N % 128 == 0 and p.slab == 16 and not p.narrow
              and STREAM_MIN_TILES <= p.blocks < (1 << 28))
    return GemmRoute('ws' if ws else 'stream' if stream else 'tiled', p.narrow, p.slab, p.blocks)


def wino_route(Cout):
    """the fused F(2x2) loader has a width rule of its own and one K-slab: (narrow, slab)"""
    return Cout <= 64, 32


def wino_tile_count(N, H, W, dil, m):
    """tiles of empanada_amd._hip.wino_tiles: per image, min(dil, H) x min(dil, W) sub-grids cut into m x m tiles"""
    rows = sum(cdiv(cdiv(H - r, dil), m) for r in range(min(dil, H)))
    cols = sum(cdiv(cdiv(W - r, dil), m) for r in range(min(dil, W)))
    return N * rows * cols


WINO_M = (2, 3, 4)         # F(m x m, 3x3): 16, 25 and 36 position GEMMs
WinoCase = namedtuple('WinoCase', 'N H W Cin Cout dil T plans fused_narrow')

# The launches of tests/test_wino_branches_gpu.py.  T: tiles at m = 2, 3, 4; plans: (narrow, slab) of the batched GEMM
# of the three-call path at m = 2, 3, 4 -- every one of them the tiled kernel's; fused_narrow: the tile width of the fused
# F(2x2) loader.
_W16, _W32, _N16, _N32 = (False, 16), (False, 32), (True, 16), (True, 32)
WINO_CASES = {
    # dilated, many tile rows, both wide slabs
    'P': WinoCase(1, 96, 100, 32, 256, 2, (2400, 1088, 624), (_W16, _W32, _W32), False),
    # 56 couts past Cout in the last 128-wide tile; the fused loader is wide with masked B rows
    'Q': WinoCase(1, 120, 124, 32, 200, 1, (3720, 1680, 930), (_W16, _W16, _W16), False),
    # three 64-wide tiles, 60 masked couts, dilation 3
    'R': WinoCase(1, 90, 94, 32, 132, 3, (2160, 990, 576), (_N16, _N16, _N16), False),
    # dilation > H and W: every off-centre tap outside the image, one-pixel sub-grids; two images
    'S': WinoCase(2, 3, 5, 32, 36, 7, (30, 30, 30), (_N32, _N32, _N32), True),
    # one pixel, the smallest Cout
    'T1': WinoCase(1, 1, 1, 32, 4, 1, (1, 1, 1), (_N32, _N32, _N32), True),
    # one column; the fused loader is narrow
    'C1': WinoCase(1, 13, 1, 64, 64, 2, (7, 5, 4), (_N32, _N32, _N32), True),
}

# (batch, M, K, N) -> (route, narrow, slab) of direct emp_gemm_nt_batched launches (tests/test_gemm_branches_gpu.py)
GEMM_CASES = {
    (16, 1100, 32, 256): ('tiled', False, 32),      # 288 blocks
    (36, 1030, 64, 256): ('tiled', False, 16),      # 648 blocks, below the stream minimum
    (25, 1500, 32, 200): ('tiled', False, 16),      # N % 128 = 72: 56 masked couts
    (16, 2100, 32, 132): ('tiled', True, 16),       # the narrow plan at slab 16
    (36, 300, 96, 40): ('tiled', True, 32),         # three slabs
    (3, 5000, 32, 384): ('tiled', False, 32),       # three cout tiles
    (16, 700, 32, 38): ('tiled', True, 32),         # N % 4 != 0: the scalar epilogue for every column
}
