"""Python restatement of the tile / K-slab selection of the tiled fp32 convolution (cg_plan and emp_conv_splitk_plan in
empanada_amd/csrc/emp_conv.hip).  The library exports the K-slab and the split count but no query for the tile width
or the residual prefetch, so the tests that aim at one variant of conv_igemm_f32_kernel state the plan they expect
through this mirror; tests/test_conv_plan_host.py keeps the mirror honest against the exported queries."""
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
