"""The strip walks of two dense-path kernels that the shapes of tests/test_hip_kernels.py do not reach.

emp_dwconv_nhwc picks RY in {32, 16, 8} output rows per block; test_dwconv_nhwc only ever gets 8.  Here: RY = 32 and
16 (the rotation of the K partial rows wraps more often, the last strip is shorter than RY, rows + K - 1 is no multiple
of K), a block count that is no multiple of 8, and RY = 8 with more than one block along x and a thread tail.

upsample_nhwc_kernel (channels-last, C % 4 == 0) walks 16-column segments of an output row keeping two source texels:
rows of several segments with a ragged last one, shrinking (the source column advances by more than one per step, both
held texels are refetched), identity, and output sizes of 1.

Both bit for bit against oracle/dense.py, and against fp64 torch on the CPU within a stated bound."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FILL = -7.0


@pytest.fixture(scope='module')
def hip():
    from empanada_amd import _hip
    _hip.load()
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return _hip


def _cdiv(a, b):
    return -(-a // b)


def _dw_plan(k, N, H, W, C):
    """rows per block and blocks along x, as emp_dwconv_nhwc chooses them"""
    TX = 4 if k == 5 else 1
    gx = _cdiv(_cdiv(W, TX) * (C // 4), 256)
    RY = 32
    while RY > 8 and gx * _cdiv(H, RY) * N < 2048:
        RY //= 2
    return RY, gx, gx * _cdiv(H, RY) * N


@pytest.mark.parametrize('k,shape,bias,RY', [
    (5, (64, 1000, 9, 8), True, 32),       # last strip 8 rows; last pixel group of a row partial (W = 9, 4 px per thread)
    (3, (67, 990, 5, 4), False, 32),       # 2 077 blocks: not a multiple of 8; last strip 30 rows
    (5, (33, 1000, 5, 4), True, 16),       # last strip 8 rows
    (5, (2, 45, 300, 16), False, 8),       # two blocks along x, 300 of 512 threads at work; last strip 5 rows
    (3, (3, 70, 260, 8), True, 8),         # three blocks along x, 520 of 768 threads; last strip 6 rows
])
def test_dwconv_strips(hip, k, shape, bias, RY):
    """bit-exact against the C oracle; within 1e-5 * (sum|x||w| + 1) of an fp64 conv2d(groups=C)"""
    from oracle import dense as OD
    N, H, W, C = shape
    ry, gx, blocks = _dw_plan(k, N, H, W, C)
    assert ry == RY
    if RY == 32:
        assert blocks >= 2048 and H % RY != 0
    if RY == 8:
        assert gx > 1 and (gx * 256) > _cdiv(W, 4 if k == 5 else 1) * (C // 4)
    if (k, N) == (3, 67):
        assert blocks == 2077 and blocks % 8 != 0
    g = torch.Generator().manual_seed(k * 1000 + H + N)
    x = torch.randn(N, H, W, C, generator=g)
    w = torch.randn(C, 1, k, k, generator=g) * 0.2
    b = torch.randn(C, generator=g) if bias else None
    w_kkc = w.reshape(C, k * k).t().contiguous()
    xd = x.cuda().permute(0, 3, 1, 2)
    got = hip.dwconv_nhwc(xd, w_kkc.cuda(), b.cuda() if bias else None, k)
    got_nhwc = got.permute(0, 2, 3, 1).cpu()
    exp = OD.dwconv_nhwc(x.numpy(), w_kkc.numpy(), b.numpy() if bias else None)
    np.testing.assert_array_equal(got_nhwc.numpy().view(np.uint32), exp.view(np.uint32))
    x64, w64 = x.permute(0, 3, 1, 2).double(), w.double()
    y = torch.nn.functional.conv2d(x64, w64, b.double() if bias else None, padding=k // 2, groups=C)
    bound = 1e-5 * (torch.nn.functional.conv2d(x64.abs(), w64.abs(), None, padding=k // 2, groups=C) + 1)
    err = (got_nhwc.permute(0, 3, 1, 2).double() - y).abs()
    print(f"dwconv k={k} {shape}: RY = {ry}, max err / bound vs fp64 = {float((err / bound).max()):.3e}")
    assert torch.all(err <= bound)


def _vector_form(x, y):
    """the condition under which emp_upsample_bilinear runs upsample_nhwc_kernel"""
    C = x.shape[1]
    strides = [x.stride(0), x.stride(2), x.stride(3), y.stride(0), y.stride(2), y.stride(3)]
    return (C % 4 == 0 and x.stride(1) == 1 and y.stride(1) == 1 and all(s % 4 == 0 for s in strides) and
            x.data_ptr() % 16 == 0 and y.data_ptr() % 16 == 0)


@pytest.mark.parametrize('shape,size', [
    ((1, 8, 5, 7), (33, 50)),              # four segments, the last with 2 columns
    ((2, 4, 40, 37), (9, 11)),             # shrinking: the source column advances by 3-4 per step
    ((1, 4, 3, 3), (3, 3)),                # identity
    ((1, 4, 6, 2), (1, 37)),               # H = 1: ry = 0
    ((2, 12, 9, 1), (17, 1)),              # W = 1: rx = 0
    ((1, 4, 2, 2), (64, 129)),             # nine segments, the last a single column
])
def test_upsample_segments(hip, shape, size):
    """bit-exact against the numpy oracle.  Against an fp64 F.interpolate(align_corners=True):
    |err| <= (2^-22 ((h-1) + (w-1)) + 2^-21) max|x| -- the source coordinate s = r * dst carries two fp32 roundings
    (the ratio and the product), |ds| <= 2^-23 (in - 1) per axis; the value is Lipschitz in s with a constant of at most
    2 max|x| per axis; the mix adds at most 8 roundings of values no larger than max|x|."""
    from oracle import dense as OD
    N, C, h, w = shape
    H, W = size
    g = torch.Generator().manual_seed(sum(shape) + 31 * H + W)
    x = torch.randn(N, h, w, C, generator=g)
    x_nchw = x.permute(0, 3, 1, 2)
    xd = x.cuda().permute(0, 3, 1, 2)                         # channels-last memory
    exp = OD.upsample_bilinear(x_nchw.numpy(), size).view(np.uint32)

    got = hip.upsample_bilinear(xd, size)
    assert _vector_form(xd, got)
    np.testing.assert_array_equal(got.cpu().numpy().view(np.uint32), exp)

    ref = torch.nn.functional.interpolate(x_nchw.double(), size=size, mode='bilinear', align_corners=True)
    bound = (2.0 ** -22 * ((h - 1) + (w - 1)) + 2.0 ** -21) * float(x.abs().max())
    err = float((got.cpu().double() - ref).abs().max())
    print(f"upsample {shape} -> {size}: max err / bound vs fp64 = {err / bound:.4f}")
    assert err <= bound

    # channels [4, 4 + C) of a C + 8 wide channels-last buffer: still the vector kernel
    buf = torch.full((N, H, W, C + 8), FILL, device='cuda')
    out = buf[..., 4:4 + C].permute(0, 3, 1, 2)
    assert _vector_form(xd, out)
    hip.upsample_bilinear(xd, size, out=out)
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), exp)
    assert torch.all(buf[..., :4] == FILL) and torch.all(buf[..., 4 + C:] == FILL)
    # channels [2, 2 + C) of a C + 3 wide one: strides that are no multiples of 4, the planar kernel's scalar stores
    buf = torch.full((N, H, W, C + 3), FILL, device='cuda')
    out = buf[..., 2:2 + C].permute(0, 3, 1, 2)
    assert not _vector_form(xd, out)
    hip.upsample_bilinear(xd, size, out=out)
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), exp)
    assert torch.all(buf[..., :2] == FILL) and torch.all(buf[..., 2 + C:] == FILL)
