"""Weight-stationary kernel (emp_conv1x1.hip) on the shapes that sum in the tiled kernel's order: the batched GEMM behind
emp_gemm_nt_batched (K, N in {64, 128}) and the 256 -> 64, 64 -> 64, 256 -> 128 pointwise convolutions behind
emp_conv_bn_act_nhwc.  Bit-exact against oracle/dense.py::conv_bn_act_nhwc with the K-slab the library reports.

A 1x1 convolution is a per-row function, so the inputs repeat a block of P distinct rows (P prime, no multiple of any
tile): the oracle runs on the P rows once and EVERY output row of the launch is compared with its row of that result."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MIN_ROWS = 262144          # PW_MIN_ROWS_PLAN of emp_conv1x1.hip: rows (batch x M for the GEMM) from which a shape is eligible


@pytest.fixture(scope='module')
def hip():
    from empanada_amd import _hip
    _hip.load()
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return _hip


def _gemm(hip, A, B):
    batch, M, K = A.shape
    N = B.shape[1]
    C = torch.full((batch, M, N), float('nan'), device='cuda')
    hip.call('emp_gemm_nt_batched', A.data_ptr(), B.data_ptr(), batch, M, N, K, C.data_ptr(), hip.stream())
    torch.cuda.synchronize()
    return C


def _gemm_case(hip, batch, M, K, N, P, slab):
    """C_b = A_b B_b^T on rows repeating with period P, compared row by row with one 1x1 oracle call per batch entry"""
    from oracle import dense as OD
    g = torch.Generator().manual_seed(1000 * K + N + batch)
    base = torch.randn(batch, P, K, generator=g)
    B = torch.randn(batch, N, K, generator=g) * (1.0 / K ** 0.5)
    idx = torch.arange(M) % P
    A = base.cuda()[:, idx.cuda()].contiguous()
    got = _gemm(hip, A, B.cuda()).cpu().numpy()
    for b in range(batch):
        exp = OD.conv_bn_act_nhwc(base[b][None, None].numpy(), B[b][:, None, None, :].numpy(), slab=slab)[0, 0]
        np.testing.assert_array_equal(got[b].view(np.uint32), exp[idx.numpy()].view(np.uint32), err_msg=f'batch entry {b}')


@pytest.mark.parametrize('K,N', [(64, 64), (128, 128), (64, 128), (128, 64)])
def test_gemm_batched_36(hip, K, N):
    """36 entries (the Winograd F(4x4,3x3) positions) at the smallest eligible M plus 17: the last tile of every entry is
    partial, and the 256 blocks' ranges of the (entry, tile) sequence start and end inside entries."""
    batch = 36
    M = -(-MIN_ROWS // batch) + 17
    slab = hip.conv_k_slab(M, N, batch)
    assert slab == 16
    _gemm_case(hip, batch, M, K, N, 523, slab)


@pytest.mark.parametrize('K,N', [(64, 64), (128, 128)])
def test_gemm_batched_3(hip, K, N):
    """three long entries: every block works inside one entry, a few cross into the next"""
    batch = 3
    M = -(-MIN_ROWS // batch) + 17
    slab = hip.conv_k_slab(M, N, batch)
    assert slab == 16
    _gemm_case(hip, batch, M, K, N, 1031, slab)


@pytest.mark.parametrize('K,N', [(64, 64), (128, 128)])
def test_gemm_plan32_stays_tiled(hip, K, N):
    """Launches for which emp_conv_k_slab answers 32 have at most 512 blocks of 128 rows, far fewer rows than the
    weight-stationary kernel asks for: they are not eligible and give the tiled kernel's result (K-slab 32)."""
    batch, M = 3, 4099 + 17
    assert batch * M < MIN_ROWS
    slab = hip.conv_k_slab(M, N, batch)
    assert slab == 32
    _gemm_case(hip, batch, M, K, N, 523, slab)


def _conv_case(hip, Cin, Cout, relu, out_slice):
    from oracle import dense as OD
    H, W = 3, 87387
    M = H * W
    assert M == MIN_ROWS + 17
    P = 4099
    assert hip.query('emp_conv1x1_ws_eligible', M, Cin, Cout, 1, 1, 1, 0, int(relu)) == 1
    assert hip.query('emp_conv1x1_ws_eligible', MIN_ROWS - 1, Cin, Cout, 1, 1, 1, 0, int(relu)) == 0
    # the order does not depend on which kernel runs: the geometry-aware answer is the tiled kernel's plan
    slab = hip.conv_k_slab(M, Cout, 1, False, Cin, geom=(1, 1, 1, 0), relu=relu)
    assert slab == hip.conv_k_slab(M, Cout, 1, False, Cin) == 16
    g = torch.Generator().manual_seed(Cin + Cout + int(relu))
    base = torch.randn(P, Cin, generator=g)
    w = torch.randn(Cout, 1, 1, Cin, generator=g) * (1.0 / Cin ** 0.5)
    sc, sh = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g)
    idx = torch.arange(M) % P
    x = base.cuda()[idx.cuda()].view(1, H, W, Cin).permute(0, 3, 1, 2)       # channels_last (1, Cin, H, W)
    out = None
    if out_slice:
        buf = torch.full((1, H, W, Cout + 96), -7.0, device='cuda').permute(0, 3, 1, 2)
        out = buf[:, 32:32 + Cout]
    got = hip.conv_bn_act_nhwc(x, w.cuda(), sc.cuda(), sh.cuda(), None, relu, 1, 0, 1, out=out)
    exp = OD.conv_bn_act_nhwc(base[None, None].numpy(), w.numpy(), sc.numpy(), sh.numpy(), None, relu, 1, 0, 1,
                              slab=slab)[0, 0]
    if not relu:
        assert (exp < 0).any()
    gotn = got.permute(0, 2, 3, 1).reshape(M, Cout).cpu().numpy()
    np.testing.assert_array_equal(gotn.view(np.uint32), exp[idx.numpy()].view(np.uint32))
    if out_slice:
        assert torch.all(buf[:, :32] == -7.0) and torch.all(buf[:, 32 + Cout:] == -7.0)


@pytest.mark.parametrize('Cin,Cout', [(256, 64), (64, 64), (256, 128)])
def test_conv_bn_relu(hip, Cin, Cout):
    """the bottleneck's conv1 shapes of layer1 / layer2 with BN + ReLU, 262 144 + 17 pixels"""
    _conv_case(hip, Cin, Cout, True, False)


def test_conv_bn_no_relu(hip):
    _conv_case(hip, 256, 64, False, False)


@pytest.mark.parametrize('Cin,Cout', [(64, 64), (256, 128)])
def test_conv_out_channel_slice(hip, Cin, Cout):
    """the output is a channel slice of a wider NHWC buffer (out_pixel_stride > Cout), as in the decoder's concat buffers:
    64- and 128-cout groups; the neighbouring channels stay untouched"""
    _conv_case(hip, Cin, Cout, True, True)


def test_conv_with_residual_stays_tiled(hip):
    """a residual on one of these shapes is not the weight-stationary kernel's business: tiled kernel, its slab (32)"""
    from oracle import dense as OD
    Cin = Cout = 64
    H, W = 3, 87387
    M, P = H * W, 4099
    slab = hip.conv_k_slab(M, Cout, 1, True, Cin, geom=(1, 1, 1, 0), relu=True)
    assert slab == 32
    g = torch.Generator().manual_seed(7)
    base = torch.randn(P, Cin, generator=g)
    rbase = torch.randn(P, Cout, generator=g)
    w = torch.randn(Cout, 1, 1, Cin, generator=g) * (1.0 / Cin ** 0.5)
    sc, sh = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g)
    idx = torch.arange(M) % P
    x = base.cuda()[idx.cuda()].view(1, H, W, Cin).permute(0, 3, 1, 2)
    res = rbase.cuda()[idx.cuda()].view(1, H, W, Cout).permute(0, 3, 1, 2)
    got = hip.conv_bn_act_nhwc(x, w.cuda(), sc.cuda(), sh.cuda(), res, True, 1, 0, 1)
    exp = OD.conv_bn_act_nhwc(base[None, None].numpy(), w.numpy(), sc.numpy(), sh.numpy(), rbase[None, None].numpy(),
                              True, 1, 0, 1, slab=slab)[0, 0]
    gotn = got.permute(0, 2, 3, 1).reshape(M, Cout).cpu().numpy()
    np.testing.assert_array_equal(gotn.view(np.uint32), exp[idx.numpy()].view(np.uint32))
