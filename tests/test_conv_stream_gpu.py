"""Persistent tile-stream form of the tiled fp32 kernel (emp_conv_stream.hip), reached through emp_conv_bn_act_nhwc and
emp_gemm_nt_batched for 1x1 / stride 1 launches without a residual whose plan is K-slab 16 and 128-wide tiles, from
2 048 tiles on.  Bit-exact against oracle/dense.py with the K-slab the library reports (16).

A 1x1 convolution is a per-row function, so the inputs repeat a block of P distinct rows (P prime, no multiple of any
tile): the oracle runs on the P rows once and EVERY output row of the launch is compared with its row of that result.

emp_conv_bn_act_proj_nhwc is not taken over by the persistent kernel (its query answers 0): the PROJ cases below pin
the results of those launches, at the sizes at which they would be eligible, on whichever kernel runs them."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MIN_TOTAL = 2048           # CS_MIN_TOTAL of emp_conv.hip: tiles (8/3 per resident block) from which a launch is eligible


def min_rows(Cout, batch=1):
    """smallest M for which batch x ceil(M / 128) x Cout / 128 tiles reach MIN_TOTAL"""
    tiles_m = -(-MIN_TOTAL // (batch * (Cout // 128)))
    return (tiles_m - 1) * 128 + 1


@pytest.fixture(scope='module')
def hip():
    from empanada_amd import _hip
    _hip.load()
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return _hip


def _eligible(hip, M, Cin, Cout, batch=1, KH=1, KW=1, stride=1, pad=0, relu=1, res=0, proj=0):
    return hip.query('emp_conv_stream_eligible', batch, M, Cin, Cout, KH, KW, stride, pad, relu, res, proj)


def _conv_case(hip, M, Cin, Cout, relu, P=4099, out_slice=False, expect_stream=True):
    from oracle import dense as OD
    slab = hip.conv_k_slab(M, Cout, 1, False, Cin, geom=(1, 1, 1, 0), relu=relu)
    assert slab == hip.conv_k_slab(M, Cout, 1, False, Cin) == 16
    g = torch.Generator().manual_seed(Cin + Cout + int(relu) + M % 1000)
    base = torch.randn(P, Cin, generator=g)
    w = torch.randn(Cout, 1, 1, Cin, generator=g) * (1.0 / Cin ** 0.5)
    sc, sh = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g)
    idx = torch.arange(M) % P
    x = base.cuda()[idx.cuda()].view(1, 1, M, Cin).permute(0, 3, 1, 2)       # channels_last (1, Cin, 1, M)
    out = buf = None
    if out_slice:
        buf = torch.full((1, 1, M, Cout + 96), -7.0, device='cuda').permute(0, 3, 1, 2)
        out = buf[:, 32:32 + Cout]
    before = hip.query('emp_conv_stream_launches')
    got = hip.conv_bn_act_nhwc(x, w.cuda(), sc.cuda(), sh.cuda(), None, relu, 1, 0, 1, out=out)
    torch.cuda.synchronize()
    assert hip.query('emp_conv_stream_launches') - before == int(expect_stream)
    exp = OD.conv_bn_act_nhwc(base[None, None].numpy(), w.numpy(), sc.numpy(), sh.numpy(), None, relu, 1, 0, 1,
                              slab=slab)[0, 0]
    if not relu:
        assert (exp < 0).any()
    gotn = got.permute(0, 2, 3, 1).reshape(M, Cout).cpu().numpy()
    np.testing.assert_array_equal(gotn.view(np.uint32), exp[idx.numpy()].view(np.uint32))
    if out_slice:
        assert torch.all(buf[:, :32] == -7.0) and torch.all(buf[:, 32 + Cout:] == -7.0)


@pytest.mark.parametrize('Cout', [128, 256])
@pytest.mark.parametrize('Cin', [16, 32, 48, 80])
def test_conv_slab_counts(hip, Cin, Cout):
    """1, 2, 3 and 5 slabs per tile -- below, at and above the ring depth, so the prefetch spans one or two tile
    boundaries -- at the smallest eligible row count plus 17 (the last pixel tile is partial); BN + ReLU"""
    M = min_rows(Cout) + 17
    assert _eligible(hip, M, Cin, Cout) == 1
    _conv_case(hip, M, Cin, Cout, True)


def test_conv_no_relu(hip):
    M = min_rows(128) + 17
    assert _eligible(hip, M, 48, 128, relu=0) == 1
    _conv_case(hip, M, 48, 128, False)


@pytest.mark.parametrize('Cout', [128, 256])
def test_threshold(hip, Cout):
    """the query on each side of the minimum, and the launch on each side takes the kernel the query names"""
    M = min_rows(Cout)
    assert _eligible(hip, M, 32, Cout) == 1
    assert _eligible(hip, M - 1, 32, Cout) == 0
    _conv_case(hip, M - 1, 32, Cout, True, expect_stream=False)
    _conv_case(hip, M, 32, Cout, True)


def test_uneven_walk(hip):
    """2 349 tiles: not a multiple of the grid, nor of 8 -- blocks get three or four tiles and the XCDs' chunks end
    inside a round"""
    tiles = MIN_TOTAL + 8 * 37 + 5
    M = (tiles - 1) * 128 + 77
    assert _eligible(hip, M, 48, 128) == 1
    _conv_case(hip, M, 48, 128, True)


def test_one_to_two_tiles_per_block(hip, monkeypatch):
    """1 157 tiles on 768 blocks (the minimum lowered for this launch): blocks with one tile and blocks with two, the
    first kind done before the others' second tile starts"""
    monkeypatch.setenv('EMP_CONV_STREAM_MIN_TILES', '1')
    tiles = 1157
    M = (tiles - 1) * 128 + 5
    assert _eligible(hip, M, 80, 128) == 1
    _conv_case(hip, M, 80, 128, True)
    monkeypatch.delenv('EMP_CONV_STREAM_MIN_TILES')
    assert _eligible(hip, M, 80, 128) == 0


@pytest.mark.parametrize('Cin,Cout', [(32, 128), (80, 256)])
def test_conv_out_channel_slice(hip, Cin, Cout):
    """the output is a channel slice of a wider NHWC buffer (out_pixel_stride > Cout), as in the decoder's concat
    buffers; the neighbouring channels stay untouched"""
    _conv_case(hip, min_rows(Cout) + 17, Cin, Cout, True, out_slice=True)


def _gemm_case(hip, batch, M, K, N, P):
    from oracle import dense as OD
    slab = hip.conv_k_slab(M, N, batch)
    assert slab == 16
    assert _eligible(hip, M, K, N, batch=batch, relu=0) == 1
    g = torch.Generator().manual_seed(1000 * K + N + batch)
    base = torch.randn(batch, P, K, generator=g)
    B = torch.randn(batch, N, K, generator=g) * (1.0 / K ** 0.5)
    idx = torch.arange(M) % P
    A = base.cuda()[:, idx.cuda()].contiguous()
    C = torch.full((batch, M, N), float('nan'), device='cuda')
    before = hip.query('emp_conv_stream_launches')
    hip.call('emp_gemm_nt_batched', A.data_ptr(), B.cuda().data_ptr(), batch, M, N, K, C.data_ptr(), hip.stream())
    torch.cuda.synchronize()
    assert hip.query('emp_conv_stream_launches') - before == 1
    got = C.cpu().numpy()
    for b in range(batch):
        exp = OD.conv_bn_act_nhwc(base[b][None, None].numpy(), B[b][:, None, None, :].numpy(), slab=slab)[0, 0]
        np.testing.assert_array_equal(got[b].view(np.uint32), exp[idx.numpy()].view(np.uint32), err_msg=f'batch entry {b}')


@pytest.mark.parametrize('K,N', [(32, 128), (256, 256)])
@pytest.mark.parametrize('batch', [36, 3])
def test_gemm_batched(hip, batch, K, N):
    """the batch folded into the tile sequence: at the smallest eligible M plus 17 the last tile of every entry is partial
    and the blocks' strided runs start and end inside entries (36 entries of 57 or 58 tiles; 3 entries of 683 or 684)"""
    _gemm_case(hip, batch, min_rows(N, batch) + 17, K, N, 523)


@pytest.mark.parametrize('keep', [False, True])
@pytest.mark.parametrize('Cin', [32, 256])
@pytest.mark.parametrize('Cout', [128, 256])
@pytest.mark.parametrize('proj_n', [1, 2])
def test_proj(hip, proj_n, Cout, Cin, keep):
    from oracle import dense as OD
    M, P = min_rows(Cout) + 17, 1031
    slab = hip.conv_k_slab(M, Cout)
    assert slab == 16
    g = torch.Generator().manual_seed(proj_n + Cout + Cin)
    base = torch.randn(P, Cin, generator=g)
    w = torch.randn(Cout, 1, 1, Cin, generator=g) * (1.0 / Cin ** 0.5)
    sc, sh = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g)
    pw = torch.randn(proj_n, Cout, generator=g) * (1.0 / Cout ** 0.5)
    idx = torch.arange(M) % P
    x = base.cuda()[idx.cuda()].view(1, 1, M, Cin).permute(0, 3, 1, 2)
    res = hip.conv_bn_act_proj_nhwc(x, w.cuda(), sc.cuda(), sh.cuda(), True, pw.cuda(), keep=keep)
    torch.cuda.synchronize()
    acc, act = res if keep else (res, None)
    exp = OD.conv_bn_act_proj_nhwc(base[None, None].numpy(), w.numpy(), sc.numpy(), sh.numpy(), True, pw.numpy(),
                                   slab=slab)[0, :, 0]                      # (n, P)
    np.testing.assert_array_equal(acc[0, :, 0].cpu().numpy().view(np.uint32), exp[:, idx.numpy()].view(np.uint32))
    if keep:
        expa = OD.conv_bn_act_nhwc(base[None, None].numpy(), w.numpy(), sc.numpy(), sh.numpy(), None, True, 1, 0, 1,
                                   slab=slab)[0, 0]
        gota = act.permute(0, 2, 3, 1).reshape(M, Cout).cpu().numpy()
        np.testing.assert_array_equal(gota.view(np.uint32), expa[idx.numpy()].view(np.uint32))


BIG = 1 << 21              # rows at which every eligible geometry is eligible


@pytest.mark.parametrize('name', ['3x3', 'stride2', 'residual', 'cout64'])
def test_ineligible_geometries(hip, name):
    """the query answers 0 whatever the size, and the launch gives the one-tile-per-block kernel's result at its slab"""
    from oracle import dense as OD
    KH, stride, pad, Cout, has_res = {'3x3': (3, 1, 1, 128, False), 'stride2': (1, 2, 0, 128, False),
                                      'residual': (1, 1, 0, 128, True), 'cout64': (1, 1, 0, 64, False)}[name]
    Cin, N, H, W = 32, 2, 37, 41
    assert _eligible(hip, BIG, Cin, Cout, KH=KH, KW=KH, stride=stride, pad=pad, res=int(has_res)) == 0
    OH = (H + 2 * pad - KH) // stride + 1
    OW = (W + 2 * pad - KH) // stride + 1
    M = N * OH * OW
    assert _eligible(hip, M, Cin, Cout, KH=KH, KW=KH, stride=stride, pad=pad, res=int(has_res)) == 0
    slab = hip.conv_k_slab(M, Cout, 1, has_res, Cin, geom=(KH, KH, stride, pad), relu=True)
    g = torch.Generator().manual_seed(len(name))
    x = torch.randn(N, H, W, Cin, generator=g)
    w = torch.randn(Cout, KH, KH, Cin, generator=g) * (1.0 / (Cin * KH * KH) ** 0.5)
    sc, sh = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g)
    res = torch.randn(N, OH, OW, Cout, generator=g) if has_res else None
    before = hip.query('emp_conv_stream_launches')
    got = hip.conv_bn_act_nhwc(x.cuda().permute(0, 3, 1, 2), w.cuda(), sc.cuda(), sh.cuda(),
                               res.cuda().permute(0, 3, 1, 2) if has_res else None, True, stride, pad, 1)
    torch.cuda.synchronize()
    assert hip.query('emp_conv_stream_launches') == before
    exp = OD.conv_bn_act_nhwc(x.numpy(), w.numpy(), sc.numpy(), sh.numpy(), res.numpy() if has_res else None, True,
                              stride, pad, 1, slab=slab)
    np.testing.assert_array_equal(got.permute(0, 2, 3, 1).cpu().numpy().view(np.uint32), exp.view(np.uint32))
