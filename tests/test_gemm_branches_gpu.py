"""emp_gemm_nt_batched called directly at the plans the Winograd paths reach only at sizes their own tests do not have
-- 128-wide tiles at K-slab 32 and 16 with 16 / 25 / 36 entries, couts masked in the last tile, three cout tiles, the
narrow plan at slab 16 -- and at launches nothing else makes: N no multiple of 4 (the scalar epilogue for every column)
and a C that is not 16-byte aligned (which must keep the launch off the weight-stationary and persistent kernels).  The
launches and their routes are tests/conv_plan_ref.py::GEMM_CASES; each test asserts the route, through the mirror and the
library's queries, before it launches.  Last, the 128-wide instantiation of emp_conv_splitk_bn_act_nhwc's first pass.

A GEMM row is a function of its A row alone, so A repeats a block of P distinct rows (P prime, no multiple of any tile):
oracle/dense.py::conv_bn_act_nhwc runs on the P rows of every entry once, at the expected K-slab, and EVERY output row of
the launch is compared with its row of that result bit for bit; the P rows are also held to an fp64 product within the
tiled convolution's stated bound, |err| <= 2e-6 * sum|a||b| + 1e-6."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_plan_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

FILL = -7.0


@pytest.fixture(scope='module')
def hip():
    from empanada_amd import _hip
    _hip.load()
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return _hip


def _operands(batch, M, K, N):
    """A (batch, M, K) on the device, its P distinct rows per entry and B (batch, N, K) on the CPU, the row map"""
    P = 523 if M >= 2 * 523 else 131
    g = torch.Generator().manual_seed(1000 * K + N + batch)
    base = torch.randn(batch, P, K, generator=g)
    B = torch.randn(batch, N, K, generator=g) * (1.0 / K ** 0.5)
    idx = torch.arange(M) % P
    A = base.cuda()[:, idx.cuda()].contiguous()
    return A, base, B, idx.numpy()


def _check(got, base, B, idx, slab, what):
    """got (batch, M, N) numpy: every row against the oracle's row, the distinct rows against fp64"""
    from oracle import dense as OD
    worst = 0.0
    for b in range(got.shape[0]):
        exp = OD.conv_bn_act_nhwc(base[b][None, None].numpy(), B[b][:, None, None, :].numpy(), slab=slab)[0, 0]
        np.testing.assert_array_equal(got[b].view(np.uint32), exp[idx].view(np.uint32), err_msg=f'batch entry {b}')
        y = base[b].double() @ B[b].double().T
        bound = 2e-6 * (base[b].double().abs() @ B[b].double().abs().T) + 1e-6
        rows = min(len(y), got.shape[1])
        err = (torch.from_numpy(got[b][:rows]).double() - y[:rows]).abs()
        assert torch.all(err <= bound[:rows]), f'batch entry {b}'
        worst = max(worst, float((err / bound[:rows]).max()))
    print(f"gemm {what}: max err / bound vs fp64 = {worst:.4f}")


@pytest.mark.parametrize('case', list(ref.GEMM_CASES), ids=lambda c: 'x'.join(map(str, c)))
def test_gemm_branch(hip, case):
    batch, M, K, N = case
    r = ref.gemm_route(batch, M, K, N)
    assert (r.route, r.narrow, r.slab) == ref.GEMM_CASES[case] and r.route == 'tiled'
    assert hip.conv_k_slab(M, N, batch) == r.slab
    assert hip.query('emp_conv_stream_eligible', batch, M, K, N, 1, 1, 1, 0, 0, 0, 0) == 0
    assert batch * M < ref.WS_MIN_ROWS or K not in (64, 128) or N not in (64, 128)
    A, base, B, idx = _operands(batch, M, K, N)
    Bd = B.cuda()
    C = torch.full((batch, M, N), float('nan'), device='cuda')
    C2 = torch.full((batch, M, N), float('nan'), device='cuda')
    assert C.data_ptr() % 16 == 0
    streams = hip.query('emp_conv_stream_launches')
    hip.call('emp_gemm_nt_batched', A.data_ptr(), Bd.data_ptr(), batch, M, N, K, C.data_ptr(), hip.stream())
    hip.call('emp_gemm_nt_batched', A.data_ptr(), Bd.data_ptr(), batch, M, N, K, C2.data_ptr(), hip.stream())
    torch.cuda.synchronize()
    assert hip.query('emp_conv_stream_launches') == streams
    got = C.cpu().numpy()
    assert not np.isnan(got).any()                           # every element written, whichever epilogue stored it
    _check(got, base, B, idx, r.slab, f"{case} {'narrow' if r.narrow else 'wide'}-{r.slab}")
    np.testing.assert_array_equal(C2.cpu().numpy().view(np.uint32), got.view(np.uint32))


def test_gemm_unaligned_c_stays_tiled(hip):
    """a launch the persistent kernel would take (36 entries, 2 052 tiles of 128 couts, slab 16), but with C one float
    past a 16-byte boundary: neither float4-storing kernel may run; the tiled kernel's scalar epilogue gives the same sum,
    and the floats before and after the matrix keep their fill"""
    batch, K, N = 36, 32, 128
    tiles_m = -(-ref.STREAM_MIN_TILES // (batch * (N // 128)))
    M = (tiles_m - 1) * 128 + 1 + 17                        # the smallest eligible M, plus 17
    r = ref.gemm_route(batch, M, K, N)
    assert (r.route, r.narrow, r.slab) == ('stream', False, 16) and r.blocks == 2052
    assert ref.gemm_route(batch, M - 18, K, N).route == 'tiled'
    assert hip.query('emp_conv_stream_eligible', batch, M, K, N, 1, 1, 1, 0, 0, 0, 0) == 1
    assert hip.conv_k_slab(M, N, batch) == 16
    A, base, B, idx = _operands(batch, M, K, N)
    Bd = B.cuda()
    n = batch * M * N
    store = torch.full((n + 8,), FILL, device='cuda')
    C = store[1:1 + n]
    assert store.data_ptr() % 16 == 0 and C.data_ptr() % 16 == 4
    streams = hip.query('emp_conv_stream_launches')
    hip.call('emp_gemm_nt_batched', A.data_ptr(), Bd.data_ptr(), batch, M, N, K, C.data_ptr(), hip.stream())
    torch.cuda.synchronize()
    assert hip.query('emp_conv_stream_launches') == streams
    assert float(store[0]) == FILL and bool(torch.all(store[1 + n:] == FILL))
    _check(C.view(batch, M, N).cpu().numpy(), base, B, idx, 16, f"{(batch, M, K, N)} unaligned C")
    # the aligned launch of the same operands is the persistent kernel's: the same bits
    C2 = torch.full((batch, M, N), float('nan'), device='cuda')
    hip.call('emp_gemm_nt_batched', A.data_ptr(), Bd.data_ptr(), batch, M, N, K, C2.data_ptr(), hip.stream())
    torch.cuda.synchronize()
    assert hip.query('emp_conv_stream_launches') == streams + 1
    assert bool(torch.equal(C2.view(torch.int32).view(-1), C.contiguous().view(torch.int32)))


@pytest.mark.parametrize('use_res', [False, True], ids=['plain', 'residual'])
def test_splitk_wide(hip, use_res):
    """emp_conv_splitk_bn_act_nhwc with 256 wide blocks per range (64 x 64 pixels, 64 -> 1024, 1x1, two ranges of one slab
    each): the <2, 0, false, 32, false, true> instantiation, which emp_conv_splitk_plan never proposes but the entry
    point accepts.  Bit-exact against the oracle, the same bits on a second call, within the split-K test's fp64 bound
    |err| <= 2e-6 * sum|x||w| * |scale| + 1e-6."""
    from oracle import dense as OD
    N, H, W, Cin, Cout, ks = 1, 64, 64, 64, 1024, 2
    M = N * H * W
    p = ref.conv_plan(M, Cout, Cin)
    assert not p.narrow and p.tiles_m * p.tiles_n == 256 and ref.conv_plan(M - 128, Cout, Cin).narrow
    assert hip.conv_splitk_plan(M, Cout, Cin, 1, 1) == ref.splitk_plan(M, Cout, Cin, 1, 1) == 1
    g = torch.Generator().manual_seed(64 + 1024 + int(use_res))
    x = torch.randn(N, H, W, Cin, generator=g)
    w = torch.randn(Cout, 1, 1, Cin, generator=g) * (1.0 / Cin ** 0.5)
    sc, sh = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g)
    res = torch.randn(N, H, W, Cout, generator=g) if use_res else None
    xd = x.cuda().permute(0, 3, 1, 2)
    resd = res.cuda().permute(0, 3, 1, 2) if use_res else None
    args = (xd, w.cuda(), sc.cuda(), sh.cuda(), resd, True, 1, 0, 1)
    got = hip.conv_splitk_bn_act_nhwc(*args, k_splits=ks)
    again = hip.conv_splitk_bn_act_nhwc(*args, k_splits=ks)
    torch.cuda.synchronize()
    got_bits = got.permute(0, 2, 3, 1).contiguous().cpu().numpy().view(np.uint32)
    exp = OD.conv_splitk_bn_act_nhwc(x.numpy(), w.numpy(), sc.numpy(), sh.numpy(), res.numpy() if use_res else None, True,
                                     1, 0, 1, ks)
    np.testing.assert_array_equal(got_bits, exp.view(np.uint32))
    np.testing.assert_array_equal(again.permute(0, 2, 3, 1).contiguous().cpu().numpy().view(np.uint32), got_bits)
    x64, w64 = x.double().view(M, Cin), w.double().view(Cout, Cin)
    y = (x64 @ w64.T) * sc.double() + sh.double()
    if use_res:
        y = y + res.double().view(M, Cout)
    y = torch.relu(y)
    bound = 2e-6 * (x64.abs() @ w64.abs().T) * sc.double().abs() + 1e-6
    err = (got.permute(0, 2, 3, 1).reshape(M, Cout).cpu().double() - y).abs()
    print(f"split-K wide{' + residual' if use_res else ''}: max err / bound vs fp64 = {float((err / bound).max()):.4f}")
    assert torch.all(err <= bound)
