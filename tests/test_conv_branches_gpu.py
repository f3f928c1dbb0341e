"""The variants of the tiled fp32 convolution (conv_igemm_f32_kernel behind emp_conv_bn_act_nhwc) that only larger
launches reach: 128-wide cout tiles with a tap gather, the 16-channel K-slab across tap changes, wide tiles with and
without the residual prefetch, the scalar epilogue on unaligned slices, rectangular / even / 7x7 filters.  The table of
launches and the plan each must resolve to is tests/conv_plan_ref.py::CONV_CASES; the shape alone chooses the variant
(no EMP_CONV_* variable is set), and each test first asserts, through the mirror of cg_plan and the library's own
queries, that it does.

Every launch is compared bit for bit with oracle/dense.py at the expected K-slab, with itself on a second call, and
with an fp64 conv2d + affine + residual + ReLU on the CPU within the bound of test_conv_bn_act_nhwc,
|err| <= 2e-6 * sum|x||w| * |scale| + 1e-6.  Inputs are randn everywhere: a tap fetched from a wrong pixel instead of
the zero page changes the sum."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_plan_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

FILL = -7.0
NAMES = sorted(ref.CONV_CASES)


@pytest.fixture(scope='module')
def hip():
    from empanada_amd import _hip
    _hip.load()
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return _hip


def _inputs(name, bn):
    """x (N,H,W,Cin), w (Cout,KH,KW,Cin), scale, shift, residual (N,OH,OW,Cout) or None, and for an 'odd' residual the
    (N,OH,OW,Cout+3) buffer it is channels [1, 1 + Cout) of -- CPU tensors, the same on every call"""
    c = ref.CONV_CASES[name]
    OH, OW = ref.out_size(c)
    g = torch.Generator().manual_seed(1000 + NAMES.index(name))
    x = torch.randn(c.N, c.H, c.W, c.Cin, generator=g)
    w = torch.randn(c.Cout, c.KH, c.KW, c.Cin, generator=g) * (1.0 / (c.Cin * c.KH * c.KW) ** 0.5)
    sc = torch.rand(c.Cout, generator=g) + 0.5 if bn else None
    sh = torch.randn(c.Cout, generator=g) if bn else None
    res = wide = None
    if c.res == 'plain':
        res = torch.randn(c.N, OH, OW, c.Cout, generator=g)
    elif c.res == 'odd':
        wide = torch.randn(c.N, OH, OW, c.Cout + 3, generator=g)
        res = wide[..., 1:1 + c.Cout]
    return x, w, sc, sh, res, wide


def _device_operands(name, bn):
    c = ref.CONV_CASES[name]
    x, w, sc, sh, res, wide = _inputs(name, bn)
    xd = x.cuda().permute(0, 3, 1, 2)
    resd = None
    if c.res == 'plain':
        resd = res.cuda().permute(0, 3, 1, 2)
    elif c.res == 'odd':
        resd = wide.cuda()[..., 1:1 + c.Cout].permute(0, 3, 1, 2)
        assert resd.data_ptr() % 16 != 0 and resd.stride(3) % 4 != 0
    return xd, w.cuda(), sc.cuda() if bn else None, sh.cuda() if bn else None, resd


def _ws_launches(hip):
    return sum(hip.query('emp_conv1x1_ws_launches', kind) for kind in (1, 2, 3))


def _bits(t_nchw):
    return t_nchw.permute(0, 2, 3, 1).contiguous().cpu().numpy().view(np.uint32)


@pytest.mark.parametrize('name,bn', [(n, True) for n in NAMES] + [('A', False)],
                         ids=NAMES + ['A-no-affine-no-relu'])
def test_conv_branch(hip, name, bn):
    """bn: BatchNorm scale / shift and ReLU; the one case without runs the identity epilogue (negative outputs kept)"""
    from oracle import dense as OD
    c = ref.CONV_CASES[name]
    OH, OW = ref.out_size(c)
    M = c.N * OH * OW
    relu = int(bn)
    has_res = c.res is not None
    # the plan, before anything is launched
    p = ref.conv_plan(M, c.Cout, c.Cin, 1, c.res == 'plain')
    assert (p.narrow, p.respf, p.slab) == (c.narrow, c.respf, c.slab)
    q = ref.conv_plan(M, c.Cout, c.Cin, 1, has_res)
    assert hip.conv_k_slab(M, c.Cout, 1, has_res, c.Cin) == q.slab
    assert hip.conv_k_slab(M, c.Cout, 1, has_res, c.Cin, geom=(c.KH, c.KW, c.stride, c.pad), relu=bool(relu)) == q.slab
    if c.res == 'odd':      # the queries take has_residual as "a residual the kernel can prefetch"; this one is not
        assert (q.slab, c.slab) == (32, 16)
    else:
        assert q.slab == c.slab
    assert hip.query('emp_conv_stream_eligible', 1, M, c.Cin, c.Cout, c.KH, c.KW, c.stride, c.pad, relu, int(has_res), 0) == 0
    assert hip.query('emp_conv1x1_ws_kind_for', M, c.Cin, c.Cout, c.KH, c.KW, c.stride, c.pad, relu, int(has_res)) == 0

    x, w, sc, sh, res, _ = _inputs(name, bn)
    xd, wd, scd, shd, resd = _device_operands(name, bn)
    streams, ws = hip.query('emp_conv_stream_launches'), _ws_launches(hip)
    got = hip.conv_bn_act_nhwc(xd, wd, scd, shd, resd, bool(relu), c.stride, c.pad, c.dil)
    again = hip.conv_bn_act_nhwc(xd, wd, scd, shd, resd, bool(relu), c.stride, c.pad, c.dil)
    torch.cuda.synchronize()
    assert hip.query('emp_conv_stream_launches') == streams and _ws_launches(hip) == ws
    got_bits = _bits(got)

    exp = OD.conv_bn_act_nhwc(x.numpy(), w.numpy(), sc.numpy() if bn else None, sh.numpy() if bn else None,
                              res.numpy() if has_res else None, bool(relu), c.stride, c.pad, c.dil, slab=c.slab)
    if not relu:
        assert (exp < 0).any()
    np.testing.assert_array_equal(got_bits, exp.view(np.uint32))
    np.testing.assert_array_equal(_bits(again), got_bits)
    if c.res == 'odd':      # an oracle fed from the query with has_residual = 1 would sum in another order
        other = OD.conv_bn_act_nhwc(x.numpy(), w.numpy(), sc.numpy(), sh.numpy(), res.numpy(), True, c.stride, c.pad,
                                    c.dil, slab=q.slab)
        assert (other.view(np.uint32) != got_bits).any()

    # fp64 on the CPU
    x64, w64 = x.permute(0, 3, 1, 2).double(), w.permute(0, 3, 1, 2).double()
    kw = dict(stride=c.stride, padding=c.pad, dilation=c.dil)
    y = torch.nn.functional.conv2d(x64, w64, None, **kw)
    bound = torch.nn.functional.conv2d(x64.abs(), w64.abs(), None, **kw)
    if bn:
        y = y * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1)
        bound = bound * sc.double().abs().view(1, -1, 1, 1)
    if has_res:
        y = y + res.permute(0, 3, 1, 2).double()
    if relu:
        y = torch.relu(y)
    bound = 2e-6 * bound + 1e-6
    err = (got.cpu().double() - y).abs()
    print(f"conv case {name}{'' if bn else ' (no affine, no ReLU)'}: max err / bound vs fp64 = {float((err / bound).max()):.4f}")
    assert torch.all(err <= bound)


@pytest.mark.parametrize('lo,extra', [(8, 16), (3, 5)], ids=['aligned', 'unaligned'])
@pytest.mark.parametrize('name', ['B', 'E', 'L'])
def test_conv_branch_out_slice(hip, name, lo, extra):
    """the output is channels [lo, lo + Cout) of a Cout + extra wide NHWC buffer: (8, 16) keeps the float4 stores, (3, 5)
    -- a base that is not 16-byte aligned and a pixel stride that is no multiple of 4 -- takes the scalar ones; the same
    bits as the plain call (which test_conv_branch holds to the oracle), and the channels on both sides keep their fill"""
    c = ref.CONV_CASES[name]
    OH, OW = ref.out_size(c)
    xd, wd, scd, shd, resd = _device_operands(name, True)
    plain = hip.conv_bn_act_nhwc(xd, wd, scd, shd, resd, True, c.stride, c.pad, c.dil)
    buf = torch.full((c.N, OH, OW, c.Cout + extra), FILL, device='cuda')
    out = buf[..., lo:lo + c.Cout].permute(0, 3, 1, 2)
    assert (out.data_ptr() % 16 == 0 and out.stride(3) % 4 == 0) == (lo == 8)
    streams, ws = hip.query('emp_conv_stream_launches'), _ws_launches(hip)
    hip.conv_bn_act_nhwc(xd, wd, scd, shd, resd, True, c.stride, c.pad, c.dil, out=out)
    torch.cuda.synchronize()
    assert hip.query('emp_conv_stream_launches') == streams and _ws_launches(hip) == ws
    np.testing.assert_array_equal(_bits(out), _bits(plain))
    assert torch.all(buf[..., :lo] == FILL) and torch.all(buf[..., lo + c.Cout:] == FILL)
