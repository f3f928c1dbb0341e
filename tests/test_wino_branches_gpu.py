"""The three Winograd convolutions (D5 F(2x2), D5c F(3x3), D5b F(4x4): emp_wino*_{input,output}_transform around
emp_wino_gemm_fused / emp_gemm_nt_batched) at the launches only larger or odder shapes reach: 128-wide tiles of the
position GEMMs at both K-slabs, couts masked in the last tile, more than two tile rows in the fused loader, dilation
beyond the image, images smaller than a tile, the output kernels' null scale / shift / ReLU arms, `out=` channel slices,
and the second trip of the six transform kernels' grid-stride loops.  The table of launches and the plan each must
resolve to is tests/conv_plan_ref.py::WINO_CASES; the shape alone chooses the plan, and each test first asserts, through
the mirror and the library's own queries, that it does -- and that neither the weight-stationary, the persistent nor the
one-kernel F(4x4) path takes the launch.

Four paths per case: 'f2' F(2x2) with the input transform in the GEMM's loader (always K-slab 32), 's2' F(2x2), 'w3'
F(3x3) and 'w4' F(4x4) in three calls (the K-slab of emp_conv_k_slab at 16 / 25 / 36 entries).  Every launch is compared
bit for bit with oracle/dense.py at that slab, with itself on a second call, and with an fp64 conv2d + affine + ReLU on
the CPU within the bounds the first Winograd tests state: |err| <= 1e-5 * sum|x||w| * |scale| + 1e-6 for F(2x2), 2e-5 *
... for F(3x3) and F(4x4).  Inputs are randn everywhere: a patch pixel fetched from a wrong place changes the sum."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_plan_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

FILL = -7.0
NAMES = sorted(ref.WINO_CASES)
# path -> (m, the fused= argument of the wrapper, coefficient of the fp64 bound)
PATHS = {'f2': (2, True, 1e-5), 's2': (2, False, 1e-5), 'w3': (3, None, 2e-5), 'w4': (4, False, 2e-5)}
# epilogue variants: (scale, shift, relu)
VARIANTS = {'bn-relu': (True, True, True), 'none': (False, False, False), 'scale': (True, False, False),
            'shift': (False, True, False)}
# (case, path) whose launch the oracle at the OTHER slab must not reproduce: one per slab of the batched GEMM, and the
# fused loader at a size for which emp_conv_k_slab would say 16
SLAB_SENSITIVE = {('P', 's2'): 16, ('P', 'w3'): 32, ('P', 'f2'): 32}
GRID_CAP = 16384 * 256     # work items (tile, 4 channels) of one trip of a transform kernel's grid-stride loop
CHUNK = 32768              # tiles per launch of the chunked comparison: 32 768 x 64 items, half the cap


@pytest.fixture(scope='module')
def hip():
    from empanada_amd import _hip
    _hip.load()
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return _hip


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """x (N,H,W,Cin), w (Cout,Cin,3,3), scale, shift -- CPU tensors, the same on every call"""
    c = ref.WINO_CASES[name]
    g = torch.Generator().manual_seed(2000 + NAMES.index(name))
    x = torch.randn(c.N, c.H, c.W, c.Cin, generator=g)
    w = torch.randn(c.Cout, c.Cin, 3, 3, generator=g) * (1.0 / (c.Cin * 9) ** 0.5)
    sc = torch.rand(c.Cout, generator=g) + 0.5
    sh = torch.randn(c.Cout, generator=g)
    return x, w, sc, sh


@functools.lru_cache(maxsize=None)
def _fp64(name):
    """conv2d(x, w) and conv2d(|x|, |w|) in float64 on the CPU, (N,H,W,Cout): computed once per case, never written to"""
    c = ref.WINO_CASES[name]
    x, w, _, _ = _inputs(name)
    x64, w64 = x.permute(0, 3, 1, 2).double(), w.double()
    y = torch.nn.functional.conv2d(x64, w64, None, padding=c.dil, dilation=c.dil).permute(0, 2, 3, 1).contiguous()
    a = torch.nn.functional.conv2d(x64.abs(), w64.abs(), None, padding=c.dil, dilation=c.dil).permute(0, 2, 3, 1).contiguous()
    return y, a


def _filter(hip, path, w):
    m = PATHS[path][0]
    return {2: hip.wino_filter_transform, 3: hip.wino3_filter_transform, 4: hip.wino4_filter_transform}[m](w)


def _launch(hip, path, xd, Ud, tiles_dev, dil, sc, sh, relu, out=None):
    m, fused, _ = PATHS[path]
    if m == 2:
        return hip.wino_conv_bn_act(xd, Ud, tiles_dev, dil, sc, sh, relu, out=out, fused=fused)
    if m == 3:
        return hip.wino3_conv_bn_act(xd, Ud, tiles_dev, dil, sc, sh, relu, out=out)
    return hip.wino4_conv_bn_act(xd, Ud, tiles_dev, dil, sc, sh, relu, out=out, fused=False)


def _oracle(path, name, tiles, sc, sh, relu, slab):
    from oracle import dense as OD
    c = ref.WINO_CASES[name]
    x, w, _, _ = _inputs(name)
    fn = {2: OD.wino_conv_bn_act, 3: OD.wino3_conv_bn_act, 4: OD.wino4_conv_bn_act}[PATHS[path][0]]
    return fn(x.numpy(), w.numpy(), tiles, c.dil, None if sc is None else sc.numpy(), None if sh is None else sh.numpy(),
              relu, slab=slab)


def _route(hip, name, path):
    """everything that must hold of the launch before it is made; returns the tile table and the slab of the oracle"""
    c = ref.WINO_CASES[name]
    m, fused, _ = PATHS[path]
    k = ref.WINO_M.index(m)
    batch = (m + 2) ** 2
    tiles = hip.wino_tiles(c.N, c.H, c.W, c.dil, m)
    T = len(tiles)
    assert T == c.T[k] == ref.wino_tile_count(c.N, c.H, c.W, c.dil, m)
    r = ref.gemm_route(batch, T, c.Cin, c.Cout)
    assert (r.route, r.narrow, r.slab) == ('tiled',) + c.plans[k]
    assert hip.conv_k_slab(T, c.Cout, batch) == r.slab
    assert hip.query('emp_conv_stream_eligible', batch, T, c.Cin, c.Cout, 1, 1, 1, 0, 0, 0, 0) == 0
    assert batch * T < ref.WS_MIN_ROWS                       # cannot go weight-stationary
    assert not hip.wino4_fused_eligible(T, c.Cin, c.Cout, True)
    if fused:
        assert ref.wino_route(c.Cout) == (c.fused_narrow, 32)
        assert c.N * c.H * c.W * c.Cin < 2 ** 31             # the wrapper keeps the fused loader
        return tiles, 32
    return tiles, r.slab


def _bits(t_nchw):
    return t_nchw.permute(0, 2, 3, 1).contiguous().cpu().numpy().view(np.uint32)


def _run_variant(hip, name, path, variant):
    c = ref.WINO_CASES[name]
    use_sc, use_sh, relu = VARIANTS[variant]
    tiles, slab = _route(hip, name, path)
    x, w, sc, sh = _inputs(name)
    sc, sh = (sc if use_sc else None), (sh if use_sh else None)
    xd = x.cuda().permute(0, 3, 1, 2)
    Ud, td = _filter(hip, path, w).cuda(), torch.from_numpy(tiles).cuda()
    scd, shd = (None if sc is None else sc.cuda()), (None if sh is None else sh.cuda())
    streams = hip.query('emp_conv_stream_launches')
    got = _launch(hip, path, xd, Ud, td, c.dil, scd, shd, relu)
    again = _launch(hip, path, xd, Ud, td, c.dil, scd, shd, relu)
    torch.cuda.synchronize()
    assert hip.query('emp_conv_stream_launches') == streams
    assert got.shape == (c.N, c.Cout, c.H, c.W)
    got_bits = _bits(got)

    exp = _oracle(path, name, tiles, sc, sh, relu, slab)
    if variant == 'none':
        assert (exp < 0).any()                               # what ReLU would have hidden is there to be compared
    np.testing.assert_array_equal(got_bits, exp.view(np.uint32))
    np.testing.assert_array_equal(_bits(again), got_bits)
    if variant == 'bn-relu' and (name, path) in SLAB_SENSITIVE:
        assert slab == SLAB_SENSITIVE[(name, path)]
        other = _oracle(path, name, tiles, sc, sh, relu, 48 - slab)
        assert (other.view(np.uint32) != got_bits).any()

    # fp64 on the CPU
    y, bound = _fp64(name)
    if use_sc:
        y, bound = y * sc.double(), bound * sc.double().abs()
    if use_sh:
        y = y + sh.double()
    if relu:
        y = torch.relu(y)
    bound = PATHS[path][2] * bound + 1e-6
    err = (got.permute(0, 2, 3, 1).cpu().double() - y).abs()
    print(f"wino case {name} path {path} epilogue {variant}: max err / bound vs fp64 = {float((err / bound).max()):.4f}")
    assert torch.all(err <= bound)


@pytest.mark.parametrize('path', list(PATHS))
@pytest.mark.parametrize('name', NAMES)
def test_wino_branch(hip, name, path):
    """scale + shift + ReLU on every case and path"""
    _run_variant(hip, name, path, 'bn-relu')


@pytest.mark.parametrize('variant', ['none', 'scale', 'shift'])
@pytest.mark.parametrize('path', list(PATHS))
@pytest.mark.parametrize('name', ['P', 'S', 'T1'])
def test_wino_epilogue(hip, name, path, variant):
    """the null-operand arms of the output transforms, none of them with ReLU: a wrong value that should be negative shows"""
    _run_variant(hip, name, path, variant)


@pytest.mark.parametrize('path', list(PATHS))
@pytest.mark.parametrize('name', ['P', 'R'])
def test_wino_out_slice(hip, name, path):
    """the output is channels [8, 8 + Cout) of a Cout + 24 wide NHWC buffer, as FusedConvBN.forward writes a concat slice:
    the same bits as the plain call (which test_wino_branch holds to the oracle), and the channels on both sides keep
    their fill"""
    c = ref.WINO_CASES[name]
    tiles, _ = _route(hip, name, path)
    x, w, sc, sh = _inputs(name)
    xd = x.cuda().permute(0, 3, 1, 2)
    Ud, td = _filter(hip, path, w).cuda(), torch.from_numpy(tiles).cuda()
    plain = _launch(hip, path, xd, Ud, td, c.dil, sc.cuda(), sh.cuda(), True)
    buf = torch.full((c.N, c.H, c.W, c.Cout + 24), FILL, device='cuda')
    out = buf[..., 8:8 + c.Cout].permute(0, 3, 1, 2)
    assert out.data_ptr() % 16 == 0 and out.stride(3) % 4 == 0 and out.stride(3) > c.Cout
    streams = hip.query('emp_conv_stream_launches')
    ret = _launch(hip, path, xd, Ud, td, c.dil, sc.cuda(), sh.cuda(), True, out=out)
    torch.cuda.synchronize()
    assert hip.query('emp_conv_stream_launches') == streams
    assert ret.data_ptr() == out.data_ptr()
    np.testing.assert_array_equal(_bits(out), _bits(plain))
    assert torch.all(buf[..., :8] == FILL) and torch.all(buf[..., 8 + c.Cout:] == FILL)


@pytest.mark.parametrize('lo,extra', [(3, 5), (2, 4), (4, 5)], ids=['base-and-stride', 'base', 'stride'])
@pytest.mark.parametrize('path', list(PATHS))
def test_wino_out_slice_rejected(hip, path, lo, extra):
    """the output transforms store float4: a slice whose base is not 16-byte aligned, or whose pixel stride is no multiple
    of 4, is refused by the entry point's argument check, before its launch -- nothing is written"""
    name = 'S'
    c = ref.WINO_CASES[name]
    tiles, _ = _route(hip, name, path)
    x, w, sc, sh = _inputs(name)
    xd = x.cuda().permute(0, 3, 1, 2)
    Ud, td = _filter(hip, path, w).cuda(), torch.from_numpy(tiles).cuda()
    buf = torch.full((c.N, c.H, c.W, c.Cout + extra), FILL, device='cuda')
    out = buf[..., lo:lo + c.Cout].permute(0, 3, 1, 2)
    assert (out.data_ptr() % 16 != 0) == (lo % 4 != 0) and (out.stride(3) % 4 != 0) == (extra % 4 != 0)
    with pytest.raises(hip.HipError, match='alignment|pixel stride'):
        _launch(hip, path, xd, Ud, td, c.dil, sc.cuda(), sh.cuda(), True, out=out)
    torch.cuda.synchronize()
    assert torch.all(buf == FILL)


# ---------------------------------------------------------------------------------------------------------------------
# the second trip of the transform kernels' grid-stride loops: more than 16 384 x 256 items of (tile, 4 channels)

GS_C = 256                 # channels: 64 items per tile, so the cap is crossed just past 65 536 tiles


def _chunks(T):
    return [(t0, min(t0 + CHUNK, T)) for t0 in range(0, T, CHUNK)]


@pytest.mark.parametrize('m', ref.WINO_M)
def test_input_transform_grid_stride(hip, m):
    """emp_wino{,3,4}_input_transform on a table of 65 536 + 517 tiles (the tiles of a small dilated two-image batch,
    repeated): V of the one launch equals, bit for bit, the V of launches of at most 32 768 tiles each -- those stay below
    the cap, on the single-trip path the small cases tie to the oracle.  Compared on the device."""
    entry = {2: 'emp_wino_input_transform', 3: 'emp_wino3_input_transform', 4: 'emp_wino4_input_transform'}[m]
    N, H, W, dil = 2, 37, 41, 2
    P = (m + 2) ** 2
    T = 65536 + 517
    base = hip.wino_tiles(N, H, W, dil, m)
    tiles = np.ascontiguousarray(np.tile(base, (-(-T // len(base)), 1))[:T])
    assert T * (GS_C // 4) > GRID_CAP and all((t1 - t0) * (GS_C // 4) <= GRID_CAP // 2 for t0, t1 in _chunks(T))
    g = torch.Generator(device='cuda').manual_seed(m)
    x = torch.randn(N, H, W, GS_C, device='cuda', generator=g)
    td = torch.from_numpy(tiles).cuda()
    V = torch.full((P, T, GS_C), float('nan'), device='cuda')
    hip.call(entry, x.data_ptr(), N, H, W, GS_C, dil, td.data_ptr(), T, V.data_ptr(), hip.stream())
    Vi = V.view(torch.int32)
    for t0, t1 in _chunks(T):
        tc = td[t0:t1].contiguous()
        Vc = torch.full((P, t1 - t0, GS_C), float('nan'), device='cuda')
        hip.call(entry, x.data_ptr(), N, H, W, GS_C, dil, tc.data_ptr(), t1 - t0, Vc.data_ptr(), hip.stream())
        assert bool(torch.equal(Vi[:, t0:t1], Vc.view(torch.int32))), f"tiles [{t0}, {t1})"
    assert not bool(torch.isnan(V).any())


@pytest.mark.parametrize('m', ref.WINO_M)
def test_output_transform_grid_stride(hip, m):
    """emp_wino{,3,4}_output_transform on the 66 048 distinct tiles of one 256 m x 258 m image, Mw drawn on the device,
    scale and shift but no ReLU: the image of the one launch equals, bit for bit, the image written by launches of at
    most 32 768 tiles each, and every pixel is written.  Compared on the device."""
    entry = {2: 'emp_wino_output_transform', 3: 'emp_wino3_output_transform', 4: 'emp_wino4_output_transform'}[m]
    N, H, W, dil = 1, 256 * m, 258 * m, 1
    P = (m + 2) ** 2
    tiles = hip.wino_tiles(N, H, W, dil, m)
    T = len(tiles)
    assert T == 66048 and len(np.unique(tiles, axis=0)) == T
    assert T * (GS_C // 4) > GRID_CAP and all((t1 - t0) * (GS_C // 4) <= GRID_CAP // 2 for t0, t1 in _chunks(T))
    assert P * T * GS_C * 4 < 2.5 * 2 ** 30
    g = torch.Generator(device='cuda').manual_seed(10 + m)
    Mw = torch.randn(P, T, GS_C, device='cuda', generator=g)
    sc = torch.rand(GS_C, device='cuda', generator=g) + 0.5
    sh = torch.randn(GS_C, device='cuda', generator=g)
    td = torch.from_numpy(tiles).cuda()
    whole = torch.full((N, H, W, GS_C), float('nan'), device='cuda')     # no finite fill: among 10^8 outputs any value occurs
    parts = torch.full((N, H, W, GS_C), float('nan'), device='cuda')
    hip.call(entry, Mw.data_ptr(), td.data_ptr(), T, N, H, W, GS_C, dil, sc.data_ptr(), sh.data_ptr(), 0,
             whole.data_ptr(), GS_C, hip.stream())
    for t0, t1 in _chunks(T):
        tc = td[t0:t1].contiguous()
        Mc = Mw[:, t0:t1].contiguous()
        hip.call(entry, Mc.data_ptr(), tc.data_ptr(), t1 - t0, N, H, W, GS_C, dil, sc.data_ptr(), sh.data_ptr(), 0,
                 parts.data_ptr(), GS_C, hip.stream())
    assert bool(torch.equal(whole.view(torch.int32), parts.view(torch.int32)))
    assert not bool(torch.isnan(whole).any())
