"""GPU: the one-kernel Winograd F(4x4,3x3) path (D5d, emp_wino4_conv_bn_act_nhwc) -- bit-exact against the oracle at
K-slab 16 and against the three-call path, and taken only where emp_wino4_fused_eligible says so."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# (N, H, W, C, dil) -> T: what the shape exercises
SHAPES = {
    'dil2': (1, 180, 190, 64, 2),        # 2 208 = 69 x 32: four sub-grids, patches and outputs crossing every border
    'dil2_partial': (1, 180, 194, 64, 2),  # 2 300 = 71 x 32 + 28: the last group is partial
    'two_images': (2, 130, 126, 64, 1),  # 2 112
    'c128': (1, 172, 172, 128, 1),       # 1 849 = 57 x 32 + 25: partial last group, both cout groups
}
TILES = {'dil2': 2208, 'dil2_partial': 2300, 'two_images': 2112, 'c128': 1849}


@pytest.fixture(scope='module')
def hip():
    from empanada_amd import _hip
    _hip.load()
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return _hip


_CASES = {}


def _case(hip, name, relu):
    """inputs, oracle result (slab 16) and torch's conv2d with its error bound; computed once per (shape, relu)"""
    key = (name, relu)
    if key not in _CASES:
        from oracle import dense as OD
        N, H, W, C, dil = SHAPES[name]
        g = torch.Generator().manual_seed(2 * C + dil + H + W)
        x = torch.randn(N, C, H, W, generator=g)
        w = torch.randn(C, C, 3, 3, generator=g) * (1.0 / (C * 9) ** 0.5)
        sc, sh = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
        tiles = hip.wino_tiles(N, H, W, dil, m=4)
        assert len(tiles) == TILES[name]
        assert hip.conv_k_slab(len(tiles), C, 36) == 16
        exp = OD.wino4_conv_bn_act(x.permute(0, 2, 3, 1).numpy(), w.numpy(), tiles, dil, sc.numpy(), sh.numpy(), relu,
                                   slab=16)
        ref = torch.nn.functional.conv2d(x, w, None, padding=dil, dilation=dil) * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)
        if relu:
            ref = torch.relu(ref)
        bound = torch.nn.functional.conv2d(x.abs(), w.abs(), None, padding=dil, dilation=dil) * sc.view(1, -1, 1, 1)
        _CASES[key] = dict(x=x.cuda().contiguous(memory_format=torch.channels_last), U=hip.wino4_filter_transform(w).cuda(),
                           tiles=torch.from_numpy(tiles).cuda(), sc=sc.cuda(), sh=sh.cuda(), dil=dil, exp=exp, ref=ref,
                           bound=bound)
    return _CASES[key]


def _check(got, c):
    np.testing.assert_array_equal(got.permute(0, 2, 3, 1).cpu().numpy().view(np.uint32), c['exp'].view(np.uint32))
    assert torch.all((got.cpu() - c['ref']).abs() <= 2e-5 * c['bound'] + 1e-6)


@pytest.mark.parametrize('name', ['dil2', 'dil2_partial', 'two_images', 'c128'])
def test_fused_bit_exact(hip, name):
    """fused=True against oracle/dense.py::wino4_conv_bn_act(slab=16), bit for bit, and within 2e-5 * sum|x||w| + 1e-6
    of torch's conv2d + affine + relu"""
    c = _case(hip, name, True)
    got = hip.wino4_conv_bn_act(c['x'], c['U'], c['tiles'], c['dil'], c['sc'], c['sh'], True, fused=True)
    _check(got, c)
    three = hip.wino4_conv_bn_act(c['x'], c['U'], c['tiles'], c['dil'], c['sc'], c['sh'], True, fused=False)
    assert torch.equal(got.view(torch.int32), three.view(torch.int32))


def test_fused_without_relu(hip):
    c = _case(hip, 'dil2_partial', False)
    got = hip.wino4_conv_bn_act(c['x'], c['U'], c['tiles'], c['dil'], c['sc'], c['sh'], False, fused=True)
    assert (got < 0).any()
    _check(got, c)


def test_fused_into_channel_slice(hip):
    """output into channels [32, 96) of a 160-channel NHWC buffer: the neighbouring channels stay untouched"""
    c = _case(hip, 'two_images', True)
    N, H, W, C, _ = SHAPES['two_images']
    buf = torch.full((N, 160, H, W), -7.0, device='cuda').contiguous(memory_format=torch.channels_last)
    out = buf[:, 32:32 + C]
    got = hip.wino4_conv_bn_act(c['x'], c['U'], c['tiles'], c['dil'], c['sc'], c['sh'], True, out=out, fused=True)
    assert got.data_ptr() == out.data_ptr()
    _check(buf[:, 32:32 + C], c)
    assert torch.all(buf[:, :32] == -7.0) and torch.all(buf[:, 32 + C:] == -7.0)


def _t_min(hip):
    """smallest T at which 64 -> 64 is eligible (eligibility is monotone in T over this range)"""
    lo, hi = 1, 1 << 19
    assert hip.wino4_fused_eligible(hi, 64, 64) and not hip.wino4_fused_eligible(lo, 64, 64)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if hip.wino4_fused_eligible(mid, 64, 64):
            hi = mid
        else:
            lo = mid
    return hi


def test_dispatch_threshold(hip, monkeypatch):
    """fused=None takes the one kernel at and above T_min, the three calls below it; None and False give the same bits"""
    t_min = _t_min(hip)
    assert t_min > 1820                                # (below that the plan's K-slab is 32)
    names = []
    real = hip.call

    def spy(name, *a, **k):
        names.append(name)
        return real(name, *a, **k)

    monkeypatch.setattr(hip, 'call', spy)
    g = torch.Generator().manual_seed(11)
    w = torch.randn(64, 64, 3, 3, generator=g) * (1.0 / (64 * 9) ** 0.5)
    U = hip.wino4_filter_transform(w).cuda()
    sc, sh = (torch.rand(64, generator=g) + 0.5).cuda(), torch.randn(64, generator=g).cuda()
    three = ['emp_wino4_input_transform', 'emp_gemm_nt_batched', 'emp_wino4_output_transform']
    for rows, fused_expected in ((-(-t_min // 128), True), ((t_min - 1) // 128, False)):
        H, W = 4 * rows, 512
        tiles = hip.wino_tiles(1, H, W, 1, m=4)
        assert (len(tiles) >= t_min) == fused_expected
        x = torch.randn(1, 64, H, W, generator=g).cuda().contiguous(memory_format=torch.channels_last)
        td = torch.from_numpy(tiles).cuda()
        del names[:]
        a = hip.wino4_conv_bn_act(x, U, td, 1, sc, sh, True)
        assert names == (['emp_wino4_conv_bn_act_nhwc'] if fused_expected else three)
        del names[:]
        b = hip.wino4_conv_bn_act(x, U, td, 1, sc, sh, True, fused=False)
        assert names == three
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        # without scale and shift the three calls are taken at any size
        del names[:]
        hip.wino4_conv_bn_act(x, U, td, 1, None, None, True)
        assert names == three


def test_never_eligible(hip):
    big = 1 << 17
    assert hip.wino4_fused_eligible(big, 64, 64)
    # (128 -> 128 runs with fused=True but is not in the enabled set: profiles/wino4_fused.md)
    for cin, cout in ((128, 128), (64, 128), (128, 64), (256, 256), (32, 64), (64, 256)):
        assert not hip.wino4_fused_eligible(big, cin, cout)
    assert not hip.wino4_fused_eligible(big, 64, 64, has_scale_shift=False)
    # the cases of test_winograd4_conv: a plan with K-slab 32, or widths outside the enabled set -- none is eligible
    for N, H, W, cin, cout, dil in [(2, 9, 11, 64, 128, 1), (1, 12, 10, 32, 40, 2), (2, 13, 8, 64, 132, 6), (1, 5, 7, 96, 64, 4),
                                    (2, 16, 16, 32, 256, 2), (8, 64, 64, 32, 64, 1)]:
        T = len(hip.wino_tiles(N, H, W, dil, m=4))
        assert hip.conv_k_slab(T, cout, 36) == 32 or (cin, cout) not in ((64, 64), (128, 128))
        assert not hip.wino4_fused_eligible(T, cin, cout)
    # enabled widths with a K-slab 32 plan: not eligible, and fused=True refuses
    N, H, W = 4, 64, 64
    tiles = hip.wino_tiles(N, H, W, 1, m=4)
    assert hip.conv_k_slab(len(tiles), 64, 36) == 32 and not hip.wino4_fused_eligible(len(tiles), 64, 64)
    tiles = torch.from_numpy(tiles).cuda()
    x = torch.zeros(N, 64, H, W, device='cuda').contiguous(memory_format=torch.channels_last)
    U = torch.zeros(36, 64, 64, device='cuda')
    one = torch.ones(64, device='cuda')
    with pytest.raises(hip.HipError):
        hip.wino4_conv_bn_act(x, U, tiles, 1, one, one, True, fused=True)
