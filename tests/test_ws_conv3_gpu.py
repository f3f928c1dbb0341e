"""Kind 3 of the weight-stationary kernel (emp_conv1x1.hip): 1x1, Cin 256, whole 128-cout groups, WITH a residual --
layer3's conv3 + identity -- behind emp_conv_bn_act_nhwc.  It sums in the order of the tiled kernel's residual-prefetch
plan (K-slab 32), so two references must hold bit for bit:
  * the tiled kernel itself: rows are independent, and the same entry on the first and on the last (threshold - 1) rows
    is below the kernel's threshold, so it runs the tiled kernel; every row of the kind-3 call lies in one of the two;
  * oracle/dense.py::conv_bn_act_nhwc on 64 sampled rows, at the slab emp_conv_k_slab_geom reports.
Values are spread over six decades, so that another summation order changes bits."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MIN_ROWS = 65536           # PW_MIN_ROWS of emp_conv1x1.hip
CIN = 256


def _min_rows(Cout):
    """kind 3 wants sixteen 32-row tiles per wave: rows x cout groups >= 8 x 65 536"""
    return max(MIN_ROWS, 8 * MIN_ROWS // (Cout // 128))


@pytest.fixture(scope='module')
def hip():
    from empanada_amd import _hip
    _hip.load()
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return _hip


def _kind(hip, M, Cin, Cout, relu, has_res):
    return hip.query('emp_conv1x1_ws_kind_for', M, Cin, Cout, 1, 1, 1, 0, relu, int(has_res))


def _spread(shape, g):
    """normal values times 10^u, u uniform in [-3, 3)"""
    return torch.randn(shape, generator=g, device='cuda') * torch.pow(10.0, 6.0 * torch.rand(shape, generator=g, device='cuda') - 3.0)


def _rows(t2d):
    """(M, ld) row-major matrix, or a column slice of one -> the (1, cols, 1, M) channels_last view the wrapper takes"""
    return t2d[None, None].permute(0, 3, 1, 2)


@pytest.mark.parametrize('sliced', [False, True])
@pytest.mark.parametrize('relu', [True, False])
@pytest.mark.parametrize('Cout', [128, 1024])
@pytest.mark.parametrize('extra', [0, 37])
def test_kind3_matches_tiled_kernel_and_oracle(hip, extra, Cout, relu, sliced):
    """extra 0: exactly the threshold (65 536 rows for eight cout groups, 524 288 for one), full 32-row tiles only; 37:
    one more full tile and a 5-row partial one.  Cout 128 / 1024: one / eight cout groups.  sliced: out and residual
    are channel slices of wider NHWC buffers."""
    from oracle import dense as OD
    n = _min_rows(Cout) - 1                                # rows of a call that stays on the tiled kernel
    M = n + 1 + extra
    assert _kind(hip, M, CIN, Cout, int(relu), True) == 3
    assert _kind(hip, n, CIN, Cout, int(relu), True) == 0
    slab = hip.conv_k_slab(M, Cout, 1, True, CIN, geom=(1, 1, 1, 0), relu=relu)
    assert slab == 32 == hip.conv_k_slab(n, Cout, 1, True, CIN, geom=(1, 1, 1, 0), relu=relu)
    g = torch.Generator(device='cuda').manual_seed(M + Cout + 2 * int(relu) + int(sliced))
    x = _spread((M, CIN), g)
    w = _spread((Cout, 1, 1, CIN), g) * (1.0 / CIN ** 0.5)
    sc = torch.rand(Cout, generator=g, device='cuda') + 0.5
    sh = torch.randn(Cout, generator=g, device='cuda')
    pad = 96 if sliced else 0                              # pixel stride Cout + 96, the slice starts at channel 32
    lo = 32 if sliced else 0
    rbuf = _spread((M, Cout + pad), g)
    obuf = torch.full((M, Cout + pad), -7.0, device='cuda')
    res, out = rbuf[:, lo:lo + Cout], obuf[:, lo:lo + Cout]
    before = hip.query('emp_conv1x1_ws_launches', 3)
    hip.conv_bn_act_nhwc(_rows(x), w, sc, sh, _rows(res), relu, 1, 0, 1, out=_rows(out))
    assert hip.query('emp_conv1x1_ws_launches', 3) == before + 1, 'the call did not run kind 3'
    if sliced:
        assert torch.all(obuf[:, :lo] == -7.0) and torch.all(obuf[:, lo + Cout:] == -7.0)
    if not relu:
        assert (out < 0).any()
    # the tiled kernel on the first and on the last n rows
    for a in (0, M - n):
        ref = torch.full((n, Cout), float('nan'), device='cuda')
        hip.conv_bn_act_nhwc(_rows(x[a:a + n]), w, sc, sh, _rows(res[a:a + n]), relu, 1, 0, 1, out=_rows(ref))
        assert torch.equal(out[a:a + n].contiguous().view(torch.int32), ref.view(torch.int32)), f'rows from {a}'
    assert hip.query('emp_conv1x1_ws_launches', 3) == before + 1, 'a reference call ran kind 3'
    # the oracle on 64 sampled rows: the first and the last eight (the partial tile, where there is one), 48 spread between
    idx = np.unique(np.concatenate([np.arange(0, 8), np.arange(M - 8, M), np.linspace(8, M - 9, 48).astype(np.int64)]))
    ti = torch.from_numpy(idx).cuda()
    exp = OD.conv_bn_act_nhwc(x[ti].cpu().numpy()[None, None], w.cpu().numpy(), sc.cpu().numpy(), sh.cpu().numpy(),
                              res[ti].cpu().numpy()[None, None], relu, 1, 0, 1, slab=slab)[0, 0]
    got = out[ti].cpu().numpy()
    np.testing.assert_array_equal(got.view(np.uint32), exp.view(np.uint32))


def test_kind3_eligibility(hip):
    assert _min_rows(1024) == MIN_ROWS and _min_rows(128) == 8 * MIN_ROWS
    for Cout in (128, 512, 1024):
        m = _min_rows(Cout)
        assert _kind(hip, m, CIN, Cout, 1, True) == 3
        assert _kind(hip, m - 1, CIN, Cout, 1, True) == 0                  # one row below the threshold
        assert _kind(hip, m, CIN, Cout, 2, True) == 0                      # the gate epilogue
    assert _kind(hip, MIN_ROWS, CIN, 1024, 1, False) == 0                  # no residual: the tiled kernel
    assert _kind(hip, 8 * MIN_ROWS, CIN, 1024, 0, False) == 0
    assert _kind(hip, 8 * MIN_ROWS, CIN, 128, 1, False) == 2               # (256 -> 128 without a residual stays kind 2)
    assert _kind(hip, 8 * MIN_ROWS, CIN, 1152, 1, True) == 0               # nine cout groups
    assert _kind(hip, 8 * MIN_ROWS, CIN, 192, 1, True) == 0                # not whole 128-cout groups
    assert _kind(hip, 8 * MIN_ROWS, 512, 1024, 1, True) == 0               # layer4's conv3
    assert _kind(hip, MIN_ROWS, 64, 256, 1, True) == 1                     # kind 1 keeps its shapes and its 64-slab order
    assert hip.conv_k_slab(MIN_ROWS, 256, 1, True, 64, geom=(1, 1, 1, 0), relu=True) == 64
    # the old query keeps answering for the call without a residual
    assert hip.query('emp_conv1x1_ws_eligible', MIN_ROWS, CIN, 1024, 1, 1, 1, 0, 1) == 0
