"""emp_upsample_bilinear_prob (D3 + D2 in one launch): bit-identical to emp_upsample_bilinear followed by
emp_logits_to_prob, writes nothing outside the view it is given, and refuses bad arguments before any launch."""
import ctypes

import pytest
import torch

# (h, w) -> (H, W): odd sizes; the vectorised store path (W % 4 == 0); W no multiple of 4 with a target that is not x4;
# a single source texel
SHAPES = [((5, 7), (20, 28)), ((8, 8), (32, 32)), ((9, 4), (33, 14)), ((1, 1), (4, 4))]


def _logits(N, C, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    x = 4 * torch.randn((N, C, h, w), generator=g)
    flat = x.view(-1)
    k = min(flat.numel(), 6)                                   # both ends of the sigmoid and of the softmax
    flat[:k] = torch.tensor([80., -80., 80., -80., 0., 80.])[:k]
    return x


@pytest.mark.gpu
@pytest.mark.parametrize('C', [1, 3])
@pytest.mark.parametrize('src,dst', SHAPES)
def test_bit_exact_against_the_two_kernels(src, dst, C):
    from empanada_amd import _hip
    x = _logits(3, C, *src, seed=7 * C + src[0]).cuda()
    up = _hip.upsample_bilinear(x, dst)
    got0 = _hip.upsample_bilinear_prob(x, dst, prob=False)
    assert got0.shape == (3, C) + dst and torch.equal(got0, up)
    exp = _hip.logits_to_prob(up)
    got1 = _hip.upsample_bilinear_prob(x, dst, prob=True)
    assert torch.equal(got1, exp)
    assert float(got1.min()) >= 0 and float(got1.max()) <= 1 and torch.isfinite(got1).all()
    if C > 1:                                                  # channels-last source, as a head's last layer may leave it
        xc = x.contiguous(memory_format=torch.channels_last)
        assert torch.equal(_hip.upsample_bilinear_prob(xc, dst, prob=True), exp)


@pytest.mark.gpu
def test_more_channels_than_the_register_form_holds():
    from empanada_amd import _hip
    x = _logits(2, 11, 5, 7, seed=3).cuda()
    exp = _hip.logits_to_prob(_hip.upsample_bilinear(x, (20, 28)))
    assert torch.equal(_hip.upsample_bilinear_prob(x, (20, 28), prob=True), exp)


@pytest.mark.gpu
@pytest.mark.parametrize('C', [1, 3])
@pytest.mark.parametrize('src,dst', SHAPES)
@pytest.mark.parametrize('prob', [False, True])
def test_writes_only_the_slices_it_is_given(src, dst, C, prob):
    from empanada_amd import _hip
    x = _logits(3, C, *src, seed=11).cuda()
    buf = torch.full((7, C) + dst, -7.5, device='cuda')
    _hip.upsample_bilinear_prob(x, dst, out=buf[2:5], prob=prob)
    exp = _hip.upsample_bilinear(x, dst)
    if prob:
        exp = _hip.logits_to_prob(exp)
    assert torch.equal(buf[2:5], exp)
    assert bool((buf[:2] == -7.5).all()) and bool((buf[5:] == -7.5).all())


def test_upsample_prob_argument_validation_without_gpu():
    """error paths return before any launch, so they run on a builder without a GPU"""
    from empanada_amd import _hip
    lib = _hip.load()
    st = (ctypes.c_int64 * 4)(64, 64, 8, 1)
    p = ctypes.c_void_p(4096)                                  # never dereferenced: every call below fails its checks
    f = lib.emp_upsample_bilinear_prob
    assert f(None, 1, 1, 8, 8, st, p, 32, 32, st, 1, None) == -1
    assert b'null' in lib.emp_last_error()
    assert f(p, 1, 1, 8, 8, st, None, 32, 32, st, 1, None) == -1
    assert f(p, 1, 1, 8, 8, None, p, 32, 32, st, 1, None) == -1
    assert f(p, 1, 1, 8, 8, st, p, 32, 32, None, 0, None) == -1
    assert b'null' in lib.emp_last_error()
    assert f(p, 1, 65, 8, 8, st, p, 32, 32, st, 1, None) == -1
    assert b'64' in lib.emp_last_error()
    for bad in ((1, 0, 8, 8, 32, 32), (1, 1, 0, 8, 32, 32), (1, 1, 8, -1, 32, 32), (1, 1, 8, 8, 0, 32),
                (1, 1, 8, 8, 32, 0), (-1, 1, 8, 8, 32, 32)):
        N, C, h, w, H, W = bad
        for prob in (0, 1):
            assert f(p, N, C, h, w, st, p, H, W, st, prob, None) == -1, bad
            assert b'shape' in lib.emp_last_error()
    assert f(p, 1, 1, 8, 8, st, p, 32, 32, st, 2, None) == -1
