"""CPU: the down-sampling statement (empanada_amd.data.resize_by_factor: cv2.resize restated, parity with the library
unpinned), VolumeDataset(scale=N), and this package's PanopticDeepLabPR with three PointRend steps against the REFERENCE
model's heads of tests/golden/downsample.npz (tools/gen_golden_downsample.py)."""
import math

import numpy as np
import pytest
import torch

from conftest import load_golden
from downsample_ref import fixture_input, fixture_model, loop_resize

SHAPES = [(72, 88), (73, 88), (40, 87), (5, 3), (1, 7), (33, 65), (7, 7)]
FACTORS = [2, 4, 8]


def test_known_answers():
    from empanada_amd.data import resize_by_factor, resize_tables
    a = np.array([[0, 1], [2, 3]], dtype=np.uint8)
    np.testing.assert_array_equal(resize_by_factor(a, 2), [[2]])
    b = (20 * np.arange(12)).reshape(3, 4).astype(np.uint8)
    np.testing.assert_array_equal(resize_by_factor(b, 2), [[30, 70], [150, 190]])        # general path: 3 != 2 * 2
    assert resize_by_factor(b, 1) is b
    for (s, d), off, coef in (((3, 2), [0, 1], [[1536, 512], [512, 1536]]),
                              ((8, 2), [1, 5], [[1024, 1024], [1024, 1024]]),
                              ((7, 2), [1, 4], [[1536, 512], [512, 1536]])):
        o, c = resize_tables(s, d)
        assert o.dtype == np.int32 and c.dtype == np.int16 and c.shape == (d, 2)
        np.testing.assert_array_equal(o, off)
        np.testing.assert_array_equal(c, coef)


@pytest.mark.parametrize('f', FACTORS)
@pytest.mark.parametrize('shape', SHAPES)
def test_resize_equals_loop_statement(shape, f):
    from empanada_amd.data import resize_by_factor
    rng = np.random.default_rng(shape[0] * 131 + shape[1] + f)
    for img in (rng.integers(0, 256, shape, dtype=np.uint8), np.full(shape, 255, np.uint8)):
        got = resize_by_factor(img, f)
        assert got.dtype == np.uint8 and got.shape == (math.ceil(shape[0] / f), math.ceil(shape[1] / f))
        np.testing.assert_array_equal(got, loop_resize(img, f))


@pytest.mark.parametrize('f', FACTORS)
@pytest.mark.parametrize('shape', SHAPES)
def test_resize_within_one_grey_level_of_bilinear(shape, f):
    """derived, not tuned: 11-bit coefficients and two truncating shifts keep the fixed-point result below one grey
    level from double-precision half-pixel bilinear interpolation (the 2 x 2 mean when both ratios are exactly 2)"""
    from empanada_amd.data import resize_by_factor
    rng = np.random.default_rng(shape[0] * 17 + shape[1] + f)
    img = rng.integers(0, 256, shape, dtype=np.uint8)
    h, w = shape
    dh, dw = math.ceil(h / f), math.ceil(w / f)
    if h == 2 * dh and w == 2 * dw:
        ref = img.astype(np.float64).reshape(dh, 2, dw, 2).mean(axis=(1, 3))
    else:
        ref = torch.nn.functional.interpolate(torch.from_numpy(img.astype(np.float64))[None, None], size=(dh, dw),
                                              mode='bilinear', align_corners=False)[0, 0].numpy()
    err = float(np.abs(resize_by_factor(img, f).astype(np.float64) - ref).max())
    assert err < 1.0, err


def test_volume_dataset_scale():
    from empanada_amd.data import VolumeDataset, resize_by_factor
    rng = np.random.default_rng(5)
    vol = rng.integers(0, 256, (9, 21, 34), dtype=np.uint8)
    for axis in range(3):
        ds = VolumeDataset(vol, axis, tfs=lambda image: {'image': image.astype(np.float32) + 1}, scale=2)
        assert len(ds) == vol.shape[axis]
        for idx in (0, len(ds) - 1):
            plane = np.take(vol, idx, axis)
            h, w = plane.shape
            item = ds[idx]
            assert item['index'] == idx and item['size'] == (h, w)
            assert item['image'].shape == (math.ceil(h / 2), math.ceil(w / 2))
            np.testing.assert_array_equal(item['image'], resize_by_factor(plane, 2).astype(np.float32) + 1)
    np.testing.assert_array_equal(VolumeDataset(vol, 0, scale=1)[3]['image'], vol[3])
    with pytest.raises(Exception, match='log base 2'):
        VolumeDataset(vol, 0, scale=3)


def test_fixture_is_consistent():
    from empanada_amd.data import resize_by_factor
    g = load_golden('downsample')
    full, small = g['full_u8'], g['small_u8']
    assert full.shape[0] >= 5 and (full.shape[1] % 2 or full.shape[2] % 2)
    for i in range(full.shape[0]):
        np.testing.assert_array_equal(resize_by_factor(full[i], 2), small[i])
    assert len(g['pan']) + len(g['pan_end']) == full.shape[0] and g['pan'].shape[1:] == full.shape[1:]
    assert len(np.unique(np.concatenate([g['pan'].ravel(), g['pan_end'].ravel()]))) >= 10


def test_three_render_steps_cpu_match_reference():
    """PanopticDeepLabPR on the host, called as the Render engine calls it for upsampling = 2 (three PointRend steps,
    1/4-resolution instance heads, input padded to 16), against the REFERENCE class's outputs; tolerance of
    test_models.py::test_mitonet_512_cpu_matches_reference"""
    from empanada_amd.inference.postprocess import factor_pad
    g = load_golden('downsample')
    m = fixture_model(g)
    for i in range(g['small_u8'].shape[0]):
        with torch.no_grad():
            out = m(factor_pad(fixture_input(g, i), 16), 3, False)
        for k in ('sem_logits', 'ctr_hmp', 'offsets'):
            ref = g[k][i:i + 1]
            assert out[k].shape == ref.shape
            np.testing.assert_allclose(out[k].numpy(), ref, rtol=1e-5, atol=1e-5 * float(np.abs(ref).max()),
                                       err_msg=f'slice {i} {k}')


def test_compat_resolves_the_resize_and_the_scaled_dataset():
    """what scripts/pdl_inference3d.py -downsample-f 2 needs from `empanada.data` before the first slice"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(root, 'compat'), root]))
    code = ("import numpy as np, empanada_amd.data as d; from empanada.data import VolumeDataset; "
            "from empanada.data.utils import resize_by_factor; assert resize_by_factor is d.resize_by_factor; "
            "item = VolumeDataset(np.zeros((4, 21, 30), np.uint8), 1, lambda image: {'image': image}, scale=2)[0]; "
            "assert item['image'].shape == (2, 15) and item['size'] == (4, 30); print('ok')")
    out = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, cwd='/tmp')
    assert out.returncode == 0 and out.stdout.strip() == 'ok', out.stderr[-2000:]
