"""Shared by tests/test_downsample_host.py and tests/test_downsample_gpu.py (not a test module).

loop_resize: the resize statement of empanada_amd/data.py's docstring once more, independently of resize_by_factor:
one destination pixel at a time, Python integers for the fixed-point part and numpy fp32 scalars for the coefficient
arithmetic.  fixture_model / fixture_input: the model and the inputs tests/golden/downsample.npz was made with
(tools/gen_golden_downsample.py)."""
import math

import numpy as np
import torch

MITO = dict(encoder='resnet50', num_classes=1, stage4_stride=16, decoder_channels=256, low_level_stages=[1],
            low_level_channels_project=[32], atrous_rates=[2, 4, 6], aspp_channels=None, aspp_dropout=0.5,
            ins_decoder=True, ins_ratio=0.5)
MITO_ENGINE = dict(thing_list=[1], label_divisor=20000, stuff_area=64, void_label=0, nms_threshold=0.1, nms_kernel=7,
                   confidence_thr=0.3, padding_factor=16, coarse_boundaries=True)     # oracle/gen_golden_r4.py::ENGINE


def loop_axis(src_len, dst_len):
    """[(first source index, a0, a1)] for every destination index of one axis"""
    scale = 1.0 / (dst_len / src_len)
    out = []
    for d in range(dst_len):
        fx = np.float32((d + 0.5) * scale - 0.5)
        s = int(math.floor(float(fx)))
        fx = np.float32(fx - np.float32(s))
        if s < 0:
            s, fx = 0, np.float32(0)
        if s >= src_len - 1:
            s, fx = src_len - 1, np.float32(0)
        a0 = int(np.int16(np.rint(np.float32((np.float32(1) - fx) * np.float32(2048)))))
        a1 = int(np.int16(np.rint(np.float32(fx * np.float32(2048)))))
        out.append((s, a0, a1))
    return out


def loop_resize(image, f):
    if f == 1:
        return image
    h, w = image.shape
    dh, dw = math.ceil(h / f), math.ceil(w / f)
    src = [[int(v) for v in row] for row in image]
    dst = np.zeros((dh, dw), dtype=np.uint8)
    if h == 2 * dh and w == 2 * dw:
        for y in range(dh):
            for x in range(dw):
                dst[y, x] = (src[2 * y][2 * x] + src[2 * y][2 * x + 1] + src[2 * y + 1][2 * x]
                             + src[2 * y + 1][2 * x + 1] + 2) >> 2
        return dst
    rows, cols = loop_axis(h, dh), loop_axis(w, dw)
    for y, (y0, b0, b1) in enumerate(rows):
        y1 = min(y0 + 1, h - 1)
        for x, (x0, a0, a1) in enumerate(cols):
            x1 = min(x0 + 1, w - 1)
            r0 = src[y0][x0] * a0 + src[y0][x1] * a1
            r1 = src[y1][x0] * a0 + src[y1][x1] * a1
            v = (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2
            assert 0 <= v <= 255
            dst[y, x] = v
    return dst


def normalised(image_u8, mean, std):
    """the numpy statement of Normalize the feeder is pinned to (tests/test_hip_kernels.py::test_device_volume_feeder)"""
    from empanada_amd.data import normalize_constants
    m255, inv = normalize_constants(mean, std)
    return (image_u8.astype(np.float32) - np.float32(m255)) * np.float32(inv)


def fixture_model(g):
    from empanada_amd.models import PanopticDeepLabPR, synthesize_weights
    m = synthesize_weights(PanopticDeepLabPR(**MITO)).eval()
    with torch.no_grad():
        for layer, damp in zip(g['damp_layer'], g['damp']):
            m.get_submodule(str(layer)).weight.mul_(float(damp))
    return m


def fixture_engine_params(g):
    return dict(MITO_ENGINE, nms_kernel=int(g['nms_kernel']))


def fixture_input(g, i):
    """slice i as the engine is given it: shrunk, normalised, (1, 1, dh, dw); not yet padded"""
    mean, std = (float(v) for v in g['norms'])
    return torch.from_numpy(normalised(g['small_u8'][i], mean, std))[None, None]
