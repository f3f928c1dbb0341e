"""Device-resident slice feeder: the reference reads one slice at a time from a zarr / ndarray on the
host (`empanada/data/volume_dataset.py:7-53`), normalises it with albumentations and pads it; here the uint8 volume
lives in HBM (1 GiB at 1024^3) and every plane is a strided view of it -- `emp_slices_to_input` gathers, normalises
and pads a batch of slices in one pass, for any of the three axes, without transposed copies.

Normalisation arithmetic: albumentations.Normalize(mean, std, max_pixel_value=255) computes, in fp32,
(x - mean*255) * (1 / (std*255)).  albumentations is not installed in this image, so this restates its published
formula: parity with the library is unpinned; the kernel is checked bit for bit against a numpy statement of the formula.

Down-sampling (`scale` = N, a power of two; the reference's `-downsample-f`): every slice is shrunk in-plane to
(ceil(h/N), ceil(w/N)) before it is normalised (`resize_by_factor`, empanada/data/utils/transforms.py:9-21, which calls
cv2.resize with its default interpolation).  cv2 is not installed in this image either, so `resize_by_factor` restates
OpenCV's published algorithm for uint8 images: the 2x2 area form ((s00 + s01 + s10 + s11 + 2) >> 2) when both ratios are
exactly 2, otherwise separable fixed-point bilinear interpolation with 11-bit coefficients (`resize_tables`).  Parity
with the library is unpinned, like Normalize; `emp_slices_to_input_scaled` and VolumeDataset(scale=N) are pinned bit for
bit to this statement.
"""
import math

import numpy as np
import torch

from . import _hip

__all__ = ['DeviceVolume', 'VolumeDataset', 'normalize_constants', 'resize_by_factor', 'resize_tables', 'scaled_size',
           'AXES']

AXES = {'xy': 0, 'xz': 1, 'yz': 2}


def normalize_constants(mean, std, max_pixel_value=255.0):
    """(mean*255, 1/(std*255)) as fp32, computed like albumentations does (fp32 products, fp32 reciprocal)"""
    m = np.float32(mean) * np.float32(max_pixel_value)
    s = np.float32(std) * np.float32(max_pixel_value)
    return float(m), float(np.reciprocal(s, dtype=np.float32))


def _check_scale(scale):
    """the reference's check (volume_dataset.py:26-27), also rejecting what math.log cannot take"""
    if isinstance(scale, bool) or not isinstance(scale, (int, np.integer)) or scale < 1 \
            or not math.log(scale, 2).is_integer():
        raise Exception(f'Image rescaling must be log base 2, got {scale}')
    return int(scale)


def scaled_size(h, w, scale_factor):
    """(ceil(h / f), ceil(w / f)): the size resize_by_factor gives (transforms.py:15-17)"""
    return math.ceil(h / scale_factor), math.ceil(w / scale_factor)


def resize_tables(src_len, dst_len):
    """One axis of OpenCV's fixed-point bilinear resize (INTER_RESIZE_COEF_BITS = 11): for every destination index the
    first source index (int32, the second tap is min(s + 1, src_len - 1)) and the coefficient pair (int16, (dst, 2)).
    The source coordinate is computed in double and rounded to fp32, the fraction and the coefficients in fp32,
    coefficients rounded half to even."""
    scale = 1.0 / (dst_len / src_len)
    fx = ((np.arange(dst_len, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(fx).astype(np.int32)
    fx = fx - s.astype(np.float32)
    edge = (s < 0) | (s >= src_len - 1)
    s = np.clip(s, 0, src_len - 1).astype(np.int32)
    fx[edge] = 0
    a0 = np.rint((np.float32(1) - fx) * np.float32(2048)).astype(np.int16)
    a1 = np.rint(fx * np.float32(2048)).astype(np.int16)
    return s, np.ascontiguousarray(np.stack([a0, a1], axis=1))


def resize_by_factor(image, scale_factor=1):
    """cv2.resize(uint8 image (h, w), (ceil(w/f), ceil(h/f))) with the default interpolation, restated (module
    docstring); f == 1 returns the image itself (transforms.py:9-21)"""
    if scale_factor == 1:
        return image
    image = np.asarray(image)
    assert image.dtype == np.uint8 and image.ndim == 2, "uint8 (h, w) image expected"
    h, w = image.shape
    dh, dw = scaled_size(h, w, scale_factor)
    if h == 2 * dh and w == 2 * dw:
        q = image.astype(np.int32)
        return ((q[0::2, 0::2] + q[0::2, 1::2] + q[1::2, 0::2] + q[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    ys, b = resize_tables(h, dh)
    xs, a = resize_tables(w, dw)
    src = image.astype(np.int32)
    x1 = np.minimum(xs + 1, w - 1)
    rows = src[:, xs] * a[:, 0].astype(np.int32) + src[:, x1] * a[:, 1].astype(np.int32)        # (h, dw)
    r0, r1 = rows[ys] >> 4, rows[np.minimum(ys + 1, h - 1)] >> 4
    b0, b1 = b[:, 0].astype(np.int32)[:, None], b[:, 1].astype(np.int32)[:, None]
    return ((((b0 * r0) >> 16) + ((b1 * r1) >> 16) + 2) >> 2).astype(np.uint8)


class DeviceVolume:
    """A (D, H, W) uint8 volume resident on the GPU, served as normalised, padded (B, 1, hp, wp) fp32 batches along
    any axis.  `len(dv.plane(axis))` slices of shape dv.plane_shape(axis); padding to a multiple of `factor`
    (factor_pad, inference/postprocess.py:25-36).  scale > 1 (a power of two): every slice is shrunk in-plane by
    resize_by_factor before it is normalised, so batches hold the scaled_shape(axis) image padded to `factor`;
    plane_shape stays the full size (what the labels are cropped to)."""

    def __init__(self, volume, mean, std, factor=16, device='cuda', scale=1):
        v = torch.as_tensor(np.ascontiguousarray(volume) if isinstance(volume, np.ndarray) else volume)
        assert v.dtype == torch.uint8 and v.dim() == 3, "uint8 (D, H, W) volume expected"
        self.vol = v.to(device).contiguous()
        self.shape = tuple(self.vol.shape)
        self.factor = int(factor)
        self.mean255, self.inv_std255 = normalize_constants(mean, std)
        self.scale = _check_scale(scale)
        self._tables = {}

    def n_slices(self, axis):
        return self.shape[AXES[axis]]

    def plane_shape(self, axis):
        d = AXES[axis]
        return tuple(s for i, s in enumerate(self.shape) if i != d)

    def scaled_shape(self, axis):
        """the plane after resize_by_factor(., scale): what the model sees before padding"""
        return scaled_size(*self.plane_shape(axis), self.scale)

    def padded_shape(self, axis):
        h, w = self.scaled_shape(axis)
        f = self.factor
        return (-(-h // f) * f, -(-w // f) * f)

    def _strides(self, axis):
        D, H, W = self.shape
        st = (H * W, W, 1)
        d = AXES[axis]
        rest = [i for i in range(3) if i != d]
        return st[d], st[rest[0]], st[rest[1]]

    def _resize_tables(self, axis):
        """device tables of the axis' plane for emp_slices_to_input_scaled (built once): row offsets, row coefficient
        pairs, column offsets, column coefficient pairs, and whether the 2x2 area form applies"""
        if axis not in self._tables:
            h, w = self.plane_shape(axis)
            dh, dw = self.scaled_shape(axis)
            tabs = [torch.from_numpy(t).to(self.vol.device) for t in resize_tables(h, dh) + resize_tables(w, dw)]
            self._tables[axis] = (tabs, int(h == 2 * dh and w == 2 * dw))
        return self._tables[axis]

    def batch(self, axis, lo, hi, out=None):
        """slices [lo, hi) of the plane -> (hi-lo, 1, hp, wp) fp32 (memory is NCHW == NHWC for one channel); `out`:
        a contiguous tensor of that shape to fill instead of a new one (e.g. a HIP graph's static input)"""
        _hip.require_gpu()
        n = hi - lo
        assert 0 <= lo <= hi <= self.n_slices(axis)
        h, w = self.plane_shape(axis)
        hp, wp = self.padded_shape(axis)
        ss, sr, sc = self._strides(axis)
        if out is None:
            out = torch.empty((n, 1, hp, wp), dtype=torch.float32, device=self.vol.device)
        assert tuple(out.shape) == (n, 1, hp, wp) and out.dtype == torch.float32 and out.is_contiguous()
        if self.scale == 1:
            _hip.call('emp_slices_to_input', self.vol.data_ptr() + lo * ss, ss, sr, sc, n, h, w, hp, wp, self.mean255,
                      self.inv_std255, out.data_ptr(), _hip.stream(), alg_bytes=n * h * w + 4 * out.numel())
            return out
        dh, dw = self.scaled_shape(axis)
        (ro, rc, co, cc), area = self._resize_tables(axis)
        _hip.call('emp_slices_to_input_scaled', self.vol.data_ptr() + lo * ss, ss, sr, sc, n, h, w, dh, dw, hp, wp,
                  ro.data_ptr(), rc.data_ptr(), co.data_ptr(), cc.data_ptr(), area, self.mean255, self.inv_std255,
                  out.data_ptr(), _hip.stream(), alg_bytes=n * h * w + 4 * out.numel())
        return out

    def batches(self, axis, batch, lo=0, hi=None):
        hi = self.n_slices(axis) if hi is None else hi
        for s in range(lo, hi, batch):
            yield s, self.batch(axis, s, min(hi, s + batch))


class VolumeDataset:
    """Map-style dataset over the slices of a volume along an axis, the reference's host-side reader
    (empanada/data/volume_dataset.py:7-53): item = {'index', 'image', 'size'} with `tfs(image=...)['image']` applied.
    `array` may be anything `array_utils.take` can slice (numpy, ZarrV2Array).  `scale` (a power of two): the slice
    is shrunk by resize_by_factor before `tfs`; 'size' stays the original (h, w), which the engine crops to."""

    def __init__(self, array, axis=0, tfs=None, scale=1):
        self.array, self.axis, self.tfs, self.scale = array, axis, tfs, _check_scale(scale)

    def __len__(self):
        return self.array.shape[self.axis]

    def __getitem__(self, idx):
        from .array_utils import take
        image = np.asarray(take(self.array, idx, self.axis))
        h, w = image.shape
        image = resize_by_factor(image, self.scale)
        assert image.shape[0] * self.scale >= h and image.shape[1] * self.scale >= w
        if self.tfs is not None:
            image = self.tfs(image=image)['image']
        return {'index': idx, 'image': image, 'size': (h, w)}
