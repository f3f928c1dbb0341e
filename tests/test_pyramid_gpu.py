"""GPU: the multiscale label pyramid -- emp_label_pool_mode (csrc/emp_pool.hip) through _hip.pool_labels,
inference/pyramid.py and infer_volume(..., pyramid=).  The checker is `mode_pool` below, a numpy restatement of the
definition in include/emp_hip.h (Z2) that shares nothing with the kernel: the values of every cell are gathered with a
validity mask, the equal valid values are counted per position, and the winner is the argmax of count * 2^32 + value.
Everything is compared bit for bit.  The engine and volume of the infer_volume cases are those of
tests/test_deflate_gpu.py."""
import itertools
import json
import os
import queue
import socket
import zlib

import numpy as np
import pytest
import torch

from empanada_amd import synthetic as SY

pytestmark = pytest.mark.gpu

FACTORS = [f for f in itertools.product((1, 2), repeat=3) if f != (1, 1, 1)]
SHAPES = [(1, 1, 1), (1, 1, 2), (2, 2, 2), (3, 3, 5), (2, 5, 130), (2, 4, 259), (3, 2, 1031), (5, 64, 64)]
DTYPES = [np.uint8, np.uint32]
_CACHE = {}


# ------------------------------------------------------------------------------------------------------ the checker
def mode_pool(a, f, tie='largest'):
    """(D, H, W) unsigned array -> its mode pooling by f = (fz, fy, fx), from the definition: the cell of output voxel
    (z, y, x) is [fz z, fz z + fz) x [fy y, ...) x [fx x, ...) clipped to the volume; the result is the value that occurs
    most often in it, the largest among values that occur equally often.  tie='smallest': the other rule, to show that
    the data tell the two apart"""
    D, H, W = a.shape
    out_shape = tuple(-(-s // v) for s, v in zip(a.shape, f))
    vals, valid = [], []
    for dz, dy, dx in itertools.product(range(f[0]), range(f[1]), range(f[2])):
        zi, yi, xi = (np.arange(n) * v + d for n, v, d in zip(out_shape, f, (dz, dy, dx)))
        ok = (zi < D)[:, None, None] & (yi < H)[None, :, None] & (xi < W)[None, None, :]
        v = a[np.minimum(zi, D - 1)][:, np.minimum(yi, H - 1)][:, :, np.minimum(xi, W - 1)]
        vals.append(np.where(ok, v, 0).astype(np.uint64))           # what an invalid position holds is never looked at
        valid.append(ok)
    vals, valid = np.stack(vals), np.stack(valid)
    counts = np.zeros(vals.shape, np.uint64)
    for i in range(len(vals)):
        for j in range(len(vals)):
            counts[i] += (valid[j] & (vals[i] == vals[j])).astype(np.uint64)
    rank = vals if tie == 'largest' else np.uint64(0xFFFFFFFF) - vals
    key = np.where(valid, (counts << np.uint64(32)) | rank, np.uint64(0))    # a valid position counts itself: key >= 2^32
    best = key.max(axis=0) & np.uint64(0xFFFFFFFF)
    if tie != 'largest':
        best = np.uint64(0xFFFFFFFF) - best
    return best.astype(a.dtype)


def test_the_checker_on_cells_counted_by_hand():
    for cell, want in (([0, 0, 0, 0, 5, 5, 5, 5], 5), ([7, 7, 3, 3, 3, 9, 9, 9], 9), ([1, 2, 3, 4, 5, 6, 7, 8], 8)):
        assert mode_pool(np.array(cell, np.uint32).reshape(2, 2, 2), (2, 2, 2)).tolist() == [[[want]]]
    assert mode_pool(np.array([7, 7, 3, 3, 3, 9, 9, 9], np.uint32).reshape(2, 2, 2), (2, 2, 2), 'smallest').tolist() == [[[3]]]
    a = np.arange(27, dtype=np.uint8).reshape(3, 3, 3)
    np.testing.assert_array_equal(mode_pool(a, (2, 2, 2)), [[[13, 14], [16, 17]], [[22, 23], [25, 26]]])


def _planted():
    """(8, 256, 256) uint16 labels, fill 0.08, seed 4321: computed once, never modified"""
    if 'planted' not in _CACHE:
        _CACHE['planted'] = SY.planted_labels((8, 256, 256), fill=0.08, seed=4321)[0]
    return _CACHE['planted']


def _dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        return torch.from_numpy(a.view(np.int32)).cuda().view(torch.uint32)
    return torch.from_numpy(a).cuda()


def _np(v):
    return v.view(torch.int32).cpu().numpy().view(np.uint32) if v.dtype == torch.uint32 else v.cpu().numpy()


def _alphabet(shape, dtype):
    """four letters, 0, 1 and the largest value among them (and one above 2^31): most cells are ties"""
    top = np.iinfo(dtype).max
    letters = np.array([0, 1, top // 2 + 1, top], dtype)
    rng = np.random.default_rng(int(np.prod(shape)) + np.dtype(dtype).itemsize)
    return letters[rng.integers(0, 4, size=shape)]


# ------------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize('dtype', DTYPES, ids=['u8', 'u32'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_kernel_equals_the_restatement(shape, dtype):
    from empanada_amd import _hip
    for content in (np.zeros(shape, dtype), _alphabet(shape, dtype)):
        dev = _dev(content)
        for f in FACTORS:
            got = _hip.pool_labels(dev, f)
            assert got.dtype == dev.dtype and got.is_cuda and got.is_contiguous()
            assert tuple(got.shape) == tuple(-(-s // v) for s, v in zip(shape, f))
            np.testing.assert_array_equal(_np(got), mode_pool(content, f), err_msg=f'{shape} {f}')


@pytest.mark.parametrize('dtype', DTYPES, ids=['u8', 'u32'])
def test_planted_labels(dtype):
    from empanada_amd import _hip
    lab = _planted().astype(dtype)                                  # uint8: the labels' low bytes
    assert lab.any()
    dev = _dev(lab)
    for f in FACTORS:
        np.testing.assert_array_equal(_np(_hip.pool_labels(dev, f)), mode_pool(lab, f), err_msg=str(f))


def test_the_tie_rule_is_under_test():
    for dtype in DTYPES:
        a = _alphabet((5, 64, 64), dtype)
        assert (mode_pool(a, (2, 2, 2)) != mode_pool(a, (2, 2, 2), 'smallest')).any()
        assert (mode_pool(a, (1, 1, 2)) != mode_pool(a, (1, 1, 2), 'smallest')).any()


def test_int32_bits_are_taken_as_they_are():
    from empanada_amd import _hip
    a = _alphabet((3, 5, 130), np.uint32)                           # half the letters are negative as int32
    for f in ((2, 2, 2), (1, 2, 2), (2, 1, 1)):
        got = _hip.pool_labels(torch.from_numpy(a.view(np.int32)).cuda(), f)
        assert got.dtype == torch.int32
        np.testing.assert_array_equal(got.cpu().numpy().view(np.uint32), mode_pool(a, f))


@pytest.mark.parametrize('dtype', DTYPES, ids=['u8', 'u32'])
def test_cells_checked_by_hand(dtype):
    from empanada_amd import _hip
    for cell, want in (([0, 0, 0, 0, 5, 5, 5, 5], 5), ([7, 7, 3, 3, 3, 9, 9, 9], 9), ([1, 2, 3, 4, 5, 6, 7, 8], 8)):
        got = _hip.pool_labels(_dev(np.array(cell, dtype).reshape(2, 2, 2)), (2, 2, 2))
        assert _np(got).tolist() == [[[want]]], cell
    for v in (0, 1, 200, int(np.iinfo(dtype).max)):                 # a clipped cell of one voxel
        for f in FACTORS:
            assert _np(_hip.pool_labels(_dev(np.full((1, 1, 1), v, dtype)), f)).tolist() == [[[v]]]
    corner = np.zeros((3, 3, 3), dtype)                             # the last cell along every axis holds one voxel
    corner[2, 2, 2] = 9
    assert int(_np(_hip.pool_labels(_dev(corner), (2, 2, 2)))[1, 1, 1]) == 9


@pytest.mark.parametrize('dtype', DTYPES, ids=['u8', 'u32'])
def test_out_argument(dtype):
    from empanada_amd import _hip
    a = _alphabet((5, 9, 131), dtype)
    dev = _dev(a)
    want = mode_pool(a, (2, 2, 2))
    tdt = torch.uint8 if dtype == np.uint8 else torch.int32
    big = torch.full((5,) + want.shape[1:], 0xA5 if dtype == np.uint8 else 0x25A5A5A5, dtype=tdt, device='cuda')
    guard = big.clone()
    out = big[1:4] if dtype == np.uint8 else big[1:4].view(torch.uint32)
    got = _hip.pool_labels(dev, (2, 2, 2), out=out)
    assert got.data_ptr() == out.data_ptr()
    np.testing.assert_array_equal(_np(got), want)
    assert torch.equal(big[0], guard[0]) and torch.equal(big[4], guard[4])          # nothing outside the slice
    again = _hip.pool_labels(dev, (2, 2, 2))
    assert torch.equal(again.view(tdt), big[1:4])
    for bad in (out[:2], out.cpu(), out[:, :, :-1], out.view(tdt).to(torch.int16)):
        with pytest.raises(ValueError):
            _hip.pool_labels(dev, (2, 2, 2), out=bad)
    with pytest.raises(ValueError, match='overlap'):
        flat = torch.zeros((2 * a.size,), dtype=tdt, device='cuda')
        src = flat[:a.size].view(a.shape)
        _hip.pool_labels(src, (2, 2, 2), out=flat[a.size - 4:a.size - 4 + want.size].view(want.shape))
    for bad in (dev.cpu(), dev[:, :, ::2], dev[0], dev.view(tdt).to(torch.float32)):
        with pytest.raises(ValueError):
            _hip.pool_labels(bad)
    for bad in ((1, 1, 1), (2, 2), (2, 3, 2), (0, 2, 2), (2, 2, 2, 2), 2, None, (2.0, 2, 2)):
        with pytest.raises(ValueError, match='factors'):
            _hip.pool_labels(dev, bad)


def test_unaligned_slab_takes_the_narrow_path():
    """rows of whole 16-byte groups, but the slab starts one element off a 16-byte address: same results"""
    from empanada_amd import _hip
    for dtype, tdt in ((np.uint32, torch.int32), (np.uint8, torch.uint8)):
        a = _alphabet((3, 6, 64), dtype)
        flat = torch.zeros((a.size + 16,), dtype=tdt, device='cuda')
        flat[1:1 + a.size] = _dev(a).view(tdt).ravel()
        dev = flat[1:1 + a.size].view(a.shape)
        assert dev.data_ptr() % 16 != 0 and dev.is_contiguous()
        for f in ((2, 2, 2), (1, 2, 1)):
            got = _hip.pool_labels(dev, f)
            np.testing.assert_array_equal(got.cpu().numpy().view(dtype), mode_pool(a, f))


def test_chained_levels():
    from empanada_amd.inference import pyramid as P
    lab = _planted().astype(np.uint32)
    for factors in (P.normalize(3), [(1, 2, 2), (2, 2, 2), (2, 1, 2)]):
        got = P.build(_dev(lab), factors)
        assert len(got) == 3
        want = lab
        for g, f in zip(got, factors):
            want = mode_pool(want, f)
            np.testing.assert_array_equal(_np(g), want)
        assert want.any()


@pytest.mark.parametrize('W', [40001, 40032], ids=['narrow', 'wide'])
def test_more_than_2_to_32_voxels(W):
    """a uint8 slab of 4.8e9 voxels: the rows checked lie on both sides of element 2^32.  W = 40001: rows that are not
    16-byte aligned; W = 40032: aligned input and output rows"""
    from empanada_amd import _hip
    if torch.cuda.mem_get_info()[0] < 16 << 30:
        pytest.skip("needs 16 GB of free device memory")
    D, H = 3, 40000
    assert D * H * W > 2 ** 32
    xv, yv = (np.arange(W) // 3 % 4).astype(np.uint8), (np.arange(H) // 2 * 3 % 4).astype(np.uint8)
    slab = torch.empty((D, H, W), dtype=torch.uint8, device='cuda')
    dx, dy = torch.from_numpy(xv).cuda(), torch.from_numpy(yv).cuda()
    for z in range(D):
        torch.add(dx[None, :], dy[:, None] + z, out=slab[z])
    slab.bitwise_and_(3)
    got = _hip.pool_labels(slab, (2, 2, 2))
    assert tuple(got.shape) == (2, 20000, -(-W // 2))
    for rows, orows in ((slice(0, 12), slice(0, 6)), (slice(H - 12, H), slice(20000 - 6, 20000))):
        host = (xv[None, None, :] + yv[None, rows, None] + np.arange(D, dtype=np.uint8)[:, None, None]) & 3
        np.testing.assert_array_equal(slab[:, rows].cpu().numpy(), host)
        np.testing.assert_array_equal(got[:, orows].cpu().numpy(), mode_pool(host, (2, 2, 2)))
    del slab, got
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------ infer_volume
NORMS = dict(mean=0.508979, std=0.148561)
ORTHO = ('xy', 'xz', 'yz')
KW = dict(norms=NORMS, labels=[1, 2], min_size=30, min_span=2, class_names={1: 'mito', 2: 'er'}, batch_pixels=1 << 22)
SHAPE = (40, 72, 88)
NAMES = {1: 'mito_pred', 2: 'er_pred'}


def _engine():
    from empanada_amd.inference import engines as EN
    from empanada_amd.models import PanopticDeepLab, prepare_for_inference, synthesize_weights
    from empanada_amd.models.panoptic_deeplab import FusedConvBNAct
    model = synthesize_weights(PanopticDeepLab(encoder='resnet18', num_classes=3))
    with torch.no_grad():                                  # offsets of a few pixels instead of hundreds
        model.ins_xy.head[1].weight.mul_(2e-2)
    model = prepare_for_inference(model, 'cuda')
    for m in model.modules():                              # the hand-written kernels: run-to-run identical outputs
        if isinstance(m, FusedConvBNAct) and 'direct' in m.candidates(False):
            m.impl = 'direct'
    return EN.PanopticDeepLabEngine3d(model, thing_list=[1], label_divisor=1000, stuff_area=16, void_label=0,
                                      nms_threshold=0.1, nms_kernel=7, confidence_thr=0.5, median_kernel_size=3,
                                      padding_factor=32)


def _run(engine, vol, path, **kw):
    from empanada_amd.inference.driver import infer_volume
    from empanada_amd.zarr_utils import ZarrV2Group
    return infer_volume(engine, vol, out=None if path is None else ZarrV2Group(str(path)), **dict(KW, **kw))


@pytest.fixture
def case(tmp_path_factory):
    """(engine, volume, the plain call's volumes, dataset contents and counts) per axes: computed once, never modified"""
    def get(axes):
        if axes not in _CACHE:
            eng = _CACHE['engine'] = _CACHE.get('engine') or _engine()
            vol = SY.em_volume(SHAPE, seed=3)
            res = _run(eng, vol, tmp_path_factory.mktemp('plain') / 'pred.zarr', axes=axes)
            assert not any(k.startswith('pyramid') for k in res)
            vols = {c: _np(v) for c, v in res['volumes'].items()}
            assert vols[1].dtype == np.uint32 and vols[2].dtype == np.uint8
            assert vols[1].max() > 0 and vols[2].max() > 0, "the random model should segment something of both classes"
            root = res['datasets'][1].path.rsplit(os.sep, 1)[0]
            assert sorted(os.listdir(root)) == ['.zgroup', 'er_pred', 'mito_pred']         # nothing new in the store
            _CACHE[axes] = (eng, vol, vols, {c: np.asarray(a[...]) for c, a in res['datasets'].items()},
                            dict(res['instances']))
        return _CACHE[axes]
    return get


def _files(array):
    return sorted((f for f in os.listdir(array.path) if not f.startswith('.')), key=lambda s: int(s.split('.')[0]))


def _expected_multiscales(cum):
    from empanada_amd.inference import pyramid as P
    return [P.multiscales(n, [n] + [f'{n}_s{l}' for l in range(1, len(cum))], cum) for n in (NAMES[1], NAMES[2])]


def _assert_pyramid(res, path, exp_vols, exp_sets, exp_counts, factors, compressor=None):
    """level 0 is what the call without pyramid= gives; every level is the restatement chained on the level-0 volume,
    in the result and in the store; the attributes hold the two entries.  Returns {class: [level arrays]}"""
    from empanada_amd.zarr_utils import ZarrV2Group
    assert dict(res['instances']) == exp_counts and tuple(res['z_range']) == (0, SHAPE[0])
    assert sorted(res['pyramid']) == sorted(res['pyramid_datasets']) == [1, 2]
    assert ('pyramid_compressed_bytes' in res) == ('compressed_bytes' in res) == (compressor is not None)
    shapes, cum, zr = [], [(1, 1, 1)], []
    s = SHAPE
    for f in factors:
        s = tuple(-(-a // b) for a, b in zip(s, f))
        shapes.append(s)
        cum.append(tuple(a * b for a, b in zip(cum[-1], f)))
        zr.append((0, s[0]))
    assert [tuple(z) for z in res['pyramid_z_ranges']] == zr
    g = ZarrV2Group(str(path), mode='r')
    levels = {}
    for c in (1, 2):
        np.testing.assert_array_equal(_np(res['volumes'][c]), exp_vols[c], err_msg=f'class {c}')
        ds = res['datasets'][c]
        assert ds.path == os.path.join(str(path), NAMES[c]) and tuple(ds.chunks) == (1,) + SHAPE[1:]
        np.testing.assert_array_equal(np.asarray(ds), exp_sets[c], err_msg=f'dataset of class {c}')
        want, levels[c] = exp_vols[c], []
        assert len(res['pyramid'][c]) == len(res['pyramid_datasets'][c]) == len(factors)
        for l, f in enumerate(factors, start=1):
            want = mode_pool(want, f)
            slab = res['pyramid'][c][l - 1]
            assert slab.is_cuda and slab.dtype == res['volumes'][c].dtype and tuple(slab.shape) == shapes[l - 1]
            np.testing.assert_array_equal(_np(slab), want, err_msg=f'class {c} level {l}')
            ds = res['pyramid_datasets'][c][l - 1]
            assert ds.path == os.path.join(str(path), f'{NAMES[c]}_s{l}') and f'{NAMES[c]}_s{l}' in g
            assert ds.shape == shapes[l - 1] and tuple(ds.chunks) == (1,) + shapes[l - 1][1:]
            assert ds.dtype == exp_sets[c].dtype and ds.meta['compressor'] == res['datasets'][c].meta['compressor']
            np.testing.assert_array_equal(np.asarray(g[f'{NAMES[c]}_s{l}']), want, err_msg=f'dataset {c} level {l}')
            assert _files(ds) == [f'{z}.0.0' for z in range(shapes[l - 1][0])]
            if compressor is not None:
                total = 0
                for z, name in enumerate(_files(ds)):
                    with open(os.path.join(ds.path, name), 'rb') as fh:
                        raw = fh.read()
                    assert zlib.decompress(raw) == want[z].tobytes()
                    total += len(raw)
                assert total == res['pyramid_compressed_bytes'][c][l - 1]
            levels[c].append(want)
        assert want.any(), f"the last level of class {c} should not be empty"
        if compressor is not None:                                  # 'compressed_bytes' keeps meaning level 0
            ds = res['datasets'][c]
            assert res['compressed_bytes'][c] == sum(os.path.getsize(os.path.join(ds.path, n)) for n in _files(ds))
    assert g.attrs == {'multiscales': _expected_multiscales(cum)}
    with open(os.path.join(str(path), '.zattrs')) as fh:
        assert json.load(fh) == g.attrs
    assert sorted(os.listdir(str(path))) == sorted(['.zattrs', '.zgroup'] + [NAMES[c] + (f'_s{l}' if l else '')
                                                   for c in (1, 2) for l in range(len(factors) + 1)])
    return levels


@pytest.mark.parametrize('pyramid', [2, [(1, 2, 2), (2, 2, 2)]], ids=['two', 'thick'])
@pytest.mark.parametrize('compressor', [None, 'zlib'])
def test_infer_volume_plain_path(tmp_path, case, pyramid, compressor):
    from empanada_amd.inference import pyramid as P
    eng, vol, vols, sets, counts = case(ORTHO)
    res = _run(eng, vol, tmp_path / 'p.zarr', axes=ORTHO, pyramid=pyramid, compressor=compressor)
    _assert_pyramid(res, tmp_path / 'p.zarr', vols, sets, counts, P.normalize(pyramid), compressor)


def test_infer_volume_without_a_store(case):
    eng, vol, vols, _, counts = case(('xy',))
    res = _run(eng, vol, None, axes=('xy',), pyramid=2)
    assert dict(res['instances']) == counts and res['datasets'] == {1: None, 2: None}
    assert res['pyramid_datasets'] == {1: [None, None], 2: [None, None]} and 'pyramid_compressed_bytes' not in res
    assert [tuple(z) for z in res['pyramid_z_ranges']] == [(0, 20), (0, 10)]
    for c in (1, 2):
        np.testing.assert_array_equal(_np(res['volumes'][c]), vols[c])
        want = vols[c]
        for slab in res['pyramid'][c]:
            want = mode_pool(want, (2, 2, 2))
            np.testing.assert_array_equal(_np(slab), want)


def test_infer_volume_windowed(tmp_path, case):
    eng, vol, _, _, _ = case(('xy',))
    kw = dict(axes=('xy',), batch_pixels=4 * 96 * 96, window_slices=8)      # 4 slices per model call, windows of 8
    plain = _run(eng, vol, tmp_path / 'raw.zarr', **kw)
    res = _run(eng, vol, tmp_path / 'p.zarr', pyramid=2, compressor='zlib', **kw)
    assert res['windows']['xy'] > 1
    _assert_pyramid(res, tmp_path / 'p.zarr', {c: _np(v) for c, v in plain['volumes'].items()},
                    {c: np.asarray(a[...]) for c, a in plain['datasets'].items()}, dict(plain['instances']),
                    [(2, 2, 2)] * 2, 'zlib')


def test_infer_volume_pipeline(tmp_path, case):
    from empanada_amd.inference.pipeline import VolumePipeline
    eng, vol, vols, sets, counts = case(ORTHO)
    pipe = VolumePipeline(eng, tune=False, graph=True, overlap=True, batch_pixels=1 << 22)
    factors = [(2, 2, 2)] * 2
    keys = [1, 2, (1, 1), (1, 2), (2, 1), (2, 2)]
    # raw chunks: one writer, with its pinned buffer, per class and level
    res = _run(eng, vol, tmp_path / 'a.zarr', axes=ORTHO, pyramid=2, pipeline=pipe)
    _assert_pyramid(res, tmp_path / 'a.zarr', vols, sets, counts, factors)
    assert res['pipeline']['graph'] is True
    assert sorted((k[0] for k in pipe._writers), key=str) == sorted(keys, key=str)
    writers = {k: (id(w), w.bufs[0].data_ptr()) for k, w in pipe._writers.items()}
    res = _run(eng, vol, tmp_path / 'b.zarr', axes=ORTHO, pyramid=2, pipeline=pipe)
    _assert_pyramid(res, tmp_path / 'b.zarr', vols, sets, counts, factors)
    assert {k: (id(w), w.bufs[0].data_ptr()) for k, w in pipe._writers.items()} == writers          # nothing re-pinned
    # zlib: one pinned buffer of compressed bytes per class and level, sized by what the level took
    res = _run(eng, vol, tmp_path / 'c.zarr', axes=ORTHO, pyramid=2, compressor='zlib', pipeline=pipe)
    _assert_pyramid(res, tmp_path / 'c.zarr', vols, sets, counts, factors, 'zlib')
    assert sorted(pipe._zbufs, key=str) == sorted(keys, key=str) and all(b.is_pinned() for b in pipe._zbufs.values())
    assert {c: pipe._zbufs[c].numel() for c in (1, 2)} == res['compressed_bytes']
    assert {c: [pipe._zbufs[(c, l)].numel() for l in (1, 2)] for c in (1, 2)} == res['pyramid_compressed_bytes']
    held = {k: b.data_ptr() for k, b in pipe._zbufs.items()}
    res = _run(eng, vol, tmp_path / 'd.zarr', axes=ORTHO, pyramid=2, compressor='zlib', pipeline=pipe)
    _assert_pyramid(res, tmp_path / 'd.zarr', vols, sets, counts, factors, 'zlib')
    assert {k: b.data_ptr() for k, b in pipe._zbufs.items()} == held                                # nothing re-pinned
    assert {k: (id(w), w.bufs[0].data_ptr()) for k, w in pipe._writers.items()} == writers
    # without pyramid= the same pipeline does what it did: no new key, nothing new in the store
    plain = _run(eng, vol, tmp_path / 'e.zarr', axes=ORTHO, pipeline=pipe)
    assert not any(k.startswith('pyramid') for k in plain)
    assert sorted(os.listdir(str(tmp_path / 'e.zarr'))) == ['.zgroup', 'er_pred', 'mito_pred']
    np.testing.assert_array_equal(np.asarray(plain['datasets'][1]), sets[1])
    pipe.close()
    assert pipe._writers == {} and pipe._zpool is None and pipe._zbufs == {}


def test_argument_errors_raise_before_gpu_work(tmp_path, case):
    from empanada_amd.inference.driver import infer_volume
    from empanada_amd.inference.pipeline import VolumePipeline
    from empanada_amd.zarr_utils import ZarrV2Group
    eng, vol, _, _, _ = case(('xy',))
    kw = {k: v for k, v in KW.items() if k != 'batch_pixels'}
    g = ZarrV2Group(str(tmp_path / 'g.zarr'))
    for bad in (0, 9, [(1, 1, 1)], [(2, 3, 2)], 'auto'):
        pipe = VolumePipeline(eng, tune=False)
        for extra in ({}, {'pipeline': pipe}, {'compressor': 'zlib'}):
            with pytest.raises(ValueError, match='pyramid'):
                infer_volume(eng, vol, out=g, pyramid=bad, **kw, **extra)
        assert pipe._streams is None and pipe._graphed is None and pipe._store == [None, None]
        assert pipe._writers == {} and pipe._zpool is None and pipe._zbufs == {}
    assert os.listdir(g.path) == ['.zgroup']


# ----------------------------------------------------------------------------------------------- two ranks over gloo
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank(rank, world, port, path, bad_path, q):
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        eng, vol = _engine(), SY.em_volume(SHAPE, seed=3)
        try:                                                # 20 % 8 != 0: both ranks refuse, before anything is written
            _run(eng, vol, bad_path, axes=ORTHO, group=dist.group.WORLD, pyramid=3)
            refused = None
        except ValueError as e:
            refused = str(e)
        res = _run(eng, vol, path, axes=ORTHO, group=dist.group.WORLD, pyramid=2)
        q.put((rank, refused, tuple(res['z_range']), [tuple(z) for z in res['pyramid_z_ranges']],
               {c: [_np(s) for s in res['pyramid'][c]] for c in res['pyramid']}, dict(res['instances'])))
    finally:
        dist.destroy_process_group()


def test_infer_volume_two_ranks(tmp_path, case):
    import torch.multiprocessing as mp
    from empanada_amd.zarr_utils import ZarrV2Group
    eng, vol, vols, sets, counts = case(ORTHO)
    one = _run(eng, vol, tmp_path / 'one.zarr', axes=ORTHO, pyramid=2)
    single = _assert_pyramid(one, tmp_path / 'one.zarr', vols, sets, counts, [(2, 2, 2)] * 2)
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    path, bad_path = str(tmp_path / 'two.zarr'), str(tmp_path / 'bad.zarr')
    procs = [ctx.Process(target=_rank, args=(r, 2, port, path, bad_path, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = {}
    while len(got) < 2:                                     # a rank that died is reported at once, not after a time limit
        try:
            item = q.get(timeout=1)
            got[item[0]] = item[1:]
        except queue.Empty:
            dead = [p.exitcode for p in procs if not p.is_alive() and p.exitcode != 0]
            assert not dead, f"a rank ended with exit code {dead[0]} before it reported"
            assert any(p.is_alive() for p in procs) or not q.empty(), "the ranks ended without reporting"
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for r in (0, 1):
        assert got[r][0] is not None and 'level 3' in got[r][0] and '[0, 20)' in got[r][0], got[r][0]
        assert got[r][4] == counts
    assert os.listdir(bad_path) == ['.zgroup']
    assert got[0][1] == (0, 20) and got[1][1] == (20, 40)
    assert got[0][2] == [(0, 10), (0, 5)] and got[1][2] == [(10, 20), (5, 10)]
    g = ZarrV2Group(path, mode='r')
    for c in (1, 2):
        np.testing.assert_array_equal(np.asarray(g[NAMES[c]]), sets[c], err_msg=f'dataset of class {c}')
        for l in (1, 2):
            np.testing.assert_array_equal(np.concatenate([got[0][3][c][l - 1], got[1][3][c][l - 1]], axis=0),
                                          single[c][l - 1], err_msg=f'class {c} level {l}')
            ds = g[f'{NAMES[c]}_s{l}']
            assert _files(ds) == [f'{z}.0.0' for z in range(single[c][l - 1].shape[0])]
            np.testing.assert_array_equal(np.asarray(ds), single[c][l - 1], err_msg=f'dataset {c} level {l}')
    assert g.attrs == {'multiscales': _expected_multiscales([(1, 1, 1), (2, 2, 2), (4, 4, 4)])}      # written once
