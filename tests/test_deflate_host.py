"""CPU: argument checks of the device deflate coder (csrc/emp_deflate.hip), its bound, and the refusals of
ZarrV2Array.write_slab_device / infer_volume(compressor=) that need no device.  Every refusal of the C entries comes
back as EMP_EINVAL before any launch; the pointers handed over are host buffers that are never read."""
import ctypes

import numpy as np
import pytest
import torch

EINVAL = -1
SEG = 4096


@pytest.fixture(scope='module')
def lib():
    from empanada_amd import _hip
    return _hip.load()


@pytest.fixture(scope='module')
def buf():
    b = ctypes.create_string_buffer(1 << 16)
    return ctypes.addressof(b), b


def _bound(L):
    return 2 + -(-9 * L // 8) + 8 * -(-L // SEG) + 6


def test_bound_is_the_formula(lib):
    from empanada_amd import _hip
    for L in (1, 2, 3, 7, 8, 9, 4095, 4096, 4097, 8192, 65 * 3, 1024 * 1024, 4 * 1024 * 1024, 4 * 2048 * 2048 + 4):
        assert _hip.deflate_bound(L, 1) == _bound(L), L
        if L % 4 == 0:
            assert _hip.deflate_bound(L, 4) == _bound(L), L
    for L, item, word in ((8, 2, b'item'), (8, 0, b'item'), (0, 1, b'chunk size'), (-4, 4, b'chunk size'),
                          (6, 4, b'chunk size')):
        assert lib.emp_deflate_bound(L, item) == EINVAL, (L, item)
        assert word in lib.emp_last_error(), (L, item, lib.emp_last_error())
    with pytest.raises(ValueError, match='item'):
        _hip.deflate_bound(16, 3)


def test_work_bytes_query(lib):
    small = lib.emp_deflate_work_bytes(2, 4096, 4)
    assert 0 < small < lib.emp_deflate_work_bytes(2, 1 << 20, 4) < lib.emp_deflate_work_bytes(8, 1 << 20, 4)
    for args, word in (((0, 4096, 4), b'shape'), ((2, 4096, 3), b'item'), ((2, 4098, 4), b'shape'), ((2, 0, 1), b'shape'),
                       ((2 ** 20, 1 << 20, 1), b'2^31'), ((1, 1 << 31, 1), b'2^31')):
        assert lib.emp_deflate_work_bytes(*args) == EINVAL, args
        assert word in lib.emp_last_error(), (args, lib.emp_last_error())


def test_count_refuses_bad_arguments(lib, buf):
    a, _ = buf
    need = lib.emp_deflate_work_bytes(3, 4096 + 64, 4)
    assert 0 < need <= 1 << 16
    good = dict(src=a, item=4, n=3, L=4096 + 64, work=a, wb=need, offs=a)

    def call(**kw):
        v = {**good, **kw}
        return lib.emp_deflate_count(v['src'], v['item'], v['n'], v['L'], v['work'], v['wb'], v['offs'], None)

    for kw, word in ((dict(src=None), b'null'), (dict(work=None), b'null'), (dict(offs=None), b'null'),
                     (dict(item=2), b'item'), (dict(item=0), b'item'), (dict(item=8), b'item'), (dict(n=0), b'shape'),
                     (dict(n=-1), b'shape'), (dict(L=0), b'shape'), (dict(L=4098), b'shape'), (dict(L=-4), b'shape'),
                     (dict(wb=need - 1), b'workspace'), (dict(wb=0), b'workspace'), (dict(src=a + 2), b'misaligned'),
                     (dict(n=2 ** 12, L=1 << 20, wb=1 << 40), b'2^31'), (dict(n=1, L=1 << 31, wb=1 << 40), b'2^31')):
        assert call(**kw) == EINVAL, kw
        assert word in lib.emp_last_error(), (kw, lib.emp_last_error())


def test_encode_refuses_bad_arguments(lib, buf):
    a, _ = buf
    need = lib.emp_deflate_work_bytes(3, 500, 1)
    assert 0 < need <= 1 << 16
    good = dict(src=a, item=1, n=3, L=500, work=a, wb=need, total=300, out=a, ob=300)

    def call(**kw):
        v = {**good, **kw}
        return lib.emp_deflate_encode(v['src'], v['item'], v['n'], v['L'], v['work'], v['wb'], v['total'], v['out'],
                                      v['ob'], None)

    for kw, word in ((dict(src=None), b'null'), (dict(work=None), b'null'), (dict(out=None), b'null'),
                     (dict(item=3), b'item'), (dict(n=0), b'shape'), (dict(L=0), b'shape'),
                     (dict(item=4, L=502), b'shape'), (dict(item=4, L=500, src=a + 1), b'misaligned'),
                     (dict(wb=need - 1), b'workspace'), (dict(total=-1), b'total'),
                     (dict(total=3 * _bound(500) + 1, ob=1 << 20), b'total'), (dict(ob=299), b'too small'),
                     (dict(n=2 ** 12, L=1 << 20, wb=1 << 40), b'2^31')):
        assert call(**kw) == EINVAL, kw
        assert word in lib.emp_last_error(), (kw, lib.emp_last_error())


def test_wrapper_needs_a_gpu_and_a_device_slab():
    from empanada_amd import _hip
    if not torch.cuda.is_available():
        with pytest.raises(_hip.HipError):
            _hip.deflate_labels(torch.zeros((2, 3, 4), dtype=torch.uint8))


def _group(tmp_path):
    from empanada_amd.zarr_utils import ZarrV2Group
    return ZarrV2Group(str(tmp_path / 'g.zarr'))


def test_write_slab_device_refusals_without_a_device(tmp_path):
    g = _group(tmp_path)
    host = torch.zeros((2, 6, 10), dtype=torch.int32)
    ok = g.create_dataset('ok', shape=(4, 6, 10), dtype=np.uint32, chunks=(1, None, None), compressor=1)
    assert ok.meta['compressor'] == {'id': 'zlib', 'level': 1}
    with pytest.raises(ValueError, match='on the GPU'):          # a host tensor, a numpy array: write_slab's business
        ok.write_slab_device(0, host)
    with pytest.raises(ValueError, match='on the GPU'):
        ok.write_slab_device(0, host.numpy())
    raw = g.create_dataset('raw', shape=(4, 6, 10), dtype=np.uint32, chunks=(1, None, None))
    with pytest.raises(ValueError, match='compressor'):
        raw.write_slab_device(0, host)
    gz = g.create_dataset('gz', shape=(4, 6, 10), dtype=np.uint32, chunks=(1, None, None),
                          compressor={'id': 'gzip', 'level': 1})
    with pytest.raises(ValueError, match='compressor'):
        gz.write_slab_device(0, host)
    for name, chunks in (('rows', (1, 3, None)), ('pairs', (2, None, None))):
        with pytest.raises(ValueError, match='chunks'):
            g.create_dataset(name, shape=(4, 6, 10), dtype=np.uint32, chunks=chunks, compressor=1).write_slab_device(0, host)
    with pytest.raises(ValueError, match='chunks'):
        g.create_dataset('flat', shape=(4, 60), dtype=np.uint32, chunks=(1, None), compressor=1).write_slab_device(0, host)
    for name, dt in (('u2', np.uint16), ('u8', np.uint64), ('f4', np.float32), ('be', '>u4')):
        with pytest.raises(ValueError, match='little-endian'):
            g.create_dataset(name, shape=(4, 6, 10), dtype=dt, chunks=(1, None, None), compressor=1).write_slab_device(0, host)
    assert not any(f for f in (tmp_path / 'g.zarr' / 'ok').iterdir() if f.name != '.zarray')   # nothing was written


def test_infer_volume_compressor_errors_come_first(tmp_path):
    """before the engine, the volume or the GPU are looked at: placeholders are enough"""
    from empanada_amd.inference.driver import infer_volume

    class Engine:
        thing_list = [1]
        label_divisor = 1000

    kw = dict(norms=dict(mean=0.5, std=0.1), labels=[1])
    with pytest.raises(ValueError, match='compressor'):
        infer_volume(Engine(), None, out=_group(tmp_path), compressor='blosc', **kw)
    with pytest.raises(ValueError, match='compressor'):
        infer_volume(Engine(), None, out=_group(tmp_path), compressor=1, **kw)
    with pytest.raises(ValueError, match='out='):
        infer_volume(Engine(), None, compressor='zlib', **kw)
    with pytest.raises(ValueError, match='ZarrV2Group'):
        infer_volume(Engine(), None, out={}, compressor='zlib', **kw)
