"""GPU: zlib streams of label slabs made on the device (csrc/emp_deflate.hip) -- _hip.deflate_labels,
ZarrV2Array.write_slab_device and infer_volume(..., compressor='zlib').  The checker is the standard library's zlib:
every chunk must inflate to the slice's bytes, end exactly at its last byte (the decoder verifies the Adler-32 itself)
and stay inside _hip.deflate_bound.  The engine and volume of the infer_volume cases are those of
tests/test_driver_gpu.py."""
import os
import queue
import socket
import zlib

import numpy as np
import pytest
import torch

from empanada_amd import synthetic as SY

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (2, 1, 3), (3, 3, 65), (2, 5, 130), (2, 2, 259), (2, 2, 261), (2, 4, 1031), (3, 64, 64)]
DTYPES = [np.uint8, np.uint32]
_CACHE = {}


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


def _check_stream(c, raw, item):
    d = zlib.decompressobj()
    got = d.decompress(bytes(c))
    assert got == raw
    assert d.eof
    assert d.unused_data == b''
    from empanada_amd import _hip
    assert len(c) <= _hip.deflate_bound(len(raw), item)


def _check(slab, data, offsets):
    """the four checks of every chunk, and the shape of (data, offsets); returns the chunks"""
    assert data.dtype == torch.uint8 and data.is_cuda and data.dim() == 1
    assert offsets.dtype == torch.int64 and not offsets.is_cuda and offsets.numel() == slab.shape[0] + 1
    offs = offsets.tolist()
    assert offs[0] == 0 and all(a <= b for a, b in zip(offs[:-1], offs[1:])) and data.numel() == offs[-1]
    host = data.cpu().numpy().tobytes()
    chunks = [host[a:b] for a, b in zip(offs[:-1], offs[1:])]
    for i, c in enumerate(chunks):
        _check_stream(c, slab[i].tobytes(), slab.dtype.itemsize)
    return chunks


def _content(kind, shape, dtype):
    n = int(np.prod(shape))
    rng = np.random.default_rng(n + np.dtype(dtype).itemsize)
    if kind == 'zeros':
        return np.zeros(shape, dtype)
    if kind == 'random':                                        # full range: all literals, 8- and 9-bit codes
        return rng.integers(0, np.iinfo(dtype).max, size=shape, dtype=dtype, endpoint=True)
    if kind == 'ones':
        return np.full(shape, np.iinfo(dtype).max, dtype)
    if kind == 'runs7':
        return (rng.integers(1, np.iinfo(dtype).max, size=n // 7 + 1, dtype=dtype).repeat(7)[:n]).reshape(shape)
    lab = _planted().ravel()                                    # from the middle of a labelled slice on
    return lab[3 * 65536 + 100 * 256:][:n].astype(dtype).reshape(shape)


@pytest.mark.parametrize('dtype', DTYPES, ids=['u8', 'u32'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_round_trip(shape, dtype):
    from empanada_amd import _hip
    for kind in ('zeros', 'random', 'ones', 'runs7', 'planted'):
        slab = _content(kind, shape, dtype)
        if kind == 'planted' and int(np.prod(shape)) > 4096:
            assert slab.any()
        _check(slab, *_hip.deflate_labels(_dev(slab)))


def test_int32_bits_are_taken_as_they_are():
    from empanada_amd import _hip
    slab = _content('runs7', (2, 5, 130), np.uint32)
    a = _check(slab, *_hip.deflate_labels(_dev(slab)))
    b = _check(slab, *_hip.deflate_labels(torch.from_numpy(slab.view(np.int32)).cuda()))
    assert a == b


@pytest.mark.parametrize('dtype', DTYPES, ids=['u8', 'u32'])
def test_every_split_of_a_repeat(dtype):
    """row r starts with r + 1 equal non-zero elements and one 255: repeats of every length -- 258 to 261 bytes and
    their multiples among them -- at every position relative to the segment borders (602 is no divisor of a segment)"""
    from empanada_amd import _hip
    slab = np.zeros((1, 600, 602), dtype)
    for r in range(600):
        slab[0, r, :r + 1] = r % 200 + 1
        slab[0, r, r + 1] = 255
    _check(slab, *_hip.deflate_labels(_dev(slab)))


@pytest.mark.parametrize('dtype', DTYPES, ids=['u8', 'u32'])
def test_chunks_are_independent_and_output_is_deterministic(dtype):
    from empanada_amd import _hip
    slab = _content('planted', (3, 64, 64), dtype)
    slab[1, 0, :9] = slab[0, -1, -1] = 7                       # chunk 1 starts with what chunk 0 ends with
    dev = _dev(slab)
    whole = _check(slab, *_hip.deflate_labels(dev))
    again = _check(slab, *_hip.deflate_labels(dev))
    assert whole == again
    alone = _check(slab[1:2], *_hip.deflate_labels(dev[1:2]))
    assert alone[0] == whole[1]


def test_slab_split_into_blocks_of_slices(monkeypatch):
    """a slab whose worst case passes the limit of one kernel call goes through in blocks: same bytes"""
    from empanada_amd import _hip
    slab = _content('planted', (5, 64, 64), np.uint32)
    dev = _dev(slab)
    whole = _check(slab, *_hip.deflate_labels(dev))
    monkeypatch.setattr(_hip, 'DEFLATE_MAX_BYTES', 2 * _hip.deflate_bound(64 * 64 * 4, 4) + 1)    # 2 + 2 + 1 slices
    assert _check(slab, *_hip.deflate_labels(dev)) == whole


def test_unaligned_slab_and_output():
    """a slab that starts 4 bytes (uint32) or 1 byte (uint8) off a 16-byte address takes the element-wise loads; an
    `out` that starts 3 bytes off takes the byte-wise ends of every segment's copy"""
    from empanada_amd import _hip
    for dtype, tdt in ((np.uint32, torch.int32), (np.uint8, torch.uint8)):
        slab = _content('planted', (2, 40, 64), dtype)
        flat = torch.zeros((slab.size + 16,), dtype=tdt, device='cuda')
        flat[1:1 + slab.size] = _dev(slab).view(tdt).ravel()
        dev = flat[1:1 + slab.size].view((2, 40, 64))
        assert dev.data_ptr() % 16 != 0 and dev.is_contiguous()
        ref = _check(slab, *_hip.deflate_labels(_dev(slab)))
        assert _check(slab, *_hip.deflate_labels(dev)) == ref
        store = torch.full((2 * _hip.deflate_bound(slab[0].nbytes, slab.itemsize) + 3,), 0xA5, dtype=torch.uint8, device='cuda')
        data, offs = _hip.deflate_labels(dev, out=store[3:])
        assert data.data_ptr() == store.data_ptr() + 3
        assert _check(slab, data, offs) == ref
        assert bool((store[:3] == 0xA5).all()) and bool((store[3 + int(offs[-1]):] == 0xA5).all())


def test_checksum_arithmetic():
    from empanada_amd import _hip
    first = np.full((1, 1, 5803), 255, np.uint8)               # the first length at which 32-bit Adler sums overflow
    _check(first, *_hip.deflate_labels(_dev(first)))
    big = np.full((1, 2048, 2048), 0xFFFFFFFF, np.uint32)      # 16 MiB: 4096 segments' sums combined mod 65521
    _check(big, *_hip.deflate_labels(_dev(big)))


def test_no_stray_writes():
    from empanada_amd import _hip
    slab = _content('planted', (3, 64, 64), np.uint32)
    dev = _dev(slab)
    data, offs = _hip.deflate_labels(dev)
    total = int(offs[-1])
    out = torch.full((total + 4096,), 0xA5, dtype=torch.uint8, device='cuda')
    data2, offs2 = _hip.deflate_labels(dev, out=out)
    assert data2.data_ptr() == out.data_ptr() and data2.numel() == total and torch.equal(offs, offs2)
    assert torch.equal(data2, data)
    assert bool((out[total:] == 0xA5).all())
    with pytest.raises(ValueError, match='out holds'):
        _hip.deflate_labels(dev, out=out[:total - 1])
    for bad in (out.cpu(), out.view(torch.int8), out[::2], out[:total // 2 * 2].view(2, -1)):
        with pytest.raises(_hip.HipError):
            _hip.deflate_labels(dev, out=bad)
    for bad in (dev.cpu(), dev.view(torch.float32), dev[:, :, ::2], dev[0]):
        with pytest.raises(_hip.HipError):
            _hip.deflate_labels(bad)


def test_it_compresses():
    from empanada_amd import _hip
    lab = _planted()
    for slab in (lab.astype(np.uint32), (lab > 0).astype(np.uint8)):
        _, offs = _hip.deflate_labels(_dev(slab))
        ref = sum(len(zlib.compress(slab[i].tobytes(), 1)) for i in range(slab.shape[0]))
        print(f"planted {slab.dtype}: {int(offs[-1])} bytes, zlib level 1 {ref}, raw {slab.nbytes}")
        assert int(offs[-1]) <= 2 * ref
    zero = torch.zeros((4, 512, 512), dtype=torch.int32, device='cuda')
    _, offs = _hip.deflate_labels(zero)
    print(f"zeros (4, 512, 512) uint32: {int(offs[-1])} bytes")
    assert 50 * int(offs[-1]) <= 4 * 512 * 512 * 4


# ------------------------------------------------------------------------------------------------------ the writer
def _files(array):
    return sorted((f for f in os.listdir(array.path) if not f.startswith('.')), key=lambda s: int(s.split('.')[0]))


def _check_files(array, expect=None):
    """every chunk file of a (1, Y, X)-chunked array is a valid stream of its slice; returns the bytes on disk"""
    data = np.asarray(array[...]) if expect is None else expect
    total = 0
    for f in _files(array):
        with open(os.path.join(array.path, f), 'rb') as fh:
            c = fh.read()
        _check_stream(c, data[int(f.split('.')[0])].tobytes(), data.dtype.itemsize)
        total += len(c)
    return total


@pytest.mark.parametrize('dtype', DTYPES, ids=['u8', 'u32'])
@pytest.mark.parametrize('pooled', [False, True])
def test_write_slab_device(tmp_path, dtype, pooled):
    import json
    from concurrent.futures import ThreadPoolExecutor
    from empanada_amd.zarr_utils import ZarrV2Group, open_zarr
    slab = _content('planted', (5, 40, 72), dtype)
    g = ZarrV2Group(str(tmp_path / 'g.zarr'))
    ds = g.create_dataset('labels', shape=(8, 40, 72), dtype=dtype, chunks=(1, None, None), compressor=1)
    pool = ThreadPoolExecutor(max_workers=4) if pooled else None
    futures, nbytes = ds.write_slab_device(2, _dev(slab), pool)
    assert len(futures) == (5 if pooled else 0)
    for f in futures:
        f.result()
    if pool is not None:
        pool.shutdown()
    full = np.zeros((8, 40, 72), dtype)
    full[2:7] = slab
    np.testing.assert_array_equal(np.asarray(ds), full)
    np.testing.assert_array_equal(np.asarray(open_zarr(str(tmp_path / 'g.zarr'))['labels']), full)
    assert _files(ds) == [f'{z}.0.0' for z in range(2, 7)]
    assert _check_files(ds, full) == nbytes
    with open(os.path.join(ds.path, '.zarray')) as fh:
        assert json.load(fh)['compressor'] == {'id': 'zlib', 'level': 1}


def test_write_slab_device_refusals(tmp_path):
    from empanada_amd.zarr_utils import ZarrV2Group
    g = ZarrV2Group(str(tmp_path / 'g.zarr'))
    dev = torch.zeros((2, 6, 10), dtype=torch.int32, device='cuda')
    kw = dict(shape=(4, 6, 10), chunks=(1, None, None), compressor=1)
    with pytest.raises(ValueError, match='compressor'):
        g.create_dataset('raw', shape=(4, 6, 10), dtype=np.uint32, chunks=(1, None, None)).write_slab_device(0, dev)
    with pytest.raises(ValueError, match='chunks'):
        g.create_dataset('rows', shape=(4, 6, 10), dtype=np.uint32, chunks=(1, 3, None), compressor=1).write_slab_device(0, dev)
    with pytest.raises(ValueError, match='little-endian'):
        g.create_dataset('u2', dtype=np.uint16, **kw).write_slab_device(0, dev.to(torch.int16))
    ok = g.create_dataset('ok', dtype=np.uint32, **kw)
    for z0, bad in ((0, dev.to(torch.uint8)), (0, dev[:, :, :5]), (0, dev[:, :5]), (3, dev), (-1, dev), (0, dev[0])):
        with pytest.raises(ValueError):
            ok.write_slab_device(z0, bad)
    assert _files(ok) == []


# ------------------------------------------------------------------------------------------------------ infer_volume
NORMS = dict(mean=0.508979, std=0.148561)
ORTHO = ('xy', 'xz', 'yz')
KW = dict(norms=NORMS, labels=[1, 2], min_size=30, min_span=2, class_names={1: 'mito', 2: 'er'}, batch_pixels=1 << 22)
SHAPE = (40, 72, 88)


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


def _np(v):
    return v.view(torch.int32).cpu().numpy().view(np.uint32) if v.dtype == torch.uint32 else v.cpu().numpy()


def _run(engine, vol, path, **kw):
    from empanada_amd.inference.driver import infer_volume
    from empanada_amd.zarr_utils import ZarrV2Group
    return infer_volume(engine, vol, out=ZarrV2Group(str(path)), **dict(KW, **kw))


@pytest.fixture
def case(tmp_path_factory):
    """(engine, volume, the plain call's volumes and dataset contents) per axes: computed once, shared, never modified"""
    def get(axes):
        if axes not in _CACHE:
            eng = _CACHE['engine'] = _CACHE.get('engine') or _engine()
            vol = SY.em_volume(SHAPE, seed=3)
            res = _run(eng, vol, tmp_path_factory.mktemp('plain') / 'pred.zarr', axes=axes)
            assert 'compressed_bytes' not in res
            assert all(a.codec is None for a in res['datasets'].values())
            vols = {c: _np(v) for c, v in res['volumes'].items()}
            assert vols[1].max() > 0 or vols[2].max() > 0, "the random model should segment something"
            _CACHE[axes] = (eng, vol, vols, {c: np.asarray(a[...]) for c, a in res['datasets'].items()},
                            dict(res['instances']))
        return _CACHE[axes]
    return get


def _assert_compressed_equals_plain(res, exp_vols, exp_sets, exp_counts):
    assert dict(res['instances']) == exp_counts and tuple(res['z_range']) == (0, SHAPE[0])
    assert sorted(res['compressed_bytes']) == sorted(exp_vols)
    on_disk = 0
    for c in exp_vols:
        got = _np(res['volumes'][c])
        assert got.dtype == exp_vols[c].dtype
        np.testing.assert_array_equal(got, exp_vols[c], err_msg=f'class {c}')
        ds = res['datasets'][c]
        assert ds.meta['compressor'] == {'id': 'zlib', 'level': 1} and ds.dtype == exp_sets[c].dtype
        assert tuple(ds.chunks) == (1,) + SHAPE[1:]
        np.testing.assert_array_equal(np.asarray(ds), exp_sets[c], err_msg=f'dataset of class {c}')
        assert len(_files(ds)) == SHAPE[0]
        n = _check_files(ds, exp_sets[c])
        assert n == res['compressed_bytes'][c]
        on_disk += n
    assert sum(res['compressed_bytes'].values()) == on_disk


@pytest.mark.parametrize('axes', [('xy',), ORTHO], ids=['stack', 'ortho'])
def test_infer_volume_plain_path(tmp_path, case, axes):
    eng, vol, vols, sets, counts = case(axes)
    res = _run(eng, vol, tmp_path / 'z.zarr', axes=axes, compressor='zlib')
    _assert_compressed_equals_plain(res, vols, sets, counts)


def test_infer_volume_windowed(tmp_path, case):
    eng, vol, _, _, _ = case(('xy',))
    kw = dict(axes=('xy',), batch_pixels=4 * 96 * 96, window_slices=8)      # 4 slices per model call, windows of 8
    plain = _run(eng, vol, tmp_path / 'raw.zarr', **kw)
    assert 'compressed_bytes' not in plain
    res = _run(eng, vol, tmp_path / 'z.zarr', compressor='zlib', **kw)
    assert res['windows']['xy'] > 1
    _assert_compressed_equals_plain(res, {c: _np(v) for c, v in plain['volumes'].items()},
                                    {c: np.asarray(a[...]) for c, a in plain['datasets'].items()}, dict(plain['instances']))


def test_infer_volume_pipeline(tmp_path, case):
    from empanada_amd.inference.pipeline import VolumePipeline
    eng, vol, vols, sets, counts = case(ORTHO)
    pipe = VolumePipeline(eng, tune=False, graph=True, overlap=True, batch_pixels=1 << 22)
    res = _run(eng, vol, tmp_path / 'z.zarr', axes=ORTHO, compressor='zlib', pipeline=pipe)
    _assert_compressed_equals_plain(res, vols, sets, counts)
    assert res['pipeline']['graph'] is True
    held = {c: b.numel() for c, b in pipe._zbufs.items()}
    assert held == res['compressed_bytes'] and all(b.is_pinned() for b in pipe._zbufs.values())
    res = _run(eng, vol, tmp_path / 'again.zarr', axes=ORTHO, compressor='zlib', pipeline=pipe)
    _assert_compressed_equals_plain(res, vols, sets, counts)
    assert {c: b.numel() for c, b in pipe._zbufs.items()} == held          # kept: it only grows
    plain = _run(eng, vol, tmp_path / 'raw.zarr', axes=ORTHO, pipeline=pipe)
    assert 'compressed_bytes' not in plain and plain['datasets'][1].codec is None
    np.testing.assert_array_equal(np.asarray(plain['datasets'][1]), sets[1])
    pipe.close()
    assert pipe._zpool is None and pipe._zbufs == {}


def test_argument_errors_raise_before_gpu_work(tmp_path, case):
    from empanada_amd.inference.driver import infer_volume
    from empanada_amd.inference.pipeline import VolumePipeline
    from empanada_amd.zarr_utils import ZarrV2Group
    eng, vol, _, _, _ = case(('xy',))
    kw = {k: v for k, v in KW.items() if k != 'batch_pixels'}
    g = ZarrV2Group(str(tmp_path / 'g.zarr'))
    for bad, word in ((dict(out=g, compressor='gzip'), 'compressor'), (dict(compressor='zlib'), 'out='),
                      (dict(out={}, compressor='zlib'), 'ZarrV2Group')):
        pipe = VolumePipeline(eng, tune=False)
        for extra in ({}, {'pipeline': pipe}):
            with pytest.raises(ValueError, match=word):
                infer_volume(eng, vol, **kw, **bad, **extra)
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


def _rank(rank, world, port, path, q):
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        res = _run(_engine(), SY.em_volume(SHAPE, seed=3), path, axes=ORTHO, group=dist.group.WORLD, compressor='zlib')
        q.put((rank, tuple(res['z_range']), dict(res['compressed_bytes']), {c: _np(v) for c, v in res['volumes'].items()},
               dict(res['instances'])))
    finally:
        dist.destroy_process_group()


def test_infer_volume_two_ranks(tmp_path, case):
    import torch.multiprocessing as mp
    from empanada_amd.zarr_utils import ZarrV2Group
    _, _, vols, sets, counts = case(ORTHO)
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    path = str(tmp_path / 'z.zarr')
    procs = [ctx.Process(target=_rank, args=(r, 2, port, path, q)) for r in range(2)]
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
    assert got[0][0] == (0, 20) and got[1][0] == (20, 40) and got[0][3] == got[1][3] == counts
    g = ZarrV2Group(path)
    for c, name in ((1, 'mito_pred'), (2, 'er_pred')):
        np.testing.assert_array_equal(np.concatenate([got[0][2][c], got[1][2][c]], axis=0), vols[c], err_msg=f'class {c}')
        ds = g[name]
        assert ds.meta['compressor'] == {'id': 'zlib', 'level': 1}
        np.testing.assert_array_equal(np.asarray(ds), sets[c], err_msg=f'dataset of class {c}')
        assert len(_files(ds)) == SHAPE[0]
        assert _check_files(ds, sets[c]) == got[0][1][c] + got[1][1][c]
        for r, (z0, z1) in ((0, (0, 20)), (1, (20, 40))):   # each rank counted its own files
            assert got[r][1][c] == sum(os.path.getsize(os.path.join(ds.path, f'{z}.0.0')) for z in range(z0, z1))
