"""CPU: the checker of the label morphology (include/emp_hip.h, E5) -- the inside distance label by label with scipy,
erode and dilate by numpy shifts over the ball's offsets -- checked against the brute-force definition and against
scipy's binary morphology, and the host logic: morphology.check, the argument errors of _hip.label_edt / label_erode /
label_dilate, and sharded.neighbour_slabs over three gloo ranks."""
import math
import os
import queue
import socket
import time

import numpy as np
import pytest
import torch

from empanada_amd import morphology as MO
from test_holes_host import planted_volume

SAMPLINGS = [(1, 1, 1), (3, 1, 1), (1, 2, 1)]
R2S = [1, 2, 3, 4, 9, 25]


# ------------------------------------------------------------------------------------------------------ the checker
def ball(r2, sampling=(1, 1, 1)):
    """[(dz, dy, dx, d2)] of the offsets with 0 < d2 <= r2"""
    reach = [math.isqrt(int(r2)) // a for a in sampling]
    out = []
    for dz in range(-reach[0], reach[0] + 1):
        for dy in range(-reach[1], reach[1] + 1):
            for dx in range(-reach[2], reach[2] + 1):
                d2 = (sampling[0] * dz) ** 2 + (sampling[1] * dy) ** 2 + (sampling[2] * dx) ** 2
                if 0 < d2 <= r2:
                    out.append((dz, dy, dx, d2))
    return out


def shifted(lab, off):
    """(S, V): S[v] = lab[v + off] where v + off lies inside the volume -- V marks those -- and 0 elsewhere"""
    S = np.zeros_like(lab)
    V = np.zeros(lab.shape, bool)
    src, dst = [], []
    for n, o in zip(lab.shape, off):
        lo, hi = max(0, -o), min(n, n - o)
        if hi <= lo:
            return S, V
        dst.append(slice(lo, hi))
        src.append(slice(lo + o, hi + o))
    S[tuple(dst)] = lab[tuple(src)]
    V[tuple(dst)] = True
    return S, V


def edt_ref(lab, sampling=(1, 1, 1), cap=65535):
    """the capped squared inside distance, label by label with scipy's exact transform; a label that fills the whole
    volume has no candidate and gives cap"""
    from scipy.ndimage import distance_transform_edt
    lab = np.asarray(lab)
    out = np.zeros(lab.shape, np.int64)
    for l in np.unique(lab):
        if l == 0:
            continue
        mask = lab == l
        if mask.all():
            out[mask] = cap
            continue
        d = distance_transform_edt(mask, sampling=[float(a) for a in sampling])
        out[mask] = np.minimum(cap, np.rint(d[mask] ** 2).astype(np.int64))
    return out.astype(np.uint16)


def edt_brute(lab, sampling=(1, 1, 1), cap=65535):
    """the definition, voxel against voxel"""
    lab = np.asarray(lab)
    pos = np.argwhere(np.ones(lab.shape, bool)).astype(np.int64) * np.asarray(sampling, np.int64)
    flat = lab.ravel()
    out = np.zeros(flat.shape, np.int64)
    for i in np.flatnonzero(flat):
        other = flat != flat[i]
        out[i] = min(cap, int(((pos[other] - pos[i]) ** 2).sum(axis=1).min())) if other.any() else cap
    return out.reshape(lab.shape).astype(np.uint16)


def erode_ref(lab, r2, sampling=(1, 1, 1)):
    lab = np.asarray(lab)
    keep = lab != 0
    for dz, dy, dx, _ in ball(r2, sampling):
        S, V = shifted(lab, (dz, dy, dx))
        keep &= ~V | (S == lab)                                 # a position outside the volume is no candidate
    return np.where(keep, lab, 0).astype(lab.dtype)


def dilate_ref(lab, r2, sampling=(1, 1, 1)):
    lab = np.asarray(lab)
    wide = lab.astype(np.uint32).astype(np.int64) if lab.dtype != np.int32 else lab.view(np.uint32).astype(np.int64)
    best_d = np.full(lab.shape, r2 + 1, np.int64)
    best_l = np.zeros(lab.shape, np.int64)
    for dz, dy, dx, d2 in ball(r2, sampling):
        S, V = shifted(wide, (dz, dy, dx))
        better = V & (S != 0) & ((d2 < best_d) | ((d2 == best_d) & (S > best_l)))
        best_d[better] = d2
        best_l[better] = S[better]
    return np.where(wide != 0, wide, best_l).astype(np.uint32).astype(lab.dtype)


def open_ref(lab, r2, sampling=(1, 1, 1)):
    return dilate_ref(erode_ref(lab, r2, sampling), r2, sampling)


def close_ref(lab, r2, sampling=(1, 1, 1)):
    lab = np.asarray(lab)
    return np.where(lab != 0, lab, erode_ref(dilate_ref(lab, r2, sampling), r2, sampling)).astype(lab.dtype)


REFS = dict(erode=erode_ref, dilate=dilate_ref, open=open_ref, close=close_ref)


def morph_ref(lab, morph):
    """what infer_volume(morph=) makes of a thing class's volume"""
    op, r2, sampling = MO.check(morph)
    return REFS[op](lab, r2, sampling)


def blobs(shape, dtype=np.uint32, seed=0):
    """a few solid boxes of distinct labels, some touching or overlapping, with single voxels punched out and single
    voxels of one more label: objects thick enough for something to survive an erosion by two or three voxels"""
    rng = np.random.default_rng(seed)
    v = np.zeros(shape, dtype)
    top = int(np.iinfo(dtype).max)
    for k in range(5):
        lo = [int(rng.integers(0, max(1, n - 2))) for n in shape]
        hi = [min(n, a + int(rng.integers(3, 12))) for n, a in zip(shape, lo)]
        v[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = [3, 7, 200, top, 9][k]
    v[rng.random(shape) < 0.004] = 0
    v[rng.random(shape) < 0.004] = 5
    return v


def structure(r2, sampling):
    reach = [math.isqrt(int(r2)) // a for a in sampling]
    s = np.zeros([2 * k + 1 for k in reach], bool)
    s[tuple(reach)] = True
    for dz, dy, dx, _ in ball(r2, sampling):
        s[reach[0] + dz, reach[1] + dy, reach[2] + dx] = True
    return s


# ------------------------------------------------------------------------------------------ the checker's own checks
@pytest.mark.parametrize('sampling', SAMPLINGS, ids=str)
def test_edt_ref_equals_the_definition_and_scipy(sampling):
    from scipy.ndimage import distance_transform_edt
    for shape, seed in (((5, 6, 9), 0), ((1, 7, 8), 1), ((4, 5, 1), 2)):
        for vol in (planted_volume(shape, np.uint32, seed), blobs(shape, np.uint8, seed)):
            for cap in (2, 10, 65535):
                np.testing.assert_array_equal(edt_ref(vol, sampling, cap), edt_brute(vol, sampling, cap))
        binary = (planted_volume(shape, np.uint8, seed) > 0).astype(np.uint8)
        if not binary.all():
            d = distance_transform_edt(binary, sampling=sampling)
            np.testing.assert_array_equal(edt_ref(binary, sampling), np.rint(d ** 2).astype(np.uint16))
    solid = np.full((3, 4, 5), 9, np.uint32)                    # the label that fills the volume: cap
    for cap in (1, 77, 65535):
        assert (edt_ref(solid, sampling, cap) == cap).all() and (edt_brute(solid, sampling, cap) == cap).all()


@pytest.mark.parametrize('sampling', SAMPLINGS, ids=str)
def test_erode_ref_is_the_threshold_of_the_distance(sampling):
    for seed in (0, 1):
        vol = planted_volume((6, 9, 11), np.uint32, seed)
        for r2 in R2S:
            if r2 < min(sampling) ** 2:
                continue
            want = np.where(edt_ref(vol, sampling, r2 + 1) > r2, vol, 0)
            np.testing.assert_array_equal(erode_ref(vol, r2, sampling), want)


@pytest.mark.parametrize('sampling', SAMPLINGS, ids=str)
def test_open_ref_is_the_binary_opening_of_every_label_and_close_ref_keeps_the_originals(sampling):
    from scipy.ndimage import binary_dilation, binary_erosion
    for vol in (planted_volume((7, 10, 12), np.uint32, 3), blobs((8, 12, 14), np.uint32, 4)):
        for r2 in (1, 2, 3, 4, 9):
            if r2 < min(sampling) ** 2:
                continue
            s = structure(r2, sampling)
            got = open_ref(vol, r2, sampling)
            for l in np.unique(vol[vol != 0]):
                want = binary_dilation(binary_erosion(vol == l, s, border_value=1), s)
                np.testing.assert_array_equal(got == l, want, err_msg=f'label {l}, r2 {r2}')
            assert ((got == vol) | (got == 0)).all()            # no voxel changes to another label
            closed = close_ref(vol, r2, sampling)
            assert (closed[vol != 0] == vol[vol != 0]).all()
            grown = dilate_ref(vol, r2, sampling)
            assert (grown[vol != 0] == vol[vol != 0]).all() and ((closed == 0) | (closed == grown)).all()


def test_dilate_ref_takes_the_nearest_and_among_equals_the_largest():
    v = np.zeros((1, 1, 7), np.uint32)
    v[0, 0, 1], v[0, 0, 5] = 3, 7
    assert dilate_ref(v, 4)[0, 0].tolist() == [3, 3, 3, 7, 7, 7, 7]
    v[0, 0, 5], v[0, 0, 6] = 0, 7
    assert dilate_ref(v, 9)[0, 0].tolist() == [3, 3, 3, 3, 7, 7, 7]
    v[0, 0, 1] = 0xffffffff
    assert dilate_ref(v, 4)[0, 0].tolist() == [0xffffffff] * 4 + [7, 7, 7]


# ------------------------------------------------------------------------------------------------------ morphology.check
def test_check_accepts():
    assert MO.check(None) is None
    assert MO.check(('erode', 1)) == ('erode', 1, (1, 1, 1))
    assert MO.check(['dilate', math.sqrt(2)]) == ('dilate', 2, (1, 1, 1))
    assert MO.check(('open', math.sqrt(3))) == ('open', 3, (1, 1, 1))
    assert MO.check(('close', 1.5, (2, 1, 1))) == ('close', 2, (2, 1, 1))
    assert MO.check(('open', np.float32(2.0), np.array([3, 1, 1]))) == ('open', 4, (3, 1, 1))
    assert MO.check(('erode', 3, (3, 3, 3))) == ('erode', 9, (3, 3, 3))
    assert MO.check(('erode', math.sqrt(65534))) == ('erode', 65534, (1, 1, 1))
    assert MO.halo_slices('erode', 9, (3, 1, 1)) == 1 and MO.halo_slices('open', 25) == 10
    assert MO.halo_slices('dilate', 3, (2, 1, 1)) == 0


@pytest.mark.parametrize('bad', [
    'open', ('open',), ('open', 1, (1, 1, 1), 2), ('thin', 1), (1, 'open'), ('open', True), ('open', '1'), ('open', None),
    ('open', 0), ('open', -1), ('open', float('nan')), ('open', float('inf')), ('open', 0.9), ('open', 256),
    ('open', 1, (1, 1)), ('open', 1, (0, 1, 1)), ('open', 1, (17, 1, 1)), ('open', 1, (1.0, 1, 1)), ('open', 1, (True, 1, 1)),
    ('open', 1, 1), ('open', 1.9, (2, 2, 2)), {'op': 'open'}, 3])
def test_check_rejects(bad):
    with pytest.raises(ValueError, match='morph'):
        MO.check(bad)


def test_infer_volume_checks_morph_before_any_work():
    from empanada_amd.inference import driver
    assert driver._check_morph(None) is None and driver._check_morph(('open', 1)) == ('open', 1, (1, 1, 1))
    with pytest.raises(ValueError, match='morph'):
        driver._check_morph(('open', 0))


# ------------------------------------------------------------------------------------------------------ _hip without a GPU
def test_argument_errors_are_raised_without_a_gpu():
    from empanada_amd import _hip
    cpu = torch.zeros((3, 4, 5), dtype=torch.uint8)
    for fn, args in ((_hip.label_edt, ()), (_hip.label_erode, (1,)), (_hip.label_dilate, (1,))):
        with pytest.raises(ValueError, match='GPU'):
            fn(cpu, *args)
        with pytest.raises(ValueError, match='GPU'):
            fn(np.zeros((3, 4, 5), np.uint8), *args)
        for sampling in ((1, 1), (0, 1, 1), (1, 17, 1), (1.0, 1, 1), (True, 1, 1), 1, None):
            with pytest.raises(ValueError, match='sampling'):
                fn(cpu, *args, sampling=sampling)
        with pytest.raises(ValueError, match='block_voxels'):
            fn(cpu, *args, block_voxels=0)
        with pytest.raises(ValueError, match='block_voxels'):
            fn(cpu, *args, block_voxels=2 ** 31)
    for cap in (0, 65536, 1.5, True, None):
        with pytest.raises(ValueError, match='cap'):
            _hip.label_edt(cpu, cap=cap)
    for fn in (_hip.label_erode, _hip.label_dilate):
        for r2 in (0, 65535, -1, 1.0, True, None):
            with pytest.raises(ValueError, match='r2'):
                fn(cpu, r2)
        with pytest.raises(ValueError, match='point'):
            fn(cpu, 3, sampling=(2, 2, 2))


# ------------------------------------------------------------------------------------------------------ neighbour_slabs
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, bounds, ns, q):
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        from empanada_amd.inference import sharded
        out = []
        for dtype in (torch.uint8, torch.uint32):
            for b in bounds:
                vol = _slab_volume(b[-1], dtype)
                slab = vol[b[rank]:b[rank + 1]].contiguous()
                for n in ns:
                    lo, hi = sharded.neighbour_slabs(slab, n, dist.group.WORLD)
                    out.append(tuple(None if t is None else (str(t.dtype), t.is_contiguous(), _host(t)) for t in (lo, hi)))
        q.put((rank, out))
    finally:
        dist.destroy_process_group()


def _host(t):
    return (t.view(torch.int32) if t.dtype == torch.uint32 else t).numpy().copy()


def _slab_volume(depth, dtype):
    v = torch.arange(depth * 2 * 3, dtype=torch.int32).reshape(depth, 2, 3) + 1
    return v.to(torch.uint8) if dtype == torch.uint8 else v.view(torch.uint32)


def test_neighbour_slabs_over_three_ranks():
    """depths of 0 and depths below n among the ranks: the slices come from the nearest ranks outward and are short
    only at the volume's ends"""
    import torch.multiprocessing as mp
    from empanada_amd.inference import sharded
    bounds = [(0, 4, 8, 12), (0, 1, 2, 9), (0, 0, 3, 5), (0, 5, 5, 6), (0, 0, 0, 4), (0, 2, 2, 2)]
    ns = (0, 1, 2, 3, 7)
    assert sharded.neighbour_slabs(_slab_volume(4, torch.uint8), 2) == (None, None)      # no process group
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 3, port, bounds, ns, q)) for r in range(3)]
    for p in procs:
        p.start()
    got, deadline = {}, time.monotonic() + 120
    try:
        while len(got) < 3:
            try:
                rank, out = q.get(timeout=1)
                got[rank] = out
            except queue.Empty:
                dead = [p.exitcode for p in procs if not p.is_alive() and p.exitcode != 0]
                assert not dead, f"a rank ended with exit code {dead[0]} before it reported"
                assert time.monotonic() < deadline, "the ranks did not report within their time limit"
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
    for rank in range(3):
        it = iter(got[rank])
        for dtype in (torch.uint8, torch.uint32):
            for b in bounds:
                vol = _host(_slab_volume(b[-1], dtype))
                for n in ns:
                    lo, hi = next(it)
                    want_lo = vol[max(0, b[rank] - n):b[rank]]
                    want_hi = vol[b[rank + 1]:b[rank + 1] + n]
                    for g, want in ((lo, want_lo), (hi, want_hi)):
                        if len(want) == 0:
                            assert g is None, (rank, b, n)
                        else:
                            assert g[0] == str(dtype) and g[1], (rank, b, n)
                            np.testing.assert_array_equal(g[2], want, err_msg=f'rank {rank}, bounds {b}, n {n}')

