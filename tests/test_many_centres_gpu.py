"""GPU: more than 4096 instance centres per slice (opt-in, up to 65535): emp_find_centers_ws, emp_group_pixels and the
fusion at large capacities, and the limit plumbed through postprocess, the engines and the sharded path.  Every
comparison is exact, against the oracle (which has no centre limit)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LIMIT = 65535


@pytest.fixture(scope='module')
def hip():
    from empanada_amd import _hip
    _hip.load()
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return _hip


def _oracle_flat(hm, thr, k):
    from oracle import postprocess as OP
    ctr = OP.find_instance_center(hm[None, None], thr, k)
    return ctr[:, 0] * hm.shape[1] + ctr[:, 1]


def _lattice(h, w, y0, x0, pitch, seed):
    rng = np.random.default_rng(seed)
    hm = np.zeros((h, w), dtype=np.float32)
    sub = hm[y0::pitch, x0::pitch]
    sub[...] = rng.random(sub.shape, dtype=np.float32) * 0.5 + 0.5
    return hm


def _detection_cases():
    rng = np.random.default_rng(41)
    rnd = (rng.random((512, 512)) ** 2).astype(np.float32)
    rnd[100:140, 200:260] = 0.7                       # a plateau: every pixel of it is a maximum of its window
    return {
        'lattice_300_k1': (_lattice(300, 300, 0, 0, 2, 1), 1, 22500),
        'lattice_765x768_k3': (_lattice(765, 768, 1, 1, 3, 2), 3, 65280),
        'random_512_plateau_k3': (rnd, 3, None),
        'width_not_multiple_of_4_k1': (_lattice(300, 301, 0, 0, 2, 3), 1, 150 * 151),
        'lattice_k7_window_clipped': (_lattice(301, 303, 0, 0, 4, 4), 7, 76 * 76),
    }


@pytest.mark.parametrize('name', list(_detection_cases()))
def test_detection_exact_and_in_raster_order(hip, name):
    from empanada_amd.inference.postprocess import centers_batched, find_instance_center
    hm, k, n_expected = _detection_cases()[name]
    exp = _oracle_flat(hm, 0.1, k)
    if n_expected is not None:
        assert len(exp) == n_expected
    assert hip.MAX_CENTERS < len(exp) <= LIMIT
    dev = torch.from_numpy(hm)[None, None].cuda()
    idx, cnt = centers_batched(dev, 0.1, k, max_centers=LIMIT)
    assert int(cnt[0]) == len(exp)
    np.testing.assert_array_equal(idx[0, :len(exp)].cpu().numpy(), exp)
    ctr = find_instance_center(dev, 0.1, k, max_centers=LIMIT).cpu().numpy()
    assert ctr.dtype == np.int64
    np.testing.assert_array_equal(ctr[:, 0] * hm.shape[1] + ctr[:, 1], exp)
    # a limit between the count and the ceiling is enough
    idx2, cnt2 = centers_batched(dev, 0.1, k, max_centers=len(exp))
    assert int(cnt2[0]) == len(exp) and idx2.shape[1] >= len(exp)
    np.testing.assert_array_equal(idx2[0, :len(exp)].cpu().numpy(), exp)
    with pytest.raises(hip.HipError, match=str(len(exp) - 1)):
        centers_batched(dev, 0.1, k, max_centers=len(exp) - 1)


def test_over_the_hard_limit_raises(hip):
    from empanada_amd.inference.postprocess import centers_batched
    hm = _lattice(768, 771, 1, 1, 3, 5)
    assert len(_oracle_flat(hm, 0.1, 3)) == 65792
    with pytest.raises(hip.HipError, match='65535') as err:
        centers_batched(torch.from_numpy(hm)[None, None].cuda(), 0.1, 3, max_centers=LIMIT)
    assert '65792' in str(err.value)
    with pytest.raises(hip.HipError):
        hip.find_centers_ws(torch.from_numpy(hm)[None].cuda(), 0.1, 3, LIMIT + 1)
    # the raw entry still counts exactly and keeps the first 65535
    idx, cnt = hip.find_centers_ws(torch.from_numpy(hm)[None].cuda(), 0.1, 3, LIMIT)
    assert int(cnt[0]) == 65792
    np.testing.assert_array_equal(idx[0].cpu().numpy(), _oracle_flat(hm, 0.1, 3)[:LIMIT])


def test_raw_entry_overflow_keeps_the_first_centres(hip):
    hm = _lattice(300, 300, 0, 0, 2, 1)
    exp = _oracle_flat(hm, 0.1, 1)
    for cap in (5000, 1, 22499, 22500):
        idx, cnt = hip.find_centers_ws(torch.from_numpy(hm)[None].cuda(), 0.1, 1, cap)
        assert idx.shape == (1, cap)
        assert int(cnt[0]) == 22500
        np.testing.assert_array_equal(idx[0].cpu().numpy(), exp[:cap])


def test_batch_of_slices_with_very_different_counts(hip):
    from empanada_amd.inference.postprocess import centers_batched
    rng = np.random.default_rng(7)
    full = _lattice(300, 300, 0, 0, 2, 1)
    spots = np.flatnonzero(full.ravel())
    counts = [0, 100, 4096, 22500]
    hm = np.zeros((4, 300, 300), dtype=np.float32)
    for d, n in enumerate(counts):
        keep = rng.choice(spots, n, replace=False)
        hm[d].ravel()[keep] = full.ravel()[keep]
    idx, cnt = centers_batched(torch.from_numpy(hm)[:, None].cuda(), 0.1, 1, max_centers=LIMIT)
    assert cnt.cpu().tolist() == counts
    for d, n in enumerate(counts):
        np.testing.assert_array_equal(idx[d, :n].cpu().numpy(), _oracle_flat(hm[d], 0.1, 1))
    idx, cnt = hip.find_centers_ws(torch.from_numpy(hm).cuda(), 0.1, 1, 30000)
    assert cnt.cpu().tolist() == counts
    for d, n in enumerate(counts):
        np.testing.assert_array_equal(idx[d, :n].cpu().numpy(), _oracle_flat(hm[d], 0.1, 1))


# ------------------------------------------------------------------------------------------------ grouping
def _nearby_centre(ctr, h, w, radius=10):
    """(ny, nx): per pixel the position of a nearest centre within `radius` (the pixel itself where there is none)"""
    occ = np.zeros((h, w), dtype=bool)
    occ[ctr[:, 0], ctr[:, 1]] = True
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    ny, nx = yy.copy(), xx.copy()
    done = np.zeros((h, w), dtype=bool)
    r = np.arange(-radius, radius + 1)
    dy, dx = (a.ravel() for a in np.meshgrid(r, r, indexing='ij'))
    for j in np.argsort(dy * dy + dx * dx, kind='stable'):
        y, x = yy + dy[j], xx + dx[j]
        ok = (y >= 0) & (y < h) & (x >= 0) & (x < w) & ~done
        ok[ok] = occ[y[ok], x[ok]]
        ny[ok], nx[ok] = y[ok], x[ok]
        done |= ok
    return ny, nx


def _centre_list(rng, K, h, w):
    """K centres, duplicates allowed; the last one (id K) sits alone in the bottom right corner"""
    flat = rng.integers(0, h * w - 1, K)
    flat[K - 1] = h * w - 1
    return np.stack([flat // w, flat % w], axis=1).astype(np.int64)


def _group(hip, ctr, off, step):
    w = off.shape[-1]
    idx = torch.from_numpy((ctr[:, 0] * w + ctr[:, 1]).astype(np.int32))[None].cuda()
    cnt = torch.tensor([len(ctr)], dtype=torch.int32).cuda()
    return hip.group_pixels(idx, cnt, torch.from_numpy(off).cuda(), step).cpu().numpy().astype(np.int64)


@pytest.mark.parametrize('family', ['structured', 'random'])
@pytest.mark.parametrize('step', [1, 4])
@pytest.mark.parametrize('K', [5000, 20000, 65535])
def test_group_pixels_many_centres(hip, K, step, family):
    from empanada_amd.inference.postprocess import group_pixels
    from oracle import postprocess as OP
    h, w = (128, 192) if K == 65535 else (192, 256)
    rng = np.random.default_rng(K * 13 + step)
    ctr = _centre_list(rng, K, h, w)
    if family == 'structured':
        # what test_group_pixels_structured_offsets does, at these K: offsets that point at nearby centres (the
        # per-wave pruning is active), half-way offsets (equidistant pairs), a duplicated centre, a band beyond
        # the 1e5 ceiling, a row of NaN / inf
        ctr[K // 2] = ctr[0]
        yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
        ny, nx = _nearby_centre(ctr, h, w)
        off = np.stack([ny - yy, nx - xx]).astype(np.float32)[None] * step
        off[0, :, :, : w // 2] *= 0.5
        off += rng.normal(0, 0.2, off.shape).astype(np.float32)
        off[0, :, -1, -1] = 0                            # the corner pixel votes for the last centre
        off[0, :, 40:44] += 3e5
        off[0, 0, 50, :20] = np.nan
        off[0, 1, 50, 20:40] = np.inf
    else:
        # locations all over the slice: every wave's box keeps all K centres, the candidate list overflows and
        # the vote walks the whole list
        off = (rng.normal(0, 40, (1, 2, h, w)) * step).astype(np.float32)
        off[0, :, -1, -1] = 0
    exp = OP.group_pixels(ctr, off, step=step)
    assert exp[0, -1, -1] == K and exp.max() == K        # the largest id (65535 = 0xFFFF) is in use
    np.testing.assert_array_equal(_group(hip, ctr, off, step), exp)
    if step == 1:
        # the public function takes an explicit list of any length up to the ceiling, without opt-in
        got = group_pixels(torch.from_numpy(ctr), torch.from_numpy(off), step=step).cpu().numpy()
        np.testing.assert_array_equal(got, exp)


def test_explicit_centre_list_over_the_ceiling_raises(hip):
    from empanada_amd.inference.postprocess import group_pixels
    ctr = torch.zeros((LIMIT + 1, 2), dtype=torch.long)
    with pytest.raises(hip.HipError, match='65535'):
        group_pixels(ctr, torch.zeros(1, 2, 16, 16))


def test_fusion_with_20000_ids(hip):
    """the histogram of emp_fuse_* without its LDS copy (cap beyond what fits)"""
    from empanada_amd.inference.postprocess import merge_semantic_and_instance
    from oracle import postprocess as OP
    rng = np.random.default_rng(12)
    H, W, K = 256, 384, 20000
    blocks = np.zeros((H // 2) * (W // 2), dtype=np.int64)
    blocks[rng.choice(blocks.size, K, replace=False)] = np.arange(1, K + 1)
    ids = np.repeat(np.repeat(blocks.reshape(H // 2, W // 2), 2, 0), 2, 1)
    ids[::7, ::5] = rng.integers(0, K + 1, ids[::7, ::5].shape)
    sem = np.repeat(np.repeat(rng.integers(0, 3, (H // 4, W // 8)), 4, 0), 8, 1).astype(np.int64)
    sem[::3, ::3] = rng.integers(0, 3, sem[::3, ::3].shape)
    thing = [1, 2]
    ins = ids * np.isin(sem, thing)
    exp = OP.merge_semantic_and_instance(sem[None], ins[None], 1000, thing, 40, 0)[0]
    for dt in (torch.uint32, torch.int64):
        pan = hip.fuse_panoptic(torch.from_numpy(sem.astype(np.uint8))[None].cuda(),
                                torch.from_numpy(ids.astype(np.int16))[None].cuda().view(torch.uint16),
                                K, 3, thing, 1000, 40, 0, up=1, out_dtype=dt)
        np.testing.assert_array_equal(pan[0].cpu().numpy().astype(np.int64), exp)
    got = merge_semantic_and_instance(torch.from_numpy(sem)[None], torch.from_numpy(ins)[None], 1000, thing, 40, 0)
    np.testing.assert_array_equal(got[0].cpu().numpy(), exp)


# ------------------------------------------------------------------------------------------------ whole stack, engines
KW = dict(thing_list=[1], label_divisor=100000, stuff_area=32, void_label=0, nms_threshold=0.1, nms_kernel=3,
          confidence_thr=0.5)


def _dense_heads(D=5, H=256, W=256, seed=3):
    """full-resolution heads with a 3-pixel lattice of centres (85 x 85 = 7225 per slice), offsets towards the
    lattice and a blocky foreground probability"""
    rng = np.random.default_rng(seed)
    ctr = np.stack([_lattice(H, W, 1, 1, 3, seed + d) for d in range(D)])[:, None]
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    ty = np.clip((yy // 3) * 3 + 1, 0, 1 + 3 * ((H - 2) // 3))
    tx = np.clip((xx // 3) * 3 + 1, 0, 1 + 3 * ((W - 2) // 3))
    off = np.stack([ty - yy, tx - xx]).astype(np.float32)[None].repeat(D, 0)
    off += rng.normal(0, 0.3, off.shape).astype(np.float32)
    sem = np.repeat(np.repeat(rng.random((D, 1, H // 8, W // 8)), 8, 2), 8, 3).astype(np.float32)
    sem += rng.normal(0, 0.1, sem.shape).astype(np.float32)
    return {'sem': np.clip(sem, 0, 1).astype(np.float32), 'ctr_hmp': ctr.astype(np.float32), 'offsets': off}


def _oracle_stack(heads, ks, cells_cache):
    """the reference's 3d engine over the stack (oracle.postprocess.post_slice: get_instance_cells + get_panoptic_seg
    on every item that leaves the median queue); the cells do not depend on the median and are computed once"""
    from oracle import postprocess as OP
    D = heads['sem'].shape[0]
    q = OP.MedianQueue(ks)
    items = []
    for t in range(D):
        q.enqueue({'sem': heads['sem'][t:t + 1].copy(), 't': t})
        o = q.get_next(['sem'])
        if o is not None:
            items.append(o)
    items += q.end()
    pans = []
    for o in items:
        t = o['t']
        if t not in cells_cache:
            cells_cache[t] = OP.get_instance_cells(heads['ctr_hmp'][t:t + 1], heads['offsets'][t:t + 1],
                                                   KW['nms_threshold'], KW['nms_kernel'], False, 1)
        sem = OP.harden_seg(o['sem'], KW['confidence_thr'])[0]
        pans.append(OP.get_panoptic_seg(sem, cells_cache[t], KW['label_divisor'], KW['thing_list'], KW['stuff_area'],
                                        KW['void_label'])[0])
    return np.stack(pans)


@pytest.fixture(scope='module')
def dense():
    heads = _dense_heads()
    cache = {}
    exp = {ks: _oracle_stack(heads, ks, cache) for ks in (1, 3)}
    assert len(_oracle_flat(heads['ctr_hmp'][0, 0], 0.1, 3)) == 7225
    assert len(np.unique(exp[3][0])) > 1000
    return heads, exp


def _dev(heads):
    return {k: torch.from_numpy(v).cuda() for k, v in heads.items()}


@pytest.mark.parametrize('ks', [1, 3])
def test_panoptic_stack_many_centres(hip, dense, ks, monkeypatch):
    from empanada_amd.inference.postprocess import panoptic_stack
    heads, exp = dense
    h = _dev(heads)
    monkeypatch.delenv('EMP_MAX_CENTERS', raising=False)
    pan, emitted = panoptic_stack(h['sem'], h['ctr_hmp'], h['offsets'], coarse_boundaries=False, median_kernel_size=ks,
                                  max_centers=LIMIT, **KW)
    assert emitted == list(range(5))
    np.testing.assert_array_equal(pan.cpu().numpy().astype(np.int64), exp[ks])
    with pytest.raises(hip.HipError, match='EMP_MAX_CENTERS'):           # the default limit stays 4096
        panoptic_stack(h['sem'], h['ctr_hmp'], h['offsets'], coarse_boundaries=False, median_kernel_size=ks, **KW)
    monkeypatch.setenv('EMP_MAX_CENTERS', '65535')
    pan2, _ = panoptic_stack(h['sem'], h['ctr_hmp'], h['offsets'], coarse_boundaries=False, median_kernel_size=ks, **KW)
    assert torch.equal(pan2.view(torch.int32), pan.view(torch.int32))
    monkeypatch.setenv('EMP_MAX_CENTERS', '7224')
    with pytest.raises(hip.HipError, match='7225'):
        panoptic_stack(h['sem'], h['ctr_hmp'], h['offsets'], coarse_boundaries=False, median_kernel_size=ks, **KW)


class Stub(torch.nn.Module):
    """hands out pre-computed head tensors slice by slice (they stay on the GPU); 'sem_logits' already holds
    probabilities"""

    def __init__(self, heads):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))
        self.heads, self.t = heads, 0

    def forward(self, x, *a, **k):
        o = {k2: v[self.t:self.t + 1].clone() for k2, v in self.heads.items()}
        o['sem_logits'] = o.pop('sem')
        self.t += 1
        return o


def _feed(eng, n, shape, *args):
    outs = []
    for _ in range(n):
        o = eng(torch.zeros(1, 1, *shape), *args)
        if o is not None:
            outs.append(o)
    outs += list(eng.end())
    return np.stack([np.asarray(o.cpu().numpy()).reshape(shape) for o in outs])


@pytest.mark.parametrize('deferred', [False, True])
def test_engines_carry_the_limit(hip, dense, monkeypatch, deferred):
    from empanada_amd.inference import engines as EN
    from empanada_amd.inference import sharded
    monkeypatch.setattr(EN, 'logits_to_prob', lambda x: x)
    monkeypatch.delenv('EMP_MAX_CENTERS', raising=False)
    heads, exp = dense
    D, _, H, W = heads['sem'].shape
    kw = dict(KW, median_kernel_size=3, deferred=deferred, deferred_batch=1)      # the stub answers one image per call
    # per slice, full-resolution engine: the first slices go through the stack form, end() through postprocess()
    eng = EN.PanopticDeepLabEngine3d(Stub(_dev(heads)).cuda(), max_centers=LIMIT, **kw)
    assert eng.max_centers == LIMIT
    np.testing.assert_array_equal(_feed(eng, D, (H, W)), exp[3])
    # per slice, render engine on full-resolution instance heads: get_instance_cells / find_instance_center
    eng = EN.PanopticDeepLabRenderEngine3d(Stub(_dev(heads)).cuda(), coarse_boundaries=False, max_centers=LIMIT, **kw)
    np.testing.assert_array_equal(_feed(eng, D, (H, W), (H, W)), exp[3])
    cells = eng.get_instance_cells(_dev(heads)['ctr_hmp'][:1], _dev(heads)['offsets'][:1])
    assert int(cells.max()) == 7225
    if deferred:
        return
    # whole stack
    pan, emitted = eng.postprocess_stack(_dev(heads))
    assert emitted == list(range(D))
    np.testing.assert_array_equal(pan.cpu().numpy().astype(np.int64), exp[3])
    h = _dev(heads)
    pan = sharded.sharded_panoptic_stack(h['sem'], h['ctr_hmp'], h['offsets'], coarse_boundaries=False,
                                         median_kernel_size=3, max_centers=LIMIT, **KW)
    np.testing.assert_array_equal(pan.cpu().numpy().astype(np.int64), exp[3])
    # without the opt-in the engines stop where they always did
    eng = EN.PanopticDeepLabEngine3d(Stub(_dev(heads)).cuda(), **kw)
    with pytest.raises(hip.HipError):
        _feed(eng, D, (H, W))
    with pytest.raises(hip.HipError):
        sharded.sharded_panoptic_stack(h['sem'], h['ctr_hmp'], h['offsets'], coarse_boundaries=False,
                                       median_kernel_size=3, **KW)


def test_default_path_untouched_by_the_opt_in(hip, monkeypatch):
    from empanada_amd import synthetic as SY
    from empanada_amd.inference.postprocess import centers_batched, panoptic_stack
    monkeypatch.delenv('EMP_MAX_CENTERS', raising=False)
    lab, cls = SY.planted_labels((6, 96, 128), fill=0.3, rmin=3, rmax=8, seed=9)
    heads = {k: v.cuda() for k, v in SY.planted_heads(lab, cls, 'xy', seed=4).items()}
    kw = dict(thing_list=[1], label_divisor=1000, stuff_area=32, void_label=0, nms_threshold=0.1, nms_kernel=7,
              confidence_thr=0.5, median_kernel_size=3)
    idx0, cnt0 = centers_batched(heads['ctr_hmp'], 0.1, 7)
    idx1, cnt1 = centers_batched(heads['ctr_hmp'], 0.1, 7, max_centers=LIMIT)
    assert 0 < int(cnt0.max()) <= hip.MAX_CENTERS
    assert idx0.shape == idx1.shape and torch.equal(cnt0, cnt1)
    for d in range(idx0.shape[0]):
        n = int(cnt0[d])
        assert torch.equal(idx0[d, :n], idx1[d, :n])
    ids0 = hip.group_pixels(idx0, cnt0, heads['offsets'].float().contiguous(), 1)
    ids1 = hip.group_pixels(idx1, cnt1, heads['offsets'].float().contiguous(), 1)
    assert torch.equal(ids0.view(torch.int16), ids1.view(torch.int16))
    pan0, _ = panoptic_stack(heads['sem'], heads['ctr_hmp'], heads['offsets'], coarse_boundaries=False, **kw)
    pan1, _ = panoptic_stack(heads['sem'], heads['ctr_hmp'], heads['offsets'], coarse_boundaries=False,
                             max_centers=LIMIT, **kw)
    assert torch.equal(pan0.view(torch.int32), pan1.view(torch.int32))
    # the new entry agrees with the old one where both apply
    hm = heads['ctr_hmp'][:, 0].float().contiguous()
    idx2, cnt2 = hip.find_centers_ws(hm, 0.1, 7, idx0.shape[1])
    assert torch.equal(cnt2, cnt0)
    for d in range(idx0.shape[0]):
        n = int(cnt0[d])
        assert torch.equal(idx0[d, :n], idx2[d, :n])
