"""GPU: planes streamed through slice windows (emp_median_harden_window, inference/windowed.py, infer_volume's
window_slices) against the whole-plane path: every comparison is exact."""
import os
import socket

import numpy as np
import pytest
import torch

from empanada_amd import synthetic as SY

pytestmark = pytest.mark.gpu

NORMS = dict(mean=0.508979, std=0.148561)
H, W = 37, 29                                              # 1073 pixels: several blocks of 256, the last one partial


@pytest.fixture(scope='module')
def hip():
    from empanada_amd import _hip
    return _hip


def _stack(D, C, thr, seed, h=H, w=W):
    """random probabilities with exact ties planted: a quarter rounded to multiples of 1/8, some equal to thr"""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((D, C, h, w), generator=g)
    pick = torch.rand(x.shape, generator=g)
    x = torch.where(pick < 0.25, torch.round(x * 8) / 8, x)
    x = torch.where(pick > 0.97, torch.full_like(x, thr), x)
    return x.cuda().contiguous()


# ----------------------------------------------------------------------------- 1. the kernel
@pytest.mark.parametrize('C', [1, 3, 9])                   # registers, prefetched LDS ring, general LDS form
@pytest.mark.parametrize('ks', [3, 7, 11])
def test_window_equals_stack_on_the_concatenation(hip, ks, C):
    m, thr = ks // 2, 0.5
    for D in (m, m + 1, ks, ks + 9):
        for has_hist in (False, True):
            for has_halo in (False, True):
                h, l = m * has_hist, m * has_halo
                S = _stack(h + D + l, C, thr, seed=1000 * ks + 10 * D + 2 * has_hist + has_halo)
                what = f'ks={ks} C={C} D={D} hist={has_hist} halo={has_halo}'
                hist = S[:h].contiguous() if has_hist else None
                halo = S[h + D:].contiguous() if has_halo else None
                prob = S[h:h + D].contiguous()
                if h + D + l < ks:                          # the contract rejects it
                    with pytest.raises(hip.HipError, match='shorter than ks'):
                        hip.median_harden_window(prob, ks, thr, hist=hist, halo=halo, want_tail=True)
                    continue
                sem, tail = hip.median_harden_window(prob, ks, thr, hist=hist, halo=halo, want_tail=True)
                esem, efilt = hip.median_harden_stack(S, ks, thr, want_prob=True)
                assert torch.equal(sem, esem[h:h + D]), what
                assert torch.equal(tail, efilt[h + D - m:h + D]), what
                assert sem.shape == (D, H, W) and tail.shape == (m, C, H, W)


def test_window_ks1_hardens_only(hip):
    for C in (1, 3):
        x = _stack(5, C, 0.5, seed=C)
        assert torch.equal(hip.median_harden_window(x, 1, 0.5), hip.median_harden_stack(x, 1, 0.5))
        with pytest.raises(hip.HipError, match='ks=1'):
            hip.median_harden_window(x, 1, 0.5, hist=x[:0])
        with pytest.raises(hip.HipError, match='ks=1'):
            hip.median_harden_window(x, 1, 0.5, want_tail=True)


def test_window_tail_in_place_of_the_history(hip):
    for C, ks in ((1, 7), (3, 5), (9, 3)):
        m = ks // 2
        S = _stack(m + 12 + m, C, 0.5, seed=77 + C)
        esem, efilt = hip.median_harden_stack(S, ks, 0.5, want_prob=True)
        hist = S[:m].clone()
        sem, tail = hip.median_harden_window(S[m:m + 12].contiguous(), ks, 0.5, hist=hist, halo=S[m + 12:].contiguous(),
                                             tail_out=hist)
        assert tail is hist
        assert torch.equal(sem, esem[m:m + 12]) and torch.equal(hist, efilt[12:m + 12])


def test_window_wrong_operands_are_errors_not_reads(hip):
    x = _stack(8, 3, 0.5, seed=5)
    m = 2
    for bad in (x[:m].double(), x[:m].cpu(), x[:m + 1].contiguous(), x[:m, :2].contiguous(), x[:m, :, :, ::2],
                x[:2 * m:2]):
        with pytest.raises(hip.HipError):
            hip.median_harden_window(x, 5, 0.5, hist=bad)
        with pytest.raises(hip.HipError):
            hip.median_harden_window(x, 5, 0.5, halo=bad)
        with pytest.raises(hip.HipError):
            hip.median_harden_window(x, 5, 0.5, tail_out=bad)
    for bad in (x.double(), x.cpu(), x[0], x[:, :, ::2]):
        with pytest.raises(hip.HipError):
            hip.median_harden_window(bad, 5, 0.5)
    for ks in (4, 0, 13, True):
        with pytest.raises(hip.HipError):
            hip.median_harden_window(x, ks, 0.5)
    with pytest.raises(hip.HipError, match='D=1'):          # a window shorter than the median's reach
        hip.median_harden_window(x[:1].contiguous(), 7, 0.5, hist=x[:3].contiguous(), halo=x[:3].contiguous())


def test_window_beyond_the_grid_cap(hip):
    """1536 x 1536 pixels > 8192 blocks x 256 lanes: the grid-stride loop runs more than once"""
    S = _stack(1 + 2 + 1, 1, 0.5, seed=9, h=1536, w=1536)
    esem, efilt = hip.median_harden_stack(S, 3, 0.5, want_prob=True)
    sem, tail = hip.median_harden_window(S[1:3], 3, 0.5, hist=S[:1], halo=S[3:], want_tail=True)
    assert torch.equal(sem, esem[1:3]) and torch.equal(tail, efilt[2:3])


# ----------------------------------------------------------------------------- 2. a chain of windows
@pytest.mark.parametrize('C', [1, 3])
def test_chain_of_unequal_windows_equals_the_whole_stack(hip, C):
    """cuts [0, 5, 8, 17, 29] with ks = 7: windows of 5, 3 (= m, the shortest the contract takes), 9 and 12 slices"""
    ks, thr, cuts = 7, 0.5, [0, 5, 8, 17, 29]
    m = ks // 2
    S = _stack(29, C, thr, seed=31 + C)
    esem, efilt = hip.median_harden_stack(S, ks, thr, want_prob=True)
    hist, sems = None, []
    for lo, hi in zip(cuts, cuts[1:]):
        halo = S[hi:hi + m].contiguous() if hi < 29 else None
        out = hip.median_harden_window(S[lo:hi].contiguous(), ks, thr, hist=hist, halo=halo,
                                       tail_out=hist, want_tail=hi < 29)
        sem, hist = out if isinstance(out, tuple) else (out, None)
        if hist is not None:
            assert torch.equal(hist, efilt[hi - m:hi]), (lo, hi)
        sems.append(sem)
    assert torch.equal(torch.cat(sems), esem)
    with pytest.raises(hip.HipError, match='D=1'):          # a one-slice window is below the median's reach
        hip.median_harden_window(S[5:6].contiguous(), ks, thr, hist=efilt[2:5].contiguous(), halo=S[6:9].contiguous())


# ----------------------------------------------------------------------------- 3. a plane
_PLANTED = {}


def _planted(coarse):
    """(heads, {ks: whole-plane pan}) of a 23 x 64 x 80 volume of small objects: computed once, never modified"""
    if coarse not in _PLANTED:
        lab, classes = SY.planted_labels((23, 64, 80), fill=0.15, rmin=3, rmax=8, seed=7)
        heads = SY.planted_heads(lab, classes, 'xy', n_classes=1, sigma=2.0, noise=0.3, device='cuda', coarse=coarse)
        _PLANTED[coarse] = (heads, {})
    return _PLANTED[coarse]


def _params(ks, coarse):
    return dict(thing_list=[1], label_divisor=1000, stuff_area=16, void_label=0, nms_threshold=0.1, nms_kernel=7,
                confidence_thr=0.5, median_kernel_size=ks, coarse_boundaries=coarse, max_centers=None, upsampling=1)


@pytest.mark.parametrize('coarse', [True, False])
@pytest.mark.parametrize('W_', [4, 8, 23, 64])
@pytest.mark.parametrize('ks', [1, 3, 7])
def test_windowed_plane_equals_whole_plane(ks, W_, coarse):
    from empanada_amd.inference import sharded, windowed
    heads, exp = _planted(coarse)
    if ks not in exp:
        exp[ks] = sharded.sharded_panoptic_stack(heads['sem'], heads['ctr_hmp'], heads['offsets'], **_params(ks, coarse))
    whole = exp[ks].view(torch.int32)
    m = ks // 2
    plan = windowed.plan_windows(23, 4, m, W_)
    assert int(whole.max()) > 0
    for lo, _ in plan[1:]:                                  # the inputs exercise the hand-over: an id on both sides
        a, b = torch.unique(whole[lo - 1]), torch.unique(whole[lo])
        assert len(set(a[a >= 1000].tolist()) & set(b[b >= 1000].tolist())) > 0, f'no instance across the cut at {lo}'
    handed, calls = [0], []

    def fill(lo, hi, bufs, at):
        calls.append((lo, hi))
        for name in ('sem', 'ctr_hmp', 'offsets'):
            handed[0] = max(handed[0], bufs[name].shape[0])
            bufs[name][at:at + hi - lo].copy_(heads[name][lo:hi])

    shapes = {k: tuple(v.shape[1:]) for k, v in heads.items()}
    info = {}
    pan = windowed.windowed_panoptic_stack(fill, plan, shapes, device='cuda', info=info, **_params(ks, coarse))
    assert pan.dtype == torch.uint32 and torch.equal(pan.view(torch.int32), whole)
    assert handed[0] <= min(W_, 23) + m
    assert sorted(calls) == calls and calls[0][0] == 0 and calls[-1][1] == 23       # every slice filled exactly once
    assert all(a[1] == b[0] for a, b in zip(calls, calls[1:]))
    assert info['windows'] == len(calls) and info['head_bytes'] > 0


def test_windowed_plane_with_a_merged_last_chunk():
    """a last chunk shorter than m is merged by the plan; the plane fills it in a second step, within W + m slices"""
    from empanada_amd.inference import sharded, windowed
    heads, _ = _planted(False)
    for n, W_, ks in ((22, 10, 7), (21, 10, 5), (23, 11, 11)):
        sub = {k: v[:n].contiguous() for k, v in heads.items()}
        whole = sharded.sharded_panoptic_stack(sub['sem'], sub['ctr_hmp'], sub['offsets'], **_params(ks, False))
        handed = [0]

        def fill(lo, hi, bufs, at):
            for name in sub:
                handed[0] = max(handed[0], bufs[name].shape[0])
                bufs[name][at:at + hi - lo].copy_(sub[name][lo:hi])

        plan = windowed.plan_windows(n, 1, ks // 2, W_)
        pan = windowed.windowed_panoptic_stack(fill, plan, {k: tuple(v.shape[1:]) for k, v in sub.items()},
                                               device='cuda', **_params(ks, False))
        assert torch.equal(pan.view(torch.int32), whole.view(torch.int32)), (n, W_, ks)
        assert handed[0] <= W_ + ks // 2


# ----------------------------------------------------------------------------- 4. the driver
def _engine(ks=3, render=False):
    from empanada_amd.inference import engines as EN
    from empanada_amd.models import PanopticDeepLab, PanopticDeepLabPR, prepare_for_inference, synthesize_weights
    from empanada_amd.models.panoptic_deeplab import FusedConvBNAct
    cls = PanopticDeepLabPR if render else PanopticDeepLab
    model = synthesize_weights(cls(encoder='resnet18', num_classes=3))
    with torch.no_grad():                                  # offsets of a few pixels instead of hundreds
        model.ins_xy.head[1].weight.mul_(2e-2)
    model = prepare_for_inference(model, 'cuda')
    for m in model.modules():                              # the hand-written kernels: run-to-run identical outputs
        if isinstance(m, FusedConvBNAct) and 'direct' in m.candidates(False):
            m.impl = 'direct'
    kw = dict(thing_list=[1], label_divisor=1000, stuff_area=16, void_label=0, nms_threshold=0.1, nms_kernel=7,
              confidence_thr=0.5, median_kernel_size=ks, padding_factor=32)
    if render:
        return EN.PanopticDeepLabRenderEngine3d(model, coarse_boundaries=True, **kw)
    return EN.PanopticDeepLabEngine3d(model, **kw)


SHAPE = (40, 72, 88)
BATCH = 4 * 96 * 96
ORTHO = ('xy', 'xz', 'yz')
KW = dict(norms=NORMS, labels=[1, 2], min_size=30, min_span=2, class_names={1: 'mito', 2: 'er'})
_CASES = {}


def _host(res):
    vols = {c: (v.view(torch.int32).cpu().numpy().view(np.uint32) if v.dtype == torch.uint32 else v.cpu().numpy())
            for c, v in res['volumes'].items()}
    sets = {c: None if a is None else (np.dtype(a.dtype), tuple(a.chunks), np.asarray(a[...]))
            for c, a in res['datasets'].items()}
    return {'volumes': vols, 'instances': dict(res['instances']), 'z_range': tuple(res['z_range']), 'datasets': sets}


def _assert_same(got, exp):
    assert got['z_range'] == exp['z_range'] and got['instances'] == exp['instances']
    for c in exp['volumes']:
        assert got['volumes'][c].dtype == exp['volumes'][c].dtype
        np.testing.assert_array_equal(got['volumes'][c], exp['volumes'][c], err_msg=f'class {c}')
        assert got['datasets'][c][:2] == exp['datasets'][c][:2]
        np.testing.assert_array_equal(got['datasets'][c][2], exp['datasets'][c][2], err_msg=f'dataset of class {c}')


def _run(engine, vol, path, **kw):
    from empanada_amd.inference.driver import infer_volume
    from empanada_amd.zarr_utils import ZarrV2Group
    res = infer_volume(engine, vol, out=ZarrV2Group(str(path)), **dict(KW, **kw))
    return res, _host(res)


@pytest.fixture
def case(tmp_path_factory):
    """(engine, volume, the unwindowed plain result) per (axes, render, ks, downsample_f): computed once, shared"""
    def get(axes, render, ks, f=1):
        key = (axes, render, ks, f)
        if key not in _CASES:
            eng = _CASES[('engine', render, ks)] = _CASES.get(('engine', render, ks)) or _engine(ks, render)
            vol = SY.em_volume(SHAPE, seed=3)
            _, exp = _run(eng, vol, tmp_path_factory.mktemp('plain') / 'pred.zarr', axes=axes, batch_pixels=BATCH,
                          downsample_f=f)
            _CASES[key] = (eng, vol, exp)
        return _CASES[key]
    return get


def _plane_bytes(eng, vol, axes, f=1):
    """4 * sum numel of the heads the unwindowed run holds for its smallest plane"""
    from empanada_amd.data import DeviceVolume
    from empanada_amd.inference import driver
    dv = DeviceVolume(vol, NORMS['mean'], NORMS['std'], 32, 'cuda', scale=f)
    out = []
    for axis in axes:
        heads = driver._plane_heads(eng, dv, axis, 0, dv.n_slices(axis), BATCH, 2 + f.bit_length() - 1)
        out.append(4 * sum(v.numel() for v in heads.values()))
    return min(out)


@pytest.mark.parametrize('ks', [3, 7])
@pytest.mark.parametrize('render', [False, True])
@pytest.mark.parametrize('axes', [ORTHO, ('xy',)])
def test_infer_volume_windowed_equals_unwindowed(tmp_path, case, axes, render, ks):
    eng, vol, exp = case(axes, render, ks)
    assert exp['volumes'][1].max() > 0 or exp['volumes'][2].max() > 0, "the random model should segment something"
    whole = _plane_bytes(eng, vol, axes)
    for i, kw in enumerate((dict(window_slices=8), dict(window_slices=12),
                            dict(window_slices='auto', mem_budget=12 * 4 * 6 * 96 * 96))):
        res, got = _run(eng, vol, tmp_path / f'w{i}.zarr', axes=axes, batch_pixels=BATCH, **kw)
        _assert_same(got, exp)
        assert set(res['windows']) == set(axes) and all(v > 1 for v in res['windows'].values()), (kw, res['windows'])
        assert 0 < res['head_bytes'] < whole, (kw, res['head_bytes'], whole)


def test_infer_volume_windowed_downsampled(tmp_path, case):
    eng, vol, exp = case(('xy',), True, 3, 2)
    res, got = _run(eng, vol, tmp_path / 'w.zarr', axes=('xy',), batch_pixels=BATCH, downsample_f=2, window_slices=8)
    _assert_same(got, exp)
    assert res['windows']['xy'] > 1 and res['head_bytes'] < _plane_bytes(eng, vol, ('xy',), 2)


# ----------------------------------------------------------------------------- 6. world size
def test_windows_with_a_process_group_of_one(tmp_path, case):
    import torch.distributed as dist
    eng, vol, exp = case(('xy',), False, 3)
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    os.environ['MASTER_ADDR'], os.environ['MASTER_PORT'] = '127.0.0.1', str(port)
    dist.init_process_group('gloo', rank=0, world_size=1)
    try:
        res, got = _run(eng, vol, tmp_path / 'w.zarr', axes=('xy',), batch_pixels=BATCH, window_slices=8,
                        group=dist.group.WORLD)
    finally:
        dist.destroy_process_group()
    _assert_same(got, exp)
    assert res['windows']['xy'] > 1


# ----------------------------------------------------------------------------- 5. the pipeline
@pytest.mark.parametrize('overlap', [True, False])
def test_pipeline_windowed_equals_plain_unwindowed(tmp_path, case, overlap):
    from empanada_amd.inference.pipeline import VolumePipeline
    eng, vol, exp = case(ORTHO, False, 3)
    pipe = VolumePipeline(eng, tune=False, graph=True, overlap=overlap, batch_pixels=BATCH)
    res, got = _run(eng, vol, tmp_path / 'a.zarr', axes=ORTHO, pipeline=pipe, window_slices=8)
    _assert_same(got, exp)
    info = res['pipeline']
    assert info['windows'] == res['windows'] and set(info['windows']) == set(ORTHO)
    assert all(v > 1 for v in info['windows'].values())
    assert info['graph'] is True and info['overlap'] is overlap and info['captures'] > 0
    assert 0 < res['head_bytes'] < _plane_bytes(eng, vol, ORTHO) * (2 if overlap else 1)
    assert eng.model.defer_up4 is False                    # the model is handed back as it was
    res, got = _run(eng, vol, tmp_path / 'b.zarr', axes=ORTHO, pipeline=pipe, window_slices=8)
    _assert_same(got, exp)
    assert res['pipeline']['captures'] == 0                # the batch shapes are known: nothing is captured again
    res, got = _run(eng, vol, tmp_path / 'c.zarr', axes=ORTHO, pipeline=pipe)           # and unwindowed on the same pipeline
    _assert_same(got, exp)
    assert 'windows' not in res['pipeline']


@pytest.mark.parametrize('render,ks,kw', [(True, 3, dict(window_slices=12)), (False, 7, dict(window_slices=4)),
                                          (True, 7, dict(window_slices='auto'))])
def test_pipeline_windowed_engines_and_short_windows(tmp_path, case, render, ks, kw):
    """the Render engine; windows shorter than the filter (W = 4 < ks = 7: the halo is borrowed from the second set);
    'auto' against the pipeline's own budget"""
    from empanada_amd.inference.pipeline import VolumePipeline
    axes = ('xy',) if kw['window_slices'] == 4 else ORTHO   # xy: 4 slices per call, so W = 4 keeps the calls
    eng, vol, exp = case(axes, render, ks)
    budget = 2 * 12 * 4 * 6 * 96 * 96 if kw['window_slices'] == 'auto' else None
    pipe = VolumePipeline(eng, tune=False, graph=True, overlap=True, batch_pixels=BATCH, mem_budget=budget)
    res, got = _run(eng, vol, tmp_path / 'a.zarr', axes=axes, pipeline=pipe, **kw)
    _assert_same(got, exp)
    assert all(v > 1 for v in res['pipeline']['windows'].values())
    assert eng.model.defer_up4 is False


def test_pipeline_windowed_argument_errors(case):
    from empanada_amd.inference.driver import infer_volume
    from empanada_amd.inference.pipeline import VolumePipeline
    eng, vol, _ = case(('xy',), False, 3)
    pipe = VolumePipeline(eng, tune=False, batch_pixels=BATCH)
    with pytest.raises(ValueError, match="pipeline's own"):
        infer_volume(eng, vol, pipeline=pipe, window_slices='auto', mem_budget=1 << 30, **KW)
    with pytest.raises(ValueError, match='window_slices'):
        infer_volume(eng, vol, pipeline=pipe, window_slices=0, **KW)
    assert pipe._streams is None and pipe._store == [None, None]
