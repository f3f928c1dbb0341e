"""GPU: down-sampled inference end to end -- the scaled slice feeder (emp_slices_to_input_scaled) bit for bit against the
loop statement of the resize, the Render engines with upsampling = 2 and the model with three PointRend steps against the
REFERENCE's outputs (tests/golden/downsample.npz, tools/gen_golden_downsample.py), and infer_volume(downsample_f=2)
against a manual composition of the pinned building blocks and against the per-slice protocol on the same heads."""
import math

import numpy as np
import pytest
import torch

from conftest import dense_tol, load_golden
from downsample_ref import (fixture_engine_params, fixture_input, fixture_model, loop_resize, normalised)

pytestmark = pytest.mark.gpu

MEAN, STD = 0.508979, 0.148561


# ----------------------------------------------------------------------------------------------- feeder
def _expected_batches(vol, ax, f, factor=16):
    planes = np.moveaxis(vol, ax, 0)
    n, h, w = planes.shape
    dh, dw = math.ceil(h / f), math.ceil(w / f)
    hp, wp = -(-dh // factor) * factor, -(-dw // factor) * factor
    exp = np.zeros((n, 1, hp, wp), dtype=np.float32)
    for s in range(n):
        exp[s, 0, :dh, :dw] = normalised(loop_resize(planes[s], f), MEAN, STD)
    return exp, (dh, dw), (hp, wp)


@pytest.mark.parametrize('f', [2, 4, 8])
@pytest.mark.parametrize('shape', [(6, 20, 37), (5, 16, 32), (3, 33, 7), (9, 64, 64)])
def test_scaled_feeder_equals_loop_statement(shape, f):
    from empanada_amd.data import DeviceVolume
    rng = np.random.default_rng(shape[0] + f)
    vol = rng.integers(0, 256, shape, dtype=np.uint8)
    dv = DeviceVolume(vol, MEAN, STD, factor=16, scale=f)
    for axis, ax in (('xy', 0), ('xz', 1), ('yz', 2)):
        exp, small, padded = _expected_batches(vol, ax, f)
        n = exp.shape[0]
        assert dv.n_slices(axis) == n and dv.scaled_shape(axis) == small and dv.padded_shape(axis) == padded
        assert dv.plane_shape(axis) == tuple(np.moveaxis(vol, ax, 0).shape[1:])
        got = torch.cat([b for _, b in dv.batches(axis, 4)], dim=0).cpu().numpy()
        np.testing.assert_array_equal(got.view(np.uint32), exp.view(np.uint32), err_msg=f'{axis} whole plane')
        lo, hi = 1, n - 1
        np.testing.assert_array_equal(dv.batch(axis, lo, hi).cpu().numpy().view(np.uint32), exp[lo:hi].view(np.uint32),
                                      err_msg=f'{axis} inner range')
        out = torch.full((hi - lo, 1) + padded, 7.0, dtype=torch.float32, device='cuda')
        assert dv.batch(axis, lo, hi, out=out) is out
        np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), exp[lo:hi].view(np.uint32),
                                      err_msg=f'{axis} out= form')


@pytest.mark.parametrize('shape', [(6, 20, 37), (5, 16, 32), (3, 33, 7)])
def test_scale_one_is_the_existing_feeder(shape):
    """what tests/test_hip_kernels.py::test_device_volume_feeder expects, from an object built with scale=1"""
    from empanada_amd.data import DeviceVolume
    rng = np.random.default_rng(shape[0])
    vol = rng.integers(0, 256, shape, dtype=np.uint8)
    dv = DeviceVolume(vol, MEAN, STD, factor=16, scale=1)
    for axis, ax in (('xy', 0), ('xz', 1), ('yz', 2)):
        planes = np.moveaxis(vol, ax, 0)
        n, h, w = planes.shape
        hp, wp = dv.padded_shape(axis)
        assert hp % 16 == 0 and wp % 16 == 0 and hp >= h and wp >= w and dv.scaled_shape(axis) == (h, w)
        exp = np.zeros((n, 1, hp, wp), dtype=np.float32)
        exp[:, 0, :h, :w] = normalised(planes, MEAN, STD)
        got = torch.cat([b for _, b in dv.batches(axis, 4)], dim=0).cpu().numpy()
        np.testing.assert_array_equal(got.view(np.uint32), exp.view(np.uint32))
        np.testing.assert_array_equal(dv.batch(axis, 1, n - 1).cpu().numpy(), exp[1:n - 1])


def test_scaled_feeder_guards():
    """bad arguments are refused before anything is launched"""
    from empanada_amd import _hip
    from empanada_amd.data import resize_tables
    h, w, dh, dw, hp, wp = 20, 37, 10, 19, 16, 32
    vol = torch.zeros((2, h, w), dtype=torch.uint8, device='cuda')
    out = torch.full((2, 1, hp, wp), 3.0, device='cuda')
    tabs = [torch.from_numpy(t).cuda() for t in resize_tables(h, dh) + resize_tables(w, dw)]
    ro, rc, co, cc = (t.data_ptr() for t in tabs)

    def call(h=h, dh=dh, hp=hp, ro=ro, cc=cc, area=0):
        _hip.call('emp_slices_to_input_scaled', vol.data_ptr(), h * w, w, 1, 2, h, w, dh, dw, hp, wp, ro, rc, co, cc,
                  area, 0.0, 1.0, out.data_ptr(), _hip.stream())

    for bad in (dict(ro=None), dict(cc=None), dict(dh=h + 1, hp=32), dict(dh=0), dict(hp=dh - 1), dict(area=1)):
        with pytest.raises(_hip.HipError):
            call(**bad)
    torch.cuda.synchronize()
    assert bool((out == 3.0).all()), "a refused call must not write"
    call()
    torch.cuda.synchronize()
    assert bool((out[:, :, dh:] == 0).all()) and bool((out[:, :, :dh, :dw] == 0).all())   # zeros in, (0 - 0) * 1 out


# ----------------------------------------------------------------------- the reference's heads, upsampling = 2
class Stub(torch.nn.Module):
    """hands out pre-computed head tensors slice by slice; 'sem_logits' already holds probabilities"""

    def __init__(self, heads):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))
        self.heads, self.t = heads, 0

    def forward(self, x, *a, **k):
        o = {k2: v[self.t:self.t + 1].clone().to(self.p.device) for k2, v in self.heads.items()}
        o['sem_logits'] = o.pop('sem')
        self.t += 1
        return o


@pytest.fixture()
def prob_passthrough(monkeypatch):
    from empanada_amd.inference import engines
    monkeypatch.setattr(engines, 'logits_to_prob', lambda x: x)
    return engines


def _fixture_heads(g):
    """the reference model's heads; probabilities with the library call the reference's logits_to_prob makes on the host"""
    return {'sem': torch.sigmoid(torch.from_numpy(g['sem_logits'])), 'ctr_hmp': torch.from_numpy(g['ctr_hmp']),
            'offsets': torch.from_numpy(g['offsets'])}


def test_render_engine3d_upsampling_2_equals_reference(prob_passthrough):
    EN = prob_passthrough
    g = load_golden('downsample')
    D, H, W = g['full_u8'].shape
    eng = EN.PanopticDeepLabRenderEngine3d(Stub(_fixture_heads(g)).cuda(), median_kernel_size=3,
                                           **fixture_engine_params(g))
    slots, outs = [], []
    for i in range(D):
        o = eng(fixture_input(g, i), (H, W), upsampling=2)
        if o is not None:
            slots.append(i)
            outs.append(o.cpu().numpy().reshape(H, W))
    assert slots == [int(s) for s in g['pan_slot']], "None in the positions where the reference returns None"
    np.testing.assert_array_equal(np.stack(outs), g['pan'].astype(np.int64))
    ends = [o.cpu().numpy().reshape(H, W) for o in eng.end(2)]
    assert len(ends) == len(g['pan_end'])
    np.testing.assert_array_equal(np.stack(ends), g['pan_end'].astype(np.int64))


def test_postprocess_stack_upsampling_2_equals_reference():
    from empanada_amd.inference import engines as EN
    g = load_golden('downsample')
    D, H, W = g['full_u8'].shape
    heads = {k: v.cuda() for k, v in _fixture_heads(g).items()}
    eng = EN.PanopticDeepLabRenderEngine3d(Stub(heads).cuda(), median_kernel_size=3, **fixture_engine_params(g))
    pan, emitted = eng.postprocess_stack(heads, upsampling=2)
    assert emitted == list(range(D)) and tuple(pan.shape[1:]) == tuple(g['sem_logits'].shape[2:])
    exp = np.concatenate([g['pan'], g['pan_end']]).astype(np.int64)
    np.testing.assert_array_equal(pan[:, :H, :W].cpu().numpy().astype(np.int64), exp)


def test_three_render_steps_gpu_within_tolerance():
    """the prepared model (hand-written kernels) called as the Render engine calls it for upsampling = 2, against the
    REFERENCE model's heads; the criteria of test_models.py::test_mitonet_512_gpu_forward_and_render_engine"""
    from empanada_amd.inference.postprocess import factor_pad
    from empanada_amd.models import prepare_for_inference
    g = load_golden('downsample')
    m = prepare_for_inference(fixture_model(g), 'cuda')
    for i in range(g['small_u8'].shape[0]):
        x = factor_pad(fixture_input(g, i), 16).cuda().contiguous(memory_format=torch.channels_last)
        with torch.no_grad():
            out = m(x, 3, False)
        figures = {}
        for k in ('ctr_hmp', 'offsets'):
            ref = g[k][i:i + 1]
            figures[k] = (float(np.abs(out[k].float().cpu().numpy() - ref).max()), dense_tol(float(np.abs(ref).max())))
        ref = g['sem_logits'][i:i + 1]
        bad = np.abs(out['sem_logits'].float().cpu().numpy() - ref) > 10 * dense_tol(float(np.abs(ref).max()))
        print(f'slice {i}: max error / tolerance {figures}; sem_logits share beyond 10 x tol {bad.mean():.3e}')
        for k, (err, tol) in figures.items():
            assert err <= tol, (i, k, err, tol)
        assert bad.mean() < 1e-3, (i, bad.mean())


# ----------------------------------------------------------------------------------------------- driver
def _as_numpy(vols, c, thing):
    v = vols[c]
    return v.view(torch.int32).cpu().numpy().view(np.uint32) if c in thing else v.cpu().numpy()


def _heads_f2(engine, vol, axes):
    from empanada_amd.data import DeviceVolume
    from empanada_amd.inference import driver
    from test_driver_gpu import NORMS
    dv = DeviceVolume(vol, NORMS['mean'], NORMS['std'], int(engine.padding_factor), 'cuda', scale=2)
    return dv, {axis: driver._plane_heads(engine, dv, axis, 0, dv.n_slices(axis), 1 << 22, 3) for axis in axes}


def _finish(trackers, shape, axes, labels, thing, min_size, min_span, device):
    """filters -> consensus (or the plane's own trackers in stack mode) -> painted volumes, as test_driver_gpu._manual"""
    from empanada_amd.inference import filters
    from empanada_amd.inference import patterns as PA
    for axis in axes:
        for tr in trackers[axis]:
            filters.remove_small_objects(tr, min_size)
            filters.remove_pancakes(tr, min_span)
    out = {}
    for c in labels:
        cts = PA.get_axis_trackers_by_class(trackers, c)
        if len(axes) == 1:
            con = cts[0]
        elif c in thing:
            con = PA.create_instance_consensus(cts, 2, 0.75, False)
            filters.remove_small_objects(con, min_size)
            filters.remove_pancakes(con, min_span)
        else:
            con = PA.create_semantic_consensus(cts, 2)
        if device:
            v = PA.fill_volume_device(shape, [con]).cpu().numpy().astype(np.uint32)
        else:
            v = np.zeros(shape, dtype=np.uint32)
            PA.fill_volume(v, con.instances)
        out[c] = v if c in thing else (v > 0).astype(np.uint8)
    return out


def _manual_f2(engine, vol, axes, min_size, min_span):
    from empanada_amd.inference import patterns as PA
    from empanada_amd.inference.postprocess import panoptic_stack
    labels, thing = [1, 2], [1]
    dv, heads = _heads_f2(engine, vol, axes)
    assert dv.shape == vol.shape
    trackers = {}
    for axis in axes:
        h, w = dv.plane_shape(axis)
        hd = heads[axis]
        assert tuple(hd['sem'].shape[2:]) == tuple(2 * s for s in dv.padded_shape(axis))
        pan, emitted = panoptic_stack(hd['sem'], hd['ctr_hmp'], hd['offsets'], thing_list=thing, label_divisor=1000,
                                      stuff_area=16, void_label=0, nms_threshold=0.1, nms_kernel=7, confidence_thr=0.5,
                                      median_kernel_size=engine.ks, coarse_boundaries=True, upsampling=2)
        assert len(emitted) == dv.n_slices(axis)
        trackers[axis] = PA.track_stack(pan[:, :h, :w].contiguous(), axis, vol.shape, labels, thing, 1000, 0.25, 0.25)
    return _finish(trackers, vol.shape, axes, labels, thing, min_size, min_span, device=True)


@pytest.mark.parametrize('shape', [(40, 72, 88), (24, 73, 90)])
@pytest.mark.parametrize('axes', [('xy', 'xz', 'yz'), ('xy',)])
def test_infer_volume_downsample_equals_manual_composition(tmp_path, axes, shape):
    from empanada_amd import synthetic as SY
    from empanada_amd.inference.driver import infer_volume
    from empanada_amd.zarr_utils import ZarrV2Group, open_zarr
    from test_driver_gpu import NORMS, _engine
    vol = SY.em_volume(shape, seed=3)
    engine = _engine(ks=3, render=True)
    out = ZarrV2Group(str(tmp_path / 'pred.zarr'))
    res = infer_volume(engine, vol, norms=NORMS, labels=[1, 2], axes=axes, min_size=30, min_span=2,
                       class_names={1: 'mito', 2: 'er'}, out=out, batch_pixels=1 << 22, downsample_f=2)
    exp = _manual_f2(engine, vol, axes, 30, 2)
    assert res['z_range'] == (0, shape[0])
    for c, name, dt in ((1, 'mito_pred', np.uint32), (2, 'er_pred', np.uint8)):
        got = _as_numpy(res['volumes'], c, [1])
        assert got.shape == shape
        np.testing.assert_array_equal(got, exp[c], err_msg=f'class {c}')
        arr = open_zarr(str(tmp_path / 'pred.zarr' / name))
        assert arr.dtype == dt and tuple(arr.shape) == shape and tuple(arr.chunks) == (1,) + shape[1:]
        np.testing.assert_array_equal(arr[...], exp[c])
    assert res['instances'][1] == len(np.unique(exp[1])) - 1
    assert exp[1].max() > 0 or exp[2].max() > 0, "the random model should segment something"


@pytest.mark.parametrize('axes', [('xy', 'xz', 'yz'), ('xy',)])
def test_infer_volume_downsample_equals_per_slice_protocol(prob_passthrough, axes):
    """the reference script's loop (pdl_inference3d.py:150-223 with -downsample-f 2) over the SAME head tensors: a stub
    model serves _plane_heads' slices one by one, the images come from VolumeDataset(scale=2)"""
    EN = prob_passthrough
    from empanada_amd import synthetic as SY
    from empanada_amd.data import VolumeDataset
    from empanada_amd.inference import patterns as PA
    from empanada_amd.inference import rle
    from empanada_amd.inference.driver import infer_volume
    from test_driver_gpu import NORMS, _engine
    shape = (40, 72, 88)
    labels, thing = [1, 2], [1]
    vol = SY.em_volume(shape, seed=3)
    engine = _engine(ks=3, render=True)
    res = infer_volume(engine, vol, norms=NORMS, labels=labels, axes=axes, min_size=30, min_span=2,
                       batch_pixels=1 << 22, downsample_f=2)
    dv, heads = _heads_f2(engine, vol, axes)
    kw = dict(thing_list=thing, label_divisor=1000, stuff_area=16, void_label=0, nms_threshold=0.1, nms_kernel=7,
              confidence_thr=0.5, median_kernel_size=3, padding_factor=32, coarse_boundaries=True)
    names = {'xy': 0, 'xz': 1, 'yz': 2}
    trackers = PA.create_axis_trackers({a: names[a] for a in axes}, labels, 1000, shape)
    for axis in axes:
        ds = VolumeDataset(vol, names[axis], tfs=lambda image: {'image': normalised(image, **NORMS)}, scale=2)
        eng = EN.PanopticDeepLabRenderEngine3d(Stub(heads[axis]).cuda(), **kw)
        matchers = PA.create_matchers(thing, 1000, 0.25, 0.25)
        stack = []
        for i in range(len(ds)):
            item = ds[i]
            assert item['image'].shape == dv.scaled_shape(axis) and item['size'] == dv.plane_shape(axis)
            pan = eng(torch.from_numpy(item['image'])[None, None], item['size'], upsampling=2)
            pans = [] if pan is None else [pan]
            if i == len(ds) - 1:
                pans += list(eng.end(2))
            for p in pans:
                p = p.cpu().numpy().reshape(item['size'])
                stack.append(PA.apply_matchers(rle.pan_seg_to_rle_seg(p, labels, 1000, thing, True), matchers))
        assert len(stack) == len(ds)
        for idx, rs in PA.backward_matching(stack, matchers, len(ds)):
            PA.update_trackers(rs, idx, trackers[axis])
        PA.finish_tracking(trackers[axis])
    exp = _finish(trackers, shape, axes, labels, thing, 30, 2, device=False)
    for c in labels:
        np.testing.assert_array_equal(_as_numpy(res['volumes'], c, thing), exp[c], err_msg=f'class {c}')
    assert exp[1].max() > 0 or exp[2].max() > 0


def test_infer_volume_downsample_arguments():
    from empanada_amd import synthetic as SY
    from empanada_amd.data import DeviceVolume
    from empanada_amd.inference.driver import infer_volume
    from test_driver_gpu import NORMS, _engine
    vol = SY.em_volume((12, 40, 48), seed=1)
    kw = dict(norms=NORMS, labels=[1, 2], axes=('xy',), min_size=10, min_span=1, batch_pixels=1 << 22)
    plain = _engine(ks=3, render=False)
    with pytest.raises(ValueError, match='Render engine'):
        infer_volume(plain, vol, downsample_f=2, **kw)
    render = _engine(ks=3, render=True)
    for bad in (3, 0, 6, 2.0):
        with pytest.raises(ValueError, match='power of two'):
            infer_volume(render, vol, downsample_f=bad, **kw)
    with pytest.raises(ValueError, match='scale'):
        infer_volume(render, DeviceVolume(vol, NORMS['mean'], NORMS['std'], 32), downsample_f=2, **kw)
    for engine in (plain, render):
        a = infer_volume(engine, vol, **kw)
        b = infer_volume(engine, vol, downsample_f=1, **kw)
        for c in (1, 2):
            assert torch.equal(a['volumes'][c].view(torch.uint8), b['volumes'][c].view(torch.uint8))
        assert a['instances'] == b['instances']
    dv = DeviceVolume(vol, NORMS['mean'], NORMS['std'], 32, scale=2)
    a = infer_volume(render, dv, downsample_f=2, **kw)
    b = infer_volume(render, vol, downsample_f=2, **kw)
    for c in (1, 2):
        assert tuple(a['volumes'][c].shape) == vol.shape
        assert torch.equal(a['volumes'][c].view(torch.uint8), b['volumes'][c].view(torch.uint8))
