"""GPU: infer_volume(..., pipeline=VolumePipeline(...)) -- tuned sites, graph replay, heads written in place by
emp_upsample_bilinear_prob, two streams, SlabWriter -- against the plain infer_volume call on the same engine: the
labelled volumes, the instance counts, the z range and the zarr datasets must be array-equal, ids included.  Volume and
engine are those of tests/test_driver_gpu.py."""
import json
import os
import socket

import numpy as np
import pytest
import torch

from empanada_amd import synthetic as SY

pytestmark = pytest.mark.gpu

NORMS = dict(mean=0.508979, std=0.148561)
ORTHO = ('xy', 'xz', 'yz')
KW = dict(norms=NORMS, labels=[1, 2], min_size=30, min_span=2, class_names={1: 'mito', 2: 'er'})
SHAPE = (40, 72, 88)                                       # 40, 72 and 88 are not all multiples of the padding factors


def _engine(ks=3, render=False, direct=True):
    from empanada_amd.inference import engines as EN
    from empanada_amd.models import PanopticDeepLab, PanopticDeepLabPR, prepare_for_inference, synthesize_weights
    from empanada_amd.models.panoptic_deeplab import FusedConvBNAct
    cls = PanopticDeepLabPR if render else PanopticDeepLab
    model = synthesize_weights(cls(encoder='resnet18', num_classes=3))
    with torch.no_grad():                                  # offsets of a few pixels instead of hundreds
        model.ins_xy.head[1].weight.mul_(2e-2)
    model = prepare_for_inference(model, 'cuda')
    for m in model.modules():                              # the hand-written kernels: run-to-run identical outputs
        if direct and isinstance(m, FusedConvBNAct) and 'direct' in m.candidates(False):
            m.impl = 'direct'
    kw = dict(thing_list=[1], label_divisor=1000, stuff_area=16, void_label=0, nms_threshold=0.1, nms_kernel=7,
              confidence_thr=0.5, median_kernel_size=ks, padding_factor=32)
    if render:
        return EN.PanopticDeepLabRenderEngine3d(model, coarse_boundaries=True, **kw)
    return EN.PanopticDeepLabEngine3d(model, **kw)


def _impls(engine):
    from empanada_amd.models.panoptic_deeplab import FusedConvBNAct
    return {n: m.impl for n, m in engine.model.named_modules() if isinstance(m, FusedConvBNAct)}


def _host(res):
    """the comparable part of a result: volumes as numpy, counts, z range, datasets (dtype, chunks, contents)"""
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
        if exp['datasets'][c] is None:
            assert got['datasets'][c] is None
            continue
        assert got['datasets'][c][:2] == exp['datasets'][c][:2]
        np.testing.assert_array_equal(got['datasets'][c][2], exp['datasets'][c][2], err_msg=f'dataset of class {c}')
        np.testing.assert_array_equal(got['datasets'][c][2][slice(*got['z_range'])], got['volumes'][c])


def _run(engine, vol, path, **kw):
    from empanada_amd.inference.driver import infer_volume
    from empanada_amd.zarr_utils import ZarrV2Group
    res = infer_volume(engine, vol, out=ZarrV2Group(str(path)), **dict(KW, **kw))
    return res, _host(res)


_CASES = {}


@pytest.fixture
def case(tmp_path_factory):
    """(engine, volume, the plain path's result) per (axes, render): computed once, shared, never modified"""
    def get(axes, render):
        key = (axes, render)
        if key not in _CASES:
            eng = _CASES[('engine', render)] = _CASES.get(('engine', render)) or _engine(render=render)
            vol = SY.em_volume(SHAPE, seed=3)
            _, exp = _run(eng, vol, tmp_path_factory.mktemp('plain') / 'pred.zarr', axes=axes, batch_pixels=1 << 22)
            assert exp['volumes'][1].max() > 0 or exp['volumes'][2].max() > 0, "the random model should segment something"
            _CASES[key] = (eng, vol, exp)
        return _CASES[key]
    return get


@pytest.mark.parametrize('render', [False, True])
@pytest.mark.parametrize('axes', [ORTHO, ('xy',)])
def test_pipeline_equals_plain_path(tmp_path, case, axes, render):
    from empanada_amd.inference.pipeline import VolumePipeline
    eng, vol, exp = case(axes, render)
    pipe = VolumePipeline(eng, tune=False, graph=True, overlap=True, batch_pixels=1 << 22)
    res, got = _run(eng, vol, tmp_path / 'pred.zarr', axes=axes, pipeline=pipe)
    _assert_same(got, exp)
    assert got['datasets'][1][0] == np.uint32 and got['datasets'][2][0] == np.uint8
    assert got['datasets'][1][1] == (1,) + SHAPE[1:]
    info = res['pipeline']
    assert info['graph'] is True and info['overlap'] is (len(axes) > 1) and info['head_bytes'] > 0
    assert sum(info['tuned'].values()) == len(_impls(eng))
    assert eng.model.defer_up4 is False                    # the model is handed back as it was


@pytest.mark.parametrize('switch', ['no_graph', 'no_overlap', 'auto_without_memory'])
def test_each_switch_alone(tmp_path, case, switch):
    from empanada_amd.inference.pipeline import VolumePipeline
    eng, vol, exp = case(ORTHO, False)
    kw = {'no_graph': dict(graph=False, overlap=True), 'no_overlap': dict(graph=True, overlap=False),
          'auto_without_memory': dict(graph=True, overlap='auto', mem_budget=1)}[switch]
    pipe = VolumePipeline(eng, tune=False, batch_pixels=1 << 22, **kw)
    res, got = _run(eng, vol, tmp_path / 'pred.zarr', axes=ORTHO, pipeline=pipe)
    _assert_same(got, exp)
    assert res['pipeline']['graph'] is (switch != 'no_graph')
    assert res['pipeline']['overlap'] is (switch == 'no_graph')


def test_planes_of_several_batches(tmp_path, case):
    """17 + 17 + 6 slices of the padded xy plane: the [s, e) views and a last batch of another size (a second graph);
    xz and yz take three calls each as well"""
    from empanada_amd.inference.pipeline import VolumePipeline
    eng, vol, _ = case(ORTHO, False)
    f = int(getattr(eng, 'padding_factor', 16))
    bp = 17 * (-(-SHAPE[1] // f) * f) * (-(-SHAPE[2] // f) * f)
    _, exp = _run(eng, vol, tmp_path / 'plain.zarr', axes=ORTHO, batch_pixels=bp)
    pipe = VolumePipeline(eng, tune=False, graph=True, overlap=True, batch_pixels=bp)
    _, got = _run(eng, vol, tmp_path / 'pred.zarr', axes=ORTHO, pipeline=pipe)
    _assert_same(got, exp)
    sizes = sorted(k[0][0] for k in pipe._graphed._graphs if k[0][2:] == (-(-SHAPE[1] // f) * f, -(-SHAPE[2] // f) * f))
    assert sizes == [6, 17]                                # the xy plane: two batch sizes, one graph each
    assert len(pipe._graphed._graphs) >= 4


def test_tuner_save_and_load(tmp_path, monkeypatch):
    from empanada_amd import models
    from empanada_amd.inference.pipeline import VolumePipeline
    vol = SY.em_volume(SHAPE, seed=3)
    eng = _engine()
    pipe = VolumePipeline(eng, tune=True, graph=True, overlap=True, batch_pixels=1 << 22)
    res, got = _run(eng, vol, tmp_path / 'a.zarr', axes=('xy',), pipeline=pipe)
    assert res['pipeline']['tuned'] and sum(res['pipeline']['tuned'].values()) == len(_impls(eng))
    _, exp = _run(eng, vol, tmp_path / 'b.zarr', axes=('xy',), batch_pixels=1 << 22)     # the now tuned engine
    _assert_same(got, exp)
    pipe.save_tune(tmp_path / 'tune.json')
    assert json.load(open(tmp_path / 'tune.json')) == _impls(eng)

    def no_timing(*a, **k):
        raise AssertionError("tune=<path> must not time anything")
    monkeypatch.setattr(models, 'tune_fused_convs', no_timing)
    fresh = _engine(direct=False)
    pipe2 = VolumePipeline(fresh, tune=str(tmp_path / 'tune.json'), graph=True, overlap=True, batch_pixels=1 << 22)
    res2, got2 = _run(fresh, vol, tmp_path / 'c.zarr', axes=('xy',), pipeline=pipe2)
    assert _impls(fresh) == _impls(eng) and res2['pipeline']['tuned'] == res['pipeline']['tuned']
    _assert_same(got2, exp)


def test_downsampled_render_engine(tmp_path):
    from empanada_amd.inference.pipeline import VolumePipeline
    eng = _CASES.get(('engine', True)) or _engine(render=True)
    vol = SY.em_volume(SHAPE, seed=3)
    _, exp = _run(eng, vol, tmp_path / 'plain.zarr', axes=ORTHO, batch_pixels=1 << 22, downsample_f=2)
    pipe = VolumePipeline(eng, tune=False, graph=True, overlap=True, batch_pixels=1 << 22)
    _, got = _run(eng, vol, tmp_path / 'pred.zarr', axes=ORTHO, downsample_f=2, pipeline=pipe)
    _assert_same(got, exp)
    assert got['volumes'][1].shape == SHAPE


def test_one_pipeline_two_volumes(tmp_path, case):
    from empanada_amd.data import DeviceVolume
    from empanada_amd.inference.pipeline import VolumePipeline
    eng, vol, exp = case(ORTHO, False)
    pipe = VolumePipeline(eng, tune=False, graph=True, overlap='auto', batch_pixels=1 << 22)
    res, got = _run(eng, vol, tmp_path / 'a.zarr', axes=ORTHO, pipeline=pipe)
    _assert_same(got, exp)
    assert res['pipeline']['overlap'] is True              # the two sets are a few MiB
    vol2 = SY.em_volume((24, 100, 40), seed=5)
    _, exp2 = _run(eng, vol2, tmp_path / 'plain2.zarr', axes=ORTHO, batch_pixels=1 << 22)
    dv = DeviceVolume(vol2, NORMS['mean'], NORMS['std'], int(getattr(eng, 'padding_factor', 16)), 'cuda')   # passed in
    _, got2 = _run(eng, dv, tmp_path / 'b.zarr', axes=ORTHO, pipeline=pipe)
    _assert_same(got2, exp2)
    _, got = _run(eng, vol, tmp_path / 'c.zarr', axes=ORTHO, pipeline=pipe)            # and back: buffers, graphs reused
    _assert_same(got, exp)


def test_unsupported_combinations_raise_before_gpu_work(case):
    from empanada_amd.inference.driver import infer_volume
    from empanada_amd.inference.pipeline import VolumePipeline
    eng, vol, _ = case(('xy',), False)
    other = _CASES.get(('engine', True)) or _engine(render=True)
    pipe = VolumePipeline(other, tune=False)
    with pytest.raises(ValueError, match='another engine'):
        infer_volume(eng, vol, pipeline=pipe, **KW)
    assert pipe._streams is None and pipe._graphed is None and pipe._store == [None, None]
    with pytest.raises(ValueError, match='batch_pixels'):
        infer_volume(eng, vol, batch_pixels=1 << 20, pipeline=VolumePipeline(eng, tune=False, batch_pixels=1 << 22), **KW)
    with pytest.raises(ValueError, match='overlap'):
        VolumePipeline(eng, overlap='sometimes')
    with pytest.raises(ValueError, match='no such file'):
        VolumePipeline(eng, tune='/nonexistent/tune.json')
    with pytest.raises(TypeError):
        infer_volume(eng, vol, NORMS, [1, 2], ORTHO, 0.25, 0.25, 30, 2, 2, 0.75, False, None, None, 1 << 22, 2, None, 1,
                     VolumePipeline(eng, tune=False))


# ----------------------------------------------------------------------------------------------- two ranks over gloo
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank(rank, world, port, q):
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        from empanada_amd import models
        from empanada_amd.inference.driver import infer_volume
        from empanada_amd.inference.pipeline import VolumePipeline
        searched = []
        tune = models.tune_fused_convs

        def counting(*a, **k):
            searched.append(rank)
            return tune(*a, **k)
        models.tune_fused_convs = counting
        eng = _engine(direct=rank == 0)                     # rank 1 starts from other choices than rank 0
        pipe = VolumePipeline(eng, tune=True, graph=True, overlap=True, batch_pixels=1 << 22)
        res = infer_volume(eng, SY.em_volume(SHAPE, seed=3), axes=ORTHO, group=dist.group.WORLD, pipeline=pipe, **KW)
        host = _host(res)
        q.put((rank, _impls(eng), len(searched), host['volumes'], host['z_range'], host['instances'], res['pipeline']))
    finally:
        dist.destroy_process_group()


def test_two_ranks_adopt_rank0_choices_and_stitch(tmp_path):
    import torch.multiprocessing as mp
    from empanada_amd.inference.driver import infer_volume
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = {}
    import queue
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
    assert got[0][0] == got[1][0], "rank 1 must adopt rank 0's per-site choices"
    assert got[0][1] == 1 and got[1][1] == 0, "only rank 0 runs the search"
    assert got[0][3] == (0, 20) and got[1][3] == (20, 40)
    assert got[0][5]['tuned'] == got[1][5]['tuned'] and got[0][4] == got[1][4]
    eng = _engine()
    from empanada_amd.models.panoptic_deeplab import FusedConvBNAct
    for n, m in eng.model.named_modules():
        if isinstance(m, FusedConvBNAct):
            m.impl = got[0][0][n]
    exp = _host(infer_volume(eng, SY.em_volume(SHAPE, seed=3), axes=ORTHO, batch_pixels=1 << 22, **KW))
    assert exp['instances'] == got[0][4]
    for c in (1, 2):
        np.testing.assert_array_equal(np.concatenate([got[0][2][c], got[1][2][c]], axis=0), exp['volumes'][c],
                                      err_msg=f'class {c}')
