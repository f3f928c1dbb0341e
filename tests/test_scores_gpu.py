"""GPU: evaluation.volume_scores (overlap table from csrc/emp_overlaps.hip, slab by slab) against the host scorer on
numpy's table and against volume_pq; against the Evaluator over two tracker json files with the metric names of the
reference's scripts/evaluate3d.py:204-209; and infer_volume(..., ground_truth=) on the engine and volume of
tests/test_driver_gpu.py, in stack and orthoplane mode, plain, with pipeline= and with window_slices=."""
import numpy as np
import pytest
import torch

from empanada_amd import evaluation as EV
from empanada_amd import synthetic as SY

pytestmark = pytest.mark.gpu

NORMS = dict(mean=0.508979, std=0.148561)
SHAPE = (20, 64, 72)
KEYS = {'IoU', 'F1_50', 'F1_75', 'Precision_50', 'Precision_75', 'Recall_50', 'Recall_75', 'PQ', 'n_gt', 'n_pred',
        'n_matched'}


def np_table(g, p):
    st = np.stack([np.asarray(g).reshape(-1).astype(np.int64), np.asarray(p).reshape(-1).astype(np.int64)], 1)
    pairs, counts = np.unique(st, axis=0, return_counts=True)
    keep = (pairs != 0).any(axis=1)
    return pairs[keep], counts[keep].astype(np.int64)


@pytest.fixture(scope='module')
def scene():
    """tests/test_pipeline_gpu.py::test_evaluator_on_tracker_jsons: one miss, one shrunk object, one false positive"""
    lab_gt, _ = SY.planted_labels(SHAPE, fill=0.2, rmin=4, rmax=10, seed=3)
    lab_pr = lab_gt.copy()
    ids = np.unique(lab_gt)[1:]
    lab_pr[lab_pr == ids[0]] = 0
    lab_pr[:, :, 36:][lab_pr[:, :, 36:] == ids[1]] = 0
    lab_pr[0:2, 0:2, 0:2] = lab_gt.max() + 5
    expected = EV.scores_from_overlaps(*np_table(lab_gt, lab_pr))
    assert expected['n_pred'] >= 2 and 0 < expected['n_matched'] < expected['n_gt']
    return lab_gt, lab_pr, expected


def _u32(a):
    return torch.from_numpy(a.astype(np.uint32).view(np.int32)).cuda().view(torch.uint32)


def test_volume_scores_on_tensors_numpy_slabs_and_zarr(scene, tmp_path):
    from empanada_amd.zarr_utils import ZarrV2Group
    gt, pr, expected = scene
    pq, n_gt, n_pred, n_matched = EV.volume_pq(gt, pr)
    assert abs(expected['PQ'] - pq) < 1e-12
    assert (expected['n_gt'], expected['n_pred'], expected['n_matched']) == (n_gt, n_pred, n_matched)

    assert EV.volume_scores(_u32(gt), _u32(pr)) == expected
    assert EV.volume_scores(torch.from_numpy(gt.astype(np.int64)).cuda(), _u32(pr)) == expected
    assert EV.volume_scores(gt, pr, slab_rows=3) == expected                   # uint16 on the host, 7 slabs, a short one
    assert EV.volume_scores(gt.astype(np.int64), _u32(pr), slab_rows=7) == expected
    assert EV.volume_scores(gt, pr) == expected

    group = ZarrV2Group(str(tmp_path / 'labels.zarr'))
    sets = {}
    for name, lab in (('gt', gt), ('pred', pr)):
        sets[name] = group.create_dataset(name, shape=SHAPE, dtype=np.uint32, chunks=(1, None, None))
        sets[name][...] = lab
    assert EV.volume_scores(sets['gt'], sets['pred'], slab_rows=6) == expected
    assert EV.volume_scores(group['gt'], _u32(pr), slab_rows=20) == expected

    pairs, counts = EV.volume_overlaps(gt, pr, slab_rows=4)
    ref_p, ref_c = np_table(gt, pr)
    np.testing.assert_array_equal(pairs, ref_p)
    np.testing.assert_array_equal(counts, ref_c)

    low = EV.volume_scores(gt, pr, iou_thr=0.4, slab_rows=5)
    assert low == EV.scores_from_overlaps(ref_p, ref_c, iou_thr=0.4)
    assert abs(low['PQ'] - EV.volume_pq(gt, pr, iou_thr=0.4)[0]) < 1e-12

    mask_g, mask_p = (gt > 0).astype(np.uint8), (pr > 0)
    stuff = EV.volume_scores(mask_g, mask_p, instances=False, slab_rows=9)
    assert stuff == {'IoU': expected['IoU']}
    assert EV.volume_scores(torch.from_numpy(mask_g).cuda(), _u32(pr), instances=False) == stuff

    with pytest.raises(ValueError):
        EV.volume_scores(gt, pr[:-1])
    with pytest.raises(ValueError):
        EV.volume_scores(gt.astype(np.int64) - 1, pr)
    with pytest.raises(ValueError):
        EV.volume_scores(gt.astype(np.float32), pr)
    with pytest.raises(ValueError):
        EV.volume_scores(gt, pr, slab_rows=0)


def test_volume_scores_equal_the_evaluator_on_tracker_jsons(scene, tmp_path):
    """the json route of scripts/evaluate3d.py:204-214 and the voxel route give the same numbers"""
    from empanada_amd.inference import patterns as PA
    gt, pr, expected = scene
    paths = []
    for name, lab in (('gt', gt), ('pred', pr)):
        pan = torch.from_numpy(np.where(lab > 0, 1000 + lab, 0).astype(np.int32)).cuda()
        tr = PA.track_stack(pan, 'xy', SHAPE, [1], [1], 1000, 0.25, 0.25)[0]
        p = str(tmp_path / f'{name}.json')
        tr.write_to_json(p)
        paths.append(p)
    ev = EV.Evaluator(semantic_metrics={'IoU': EV.iou},
                      instance_metrics={'F1_50': EV.f1_50, 'F1_75': EV.f1_75, 'Precision_50': EV.precision_50,
                                        'Precision_75': EV.precision_75, 'Recall_50': EV.recall_50,
                                        'Recall_75': EV.recall_75},
                      panoptic_metrics={'PQ': EV.panoptic_quality})
    res = ev(paths[0], paths[1])
    got = EV.volume_scores(_u32(gt), _u32(pr))
    assert set(res) == KEYS - {'n_gt', 'n_pred', 'n_matched'} and set(got) == KEYS
    for k, v in res.items():
        print(k, v, got[k])
        assert abs(v - got[k]) < 1e-12, k


# ---------------------------------------------------------------------------------------------------- infer_volume
def _engine(ks=3):
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
                                      nms_threshold=0.1, nms_kernel=7, confidence_thr=0.5, median_kernel_size=ks,
                                      padding_factor=32)


def _np_vol(v):
    return v.view(torch.int32).cpu().numpy().view(np.uint32) if v.dtype == torch.uint32 else v.cpu().numpy()


@pytest.fixture(scope='module')
def driver_case():
    """engine and volume of tests/test_driver_gpu.py, the plain orthoplane result without a ground truth, and a ground
    truth made from it: `own` as predicted, `other` with a block cleared and a block added in both classes"""
    from empanada_amd.inference.driver import infer_volume
    engine = _engine()
    vol = SY.em_volume((40, 72, 88), seed=3)
    kw = dict(norms=NORMS, labels=[1, 2], min_size=30, min_span=2, batch_pixels=1 << 22)
    plain = infer_volume(engine, vol, **kw)
    own = {c: _np_vol(plain['volumes'][c]).copy() for c in (1, 2)}
    assert own[1].max() > 0 or own[2].max() > 0, "the random model should segment something"
    other = {c: own[c].copy() for c in (1, 2)}
    for c in (1, 2):
        other[c][:, 10:30, 20:40] = 0
        other[c][5:9, 40:60, 50:80] = 1 if c == 2 else 1000 + 777
    return engine, vol, kw, plain, own, other


@pytest.mark.parametrize('axes', [('xy', 'xz', 'yz'), ('xy',)])
def test_infer_volume_scores_its_result(driver_case, axes):
    from empanada_amd.inference.driver import infer_volume
    engine, vol, kw, plain, own, other = driver_case
    assert set(plain) == {'volumes', 'z_range', 'instances', 'datasets'}              # the parent commit's keys
    ortho = len(axes) == 3
    # orthoplane mode: class 1 against the plain run's own volume (the same inference, so against itself), class 2
    # against the altered one; stack mode, whose volumes the fixture does not hold: both against the altered ones
    truth = {1: own[1] if ortho else other[1], 2: other[2]}
    res = infer_volume(engine, vol, axes=axes, ground_truth={1: truth[1], 2: torch.from_numpy(truth[2]).cuda()}, **kw)
    assert set(res) == set(plain) | {'scores'} and set(res['scores']) == {1, 2}
    assert set(res['scores'][1]) == KEYS and set(res['scores'][2]) == {'IoU'}
    print(axes, res['scores'])
    assert res['scores'][1] == EV.volume_scores(truth[1], res['volumes'][1])
    assert res['scores'][2] == EV.volume_scores(truth[2], res['volumes'][2], instances=False)
    assert res['scores'][1] == EV.scores_from_overlaps(*np_table(truth[1], _np_vol(res['volumes'][1])))
    if ortho:
        for c in (1, 2):
            assert torch.equal(res['volumes'][c].view(torch.uint8), plain['volumes'][c].view(torch.uint8))
        s = res['scores'][1]
    else:
        s = EV.volume_scores(res['volumes'][1], res['volumes'][1])
    # against itself: every instance matched at IoU 1 (PQ divides by tp + 1e-5)
    assert s['n_gt'] == s['n_pred'] == s['n_matched'] == res['instances'][1]
    assert s['F1_50'] == s['F1_75'] == s['Precision_75'] == s['Recall_75'] == 1 and s['PQ'] == pytest.approx(1, abs=1e-4)
    assert s['IoU'] == 1
    only = infer_volume(engine, vol, axes=('xy',), ground_truth={2: other[2]}, **kw) if not ortho else None
    assert only is None or set(only['scores']) == {2}


def test_pipeline_and_windows_give_the_same_scores(driver_case):
    from empanada_amd.inference.driver import infer_volume
    from empanada_amd.inference.pipeline import VolumePipeline
    engine, vol, kw, plain, own, other = driver_case
    expected = {1: EV.volume_scores(other[1], plain['volumes'][1]),
                2: EV.volume_scores(other[2], plain['volumes'][2], instances=False)}
    res = infer_volume(engine, vol, ground_truth=other, window_slices=8, **kw)
    assert res['scores'] == expected and 'windows' in res
    pipe = VolumePipeline(engine, tune=False, graph=True, overlap=True, batch_pixels=1 << 22)
    piped = infer_volume(engine, vol, ground_truth=other, pipeline=pipe,
                         **{k: v for k, v in kw.items() if k != 'batch_pixels'})
    assert piped['scores'] == expected and 'pipeline' in piped
    without = infer_volume(engine, vol, pipeline=pipe, **{k: v for k, v in kw.items() if k != 'batch_pixels'})
    assert 'scores' not in without


class _Counting(torch.nn.Module):
    def __init__(self, inner):
        super().__init__()
        self.inner = inner
        self.calls = 0

    def forward(self, *args, **kwargs):
        self.calls += 1
        return self.inner(*args, **kwargs)


def test_a_wrong_ground_truth_is_refused_before_the_model_runs(driver_case):
    from empanada_amd.inference.driver import infer_volume
    engine, vol, kw, plain, own, other = driver_case
    model = engine.model
    engine.model = _Counting(model)
    try:
        for gt in ({1: other[1][:-1]}, {2: other[2][:, :, :-1]}, {1: other[1], 2: other[2].reshape(40, 88, 72)},
                   {3: other[1]}):
            with pytest.raises(ValueError):
                infer_volume(engine, vol, ground_truth=gt, **kw)
            with pytest.raises(ValueError):
                infer_volume(engine, vol, ground_truth=gt, window_slices=8, **kw)
        assert engine.model.calls == 0
    finally:
        engine.model = model
