"""CPU: the host half of the voxel-level scorer (empanada_amd/evaluation.py: merge_overlaps, scores_from_overlaps,
gather_overlaps).  The overlap table the HIP kernel produces is stood in for by numpy's unique over the stacked labels
(tests/test_overlaps_gpu.py pins the kernel to that same expression), the assignment per connected component is checked
against a dense scipy assignment built here and against volume_pq, and the sum over ranks runs under gloo, world 2."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
from scipy.optimize import linear_sum_assignment

from empanada_amd import evaluation as EV
from empanada_amd import synthetic as SY

SHAPE = (20, 64, 72)
SEEDS = (3, 5, 11)


def np_table(g, p):
    """the overlap table: distinct (g, p) != (0, 0) with their voxel counts, ascending"""
    st = np.stack([np.asarray(g).reshape(-1).astype(np.int64), np.asarray(p).reshape(-1).astype(np.int64)], 1)
    pairs, counts = np.unique(st, axis=0, return_counts=True)
    keep = (pairs != 0).any(axis=1)
    return pairs[keep], counts[keep].astype(np.int64)


def perturbed(seed):
    """tests/test_pipeline_gpu.py::test_evaluator_on_tracker_jsons: one miss, one shrunk object, one false positive"""
    lab_gt, _ = SY.planted_labels(SHAPE, fill=0.2, rmin=4, rmax=10, seed=seed)
    lab_pr = lab_gt.copy()
    ids = np.unique(lab_gt)[1:]
    lab_pr[lab_pr == ids[0]] = 0
    lab_pr[:, :, 36:][lab_pr[:, :, 36:] == ids[1]] = 0
    lab_pr[0:2, 0:2, 0:2] = lab_gt.max() + 5
    return lab_gt, lab_pr


def straddling():
    """One prediction (7) over two ground-truth objects: 900 of the 1000 voxels of object 1 (IoU 900 / 1150 = 0.78) and
    150 of the 1000 of object 2 (IoU 150 / 1900 = 0.08); prediction 8 holds the other 850 voxels of object 2 (IoU 0.85).
    Objects 3 and 4 share prediction 9 alone: 800 of 1000 (IoU 800 / 1200 = 0.67) and 200 of 1000 (IoU 200 / 1800 =
    0.11), so the assignment has to choose, and the loser is left without a match.  Every optimum is unique by a wide margin."""
    gt = np.zeros((10, 40, 60), dtype=np.uint16)
    pr = np.zeros_like(gt)
    gt[:, 0:10, 0:10] = 1
    gt[:, 0:10, 10:20] = 2
    pr[:, 0:9, 0:10] = 7                     # 900 voxels of object 1
    pr[:, 0:10, 10:20] = 8
    pr[:, 0:10, 10:20][:, :, :2][:, :7] = 7  # 140 voxels of object 2 ...
    pr[0, 7, 10:20] = 7                      # ... and 10 more: 150, prediction 8 keeps 850
    gt[:, 20:30, 0:10] = 3
    gt[:, 20:30, 30:40] = 4
    pr[:, 20:28, 0:10] = 9                   # 800 voxels of object 3
    pr[:, 20:22, 30:40] = 9                  # 200 voxels of object 4
    return gt, pr


def dense_match(gt, pred, thr, noise=None):
    """rle_matcher's rule (inference/matcher.py:36-52) on the dense IoU matrix of two label volumes: Hungarian
    assignment maximising the total IoU, matches below thr dropped.  noise: a generator that jitters the matrix by
    1e-9, to probe whether the optimum is unique."""
    gl, gi = np.unique(gt, return_inverse=True)
    pl, pi = np.unique(pred, return_inverse=True)
    joint = np.zeros((len(gl), len(pl)), dtype=np.int64)
    np.add.at(joint, (gi.reshape(-1), pi.reshape(-1)), 1)
    gk, pk = gl != 0, pl != 0
    inter = joint[gk][:, pk].astype(np.float64)
    ga = joint[gk].sum(axis=1).astype(np.float64)
    pa = joint[:, pk].sum(axis=0).astype(np.float64)
    gl, pl = gl[gk], pl[pk]
    iou = inter / (ga[:, None] + pa[None, :] - inter)
    cost = iou if noise is None else iou + noise.uniform(-1e-9, 1e-9, size=iou.shape)
    rows, cols = linear_sum_assignment(cost, maximize=True)
    keep = iou[rows, cols] >= thr
    rows, cols = rows[keep], cols[keep]
    return dict(gt_matched=gl[rows], gt_unmatched=np.setdiff1d(gl, gl[rows]), pred_matched=pl[cols],
                pred_unmatched=np.setdiff1d(pl, pl[cols]), matched_ious=iou[rows, cols])


SCENES = {f'planted{seed}': (lambda seed=seed: perturbed(seed)) for seed in SEEDS}
SCENES['straddling'] = straddling


@pytest.fixture(scope='module')
def scenes():
    out = {}
    for name, make in SCENES.items():
        gt, pr = make()
        out[name] = (gt, pr, np_table(gt, pr))
    return out


# ------------------------------------------------------------------------------------------------ merge_overlaps
@pytest.mark.parametrize('split', [(20,), (10, 10), (3, 3, 3, 3, 3, 3, 2), (1, 19), (7, 1, 12), (1,) * 20])
def test_merge_of_slabs_is_the_table_of_the_volume(scenes, split):
    gt, pr, (pairs, counts) = scenes['planted3']
    b = np.concatenate([[0], np.cumsum(split)])
    assert b[-1] == gt.shape[0]
    tables = [np_table(gt[lo:hi], pr[lo:hi]) for lo, hi in zip(b[:-1], b[1:])]
    got_p, got_c = EV.merge_overlaps(tables)
    assert got_p.dtype == np.int64 and got_c.dtype == np.int64
    np.testing.assert_array_equal(got_p, pairs)
    np.testing.assert_array_equal(got_c, counts)
    tp, tc = EV.merge_overlaps([(torch.from_numpy(p), torch.from_numpy(c)) for p, c in tables][::-1])
    assert isinstance(tp, torch.Tensor) and tp.dtype == torch.int64 and tc.dtype == torch.int64
    np.testing.assert_array_equal(tp.numpy(), pairs)
    np.testing.assert_array_equal(tc.numpy(), counts)


def test_merge_of_nothing_and_of_large_labels():
    p, c = EV.merge_overlaps([])
    assert p.shape == (0, 2) and c.shape == (0,)
    p, c = EV.merge_overlaps([(np.zeros((0, 2), np.int64), np.zeros(0, np.int64))] * 2)
    assert p.shape == (0, 2) and c.shape == (0,)
    big = 2 ** 32 - 1
    a = (np.array([[big, 1], [0, big], [2 ** 31, 0]]), np.array([2 ** 31, 5, 7]))
    b = (np.array([[0, big], [big, 1], [1, 1]]), np.array([1, 2 ** 31, 3]))
    for tables in ([a, b], [(torch.tensor(a[0]), torch.tensor(a[1])), (torch.tensor(b[0]), torch.tensor(b[1]))]):
        p, c = EV.merge_overlaps(tables)
        np.testing.assert_array_equal(np.asarray(p), [[0, big], [1, 1], [2 ** 31, 0], [big, 1]])
        np.testing.assert_array_equal(np.asarray(c), [6, 3, 7, 2 ** 32])      # a sum past int32, exact


# ------------------------------------------------------------------------------------------- scores_from_overlaps
@pytest.mark.parametrize('thr', [0.5, 0.4])
@pytest.mark.parametrize('name', list(SCENES))
def test_scores_equal_the_dense_routes(scenes, name, thr):
    gt, pr, (pairs, counts) = scenes[name]
    scores, match = EV.scores_from_overlaps(pairs, counts, iou_thr=thr, return_instances=True)

    pq, n_gt, n_pred, n_matched = EV.volume_pq(torch.from_numpy(gt.astype(np.int64)), torch.from_numpy(pr.astype(np.int64)),
                                               iou_thr=thr)
    assert abs(scores['PQ'] - pq) < 1e-12
    assert (scores['n_gt'], scores['n_pred'], scores['n_matched']) == (n_gt, n_pred, n_matched)

    ref = dense_match(gt, pr, thr)
    order = np.argsort(ref['gt_matched'])
    np.testing.assert_array_equal(match['gt_matched'], ref['gt_matched'][order])
    np.testing.assert_array_equal(match['pred_matched'], ref['pred_matched'][order])
    np.testing.assert_allclose(match['matched_ious'], ref['matched_ious'][order], rtol=0, atol=1e-15)
    np.testing.assert_array_equal(match['gt_unmatched'], ref['gt_unmatched'])
    np.testing.assert_array_equal(match['pred_unmatched'], ref['pred_unmatched'])
    # the optimum is unique: no jitter of the matrix far below any IoU difference of the scene moves a match
    rng = np.random.default_rng(0)
    for _ in range(5):
        again = dense_match(gt, pr, thr, noise=rng)
        np.testing.assert_array_equal(again['gt_matched'], ref['gt_matched'])
        np.testing.assert_array_equal(again['pred_matched'], ref['pred_matched'])

    for key, fn in (('F1_50', EV.f1_50), ('F1_75', EV.f1_75), ('Precision_50', EV.precision_50),
                    ('Precision_75', EV.precision_75), ('Recall_50', EV.recall_50), ('Recall_75', EV.recall_75),
                    ('PQ', EV.panoptic_quality)):
        assert abs(scores[key] - fn(**ref)) < 1e-12, key
    inter = np.count_nonzero((gt > 0) & (pr > 0))
    union = np.count_nonzero((gt > 0) | (pr > 0))
    assert scores['IoU'] == inter / union
    assert set(scores) == {'IoU', 'F1_50', 'F1_75', 'Precision_50', 'Precision_75', 'Recall_50', 'Recall_75', 'PQ',
                           'n_gt', 'n_pred', 'n_matched'}


def test_planted_scenes_have_a_miss_a_shrunk_object_and_a_false_positive(scenes):
    for seed in SEEDS:
        gt, pr, (pairs, counts) = scenes[f'planted{seed}']
        s = EV.scores_from_overlaps(pairs, counts)
        assert s['n_gt'] >= 4 and s['n_pred'] == s['n_gt'], seed       # one lost, one invented
        assert s['n_matched'] <= s['n_gt'] - 1 and s['F1_75'] <= s['F1_50'] < 1 and 0 < s['PQ'] < 1


def test_the_straddling_prediction_takes_the_larger_object(scenes):
    gt, pr, (pairs, counts) = scenes['straddling']
    table = {(int(g), int(p)): int(c) for (g, p), c in zip(pairs, counts)}
    assert table[(1, 7)] == 900 and table[(2, 7)] == 150 and table[(2, 8)] == 850
    assert table[(3, 9)] == 800 and table[(4, 9)] == 200
    scores, match = EV.scores_from_overlaps(pairs, counts, return_instances=True)
    assert list(match['gt_matched']) == [1, 2, 3] and list(match['pred_matched']) == [7, 8, 9]
    np.testing.assert_allclose(match['matched_ious'], [900 / 1150, 850 / 1000, 800 / 1200], rtol=0, atol=1e-15)
    assert list(match['gt_unmatched']) == [4] and len(match['pred_unmatched']) == 0
    assert scores['F1_50'] == 3 / 3.5 and scores['F1_75'] == 2 / (2 + 0.5 * 1 + 0.5 * 2)
    # with the bar at 0.1 object 4 still goes unmatched: prediction 9 is taken, IoU 0.11 or not
    low = EV.scores_from_overlaps(pairs, counts, iou_thr=0.1)
    assert low['n_matched'] == 3


def test_empty_sides_single_object_and_stuff():
    none = (np.zeros((0, 2), np.int64), np.zeros(0, np.int64))
    s = EV.scores_from_overlaps(*none)
    assert s['IoU'] == 1 and s['PQ'] == 1 and s['F1_50'] == 1 and s['Precision_75'] == 1 and s['Recall_75'] == 1
    assert (s['n_gt'], s['n_pred'], s['n_matched']) == (0, 0, 0)

    gt = np.zeros((4, 6, 8), np.uint8)
    gt[1:3, 2:5, 2:6] = 9
    for g, p, n_gt, n_pred in ((gt, np.zeros_like(gt), 1, 0), (np.zeros_like(gt), gt, 0, 1)):
        s = EV.scores_from_overlaps(*np_table(g, p))
        assert s['IoU'] == 0 and s['PQ'] == 0 and s['F1_50'] == 0
        assert (s['n_gt'], s['n_pred'], s['n_matched']) == (n_gt, n_pred, 0)

    pr = np.zeros_like(gt)
    pr[1:3, 2:5, 3:6] = 4                                              # 18 of the object's 24 voxels
    s = EV.scores_from_overlaps(*np_table(gt, pr))
    assert s['IoU'] == 18 / 24 and s['n_matched'] == 1 and s['F1_50'] == 1 and s['F1_75'] == 1
    assert abs(s['PQ'] - (18 / 24) / (1 + 1e-5)) < 1e-15
    s = EV.scores_from_overlaps(*np_table(gt, gt))
    assert s['IoU'] == 1 and s['F1_75'] == 1 and abs(s['PQ'] - 1) < 2e-5

    stuff = EV.scores_from_overlaps(*np_table(gt, pr), instances=False)
    assert stuff == {'IoU': 18 / 24}
    assert EV.scores_from_overlaps(*none, instances=False) == {'IoU': 1}
    t = np_table(gt, pr)
    assert EV.scores_from_overlaps(torch.from_numpy(t[0]), torch.from_numpy(t[1])) == EV.scores_from_overlaps(*t)
    with pytest.raises(ValueError):
        EV.scores_from_overlaps(*t, iou_thr=0.0)
    with pytest.raises(ValueError):
        EV.scores_from_overlaps(t[0], t[1][:-1])


# ------------------------------------------------------------------------------------------------ over the ranks
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, bounds, q):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        gt, pr = perturbed(3)
        lo, hi = int(bounds[rank]), int(bounds[rank + 1])
        pairs, counts = np_table(gt[lo:hi], pr[lo:hi])
        if rank == 1:                                                   # torch tables travel as well as numpy ones
            pairs, counts = torch.from_numpy(pairs), torch.from_numpy(counts)
        pairs, counts = EV.gather_overlaps(pairs, counts)
        q.put((rank, np.asarray(pairs), np.asarray(counts), EV.scores_from_overlaps(pairs, counts)))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize('split', [(10, 10), (20, 0)])
def test_every_rank_gets_the_scores_of_the_whole_volume(scenes, split):
    """world 2 under gloo; (20, 0): a rank whose share is empty"""
    gt, pr, (pairs, counts) = scenes['planted3']
    expected = EV.scores_from_overlaps(pairs, counts)
    bounds = np.concatenate([[0], np.cumsum(split)])
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, bounds, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = [q.get(timeout=180) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert sorted(g[0] for g in got) == [0, 1]
    for _, got_pairs, got_counts, scores in got:
        np.testing.assert_array_equal(got_pairs, pairs)
        np.testing.assert_array_equal(got_counts, counts)
        assert scores == expected


def test_gather_without_a_process_group_sorts_the_table(scenes):
    _, _, (pairs, counts) = scenes['straddling']
    p, c = EV.gather_overlaps(pairs[::-1], counts[::-1])
    np.testing.assert_array_equal(p, pairs)
    np.testing.assert_array_equal(c, counts)
