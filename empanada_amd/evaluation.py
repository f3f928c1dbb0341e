"""Panoptic quality between two labelled volumes (the "PQ vs CPU ref" half of the headline metric).

Formula: empanada/evaluation/panoptic_metrics.py:3-54; matching: Hungarian on the instance IoU matrix with the
matches kept at IoU >= 0.5 (empanada/evaluation/evaluator.py:88-89 -> rle_matcher, inference/matcher.py:136-232).
The IoU table comes from one joint histogram of (gt label, pred label) over the voxels.

Two routes to that histogram: `volume_pq` builds it densely with library calls (small volumes, and the independent check
of the other route); `volume_scores` reads it as a SPARSE table of (gt label, pred label, voxels) from
_hip.label_overlaps (csrc/emp_overlaps.hip) slab by slab, rank by rank, and scores it with `scores_from_overlaps`:
IoU, F1 / precision / recall at 0.5 and 0.75 and PQ, what scripts/evaluate3d.py:204-218 prints per class.
"""
import numpy as np
import torch
from scipy.optimize import linear_sum_assignment

from .tables import _SLAB_VOXELS, _labels_to_device, gather_keyed, merge_keyed, volume_slabs, volume_table  # noqa: F401

__all__ = ['panoptic_quality', 'volume_pq', 'merge_overlaps', 'gather_overlaps', 'scores_from_overlaps', 'volume_overlaps',
           'volume_scores', 'f1', 'ap', 'precision', 'recall', 'f1_50', 'f1_75', 'precision_50',
           'precision_75', 'recall_50', 'recall_75', 'iou', 'Evaluator']


def panoptic_quality(gt_matched, gt_unmatched, pred_matched, pred_unmatched, matched_ious):
    """panoptic_metrics.py:3-54"""
    matched_ious = np.asarray(matched_ious, dtype=float)
    fn = len(gt_unmatched)
    fp = len(pred_unmatched)
    tp_ious = matched_ious[matched_ious >= 0.5]
    tp = len(tp_ious)
    failed = np.count_nonzero(matched_ious < 0.5)
    fp += failed
    fn += failed
    if tp + fp + fn == 0:
        return 1
    sq = tp_ious.sum() / (tp + 1e-5)
    rq = tp / (tp + 0.5 * fp + 0.5 * fn)
    return sq * rq


def volume_pq(gt, pred, iou_thr=0.5):
    """PQ of `pred` against `gt` (integer label volumes of equal shape, 0 = background; numpy or torch).
    Returns (pq, n_gt, n_pred, n_matched)."""
    g = torch.as_tensor(np.asarray(gt).astype(np.int64) if not isinstance(gt, torch.Tensor) else gt).reshape(-1).long()
    p = torch.as_tensor(np.asarray(pred).astype(np.int64) if not isinstance(pred, torch.Tensor) else pred).reshape(-1).long()
    if p.device != g.device:
        p = p.to(g.device)
    gl, gi = torch.unique(g, return_inverse=True)
    pl, pi = torch.unique(p, return_inverse=True)
    joint = torch.bincount(gi * len(pl) + pi, minlength=len(gl) * len(pl)).reshape(len(gl), len(pl)).cpu().numpy()
    gl, pl = gl.cpu().numpy(), pl.cpu().numpy()
    gk, pk = gl != 0, pl != 0
    inter = joint[gk][:, pk].astype(np.float64)
    ga = joint[gk].sum(axis=1).astype(np.float64)
    pa = joint[:, pk].sum(axis=0).astype(np.float64)
    gl, pl = gl[gk], pl[pk]
    if len(gl) == 0 or len(pl) == 0:
        return panoptic_quality([], gl, [], pl, []), len(gl), len(pl), 0
    iou = inter / (ga[:, None] + pa[None, :] - inter)
    rows, cols = linear_sum_assignment(iou, maximize=True)
    keep = iou[rows, cols] >= iou_thr
    rows, cols = rows[keep], cols[keep]
    pq = panoptic_quality(gl[rows], np.setdiff1d(gl, gl[rows]), pl[cols], np.setdiff1d(pl, pl[cols]), iou[rows, cols])
    return float(pq), len(gl), len(pl), int(len(rows))


# ----------------------------------------------------------------------------- detection metrics
def _counts(gt_unmatched, pred_unmatched, matched_ious, iou_thr):
    matched_ious = np.asarray(matched_ious, dtype=float)
    tp = int(np.count_nonzero(matched_ious >= iou_thr))
    failed = int(np.count_nonzero(matched_ious < iou_thr))       # a failed match costs one fp and one fn
    return tp, len(pred_unmatched) + failed, len(gt_unmatched) + failed


def f1(gt_matched, gt_unmatched, pred_matched, pred_unmatched, matched_ious, iou_thr=0.5):
    """instance_metrics.py:3-54 (1 for two empty masks)"""
    tp, fp, fn = _counts(gt_unmatched, pred_unmatched, matched_ious, iou_thr)
    return 1 if tp + fp + fn == 0 else tp / (tp + 0.5 * fp + 0.5 * fn)


def ap(gt_matched, gt_unmatched, pred_matched, pred_unmatched, matched_ious, iou_thr=0.5):
    """instance_metrics.py:56-108"""
    tp, fp, fn = _counts(gt_unmatched, pred_unmatched, matched_ious, iou_thr)
    return 1 if tp + fp + fn == 0 else tp / (tp + fp + fn)


def precision(gt_matched, gt_unmatched, pred_matched, pred_unmatched, matched_ious, iou_thr=0.5):
    """instance_metrics.py:110-156"""
    tp, fp, _ = _counts(gt_unmatched, pred_unmatched, matched_ious, iou_thr)
    return 1 if tp + fp == 0 else tp / (tp + fp)


def recall(gt_matched, gt_unmatched, pred_matched, pred_unmatched, matched_ious, iou_thr=0.5):
    """instance_metrics.py:158-206"""
    tp, _, fn = _counts(gt_unmatched, pred_unmatched, matched_ious, iou_thr)
    return 1 if tp + fn == 0 else tp / (tp + fn)


def f1_50(**kw): return f1(**kw, iou_thr=0.5)
def f1_75(**kw): return f1(**kw, iou_thr=0.75)
def precision_50(**kw): return precision(**kw, iou_thr=0.5)
def precision_75(**kw): return precision(**kw, iou_thr=0.75)
def recall_50(**kw): return recall(**kw, iou_thr=0.5)
def recall_75(**kw): return recall(**kw, iou_thr=0.75)


def iou(gt_rle, pred_rle):
    """semantic_metrics.py:4-26: IoU of two (n, 2) (start, run) tables."""
    from .array_utils import rle_iou
    if len(gt_rle) == 0 and len(pred_rle) == 0:
        return 1
    if len(gt_rle) == 0 or len(pred_rle) == 0:
        return 0
    return rle_iou(gt_rle[:, 0], gt_rle[:, 1], pred_rle[:, 0], pred_rle[:, 1])


class Evaluator:
    """evaluator.py:24-122: scores a predicted tracker json against a ground-truth tracker json (the files
    InstanceTracker.write_to_json produces).  Matching runs through the product rle_matcher (box screening and
    run intersections in libemp_hip.so).

    Deviation, on purpose: the reference hands the json's {'box', 'rle'} entries straight to rle_matcher, which
    reads 'starts'/'runs' and therefore raises KeyError on any non-empty file (evaluator.py:88-89 with
    matcher.py:104-118); here the rle strings are decoded first."""

    def __init__(self, semantic_metrics=None, instance_metrics=None, panoptic_metrics=None):
        self.semantic_metrics = semantic_metrics
        self.instance_metrics = instance_metrics
        self.panoptic_metrics = panoptic_metrics

    @staticmethod
    def _unpack_instance_dict(instance_dict):
        labels, boxes, encodings = [], [], []
        for k, v in instance_dict.items():
            labels.append(int(k))
            boxes.append(v['box'])
            encodings.append(v['rle'])
        return np.array(labels), np.array(boxes), encodings

    @staticmethod
    def _decoded(instance_dict):
        from .array_utils import string_to_rle
        out = {}
        for k, v in instance_dict.items():
            starts, runs = string_to_rle(v['rle'])
            out[int(k)] = {'box': tuple(v['box']), 'starts': starts, 'runs': runs}
        return out

    def __call__(self, gt_json_fpath, pred_json_fpath, return_instances=False):
        import json
        from .array_utils import merge_rles, string_to_rle
        from .inference.matcher import rle_matcher
        with open(gt_json_fpath) as f:
            gt_json = json.load(f)
        with open(pred_json_fpath) as f:
            pred_json = json.load(f)
        assert gt_json['class_id'] == pred_json['class_id'], "Prediction and ground truth classes must match!"

        _, _, gt_enc = self._unpack_instance_dict(gt_json['instances'])
        _, _, pred_enc = self._unpack_instance_dict(pred_json['instances'])
        semantic_results, instance_results, panoptic_results = {}, {}, {}

        if self.semantic_metrics is not None:
            gt_rle = np.concatenate([np.stack(string_to_rle(e), axis=1) for e in gt_enc])
            if len(pred_enc) > 1:                        # evaluator.py:6-22 (a single prediction scores as [-1, -1])
                pr = np.concatenate([np.stack(string_to_rle(e), axis=1) for e in pred_enc])
                pred_rle = np.stack(merge_rles(pr[:, 0], pr[:, 1]), axis=1)
            else:
                pred_rle = np.array([[-1, -1]])
            semantic_results = {n: fn(gt_rle, pred_rle) for n, fn in self.semantic_metrics.items()}

        gt_matched = pred_matched = gt_unmatched = pred_unmatched = matched_ious = None
        if self.instance_metrics is not None or self.panoptic_metrics is not None:
            matched, all_labels, matched_ious = rle_matcher(self._decoded(gt_json['instances']),
                                                            self._decoded(pred_json['instances']))
            gt_matched, pred_matched = matched
            gt_unmatched = np.setdiff1d(all_labels[0], gt_matched)
            pred_unmatched = np.setdiff1d(all_labels[1], pred_matched)
            kw = dict(gt_matched=gt_matched, pred_matched=pred_matched, gt_unmatched=gt_unmatched,
                      pred_unmatched=pred_unmatched, matched_ious=matched_ious)
            if self.instance_metrics is not None:
                instance_results = {n: fn(**kw) for n, fn in self.instance_metrics.items()}
            if self.panoptic_metrics is not None:
                panoptic_results = {n: fn(**kw) for n, fn in self.panoptic_metrics.items()}

        results = {**semantic_results, **instance_results, **panoptic_results}
        if return_instances:
            return results, dict(gt_matched=gt_matched, pred_matched=pred_matched, gt_unmatched=gt_unmatched,
                                 pred_unmatched=pred_unmatched, matched_ious=matched_ious)
        return results


# ----------------------------------------------------------------------------- scores from the sparse overlap table
def _table(pairs, counts):
    """(pairs, counts) as one (n, 3) int64 table; a tensor, on its device, if either is one"""
    dev = next((x.device for x in (pairs, counts) if isinstance(x, torch.Tensor)), None)
    if dev is None:
        return np.concatenate([np.asarray(pairs, dtype=np.int64).reshape(-1, 2),
                               np.asarray(counts, dtype=np.int64).reshape(-1, 1)], axis=1)
    return torch.cat([torch.as_tensor(pairs).to(dev).reshape(-1, 2).long(),
                      torch.as_tensor(counts).to(dev).reshape(-1, 1).long()], dim=1)


def _merge3(tables):
    return merge_keyed(tables, 3, [0, 1], [2])


def _gather3(table, group):
    return gather_keyed(table, 3, _merge3, group)


def _split(table):
    """an (n, 3) table as (pairs, counts), each contiguous"""
    if isinstance(table, torch.Tensor):
        return table[:, :2].contiguous(), table[:, 2].contiguous()
    return np.ascontiguousarray(table[:, :2]), np.ascontiguousarray(table[:, 2])


def merge_overlaps(tables):
    """Sum of overlap tables: `tables` is a sequence of (pairs (n, 2), counts (n,)) -- of a volume's slabs, of the
    ranks' shares -- and the result is one such table with every distinct pair once, its counts added, ascending by
    (gt label, pred label).  numpy in, numpy out; with any torch tensor among them the result is a torch table on that
    tensor's device.  Integer sums: exact whatever the order."""
    return _split(_merge3([_table(p, c) for p, c in tables]))


def gather_overlaps(pairs, counts, group=None):
    """The ranks' overlap tables added up: every rank of `group` passes its own table and receives the table of all of
    them (one count all-gather + one padded all-gather, as the run tables travel in inference/sharded.py).  Without an
    initialised process group the table comes back merged with itself, i.e. sorted."""
    return _split(_gather3(_table(pairs, counts), group))


def _match_components(gi, pi, iou, n_g):
    """Maximum-IoU assignment on the bipartite graph of the pairs with a positive intersection, one connected component
    at a time: edges (gi[k], pi[k]) with weight iou[k] > 0.  Pairs that do not intersect have IoU 0 and add nothing to
    the optimum, so this is the assignment of the dense matrix wherever that optimum is unique.  Returns the indices k
    of the chosen edges."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    if len(gi) == 0:
        return np.zeros(0, np.int64)
    n = n_g + int(pi.max()) + 1
    graph = coo_matrix((np.ones(len(gi), np.int8), (gi, n_g + pi)), shape=(n, n))
    comp = connected_components(graph, directed=False)[1][gi]
    order = np.argsort(comp, kind='stable')
    bounds = np.flatnonzero(np.concatenate([[True], comp[order][1:] != comp[order][:-1], [True]]))
    single = np.diff(bounds) == 1
    chosen = [order[bounds[:-1][single]]]                               # an edge alone in its component is the match
    for lo, hi in zip(bounds[:-1][~single], bounds[1:][~single]):
        e = order[lo:hi]
        gu, gr = np.unique(gi[e], return_inverse=True)
        pu, pc = np.unique(pi[e], return_inverse=True)
        block = np.zeros((len(gu), len(pu)), dtype=np.float64)
        block[gr, pc] = iou[e]
        slot = np.full(block.shape, -1, dtype=np.int64)
        slot[gr, pc] = e
        rows, cols = linear_sum_assignment(block, maximize=True)
        k = slot[rows, cols]
        chosen.append(k[k >= 0])                                        # a zero entry is no pair at all
    return np.sort(np.concatenate(chosen))


def scores_from_overlaps(pairs, counts, iou_thr=0.5, instances=True, return_instances=False):
    """Scores of a predicted label volume against the ground truth from their overlap table alone: `pairs` (n, 2) the
    distinct (gt label, pred label) != (0, 0) with `counts` (n,) voxels each, as _hip.label_overlaps / merge_overlaps
    give them (numpy or torch).  No GPU is needed.

    The area of a label is its row (column) sum, IoU is formed only for the pairs that intersect, and the assignment
    that maximises the total IoU is solved per connected component of those pairs; matches with IoU >= iou_thr
    (> 0) are kept -- what rle_matcher does on the dense IoU matrix (inference/matcher.py:48-52), and the same result
    whenever that optimum is unique.  The match then goes through this module's metric functions, so the numbers follow
    the Evaluator's rules (f1_75 counts a match below 0.75 as one false positive and one false negative, PQ does the
    same below 0.5).

    Returns {'IoU', 'F1_50', 'F1_75', 'Precision_50', 'Precision_75', 'Recall_50', 'Recall_75', 'PQ', 'n_gt',
    'n_pred', 'n_matched'}; with instances=False (stuff classes) {'IoU'} alone.  'IoU' is that of the two foreground
    masks: voxels where both are non-zero over voxels where either is, 1 when both volumes are empty and 0 when one is.
    The reference's Evaluator scores a class with fewer than two predicted instances as the run table [[-1, -1]]
    (evaluation/evaluator.py:6-22), an accident of its run merging; that is not reproduced here: one predicted
    instance is scored like any other number.  With return_instances the match itself is returned as well:
    (scores, {'gt_matched', 'gt_unmatched', 'pred_matched', 'pred_unmatched', 'matched_ious'})."""
    if isinstance(pairs, torch.Tensor):
        pairs = pairs.cpu().numpy()
    if isinstance(counts, torch.Tensor):
        counts = counts.cpu().numpy()
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    counts = np.asarray(counts, dtype=np.int64).reshape(-1)
    if len(pairs) != len(counts):
        raise ValueError(f"scores_from_overlaps: {len(pairs)} pairs, {len(counts)} counts")
    if not iou_thr > 0:
        raise ValueError(f"scores_from_overlaps: iou_thr must be > 0 (got {iou_thr}): pairs that do not intersect are "
                         "not in the table")
    g, p = pairs[:, 0], pairs[:, 1]
    both = int(counts[(g > 0) & (p > 0)].sum())
    either = int(counts[(g > 0) | (p > 0)].sum())
    scores = {'IoU': 1.0 if either == 0 else both / either}
    if not instances:
        return (scores, None) if return_instances else scores
    gl, g_idx = np.unique(g[g > 0], return_inverse=True)
    pl, p_idx = np.unique(p[p > 0], return_inverse=True)
    ga = np.zeros(len(gl), np.int64)
    pa = np.zeros(len(pl), np.int64)
    np.add.at(ga, g_idx.reshape(-1), counts[g > 0])
    np.add.at(pa, p_idx.reshape(-1), counts[p > 0])
    edge = (g > 0) & (p > 0)
    gi = np.searchsorted(gl, g[edge])
    pi = np.searchsorted(pl, p[edge])
    inter = counts[edge].astype(np.float64)
    iou_e = inter / (ga[gi].astype(np.float64) + pa[pi].astype(np.float64) - inter)
    k = _match_components(gi, pi, iou_e, len(gl))
    k = k[iou_e[k] >= iou_thr]
    match = dict(gt_matched=gl[gi[k]], gt_unmatched=np.setdiff1d(gl, gl[gi[k]]), pred_matched=pl[pi[k]],
                 pred_unmatched=np.setdiff1d(pl, pl[pi[k]]), matched_ious=iou_e[k])
    scores.update(F1_50=float(f1_50(**match)), F1_75=float(f1_75(**match)),
                  Precision_50=float(precision_50(**match)), Precision_75=float(precision_75(**match)),
                  Recall_50=float(recall_50(**match)), Recall_75=float(recall_75(**match)),
                  PQ=float(panoptic_quality(**match)), n_gt=len(gl), n_pred=len(pl), n_matched=int(len(k)))
    return (scores, match) if return_instances else scores


def volume_overlaps(gt, pred, *, slab_rows=None, group=None):
    """The overlap table of two label volumes of equal shape as a numpy (pairs, counts): `gt` and `pred` are numpy
    arrays, tensors or anything that has a shape and can be sliced along axis 0 (a ZarrV2Array, say).  Every slab of
    slab_rows indices along axis 0 goes to the device (host data is uploaded slab by slab, so neither volume has to be
    resident as a whole) and through _hip.label_overlaps, and the tables are added; slab_rows=None takes device tensors
    whole and host data in slabs of about 2^27 voxels.  With `group` the ranks' tables are added too: every rank passes
    its own share of the volume and all receive the table of the whole."""
    from . import _hip
    _hip.require_gpu()
    if tuple(gt.shape) != tuple(pred.shape):
        raise ValueError(f"volume_scores: gt is {tuple(gt.shape)}, pred {tuple(pred.shape)}")
    if len(gt.shape) < 1:
        raise ValueError("volume_scores: the volumes need at least one axis")
    on_dev = [x.device for x in (gt, pred) if isinstance(x, torch.Tensor) and x.is_cuda]
    if len(set(on_dev)) > 1:
        raise ValueError(f"volume_scores: gt and pred are on different devices ({on_dev[0]}, {on_dev[1]})")
    dev = on_dev[0] if on_dev else torch.device('cuda', torch.cuda.current_device())
    slabs = volume_slabs("volume_scores", gt.shape, slab_rows, len(on_dev) == 2, what="indices along axis 0")
    tables = []
    for z, z1, _, _ in slabs:
        g = _labels_to_device(gt[z:z1], dev)
        p = _labels_to_device(pred[z:z1], dev)
        tables.append(_table(*_hip.label_overlaps(g, p)))
        del g, p
    return _split(volume_table(tables, 3, _merge3, _gather3, group, dev))


def volume_scores(gt, pred, *, instances=True, iou_thr=0.5, slab_rows=None, group=None):
    """scores_from_overlaps of two label volumes of equal shape (see there for what is returned): the table is read on
    the device by volume_overlaps -- slab by slab for host data, nothing widened, and added over the ranks of `group`,
    each of which passes its own share and receives the scores of the whole."""
    pairs, counts = volume_overlaps(gt, pred, slab_rows=slab_rows, group=group)
    return scores_from_overlaps(pairs, counts, iou_thr=iou_thr, instances=instances)
