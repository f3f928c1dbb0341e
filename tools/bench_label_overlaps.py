"""Time of the overlap table of two resident uint32 label volumes (_hip.label_overlaps, csrc/emp_overlaps.hip) next to
the route evaluation.volume_pq takes to the same numbers (widen to int64, torch.unique(return_inverse) twice, bincount
into the dense gt x pred table).  The truth is synthetic.planted_labels, the prediction a copy moved by two voxels
along x with every tenth object dropped and the ids changed.  HIP events around whole calls, after warm-up; the
wrapper's two entry points (count + scan; extract + sort + reduce) are also timed apart through _hip.PROFILE.
profiles/label_overlaps.md holds a run.

usage: PYTHONPATH=. python tools/bench_label_overlaps.py [--sizes 512 1024] [--dense-up-to 512] [--iters 10] [--json FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from empanada_amd import _hip                                   # noqa: E402
from empanada_amd import synthetic as SY                        # noqa: E402

HBM_PEAK = 8.0e12          # bytes/s, MI355X specification; about 6.3e12 is what a plain copy reaches


def volumes(S, dev):
    lab, _ = SY.planted_labels((S, S, S), fill=0.08, rmin=6, rmax=24, seed=4321)
    gt = torch.from_numpy(lab.astype(np.int32)).to(dev)
    pred = torch.roll(gt, 2, dims=2)
    pred[:, :, :2] = 0
    pred = torch.where((pred > 0) & (pred % 10 != 0), pred + 100000, torch.zeros_like(pred))
    return gt.view(torch.uint32), pred.contiguous().view(torch.uint32), int(lab.max())


def timed(fn, warmup, iters):
    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return out, ms


def peak_extra(fn):
    """peak of torch's allocations during fn() above what was held before it"""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    return out, torch.cuda.max_memory_allocated() - base


def dense_route(gt, pred):
    """the table part of evaluation.volume_pq, on device tensors"""
    g, p = gt.view(torch.int32).reshape(-1).long(), pred.view(torch.int32).reshape(-1).long()
    gl, gi = torch.unique(g, return_inverse=True)
    pl, pi = torch.unique(p, return_inverse=True)
    joint = torch.bincount(gi * len(pl) + pi, minlength=len(gl) * len(pl)).reshape(len(gl), len(pl))
    return gl, pl, joint


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[512, 1024])
    ap.add_argument('--dense-up-to', type=int, default=512)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    _hip.require_gpu()
    dev = torch.device('cuda')
    rows = []
    for S in a.sizes:
        gt, pred, n_obj = volumes(S, dev)
        in_bytes = gt.numel() * 8
        info = {}
        (pairs, counts), ms = timed(lambda: _hip.label_overlaps(gt, pred, info=info), 3, a.iters)
        _, extra = peak_extra(lambda: _hip.label_overlaps(gt, pred))
        _hip.PROFILE = {}
        for _ in range(a.iters):
            _hip.label_overlaps(gt, pred)
        torch.cuda.synchronize()
        steps = {k: float(np.median([e0.elapsed_time(e1) for e0, e1, _, _ in v])) for k, v in _hip.PROFILE.items()}
        _hip.PROFILE = None
        med = float(np.median(ms))
        row = dict(size=S, objects=n_obj, input_bytes=in_bytes, spans=info['spans'], pairs=int(pairs.shape[0]),
                   new_ms_median=med, new_ms_min=float(min(ms)), new_ms_max=float(max(ms)),
                   new_input_bytes_per_s=in_bytes / (med * 1e-3), new_share_of_hbm_peak=in_bytes / (med * 1e-3) / HBM_PEAK,
                   new_peak_temp_bytes=int(extra), new_work_bytes=info['work_bytes'], step_ms_median=steps,
                   step_bytes_per_s={k: in_bytes / (v * 1e-3) for k, v in steps.items()})
        if S <= a.dense_up_to:
            (gl, pl, joint), dms = timed(lambda: dense_route(gt, pred), 1, max(3, a.iters // 3))
            _, dextra = peak_extra(lambda: dense_route(gt, pred))
            gi, pi = torch.nonzero(joint, as_tuple=True)
            keep = (gl[gi] != 0) | (pl[pi] != 0)
            same = (torch.equal(torch.stack([gl[gi][keep], pl[pi][keep]], 1), pairs)
                    and torch.equal(joint[gi, pi][keep], counts))
            row.update(dense_ms_median=float(np.median(dms)), dense_ms_min=float(min(dms)), dense_peak_temp_bytes=int(dextra),
                       dense_table_cells=int(joint.numel()), tables_equal=bool(same),
                       speedup=float(np.median(dms)) / med)
            del gl, pl, joint
        rows.append(row)
        print(json.dumps(row), flush=True)
        del gt, pred, pairs, counts
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, 'w') as fh:
            json.dump(rows, fh, indent=1)


if __name__ == '__main__':
    main()
