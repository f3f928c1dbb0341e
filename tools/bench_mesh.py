"""Surface meshes of a resident label volume (_hip.label_mesh / mesh_finish / mesh_smooth, csrc/emp_label_mesh.hip)
against a device copy of the same bytes.

The volume is synthetic.planted_labels(fill=0.08, rmin=6, rmax=24, seed=4321) as uint32 labels, the volume that
tools/bench_measure.py and bench_separate.py use (6 781 objects at 1024^3).  In one process: --warmup rounds, then
--rounds rounds in which label_mesh (emit), mesh_finish (finish), 10 iterations of mesh_smooth (smooth) and `b.copy_(a)`
of the volume into a buffer of its size follow each other.  The three steps are timed as a whole by the wall clock
between device synchronisations (allocations and host syncs included), their entry points by HIP events (_hip.PROFILE),
the copy by events of its own; every time is also given as a multiple of the copy of the same round.  The peak of
torch's allocator over a round is reported against the card's HBM.

usage: PYTHONPATH=. python tools/bench_mesh.py [--sizes 512 1024] [--rounds 5] [--iterations 10] [--json FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from empanada_amd import _hip                                   # noqa: E402
from empanada_amd import synthetic as SY                        # noqa: E402

HBM_BYTES = 288e9          # MI355X specification


def stats(ms):
    return dict(median=float(np.median(ms)), min=float(min(ms)), max=float(max(ms)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[512, 1024])
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--iterations', type=int, default=10)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    _hip.require_gpu()
    dev = torch.device('cuda')
    rows = []
    for S in a.sizes:
        lab, _ = SY.planted_labels((S, S, S), fill=0.08, rmin=6, rmax=24, seed=4321)
        vol = torch.from_numpy(lab.astype(np.uint32).view(np.int32)).to(dev).view(torch.uint32)
        del lab
        nbytes = vol.numel() * 4
        buf = torch.empty_like(vol.view(torch.int32))
        wall = {'emit': [], 'finish': [], 'smooth': []}
        copies, info, finfo = [], {}, {}
        _hip.PROFILE = None
        base = torch.cuda.memory_allocated()
        for i in range(a.warmup + a.rounds):
            if i == a.warmup:
                _hip.PROFILE = {}
                torch.cuda.reset_peak_memory_stats()
            t = []
            torch.cuda.synchronize()
            t.append(time.perf_counter())
            keys, quads = _hip.label_mesh(vol, info=info)
            torch.cuda.synchronize()
            t.append(time.perf_counter())
            vertices, faces, objects = _hip.mesh_finish(keys, quads, vol.shape, info=finfo)
            del keys, quads
            torch.cuda.synchronize()
            t.append(time.perf_counter())
            smooth = _hip.mesh_smooth(vertices, faces, a.iterations)
            torch.cuda.synchronize()
            t.append(time.perf_counter())
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            buf.copy_(vol.view(torch.int32))
            e1.record()
            torch.cuda.synchronize()
            if i >= a.warmup:
                for k, (t0, t1) in zip(wall, zip(t[:-1], t[1:])):
                    wall[k].append((t1 - t0) * 1e3)
                copies.append(e0.elapsed_time(e1))
            nv, nq, n = int(vertices.shape[0]), int(faces.shape[0]), int(objects.shape[0])
            del vertices, faces, objects, smooth
        peak = torch.cuda.max_memory_allocated() - base
        entry = {k: stats([e0.elapsed_time(e1) for e0, e1, _, _ in v]) for k, v in _hip.PROFILE.items()}
        calls = {k: len(v) // a.rounds for k, v in _hip.PROFILE.items()}
        _hip.PROFILE = None
        copy = float(np.median(copies))
        row = dict(size=S, rounds=a.rounds, warmup=a.warmup, iterations=a.iterations, bytes=nbytes, objects=n,
                   vertices=nv, quads=nq, blocks=info['blocks'], emit_work_bytes=info['work_bytes'],
                   finish_work_bytes=finfo['work_bytes'], wall_ms={k: stats(v) for k, v in wall.items()},
                   copy_ms=stats(copies), over_copy={k: float(np.median(v)) / copy for k, v in wall.items()},
                   entry_ms=entry, entry_calls_per_round=calls, peak_bytes_beside_volume_and_copy=int(peak),
                   peak_share_of_hbm=(peak + 2 * nbytes) / HBM_BYTES)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del vol, buf
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, 'w') as fh:
            json.dump(rows, fh, indent=1)


if __name__ == '__main__':
    main()
