"""Filling the enclosed holes of a resident label volume (_hip.label_holes, holes.plan, the paint in place;
csrc/emp_holes.hip) against a device copy of the same bytes and against _hip.label_components of the same volume.

The volume is synthetic.planted_labels(fill=0.08, rmin=6, rmax=24, seed=4321), the one of tools/bench_components.py, as
uint32 labels, with a cavity planted into every --every-th object: a box of (2 r + 1)^3 voxels, r = --radius, zeroed at
the centre of the object's bounding box (where the box centre lies inside the object and deep enough the cavity is
closed and walled by the object alone; the plan's stats say how many were).  Per round, in one process: the volume is
restored from a pristine copy (`a.copy_(b)`, timed by HIP events: the yardstick), then label_holes + plan + paint in
place run, timed as a whole by the wall clock (allocations and host syncs included) and per entry point by HIP events
(_hip.PROFILE): emp_label_holes_count is step 1, emp_label_holes step 2, emp_label_components_paint the fill; then
_hip.label_components(volume, 26) of the same (filled) volume by the wall clock and its two entry points by events.

usage: PYTHONPATH=. python tools/bench_holes.py [--sizes 512 1024] [--rounds 10] [--json FILE]
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
from empanada_amd import holes as HO                            # noqa: E402
from empanada_amd import synthetic as SY                        # noqa: E402


def stats(ms):
    return dict(median=float(np.median(ms)), min=float(min(ms)), max=float(max(ms)))


def plant_cavities(vol, every, radius):
    """zero a (2 r + 1)^3 box at the centre of the bounding box of every `every`-th object; returns how many"""
    table = _hip.label_components(vol, 26).table.cpu().numpy()
    D, H, W = vol.shape
    bits = vol.view(torch.int32)
    n = 0
    for row in table[::every]:
        c = [(int(row[3 + a]) + int(row[6 + a])) // 2 for a in range(3)]
        if all(radius < c[a] < s - 1 - radius for a, s in enumerate((D, H, W))):
            bits[c[0] - radius:c[0] + radius + 1, c[1] - radius:c[1] + radius + 1, c[2] - radius:c[2] + radius + 1] = 0
            n += 1
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[512, 1024])
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--every', type=int, default=3, help='a cavity in every n-th object')
    ap.add_argument('--radius', type=int, default=2)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    _hip.require_gpu()
    dev = torch.device('cuda')
    rows = []
    for S in a.sizes:
        lab, _ = SY.planted_labels((S, S, S), fill=0.08, rmin=6, rmax=24, seed=4321)
        vol = torch.from_numpy(lab.astype(np.uint32).view(np.int32)).to(dev).view(torch.uint32)
        del lab
        planted = plant_cavities(vol, a.every, a.radius)
        pristine = vol.view(torch.int32).clone()
        row = dict(size=S, rounds=a.rounds, warmup=a.warmup, bytes=vol.numel() * 4, cavities_planted=planted)
        info, cinfo, wall, cwall, copies, plan_ms, st = {}, {}, [], [], [], [], None
        _hip.PROFILE = None
        for i in range(a.warmup + a.rounds):
            if i == a.warmup:
                _hip.PROFILE = {}
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            vol.view(torch.int32).copy_(pristine)
            e1.record()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            lh = _hip.label_holes(vol, info=info)
            t1 = time.perf_counter()
            lut, st = HO.plan(lh.table, vol.shape)
            t2 = time.perf_counter()
            lh.paint(lut)
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            lc = _hip.label_components(vol, 26, info=cinfo)
            torch.cuda.synchronize()
            t4 = time.perf_counter()
            if i >= a.warmup:
                copies.append(e0.elapsed_time(e1))
                wall.append((t3 - t0) * 1e3)
                plan_ms.append((t2 - t1) * 1e3)
                cwall.append((t4 - t3) * 1e3)
            n_cav, n_comp = lh.n, lc.n
            del lh, lc
        prof = _hip.PROFILE
        _hip.PROFILE = None
        entry = {k: stats([e0.elapsed_time(e1) for e0, e1, _, _ in v]) for k, v in prof.items()}
        copy = float(np.median(copies))
        dev_ms = sum(entry[k]['median'] for k in ('emp_label_holes_count', 'emp_label_holes', 'emp_label_components_paint'))
        e3_ms = entry['emp_label_measure_count']['median'] + entry['emp_label_components']['median']
        row.update(components=n_cav, objects=n_comp, zero_runs=info['runs'], label_runs=cinfo['runs'],
                   work_bytes=info['work_bytes'], plan=st, entry_ms=entry, copy_ms=stats(copies),
                   fill_wall_ms=stats(wall), plan_host_ms=stats(plan_ms), label_components_wall_ms=stats(cwall),
                   entries_over_copy=dev_ms / copy, fill_wall_over_copy=float(np.median(wall)) / copy,
                   entries_over_e3_entries=dev_ms / e3_ms,
                   fill_wall_over_label_components_wall=float(np.median(wall)) / float(np.median(cwall)))
        rows.append(row)
        print(json.dumps(row), flush=True)
        del vol, pristine
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, 'w') as fh:
            json.dump(rows, fh, indent=1)


if __name__ == '__main__':
    main()
