"""Skeletons of a resident label volume (_hip.label_thin / label_graph / graph_finish / label_edt,
csrc/emp_label_thin.hip) against a device copy of the same bytes and against _hip.label_grow.

The volume is synthetic.planted_labels(fill=0.08, rmin=6, rmax=24, seed=4321) as uint32 labels, the volume that
tools/bench_measure.py, bench_separate.py and bench_mesh.py use (6 781 objects at 1024^3).  In one process: --warmup
rounds, then --rounds rounds in which follow each other -- a device copy of the volume (`b.copy_(a)`, the yardstick),
_hip.label_thin (thin), _hip.label_graph + graph_finish of the skeleton (graph), _hip.label_edt of the volume at the cap
and the gather at the vertices (radius), and _hip.label_grow from the cores that _hip.label_erode leaves at --radius,
every core a seed with its object's label, back to the whole objects (grow).  Each is timed by the wall clock between device synchronisations (allocations and host syncs
included) and also given as a multiple of the copy of the same round.  One more, untimed, thinning is driven step by
step and reads after every mark how many tiles are due for the passes.

usage: PYTHONPATH=. python tools/bench_skeleton.py [--sizes 512 1024] [--rounds 3] [--json FILE] [--md FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from empanada_amd import _hip                                   # noqa: E402
from empanada_amd import separation as SP                       # noqa: E402
from empanada_amd import synthetic as SY                        # noqa: E402
from bench_separate import stats, timed, fmt                    # noqa: E402


def _align(x, a=256):
    return -(-x // a) * a


def due_tiles(thin):
    """tiles due for the passes, over the z-blocks: the second byte array of emp_label_thin's workspace (16 bytes of
    counters, the int32 list, the marks for the mark step, the marks for the passes, each on a multiple of 256)"""
    D, H, W = (int(s) for s in thin.slab.shape)
    total = 0
    for b in thin._blocks:
        n = -(-(b['z1'] - b['z0']) // 8) * -(-H // 8) * -(-W // 64)
        at = _align(_align(256 + 4 * n) + n)
        total += int(b['work'][at:at + n].sum())
    return total


def due_profile(vol):
    thin = _hip.LabelThin(vol)
    listed, due, deleted = sum(b['listed'] for b in thin._blocks), [], []
    while True:
        thin.mark()
        due.append(due_tiles(thin))
        for s in range(8):
            thin.run_pass(s)
        deleted.append(thin.deleted())
        if deleted[-1] == 0:
            return listed, due, deleted


def markdown(rows, a):
    head = "| | " + " | ".join(f"{r['size']}³" for r in rows) + " |"
    lines = ["# Skeletons of the labelled objects: `_hip.label_thin` / `label_graph` against a device copy and E6", "",
             f"`tools/bench_skeleton.py --sizes {' '.join(str(r['size']) for r in rows)} --rounds {a.rounds}`: "
             "median (min – max) of the wall clock in ms between device synchronisations, one process, the "
             "measurements of a round in turn.", "", head, "|---|" + "---|" * len(rows)]
    names = {'copy': 'device copy of the volume', 'thin': '`_hip.label_thin`', 'graph': '`label_graph` + `graph_finish`',
             'radius': f'`_hip.label_edt`, cap {a.cap}, and the gather', 'grow': f'`_hip.label_grow` from the cores of an erosion by r = {a.radius}'}
    for k, name in names.items():
        lines.append(f"| {name} | " + " | ".join(fmt(r['wall_ms'][k]) for r in rows) + " |")
    for k in ('thin', 'graph', 'radius', 'grow'):
        lines.append(f"| {k} / copy | " + " | ".join(f"{r['over_copy'][k]:.1f}" for r in rows) + " |")
    for k, name in (('objects', 'objects'), ('voxels', 'labelled voxels'), ('vertices', 'skeleton voxels'),
                    ('edges', 'edges'), ('iterations', 'iterations'), ('launches', 'launches of mark and pass'),
                    ('tiles', 'tiles'), ('listed', 'listed tiles')):
        lines.append(f"| {name} | " + " | ".join(f"{r[k]:,}" for r in rows) + " |")
    lines += ["", "Share of the listed tiles that are due for the passes, per iteration (and voxels deleted):", ""]
    for r in rows:
        lines.append(f"* {r['size']}³: " + ", ".join(f"{d / max(r['listed'], 1):.2f} ({n:,})"
                                                      for d, n in zip(r['due_per_iteration'], r['deleted_per_iteration'])))
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[512, 1024])
    ap.add_argument('--radius', type=int, default=6)
    ap.add_argument('--cap', type=int, default=4096)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--json', default=None)
    ap.add_argument('--md', default=None, help='write the table as markdown')
    a = ap.parse_args()
    r2, min_core, _ = SP.check((a.radius, 1))
    _hip.require_gpu()
    dev = torch.device('cuda')
    rows = []
    for S in a.sizes:
        lab, _ = SY.planted_labels((S, S, S), fill=0.08, rmin=6, rmax=24, seed=4321)
        vol = torch.from_numpy(lab.astype(np.uint32).view(np.int32)).to(dev).view(torch.uint32)
        del lab
        other = torch.empty_like(vol.view(torch.int32))
        seeds = _hip.label_erode(vol, r2)
        n_seeds = int(torch.unique(seeds.view(torch.int32)).numel()) - 1
        wall, info, ginfo = {}, {}, {}
        for i in range(a.warmup + a.rounds):
            def radius(keys):
                edt = _hip.label_edt(vol, (1, 1, 1), a.cap)
                return edt.view(torch.int16).reshape(-1)[keys & 0xffffffff].to(torch.int32) & 0xffff
            steps = [('copy', lambda: other.copy_(vol.view(torch.int32))),
                     ('thin', lambda: _hip.label_thin(vol, info=info))]
            out = {}
            for k, fn in steps:
                ms, out[k] = timed(fn)
                if i >= a.warmup:
                    wall.setdefault(k, []).append(ms)
            ms, g = timed(lambda: _hip.graph_finish(*_hip.label_graph(out['thin'], info=ginfo), vol.shape))
            keys = _hip.label_graph(out['thin'])[0][0]
            ms_r, _ = timed(lambda: radius(keys))
            ms_g, _ = timed(lambda: _hip.label_grow(vol, seeds).owners())
            if i >= a.warmup:
                for k, v in (('graph', ms), ('radius', ms_r), ('grow', ms_g)):
                    wall.setdefault(k, []).append(v)
            n_obj = int(g[3].shape[0])
            del out, g, keys
        listed, due, deleted = due_profile(vol)
        copy = float(np.median(wall['copy']))
        row = dict(size=S, rounds=a.rounds, warmup=a.warmup, bytes=vol.numel() * 4, objects=n_obj, seeds=n_seeds,
                   voxels=int(torch.count_nonzero(vol.view(torch.int32))), vertices=ginfo['vertices'],
                   edges=ginfo['edges'], iterations=info['iterations'], launches=info['launches'],
                   tiles=-(-S // 8) * -(-S // 8) * -(-S // 64), listed=listed, due_per_iteration=due,
                   deleted_per_iteration=deleted, wall_ms={k: stats(v) for k, v in wall.items()},
                   over_copy={k: float(np.median(v)) / copy for k, v in wall.items()})
        rows.append(row)
        print(json.dumps(row), flush=True)
        del vol, other, seeds
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, 'w') as fh:
            json.dump(rows, fh, indent=1)
    if a.md:
        with open(a.md, 'w') as fh:
            fh.write(markdown(rows, a))


if __name__ == '__main__':
    main()
