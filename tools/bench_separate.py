"""Separation of touching objects in a resident label volume (separation.separate_volume, _hip.label_grow;
csrc/emp_label_grow.hip) against a device copy of the same bytes and against _hip.label_erode at the same radius.

The volume is synthetic.planted_labels(fill=0.08, rmin=6, rmax=24, seed=4321), the one of tools/bench_morph.py, as
uint32 labels, with a share of the objects planted as touching pairs: every object whose label is a multiple of
--every gets a twin under the same label, itself moved by --shift voxels along x, wherever the twin meets background
(so a twin may also come to touch another object).  Per size, in one process: --warmup rounds, then --rounds rounds of
every measurement in turn -- a device copy of the volume (`a.copy_(b)`, the yardstick), _hip.label_erode at the radius,
_hip.label_grow alone on the seeds that separate_volume makes, and separate_volume on a fresh copy of the volume (the
copy is not timed).  Each is timed by the wall clock around a call that ends in a device synchronise (allocations
included), and the entry points by HIP events (_hip.PROFILE).

usage: PYTHONPATH=. python tools/bench_separate.py [--sizes 512 1024] [--radius 6] [--rounds 5] [--json FILE] [--md FILE]
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
from empanada_amd import components as CP                       # noqa: E402
from empanada_amd import separation as SP                       # noqa: E402
from empanada_amd import synthetic as SY                        # noqa: E402


def stats(ms):
    return dict(median=float(np.median(ms)), min=float(min(ms)), max=float(max(ms)))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def fmt(s):
    return f"{s['median']:.2f} ({s['min']:.2f} – {s['max']:.2f})"


def planted(S, every, shift, dev):
    """the bench's objects with every `every`-th one doubled `shift` voxels along x under its own label"""
    lab, _ = SY.planted_labels((S, S, S), fill=0.08, rmin=6, rmax=24, seed=4321)
    vol = torch.from_numpy(lab.astype(np.int32)).to(dev)
    del lab
    twin = torch.roll(vol, shift, dims=2)
    twin[:, :, :shift] = 0
    vol = torch.where((vol == 0) & (twin % every == 0), twin, vol)
    return vol.contiguous().view(torch.uint32)


def seeds_of(vol, r2, min_core):
    """the seed volume that separate_volume grows: its steps 1 to 3"""
    cores = _hip.label_components(_hip.label_erode(vol, r2), 6)
    ids, _ = SP._seeds(CP.merged_table(cores, 6)[0], min_core)
    return cores.paint(torch.from_numpy(ids).to(vol.device), dtype=torch.uint32), int(ids.max(initial=0))


def markdown(rows, a):
    r = a.radius
    lines = ["# Separating touching objects: `separation.separate_volume` / `_hip.label_grow` against a device copy and E5", "",
             f"MI355X, one GPU, `PYTHONPATH=. python tools/bench_separate.py --sizes {' '.join(str(x['size']) for x in rows)} "
             f"--radius {r} --rounds {a.rounds}` ({a.warmup} warm-up rounds, then {a.rounds} rounds; median (min – max), ms, "
             "wall clock around a call that ends in a device synchronise, allocations included).  Volume: "
             "`synthetic.planted_labels((S, S, S), fill=0.08, rmin=6, rmax=24, seed=4321)` as uint32 labels, every object "
             f"whose label is a multiple of {a.every} doubled {a.shift} voxels along x under its own label.", ""]
    head = "| uint32 labels | " + " | ".join(f"{x['size']}³ ({x['bytes'] / 1e9:.2f} GB), {x['stats']['objects_in']} objects"
                                             for x in rows) + " |"
    lines += [head, "|---|" + "---|" * len(rows)]
    names = {'copy': 'device copy of the volume', 'erode': f'`_hip.label_erode`, r = {r}',
             'grow': '`_hip.label_grow` alone, on the seeds of that erosion',
             'separate': f'`separate_volume`, r = {r}, min_core = {a.min_core}'}
    for k in ('copy', 'erode', 'grow', 'separate'):
        lines.append(f"| {names[k]} | " + " | ".join(fmt(x['wall_ms'][k]) for x in rows) + " |")
    for k in ('erode', 'grow', 'separate'):
        lines.append(f"| {names[k]} over the copy | " + " | ".join(f"{x['over_copy'][k]:.1f}" for x in rows) + " |")
    lines.append("| `emp_label_grow_*` by HIP events, one growth: init + sweeps + owners | " + " | ".join(
        f"{x['grow_event_ms']['median']:.2f}" for x in rows) + " |")
    lines.append("| of that: init / all sweeps / owners | " + " | ".join(
        " / ".join(f"{x['entry_ms'][k]['median']:.2f}" for k in ('emp_label_grow_init', 'emp_label_grow_sweep',
                                                                   'emp_label_grow_paint')) for x in rows) + " |")
    lines.append("| sweeps of one growth: needed (the last one stores nothing) / launched | " + " | ".join(
        f"{x['grow']['sweeps_needed']} / {x['grow']['sweeps']}" for x in rows) + " |")
    lines.append("| listed tiles of 8 x 8 x 64 (hold a labelled voxel) of all tiles | " + " | ".join(
        f"{x['grow']['active_tiles']:,} of {x['tiles']:,}" for x in rows) + " |")
    lines.append("| seeds | " + " | ".join(f"{x['seeds']:,}" for x in rows) + " |")
    lines.append("| objects separated / pieces added / voxels moved | " + " | ".join(
        f"{x['stats']['objects_separated']:,} / {x['stats']['pieces_added']:,} / {x['stats']['voxels_moved']:,}" for x in rows) + " |")
    lines.append("| workspace of the growth, bytes (state, 8 per voxel, included) | " + " | ".join(
        f"{x['grow']['work_bytes']:,}" for x in rows) + " |")
    lines.append("")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[512, 1024])
    ap.add_argument('--radius', type=float, default=6)
    ap.add_argument('--min-core', type=int, default=1)
    ap.add_argument('--every', type=int, default=4)
    ap.add_argument('--shift', type=int, default=16)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--json', default=None)
    ap.add_argument('--md', default=None, help='write the table as markdown (profiles/label_separate.md)')
    a = ap.parse_args()
    a.radius = int(a.radius) if float(a.radius).is_integer() else a.radius
    r2, min_core, sampling = SP.check((a.radius, a.min_core))
    _hip.require_gpu()
    dev = torch.device('cuda')
    rows = []
    for S in a.sizes:
        vol = planted(S, a.every, a.shift, dev)
        other = torch.empty_like(vol.view(torch.int32))
        seeds, n_seeds = seeds_of(vol, r2, min_core)
        row = dict(size=S, rounds=a.rounds, warmup=a.warmup, bytes=vol.numel() * 4, radius=a.radius, seeds=n_seeds,
                   tiles=-(-S // 8) * -(-S // 8) * -(-S // 64))
        wall, events, entry = {}, [], {}
        for i in range(a.warmup + a.rounds):
            keep = i >= a.warmup
            ms, _ = timed(lambda: other.copy_(vol.view(torch.int32)))
            if keep:
                wall.setdefault('copy', []).append(ms)
            ms, out = timed(lambda: _hip.label_erode(vol, r2))
            del out
            if keep:
                wall.setdefault('erode', []).append(ms)
            info = {}
            _hip.PROFILE = {}
            ms, g = timed(lambda: _hip.label_grow(vol, seeds, info=info).owners())
            prof, _hip.PROFILE = _hip.PROFILE, None
            del g
            row['grow'] = dict(info)
            if keep:
                wall.setdefault('grow', []).append(ms)
                events.append(sum(e0.elapsed_time(e1) for k, v in prof.items() if k.startswith('emp_label_grow')
                                  for e0, e1, _, _ in v))
                for k, v in prof.items():
                    if k.startswith('emp_label_grow'):
                        entry.setdefault(k, []).append(sum(e0.elapsed_time(e1) for e0, e1, _, _ in v))
            work = vol.view(torch.int32).clone().view(torch.uint32)
            ms, (_, st) = timed(lambda: SP.separate_volume(work, work.shape, r2, min_core, sampling))
            row['stats'] = st
            del work
            if keep:
                wall.setdefault('separate', []).append(ms)
        copy = float(np.median(wall['copy']))
        row.update(wall_ms={k: stats(v) for k, v in wall.items()}, grow_event_ms=stats(events), entry_ms={k: stats(v) for k, v in entry.items()},
                   over_copy={k: float(np.median(v)) / copy for k, v in wall.items() if k != 'copy'})
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
