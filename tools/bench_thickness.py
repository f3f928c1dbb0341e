"""Local thickness of a resident label volume (_hip.label_thickness, csrc/emp_label_thick.hip) against a device copy of
the same bytes and against _hip.label_edt at the same cap.

The volume is synthetic.planted_labels(fill=0.08, rmin=6, rmax=24, seed=4321) as uint32 labels, the volume that
tools/bench_measure.py, bench_morph.py, bench_separate.py, bench_mesh.py, bench_skeleton.py and bench_contacts.py use
(6 781 objects at 1024^3).  In one process: --warmup rounds, then --rounds rounds in which follow each other -- a device
copy of the volume (`b.copy_(a)`, the yardstick) and, per cap of --caps, _hip.label_edt and _hip.label_thickness at that
cap.  Each is timed by the wall clock between device synchronisations (allocations and host syncs included) and also
given as a multiple of the copy and of the edt of the same round.  One more, untimed, round per cap runs with
_hip.PROFILE and gives the device time of every ABI call by HIP events: the edt over the extended blocks, the lists
(count, scan, sort), the resolve gather and the table (emp_label_overlaps_count + emp_label_overlaps on the widened map).

--cpu CORNER times the CPU route instead and needs no GPU: on the [0, CORNER)^3 corner of the --sizes[0] volume, the
capped edt object by object (scipy, each in its bounding box) and then, per distinct d2 value, one exact Euclidean
transform of the whole corner -- the checker of tests/thickness_ref.py.

usage: PYTHONPATH=. python tools/bench_thickness.py [--sizes 512 1024] [--caps 64 256 1024] [--rounds 3] [--json FILE]
       [--md FILE] | --cpu 256 [--caps 64]
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
from bench_separate import stats, timed, fmt                    # noqa: E402

PHASES = (('edt', ('emp_label_thick_edt',)), ('lists', ('emp_label_thick_lists',)),
          ('resolve', ('emp_label_thick_resolve',)), ('table', ('emp_label_overlaps_count', 'emp_label_overlaps')))


def phases(fn):
    """device milliseconds per phase of one run of fn, from the events of _hip.PROFILE"""
    _hip.PROFILE = {}
    try:
        fn()
        torch.cuda.synchronize()
        return {k: float(sum(e0.elapsed_time(e1) for name in names for e0, e1, _, _ in _hip.PROFILE.get(name, [])))
                for k, names in PHASES}
    finally:
        _hip.PROFILE = None


def cpu_route(lab, cap):
    """seconds of (the edt object by object, the covering transform per distinct d2) on the host, and the distinct values"""
    from scipy.ndimage import distance_transform_edt, find_objects
    t0 = time.perf_counter()
    d2 = np.zeros(lab.shape, np.int64)
    for i, box in enumerate(find_objects(lab.astype(np.int64))):
        if box is None:
            continue
        grown = tuple(slice(max(s.start - 1, 0), min(s.stop + 1, n)) for s, n in zip(box, lab.shape))
        mask = lab[grown] == i + 1
        if mask.all():
            d2[grown][mask] = cap
            continue
        d = distance_transform_edt(mask)
        d2[grown][mask] = np.minimum(cap, np.rint(d[mask] ** 2).astype(np.int64))
    t1 = time.perf_counter()
    t2 = np.zeros(lab.shape, np.int64)
    grid = np.indices(lab.shape).astype(np.int32)
    values = [int(u) for u in np.unique(d2) if u]
    for u in values:
        _, idx = distance_transform_edt(d2 != u, return_indices=True)
        sq = ((idx - grid).astype(np.int64) ** 2).sum(axis=0)
        t2[sq < u] = u
    return t1 - t0, time.perf_counter() - t1, len(values)


def markdown(rows, a):
    head = "| | " + " | ".join(f"{w['size']}³" for w in rows) + " |"
    lines = ["# Local thickness: `_hip.label_thickness` against a device copy and `label_edt`", "",
             f"`tools/bench_thickness.py --sizes {' '.join(str(w['size']) for w in rows)} --caps "
             f"{' '.join(str(c) for c in a.caps)} --rounds {a.rounds}`: median (min – max) of the wall clock in ms between "
             "device synchronisations, one process, the measurements of a round in turn.", "", head,
             "|---|" + "---|" * len(rows)]
    lines.append("| device copy of the volume | " + " | ".join(fmt(w['wall_ms']['copy']) for w in rows) + " |")
    for c in a.caps:
        lines.append(f"| `_hip.label_edt`, cap {c} | " + " | ".join(fmt(w['wall_ms'][f'edt_{c}']) for w in rows) + " |")
        lines.append(f"| `_hip.label_thickness`, cap {c} | " + " | ".join(fmt(w['wall_ms'][f'thick_{c}']) for w in rows) + " |")
        lines.append(f"| cap {c}: thickness / copy | " + " | ".join(f"{w['over_copy'][str(c)]:.1f}" for w in rows) + " |")
        lines.append(f"| cap {c}: thickness / edt | " + " | ".join(f"{w['over_edt'][str(c)]:.2f}" for w in rows) + " |")
        for ph, _ in PHASES:
            lines.append(f"| cap {c}: {ph}, device ms | " + " | ".join(f"{w['phase_ms'][str(c)][ph]:.2f}" for w in rows) + " |")
        for what in ('blocks', 'candidates', 'capped', 'lists', 'longest', 'work_bytes', 'rows'):
            lines.append(f"| cap {c}: {what} | " + " | ".join(f"{w['counts'][str(c)][what]:,}" for w in rows) + " |")
        lines.append(f"| cap {c}: mean list | " + " | ".join(
            f"{w['counts'][str(c)]['candidates'] / max(w['counts'][str(c)]['lists'], 1):.0f}" for w in rows) + " |")
    lines.append("| tiles of the volume | " + " | ".join(f"{w['all_tiles']:,}" for w in rows) + " |")
    lines.append("| labelled voxels | " + " | ".join(f"{w['voxels']:,}" for w in rows) + " |")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[512, 1024])
    ap.add_argument('--caps', type=int, nargs='+', default=[64, 256, 1024])
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--cpu', type=int, default=None, help='time the CPU route on this corner of the volume; no GPU needed')
    ap.add_argument('--json', default=None)
    ap.add_argument('--md', default=None, help='write the table as markdown')
    a = ap.parse_args()
    if a.cpu is not None:
        S, n = a.sizes[0], a.cpu
        lab, _ = SY.planted_labels((S, S, S), fill=0.08, rmin=6, rmax=24, seed=4321)
        corner = np.ascontiguousarray(lab[:n, :n, :n])
        for cap in a.caps:
            edt_s, cover_s, values = cpu_route(corner, cap)
            print(json.dumps(dict(cpu_corner=n, of=S, cap=cap, edt_s=edt_s, cover_s=cover_s, distinct_d2=values,
                                  voxels=int((corner != 0).sum()))), flush=True)
        return
    _hip.require_gpu()
    dev = torch.device('cuda')
    rows = []
    for S in a.sizes:
        lab, _ = SY.planted_labels((S, S, S), fill=0.08, rmin=6, rmax=24, seed=4321)
        bits = torch.from_numpy(lab.astype(np.uint32).view(np.int32)).to(dev)
        del lab
        vol = bits.view(torch.uint32)
        other = torch.empty_like(bits)
        wall, counts, phase_ms = {}, {}, {}
        for i in range(a.warmup + a.rounds):
            steps = [('copy', lambda: other.copy_(bits))]
            for c in a.caps:
                info = counts.setdefault(str(c), {})
                steps.append((f'edt_{c}', lambda c=c: _hip.label_edt(vol, (1, 1, 1), c)))
                steps.append((f'thick_{c}', lambda c=c, info=info: _hip.label_thickness(vol, c, info=info)))
            for k, fn in steps:
                ms, out = timed(fn)
                if i >= a.warmup:
                    wall.setdefault(k, []).append(ms)
                if k.startswith('thick_'):
                    counts[k[6:]]['rows'] = int(out[1].shape[0])
                del out
        for c in a.caps:
            phase_ms[str(c)] = phases(lambda: _hip.label_thickness(vol, c))
        copy = float(np.median(wall['copy']))
        row = dict(size=S, rounds=a.rounds, warmup=a.warmup, caps=a.caps, bytes=vol.numel() * 4,
                   voxels=int(torch.count_nonzero(bits)), all_tiles=-(-S // 8) * -(-S // 8) * -(-S // 64),
                   counts=counts, phase_ms=phase_ms, wall_ms={k: stats(v) for k, v in wall.items()},
                   over_copy={str(c): float(np.median(wall[f'thick_{c}'])) / copy for c in a.caps},
                   over_edt={str(c): float(np.median(wall[f'thick_{c}'])) / float(np.median(wall[f'edt_{c}']))
                             for c in a.caps})
        rows.append(row)
        print(json.dumps(row), flush=True)
        del vol, bits, other
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, 'w') as fh:
            json.dump(rows, fh, indent=1)
    if a.md:
        with open(a.md, 'w') as fh:
            fh.write(markdown(rows, a))


if __name__ == '__main__':
    main()
