"""Contact tables of a resident label volume (_hip.label_contacts, csrc/emp_label_contacts.hip) against a device copy of
the same bytes and against _hip.label_edt.

The volume is synthetic.planted_labels(fill=0.08, rmin=6, rmax=24, seed=4321) as uint32 labels, the volume that
tools/bench_measure.py, bench_separate.py, bench_mesh.py and bench_skeleton.py use (6 781 objects at 1024^3).  In one
process: --warmup rounds, then --rounds rounds in which follow each other -- a device copy of the volume (`b.copy_(a)`, the
yardstick), _hip.label_edt at cap r2 + 1 for the large radius, _hip.label_contacts of the volume with itself at r = 1 and
at r = --radius, and _hip.label_contacts of the volume against a copy of itself shifted by --shift voxels along every
axis under other ids, at r = --radius, so that every object has partners.  Each is timed by the wall clock between device
synchronisations (allocations and host syncs included) and also given as a multiple of the copy and of the edt of the
same round.  One more, untimed, round per case runs with _hip.PROFILE and gives the device time of every ABI call: the
count walk (with the tile list), the emit walk, the sort and the row reduce.

usage: PYTHONPATH=. python tools/bench_contacts.py [--sizes 512 1024] [--rounds 3] [--json FILE] [--md FILE]
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
from bench_separate import stats, timed, fmt                    # noqa: E402

PHASES = (('count', 'emp_label_contacts_count'), ('emit', 'emp_label_contacts_emit'), ('sort', 'emp_sort_u64_i32'),
          ('rows', 'emp_label_contacts_rows'), ('reduce', 'emp_label_contacts_reduce'))


def phases(fn):
    """device milliseconds per ABI call of one run of fn, from the events of _hip.PROFILE"""
    _hip.PROFILE = {}
    try:
        fn()
        torch.cuda.synchronize()
        return {k: float(sum(e0.elapsed_time(e1) for e0, e1, _, _ in _hip.PROFILE.get(name, []))) for k, name in PHASES}
    finally:
        _hip.PROFILE = None


def markdown(rows, a):
    r = a.radius
    head = "| | " + " | ".join(f"{w['size']}³" for w in rows) + " |"
    lines = ["# Contact sites between labelled objects: `_hip.label_contacts` against a device copy and `label_edt`", "",
             f"`tools/bench_contacts.py --sizes {' '.join(str(w['size']) for w in rows)} --rounds {a.rounds}`: "
             "median (min – max) of the wall clock in ms between device synchronisations, one process, the "
             "measurements of a round in turn.", "", head, "|---|" + "---|" * len(rows)]
    names = {'copy': 'device copy of the volume', 'edt': f'`_hip.label_edt`, cap {r * r + 1}',
             'same_1': '`label_contacts`, same volume, r = 1', f'same_{r}': f'`label_contacts`, same volume, r = {r}',
             f'two_{r}': f'`label_contacts`, against the shifted copy, r = {r}'}
    cases = [k for k in names if k not in ('copy', 'edt')]
    for k, name in names.items():
        lines.append(f"| {name} | " + " | ".join(fmt(w['wall_ms'][k]) for w in rows) + " |")
    for k in cases:
        lines.append(f"| {k} / copy | " + " | ".join(f"{w['over_copy'][k]:.1f}" for w in rows) + " |")
    for k in cases:
        lines.append(f"| {k} / edt | " + " | ".join(f"{w['over_edt'][k]:.2f}" for w in rows) + " |")
    for k in cases:
        for what in ('blocks', 'tiles', 'records', 'rows'):
            lines.append(f"| {k}: {what} | " + " | ".join(f"{w['counts'][k][what]:,}" for w in rows) + " |")
        for ph, _ in PHASES:
            lines.append(f"| {k}: {ph}, device ms | " + " | ".join(f"{w['phase_ms'][k][ph]:.2f}" for w in rows) + " |")
    lines.append("| tiles of the volume | " + " | ".join(f"{w['all_tiles']:,}" for w in rows) + " |")
    lines.append("| labelled voxels | " + " | ".join(f"{w['voxels']:,}" for w in rows) + " |")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[512, 1024])
    ap.add_argument('--radius', type=int, default=4)
    ap.add_argument('--shift', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--json', default=None)
    ap.add_argument('--md', default=None, help='write the table as markdown')
    a = ap.parse_args()
    _hip.require_gpu()
    dev = torch.device('cuda')
    r, r2 = a.radius, a.radius * a.radius
    rows = []
    for S in a.sizes:
        lab, _ = SY.planted_labels((S, S, S), fill=0.08, rmin=6, rmax=24, seed=4321)
        bits = torch.from_numpy(lab.astype(np.uint32).view(np.int32)).to(dev)
        del lab
        vol = bits.view(torch.uint32)
        moved = torch.roll(bits, (a.shift, a.shift, a.shift), dims=(0, 1, 2))
        moved[:a.shift] = 0
        moved[:, :a.shift] = 0
        moved[:, :, :a.shift] = 0
        moved = torch.where(moved != 0, moved + 1000000, moved).contiguous().view(torch.uint32)
        other = torch.empty_like(bits)
        cases = {'same_1': (None, 1), f'same_{r}': (None, r2), f'two_{r}': (moved, r2)}
        wall, counts, phase_ms = {}, {}, {}
        for i in range(a.warmup + a.rounds):
            steps = [('copy', lambda: other.copy_(bits)), ('edt', lambda: _hip.label_edt(vol, (1, 1, 1), r2 + 1))]
            for k, (b, q) in cases.items():
                info = counts.setdefault(k, {})
                steps.append((k, lambda b=b, q=q, info=info: _hip.label_contacts(vol, b, q, info=info)))
            for k, fn in steps:
                ms, out = timed(fn)
                if i >= a.warmup:
                    wall.setdefault(k, []).append(ms)
                if k in cases:
                    counts[k]['rows'] = int(out.shape[0])
                del out
        for k, (b, q) in cases.items():
            phase_ms[k] = phases(lambda: _hip.label_contacts(vol, b, q))
        copy, edt = float(np.median(wall['copy'])), float(np.median(wall['edt']))
        row = dict(size=S, rounds=a.rounds, warmup=a.warmup, radius=r, shift=a.shift, bytes=vol.numel() * 4,
                   voxels=int(torch.count_nonzero(bits)), all_tiles=-(-S // 8) * -(-S // 8) * -(-S // 64),
                   counts=counts, phase_ms=phase_ms, wall_ms={k: stats(v) for k, v in wall.items()},
                   over_copy={k: float(np.median(v)) / copy for k, v in wall.items()},
                   over_edt={k: float(np.median(v)) / edt for k, v in wall.items()})
        rows.append(row)
        print(json.dumps(row), flush=True)
        del vol, bits, moved, other
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, 'w') as fh:
            json.dump(rows, fh, indent=1)
    if a.md:
        with open(a.md, 'w') as fh:
            fh.write(markdown(rows, a))


if __name__ == '__main__':
    main()
