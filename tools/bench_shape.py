"""Shape sums of a resident label volume (_hip.shape_labels, csrc/emp_label_shape.hip) against a device copy of the
same bytes, against _hip.measure_labels and against _hip.label_graph of the thinned volume, whose kernel builds the same
neighbourhood masks from global memory.

The volume is synthetic.planted_labels(fill=0.08, rmin=6, rmax=24, seed=4321) as uint32 labels, the volume that
tools/bench_measure.py, bench_skeleton.py and bench_thickness.py use (6 781 objects at 1024^3).  In one process: the
volume is thinned once (untimed), then --warmup rounds, then --rounds rounds in which follow each other a device copy of
the volume (`b.copy_(a)`, the yardstick), _hip.measure_labels, _hip.shape_labels and _hip.label_graph of the skeleton.
Each is timed by the wall clock between device synchronisations (allocations and host syncs included) and also given as
a multiple of the copy and of measure_labels of the same run.  One more, untimed, run of shape_labels with _hip.PROFILE
gives the device time of every ABI call by HIP events: the run count, the label list (extract, sort, compact) and the
tile pass.

usage: PYTHONPATH=. python tools/bench_shape.py [--sizes 512 1024] [--rounds 5] [--json FILE] [--md FILE]
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

PHASES = (('count', ('emp_label_measure_count',)), ('labels', ('emp_label_shape_labels',)), ('tiles', ('emp_label_shape',)))


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


def markdown(rows, a):
    head = "| | " + " | ".join(f"{w['size']}³" for w in rows) + " |"
    lines = ["# Shape sums: `_hip.shape_labels` against a device copy, `measure_labels` and `label_graph`", "",
             f"`tools/bench_shape.py --sizes {' '.join(str(w['size']) for w in rows)} --rounds {a.rounds}`: median (min – "
             "max) of the wall clock in ms between device synchronisations, one process, the measurements of a round in "
             "turn.", "", head, "|---|" + "---|" * len(rows)]
    for k, what in (('copy', 'device copy of the volume'), ('measure', '`_hip.measure_labels`'),
                    ('shape', '`_hip.shape_labels`'), ('graph', '`_hip.label_graph` of the skeleton')):
        lines.append(f"| {what} | " + " | ".join(fmt(w['wall_ms'][k]) for w in rows) + " |")
    lines.append("| shape / copy | " + " | ".join(f"{w['over_copy']:.1f}" for w in rows) + " |")
    lines.append("| shape / measure | " + " | ".join(f"{w['over_measure']:.2f}" for w in rows) + " |")
    for ph, _ in PHASES:
        lines.append(f"| {ph}, device ms | " + " | ".join(f"{w['phase_ms'][ph]:.2f}" for w in rows) + " |")
    for what in ('blocks', 'tiles', 'spilled', 'work_bytes', 'rows'):
        lines.append(f"| {what} | " + " | ".join(f"{w['counts'][what]:,}" for w in rows) + " |")
    lines.append("| tiles of the volume | " + " | ".join(f"{w['all_tiles']:,}" for w in rows) + " |")
    lines.append("| labelled voxels | " + " | ".join(f"{w['voxels']:,}" for w in rows) + " |")
    lines.append("| voxels of the skeleton | " + " | ".join(f"{w['skeleton_voxels']:,}" for w in rows) + " |")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[512, 1024])
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--json', default=None)
    ap.add_argument('--md', default=None, help='write the table as markdown')
    a = ap.parse_args()
    _hip.require_gpu()
    dev = torch.device('cuda')
    rows = []
    for S in a.sizes:
        lab, _ = SY.planted_labels((S, S, S), fill=0.08, rmin=6, rmax=24, seed=4321)
        bits = torch.from_numpy(lab.astype(np.uint32).view(np.int32)).to(dev)
        del lab
        vol = bits.view(torch.uint32)
        other = torch.empty_like(bits)
        skel = _hip.label_thin(vol)
        wall, counts = {}, {}
        steps = [('copy', lambda: other.copy_(bits)), ('measure', lambda: _hip.measure_labels(vol)),
                 ('shape', lambda: _hip.shape_labels(vol, info=counts)), ('graph', lambda: _hip.label_graph(skel))]
        for i in range(a.warmup + a.rounds):
            for k, fn in steps:
                ms, out = timed(fn)
                if i >= a.warmup:
                    wall.setdefault(k, []).append(ms)
                if k == 'shape':
                    counts['rows'] = int(out.shape[0])
                del out
        copy, measure, shape = (float(np.median(wall[k])) for k in ('copy', 'measure', 'shape'))
        row = dict(size=S, rounds=a.rounds, warmup=a.warmup, bytes=vol.numel() * 4, voxels=int(torch.count_nonzero(bits)),
                   skeleton_voxels=int(torch.count_nonzero(skel.view(torch.int32))),
                   all_tiles=-(-S // 8) * -(-S // 8) * -(-S // 64), counts=counts,
                   phase_ms=phases(lambda: _hip.shape_labels(vol)), wall_ms={k: stats(v) for k, v in wall.items()},
                   over_copy=shape / copy, over_measure=shape / measure)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del vol, bits, other, skel
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, 'w') as fh:
            json.dump(rows, fh, indent=1)
    if a.md:
        with open(a.md, 'w') as fh:
            fh.write(markdown(rows, a))


if __name__ == '__main__':
    main()
