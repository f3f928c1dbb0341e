"""Label morphology of a resident label volume (_hip.label_edt, morphology.morph_volume; csrc/emp_label_morph.hip)
against a device copy of the same bytes and against _hip.label_components of the same volume.

The volume is synthetic.planted_labels(fill=0.08, rmin=6, rmax=24, seed=4321), the one of tools/bench_components.py and
tools/bench_holes.py, as uint32 labels.  Per size, in one process: --warmup rounds, then --rounds rounds of every
measurement in turn -- a device copy of the volume (`a.copy_(b)`, the yardstick) and _hip.label_components(volume, 26),
then label_edt at cap 65535 and erode / dilate / open / close at every radius.  Each is timed by the wall clock around
a call that ends in a device synchronise (allocations included), and the entry points by HIP events (_hip.PROFILE).

usage: PYTHONPATH=. python tools/bench_morph.py [--sizes 512 1024] [--radii 1 2 4] [--rounds 5] [--json FILE] [--md FILE]
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
from empanada_amd import morphology as MO                       # noqa: E402
from empanada_amd import synthetic as SY                        # noqa: E402

OPS = ('erode', 'dilate', 'open', 'close')


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


def markdown(rows, a):
    lines = ["# Label morphology: `emp_label_edt` / `emp_label_erode` / `emp_label_dilate` against a device copy and E3", "",
             f"MI355X, one GPU, `PYTHONPATH=. python tools/bench_morph.py --sizes {' '.join(str(r['size']) for r in rows)} "
             f"--rounds {a.rounds}` ({a.warmup} warm-up rounds, then {a.rounds} rounds; median (min – max), ms, wall clock "
             "around a call that ends in a device synchronise, allocations included).  Volume: "
             "`synthetic.planted_labels((S, S, S), fill=0.08, rmin=6, rmax=24, seed=4321)` as uint32 labels, the one of "
             "`profiles/label_holes.md`.", ""]
    head = "| uint32 labels | " + " | ".join(f"{r['size']}³ ({r['bytes'] / 1e9:.2f} GB), {r['objects']} objects" for r in rows) + " |"
    lines += [head, "|---|" + "---|" * len(rows)]
    keys = ['copy', 'label_components', 'edt'] + [f'{op} r={r}' for r in a.radii for op in OPS]
    names = {'copy': 'device copy of the volume', 'label_components': '`_hip.label_components(volume, 26)`',
             'edt': '`_hip.label_edt`, cap 65535'}
    for k in keys:
        lines.append(f"| {names.get(k, k)} | " + " | ".join(fmt(r['wall_ms'][k]) for r in rows) + " |")
    for k in keys[1:]:
        lines.append(f"| {names.get(k, k)} over the copy | " + " | ".join(f"{r['over_copy'][k]:.1f}" for r in rows) + " |")
    lines.append("| workspace of a call, bytes: edt or erode / dilate | " + " | ".join(
        f"{r['work_bytes']['edt']:,} / {r['work_bytes']['dilate']:,}" for r in rows) + " |")
    lines += ["", "Entry points by HIP events, all radii together (median ms): " + "; ".join(
        f"{r['size']}³: " + ", ".join(f"`{k}` {v['median']:.2f}" for k, v in sorted(r['entry_ms'].items())) for r in rows), ""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[512, 1024])
    ap.add_argument('--radii', type=float, nargs='+', default=[1, 2, 4])
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--json', default=None)
    ap.add_argument('--md', default=None, help='write the table as markdown (profiles/label_morph.md)')
    a = ap.parse_args()
    a.radii = [int(r) if float(r).is_integer() else r for r in a.radii]
    _hip.require_gpu()
    dev = torch.device('cuda')
    rows = []
    for S in a.sizes:
        lab, _ = SY.planted_labels((S, S, S), fill=0.08, rmin=6, rmax=24, seed=4321)
        vol = torch.from_numpy(lab.astype(np.uint32).view(np.int32)).to(dev).view(torch.uint32)
        del lab
        other = torch.empty_like(vol.view(torch.int32))
        row = dict(size=S, rounds=a.rounds, warmup=a.warmup, bytes=vol.numel() * 4)
        wall, work, moved = {}, {}, {}
        _hip.PROFILE = None
        for i in range(a.warmup + a.rounds):
            if i == a.warmup:
                _hip.PROFILE = {}
            keep = i >= a.warmup
            ms, _ = timed(lambda: other.copy_(vol.view(torch.int32)))
            if keep:
                wall.setdefault('copy', []).append(ms)
            ms, lc = timed(lambda: _hip.label_components(vol, 26))
            row['objects'] = lc.n
            del lc
            if keep:
                wall.setdefault('label_components', []).append(ms)
            info = {}
            ms, out = timed(lambda: _hip.label_edt(vol, info=info))
            work['edt'] = info['work_bytes']
            del out
            if keep:
                wall.setdefault('edt', []).append(ms)
            for r in a.radii:
                for op in OPS:
                    _, r2, sampling = MO.check((op, r))
                    ms, (out, st) = timed(lambda: MO.morph_volume(vol, vol.shape, op, r2, sampling))
                    moved[f'{op} r={r}'] = (st['voxels_removed'], st['voxels_added'])
                    del out
                    if keep:
                        wall.setdefault(f'{op} r={r}', []).append(ms)
            info = {}
            _hip.label_dilate(vol, 1, info=info)
            work['dilate'] = info['work_bytes']
        torch.cuda.synchronize()
        prof = _hip.PROFILE
        _hip.PROFILE = None
        copy = float(np.median(wall['copy']))
        row.update(wall_ms={k: stats(v) for k, v in wall.items()},
                   over_copy={k: float(np.median(v)) / copy for k, v in wall.items() if k != 'copy'},
                   over_label_components={k: float(np.median(v)) / float(np.median(wall['label_components']))
                                          for k, v in wall.items() if k not in ('copy', 'label_components')},
                   entry_ms={k: stats([e0.elapsed_time(e1) for e0, e1, _, _ in v]) for k, v in prof.items()
                             if k.startswith(('emp_label_edt', 'emp_label_erode', 'emp_label_dilate'))},
                   work_bytes=work, voxels_removed_added=moved)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del vol, other
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, 'w') as fh:
            json.dump(rows, fh, indent=1)
    if a.md:
        with open(a.md, 'w') as fh:
            fh.write(markdown(rows, a))


if __name__ == '__main__':
    main()
