"""One level of the label pyramid, emp_label_pool_mode (csrc/emp_pool.hip), against a plain device-to-device copy of the
same number of bytes, in one process on one device.  The volume is synthetic.planted_labels(fill=0.08, rmin=6, rmax=24,
seed=4321), as uint32 labels and as a uint8 mask (label > 0, what a stuff class holds).  For every dtype and factor
triple: HIP events around single launches, warm-up launches first, then the kernel and the copy alternate for --reps
rounds; medians (and minima).  "Algorithmic bytes" of a level are its input plus its output, read and written once;
the copy moves half that many bytes (reads them, writes them), so both are quoted as bytes read + written per second.
Last, per dtype, pyramid.build of --levels chained (2, 2, 2) levels: what a whole pyramid of one class costs on the device.
profiles/label_pyramid.md holds a run.

usage: PYTHONPATH=. python tools/bench_label_pool.py [--size 1024] [--reps 20] [--warmup 5] [--levels 3] [--json FILE]
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

HBM_PEAK = 8.0e12          # bytes/s, MI355X specification


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    return e0, e1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=1024)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--factors', default='2,2,2;1,2,2')
    ap.add_argument('--levels', type=int, default=3)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    _hip.require_gpu()
    S = a.size
    factors = [tuple(int(v) for v in f.split(',')) for f in a.factors.split(';')]
    lab, _ = SY.planted_labels((S, S, S), fill=0.08, rmin=6, rmax=24, seed=4321)
    rows = []
    for name in ('uint32', 'uint8'):
        if name == 'uint32':
            vol = torch.from_numpy(lab.astype(np.int32)).cuda().view(torch.uint32)
        else:
            vol = torch.from_numpy((lab > 0).astype(np.uint8)).cuda()
        item = vol.element_size()
        for f in factors:
            out = torch.empty(_hip.pooled_shape(vol.shape, f), dtype=vol.dtype, device='cuda')
            alg = (vol.numel() + out.numel()) * item
            # the yardstick: a copy that reads alg / 2 bytes and writes alg / 2 bytes
            a8 = torch.empty((alg // 2,), dtype=torch.uint8, device='cuda').random_(0, 256)
            b8 = torch.empty_like(a8)
            for _ in range(a.warmup):
                _hip.pool_labels(vol, f, out=out)
                b8.copy_(a8)
            ev = {'pool': [], 'copy': []}
            for _ in range(a.reps):                              # the two alternate
                ev['pool'].append(timed(lambda: _hip.pool_labels(vol, f, out=out)))
                ev['copy'].append(timed(lambda: b8.copy_(a8)))
            torch.cuda.synchronize()
            ms = {k: np.array([e0.elapsed_time(e1) for e0, e1 in v]) for k, v in ev.items()}
            row = dict(size=S, dtype=name, factors=list(f), in_bytes=vol.numel() * item, out_bytes=out.numel() * item,
                       algorithmic_bytes=alg, reps=a.reps, warmup=a.warmup, nonzero_out=int((out.view(torch.uint8) != 0).sum()))
            for k, v in ms.items():
                med = float(np.median(v))
                row[k] = dict(median_ms=med, min_ms=float(v.min()), max_ms=float(v.max()),
                              bytes_per_s=alg / (med * 1e-3), share_of_hbm_peak=alg / (med * 1e-3) / HBM_PEAK)
            row['pool_over_copy_rate'] = row['pool']['bytes_per_s'] / row['copy']['bytes_per_s']
            rows.append(row)
            print(json.dumps(row), flush=True)
            del out, a8, b8
        # a whole pyramid of this volume: --levels chained (2, 2, 2) levels, allocation of the level slabs included
        from empanada_amd.inference import pyramid
        fl = pyramid.normalize(a.levels)
        for _ in range(a.warmup):
            pyramid.build(vol, fl)
        ev = [timed(lambda: pyramid.build(vol, fl)) for _ in range(a.reps)]
        torch.cuda.synchronize()
        ms = np.array([e0.elapsed_time(e1) for e0, e1 in ev])
        row = dict(size=S, dtype=name, levels=a.levels, build_median_ms=float(np.median(ms)), build_min_ms=float(ms.min()),
                   build_max_ms=float(ms.max()))
        rows.append(row)
        print(json.dumps(row), flush=True)
        del vol
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, 'w') as fh:
            json.dump(rows, fh, indent=1)


if __name__ == '__main__':
    main()
