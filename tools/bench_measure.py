"""Per-object measurements of a resident label volume (_hip.measure_labels, csrc/emp_measure.hip) against a device copy
of the same bytes and against the host.

The volume is synthetic.planted_labels(fill=0.08, rmin=6, rmax=24, seed=4321), measured as uint32 labels and as the
uint8 mask (label > 0, what a stuff class holds).  Per array, in one process: 3 warm-up rounds, then measure_labels and
`b.copy_(a)` of the array into a buffer of its size alternate for --rounds rounds.  The two entry points of the kernel
are timed by HIP events (_hip.PROFILE): emp_label_measure_count is the count pass + the scan of the row counts,
emp_label_measure the extract pass + fix-up + sort + reduce; the copy by events of its own; measure_labels as a whole
(allocations and its two host syncs included) by the wall clock.  A per-kernel split of emp_label_measure and the bytes
fetched come from separate profiler runs of --only-device (see profiles/label_measure.md).
--host-size S: the same table from numpy / scipy.ndimage on the host for the S^3 volume (bincount for voxels and index
sums, ndimage.find_objects for the boxes, three shifted comparisons + bincount for the faces), checked against the
device table.

usage: PYTHONPATH=. python tools/bench_measure.py [--sizes 512 1024] [--rounds 10] [--host-size 512] [--json FILE]
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

HBM_PEAK = 8.0e12          # bytes/s, MI355X specification


def host_table(lab):
    """the table of include/emp_hip.h (E2) for a uint32 host volume with library calls; labels must be small integers"""
    from scipy import ndimage
    n = int(lab.max()) + 1
    flat = lab.ravel()
    out = np.zeros((n, 14), np.int64)
    out[:, 0] = np.arange(n)
    out[:, 1] = np.bincount(flat, minlength=n)
    for axis, col in enumerate((8, 9, 10)):
        shape = [1, 1, 1]
        shape[axis] = lab.shape[axis]
        idx = np.broadcast_to(np.arange(lab.shape[axis], dtype=np.float64).reshape(shape), lab.shape)
        out[:, col] = np.rint(np.bincount(flat, weights=idx.ravel(), minlength=n)).astype(np.int64)   # sums < 2^53: exact
    for i, box in enumerate(ndimage.find_objects(lab.astype(np.int32))):
        if box is not None:
            out[i + 1, 2:5] = [s.start for s in box]
            out[i + 1, 5:8] = [s.stop for s in box]
    for axis, col in enumerate((11, 12, 13)):
        pad = [(0, 0)] * 3
        pad[axis] = (1, 1)
        p = np.pad(lab, pad)
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[axis], hi[axis] = slice(0, -2), slice(2, None)
        faces = (lab != p[tuple(lo)]).astype(np.uint8) + (lab != p[tuple(hi)])
        out[:, col] = np.rint(np.bincount(flat, weights=faces.ravel(), minlength=n)).astype(np.int64)
    return out[1:][out[1:, 1] > 0]


def stats(ms):
    return dict(median=float(np.median(ms)), min=float(min(ms)), max=float(max(ms)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[512, 1024])
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--host-size', type=int, default=512, help='0: no host baseline')
    ap.add_argument('--only-device', choices=['u32', 'u8'], default=None,
                    help='no timing: --rounds calls of measure_labels on that array alone, for a profiler run')
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    _hip.require_gpu()
    dev = torch.device('cuda')
    rows = []
    for S in a.sizes:
        lab, _ = SY.planted_labels((S, S, S), fill=0.08, rmin=6, rmax=24, seed=4321)
        host = lab.astype(np.uint32)
        del lab
        vol = torch.from_numpy(host.view(np.int32)).to(dev).view(torch.uint32)
        mask = (vol.view(torch.int32) != 0).to(torch.uint8)
        arrays = {'u32': vol, 'u8': mask}
        if a.only_device:
            for _ in range(a.rounds):
                table = _hip.measure_labels(arrays[a.only_device])
            torch.cuda.synchronize()
            print(json.dumps(dict(size=S, array=a.only_device, rows=int(table.shape[0]), rounds=a.rounds)), flush=True)
            continue
        row = dict(size=S, rounds=a.rounds, warmup=a.warmup)
        for name, arr in arrays.items():
            nbytes = arr.numel() * arr.element_size()
            buf = torch.empty_like(arr.view(torch.int32) if name == 'u32' else arr)
            src = arr.view(torch.int32) if name == 'u32' else arr
            info, wall, copies = {}, [], []
            _hip.PROFILE = None
            for i in range(a.warmup + a.rounds):
                if i == a.warmup:
                    _hip.PROFILE = {}
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                table = _hip.measure_labels(arr, info=info)
                torch.cuda.synchronize()
                if i >= a.warmup:
                    wall.append((time.perf_counter() - t0) * 1e3)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                buf.copy_(src)
                e1.record()
                torch.cuda.synchronize()
                if i >= a.warmup:
                    copies.append(e0.elapsed_time(e1))
            entry = {k: stats([e0.elapsed_time(e1) for e0, e1, _, _ in v]) for k, v in _hip.PROFILE.items()}
            _hip.PROFILE = None
            both = entry['emp_label_measure_count']['median'] + entry['emp_label_measure']['median']
            row[name] = dict(bytes=nbytes, objects=int(table.shape[0]), runs=info['runs'], blocks=info['blocks'],
                             work_bytes=info['work_bytes'], entry_ms=entry, copy_ms=stats(copies),
                             measure_labels_wall_ms=stats(wall), both_entries_over_copy=both / float(np.median(copies)),
                             count_read_bytes_per_s=nbytes / (entry['emp_label_measure_count']['median'] * 1e-3),
                             copy_bytes_read_plus_written_per_s=2 * nbytes / (float(np.median(copies)) * 1e-3),
                             count_share_of_hbm_peak=nbytes / (entry['emp_label_measure_count']['median'] * 1e-3) / HBM_PEAK)
            if name == 'u32' and S == a.host_size:
                t0 = time.perf_counter()
                want = host_table(host)
                row['host_numpy_scipy_s'] = time.perf_counter() - t0
                row['host_table_equals_device'] = bool(np.array_equal(want, table.cpu().numpy()))
            del buf
        rows.append(row)
        print(json.dumps(row), flush=True)
        del vol, mask, arrays, host
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, 'w') as fh:
            json.dump(rows, fh, indent=1)


if __name__ == '__main__':
    main()
