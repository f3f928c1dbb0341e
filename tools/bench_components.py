"""3D connected components of a resident label volume (_hip.label_components, csrc/emp_components.hip) against a device
copy of the same bytes and against the host.

The volume is synthetic.planted_labels(fill=0.08, rmin=6, rmax=24, seed=4321), labelled as uint32 labels and as the
uint8 mask (label > 0: a binary mask becomes instances).  Per array and connectivity, in one process: --warmup rounds,
then label_components, a paint of the components' numbers into a fresh uint32 volume, an in-place paint that changes
nothing, and `b.copy_(a)` of the array into a buffer of its size alternate for --rounds rounds.  The entry points are
timed by HIP events (_hip.PROFILE): emp_label_measure_count is step 1 (count pass + scan), emp_label_components step 2
(extract + union-find + numbering + reduce), emp_label_components_paint step 3; the copy by events of its own;
label_components as a whole (allocations and its two host syncs included) by the wall clock.
--host-size S: the same table from scipy.ndimage.label on the host for the S^3 uint32 volume (one call per label inside
the label's bounding box), checked against the device table.

usage: PYTHONPATH=. python tools/bench_components.py [--sizes 512 1024] [--rounds 10] [--host-size 512] [--json FILE]
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
from empanada_amd import synthetic as SY                        # noqa: E402


def host_table(lab, connectivity):
    """the table of include/emp_hip.h (E3) for a host volume with library calls: ndimage.label per label, in its box"""
    from scipy import ndimage
    structure = ndimage.generate_binary_structure(3, {6: 1, 18: 2, 26: 3}[connectivity])
    D, H, W = lab.shape
    rows = []
    for i, box in enumerate(ndimage.find_objects(lab.astype(np.int32))):
        if box is None:
            continue
        cc, n = ndimage.label(lab[box] == i + 1, structure=structure)
        off = [s.start for s in box]
        for k, sub in enumerate(ndimage.find_objects(cc), start=1):
            mask = cc[sub] == k
            z, y, x = (int(v[0]) + s.start + o for v, s, o in zip(np.nonzero(mask), sub, off))   # nonzero is in raster order
            rows.append([i + 1, int(mask.sum()), (z * H + y) * W + x, *(s.start + o for s, o in zip(sub, off)),
                         *(s.stop + o for s, o in zip(sub, off))])
    t = np.array(rows, np.int64).reshape(-1, 9)
    return t[np.argsort(t[:, 2], kind='stable')]


def stats(ms):
    return dict(median=float(np.median(ms)), min=float(min(ms)), max=float(max(ms)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[512, 1024])
    ap.add_argument('--connectivities', type=int, nargs='+', default=[6, 18, 26])
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--host-size', type=int, default=512, help='0: no host baseline')
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
        row = dict(size=S, rounds=a.rounds, warmup=a.warmup)
        for name, arr in (('u32', vol), ('u8', mask)):
            nbytes = arr.numel() * arr.element_size()
            src = arr.view(torch.int32) if name == 'u32' else arr
            buf = torch.empty_like(src)
            fresh = torch.empty(arr.shape, dtype=torch.int32, device=dev)
            row[name] = dict(bytes=nbytes)
            for c in a.connectivities:
                info, wall, copies = {}, [], []
                _hip.PROFILE = None
                for i in range(a.warmup + a.rounds):
                    if i == a.warmup:
                        _hip.PROFILE = {}
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    lc = _hip.label_components(arr, c, info=info)
                    torch.cuda.synchronize()
                    if i >= a.warmup:
                        wall.append((time.perf_counter() - t0) * 1e3)
                    numbers = torch.arange(1, lc.n + 1, device=dev)
                    lc.paint(numbers, out=fresh)                       # components' numbers into a fresh uint32 volume
                    lc.paint(lc.table[:, 0], out=arr)                  # in place, every value stays: O(runs)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    buf.copy_(src)
                    e1.record()
                    torch.cuda.synchronize()
                    if i >= a.warmup:
                        copies.append(e0.elapsed_time(e1))
                prof = _hip.PROFILE
                _hip.PROFILE = None
                entry = {k: stats([e0.elapsed_time(e1) for e0, e1, _, _ in v]) for k, v in prof.items()}
                # the two paints alternate under one name: even calls are the fresh volume, odd ones in place
                paints = [e0.elapsed_time(e1) for e0, e1, _, _ in prof['emp_label_components_paint']]
                entry['emp_label_components_paint'] = dict(fresh_u32=stats(paints[0::2]), in_place_same=stats(paints[1::2]))
                two = entry['emp_label_measure_count']['median'] + entry['emp_label_components']['median']
                copy = float(np.median(copies))
                row[name][f'c{c}'] = dict(components=lc.n, runs=info['runs'], blocks=info['blocks'],
                                          work_bytes=info['work_bytes'], entry_ms=entry, copy_ms=stats(copies),
                                          label_components_wall_ms=stats(wall), steps_1_2_over_copy=two / copy,
                                          step_2_over_copy=entry['emp_label_components']['median'] / copy,
                                          paint_fresh_over_copy=float(np.median(paints[0::2])) / copy)
                if name == 'u32':
                    _, st = CP.plan(lc.table, 500, 4)
                    row[name][f'c{c}']['plan_min_size_500_min_span_4'] = st
                if name == 'u32' and S == a.host_size and c == 26:
                    t0 = time.perf_counter()
                    want = host_table(host, c)
                    row['host_scipy_label_s'] = time.perf_counter() - t0
                    row['host_table_equals_device'] = bool(np.array_equal(want, lc.table.cpu().numpy()))
                del lc
            del buf, fresh
        rows.append(row)
        print(json.dumps(row), flush=True)
        del vol, mask, host
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, 'w') as fh:
            json.dump(rows, fh, indent=1)


if __name__ == '__main__':
    main()
