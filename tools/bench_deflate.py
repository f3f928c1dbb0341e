"""Writing a resident uint32 label volume into a (1, Y, X)-chunked zarr array, three routes in one process:
  (a) cpu_zlib   the only compressed route before the device coder: raw device -> pinned copy of the volume, then
                 ZarrV2Array.write_slab on a compressor=1 dataset, zlib.compress on a four-thread pool;
  (b) raw        the same with compressor=None (what infer_volume does by default), for context;
  (c) device     ZarrV2Array.write_slab_device: zlib streams made on the GPU (csrc/emp_deflate.hip), only those copied.
The volume is synthetic.planted_labels(fill=0.08, rmin=6, rmax=24, seed=4321).  Every route writes into a directory of
its own under --dir (a tmpfs by default).  Wall time around copy + write, ending in a device synchronise and drained
writes; 3 warm-up rounds, then the routes alternate for --rounds rounds.  The two entry points of the coder are also
timed by HIP events (_hip.PROFILE) and set against the 8 TB/s HBM peak by the raw bytes each pass reads.
profiles/deflate_labels.md holds a run.

usage: PYTHONPATH=. python tools/bench_deflate.py [--sizes 512 1024] [--rounds 5] [--dir /dev/shm] [--json FILE]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from empanada_amd import _hip                                   # noqa: E402
from empanada_amd import synthetic as SY                        # noqa: E402
from empanada_amd.zarr_utils import ZarrV2Group                 # noqa: E402

HBM_PEAK = 8.0e12          # bytes/s, MI355X specification


def disk_bytes(ds):
    return sum(os.path.getsize(os.path.join(ds.path, f)) for f in os.listdir(ds.path) if not f.startswith('.'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[512, 1024])
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--dir', default='/dev/shm' if os.path.isdir('/dev/shm') else None)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    _hip.require_gpu()
    dev = torch.device('cuda')
    rows = []
    for S in a.sizes:
        lab, _ = SY.planted_labels((S, S, S), fill=0.08, rmin=6, rmax=24, seed=4321)
        host = lab.astype(np.uint32)
        vol = torch.from_numpy(host.view(np.int32)).to(dev).view(torch.uint32)
        raw_bytes = host.nbytes
        root = tempfile.mkdtemp(prefix='bench_deflate_', dir=a.dir)
        pool = ThreadPoolExecutor(max_workers=4)
        try:
            sets = {r: ZarrV2Group(os.path.join(root, r)).create_dataset(
                        'labels', shape=(S, S, S), dtype=np.uint32, chunks=(1, None, None),
                        compressor=None if r == 'raw' else 1) for r in ('cpu_zlib', 'raw', 'device')}
            pinned = torch.empty((S, S, S), dtype=torch.int32).pin_memory()        # routes (a), (b): the whole slab
            grown = {}

            def small(n):                                                          # route (c): grows, never shrinks
                if 'buf' not in grown or grown['buf'].numel() < n:
                    grown['buf'] = torch.empty((n,), dtype=torch.uint8).pin_memory()
                return grown['buf']

            def copy_then_write(ds):
                pinned.copy_(vol.view(torch.int32), non_blocking=True)
                torch.cuda.current_stream().synchronize()
                for f in ds.write_slab(0, pinned.numpy().view(np.uint32), pool):
                    f.result()

            def on_device(ds):
                futures, n = ds.write_slab_device(0, vol, pool, host=small)
                for f in futures:
                    f.result()
                return n

            routes = {'cpu_zlib': lambda: copy_then_write(sets['cpu_zlib']), 'raw': lambda: copy_then_write(sets['raw']),
                      'device': lambda: on_device(sets['device'])}
            secs = {r: [] for r in routes}
            for i in range(a.warmup + a.rounds):
                for r, fn in routes.items():                                       # the routes alternate
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    if i >= a.warmup:
                        secs[r].append(time.perf_counter() - t0)
            # what the device route left on disk is the volume (every 37th slice through zlib.decompress)
            for z in range(0, S, 37):
                assert np.array_equal(sets['device'][z], host[z]), f"slice {z} of the device route differs"
            assert np.array_equal(sets['cpu_zlib'][S // 2], host[S // 2])
            # the two entry points, events around each
            _hip.PROFILE = {}
            for _ in range(a.rounds):
                _hip.deflate_labels(vol)
            torch.cuda.synchronize()
            # a slab above the int32 limit of one call goes through in blocks of slices: a slab's time is their sum
            calls = {k: len(v) // a.rounds for k, v in _hip.PROFILE.items()}
            steps = {k: float(np.median(np.array([e0.elapsed_time(e1) for e0, e1, _, _ in v]).reshape(a.rounds, -1).sum(1)))
                     for k, v in _hip.PROFILE.items()}
            _hip.PROFILE = None
            row = dict(size=S, objects=int(lab.max()), raw_bytes=raw_bytes, rounds=a.rounds, warmup=a.warmup, dir=a.dir,
                       bytes_on_disk={r: disk_bytes(ds) for r, ds in sets.items()})
            for r, s in secs.items():
                row[r + '_s'] = dict(median=float(np.median(s)), min=float(min(s)), max=float(max(s)))
            row['device_slowest_below_cpu_zlib_fastest'] = bool(max(secs['device']) < min(secs['cpu_zlib']))
            row['size_ratio_device_over_cpu_zlib'] = row['bytes_on_disk']['device'] / row['bytes_on_disk']['cpu_zlib']
            row['raw_over_device'] = raw_bytes / row['bytes_on_disk']['device']
            row['entry_ms_median_per_slab'] = steps
            row['entry_calls_per_slab'] = calls
            row['entry_input_bytes_per_s'] = {k: raw_bytes / (v * 1e-3) for k, v in steps.items()}
            row['entry_share_of_hbm_peak'] = {k: v / HBM_PEAK for k, v in row['entry_input_bytes_per_s'].items()}
            rows.append(row)
            print(json.dumps(row), flush=True)
        finally:
            pool.shutdown()
            shutil.rmtree(root, ignore_errors=True)
        del vol, pinned, host, lab
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, 'w') as fh:
            json.dump(rows, fh, indent=1)


if __name__ == '__main__':
    main()
