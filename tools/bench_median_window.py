"""Device time of emp_median_harden_window against emp_median_harden_stack on the same resident block
(profiles/windowed_planes.md).  Needs the GPU.

    python tools/bench_median_window.py [--slices 256] [--size 1024] [--classes 1,5] [--ks 7] [--calls 20]

Per C: a (slices, C, size, size) fp32 block of random probabilities; each form is called three times untimed, then
`--calls` times, every call between two HIP events; the median of those is reported.  `stack`: emp_median_harden_stack
without out_prob (what a whole plane costs today); `window`: the window entry on the same block, no ends; `window+ends`:
with a history, a halo and the tail written over the history, as a middle step of a plane runs it.  One JSON line.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from empanada_amd import _hip  # noqa: E402


def device_ms(fn, calls):
    for _ in range(3):
        fn()
    times = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return sorted(times)[len(times) // 2], min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--slices', type=int, default=256)
    ap.add_argument('--size', type=int, default=1024)
    ap.add_argument('--classes', default='1,5')
    ap.add_argument('--ks', type=int, default=7)
    ap.add_argument('--calls', type=int, default=20)
    args = ap.parse_args()
    _hip.require_gpu()
    m = args.ks // 2
    row = {'slices': args.slices, 'size': args.size, 'ks': args.ks, 'calls': args.calls,
           'device': torch.cuda.get_device_name(0)}
    for C in (int(c) for c in args.classes.split(',')):
        x = torch.rand((args.slices, C, args.size, args.size), device='cuda')
        hist, halo = torch.rand_like(x[:m]), torch.rand_like(x[:m])
        forms = {'stack': lambda: _hip.median_harden_stack(x, args.ks, 0.5),
                 'window': lambda: _hip.median_harden_window(x, args.ks, 0.5),
                 'window+ends': lambda: _hip.median_harden_window(x, args.ks, 0.5, hist=hist, halo=halo, tail_out=hist)}
        gb = (4 * C + 1) * args.slices * args.size ** 2 / 1e9
        row[f'C={C}'] = {}
        for name, fn in forms.items():
            med, lo, hi = device_ms(fn, args.calls)
            row[f'C={C}'][name] = {'median_ms': round(med, 3), 'min_ms': round(lo, 3), 'max_ms': round(hi, 3),
                                   'TB_per_s': round(gb / med, 3)}
        del x, hist, halo
        torch.cuda.empty_cache()
    print(json.dumps(row), flush=True)


if __name__ == '__main__':
    main()
