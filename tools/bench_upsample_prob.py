"""HIP-event timing of emp_upsample_bilinear_prob on a head's shape (32 slices of 256^2 -> 1024^2 per call) against the
calls it replaces: emp_upsample_bilinear (planar) and emp_upsample_bilinear + emp_logits_to_prob.  Needs the GPU.

    python tools/bench_upsample_prob.py [--n 32] [--size 1024] [--reps 20]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from empanada_amd import _hip  # noqa: E402


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=32)
    ap.add_argument('--size', type=int, default=1024)
    ap.add_argument('--reps', type=int, default=20)
    args = ap.parse_args()
    _hip.require_gpu()
    H = args.size
    for C in (1, 2, 3):
        x = torch.randn((args.n, C, H // 4, H // 4), device='cuda')
        out = torch.empty((args.n, C, H, H), device='cuda')
        nbytes = 4 * (x.numel() + out.numel())
        up = timed(lambda: _hip.upsample_bilinear(x, (H, H), out=out), args.reps)
        two = timed(lambda: _hip.logits_to_prob(_hip.upsample_bilinear(x, (H, H), out=out), out=out), args.reps)
        f0 = timed(lambda: _hip.upsample_bilinear_prob(x, (H, H), out=out, prob=False), args.reps)
        f1 = timed(lambda: _hip.upsample_bilinear_prob(x, (H, H), out=out, prob=True), args.reps)
        print(json.dumps({'C': C, 'n': args.n, 'size': H, 'upsample_ms': round(up, 4), 'upsample_TBps': round(nbytes / up / 1e9, 2),
                          'upsample_then_prob_ms': round(two, 4), 'fused_prob0_ms': round(f0, 4),
                          'fused_prob1_ms': round(f1, 4), 'fused_prob1_TBps': round(nbytes / f1 / 1e9, 2)}), flush=True)


if __name__ == '__main__':
    main()
