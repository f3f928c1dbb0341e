"""Times of the many-centres path (profiles/many_centres.md): emp_find_centers_ws against emp_find_centers on the
same heat map at the same capacity, and emp_group_pixels per slice at K = 4096 / 16384 / 65535 on 512^2 coarse heads
(step 4) with offsets that point at the nearest centre ("structured") and with random offsets (every wave falls back
to the walk over all K centres).  Device events around `reps` calls after a warm-up; needs the GPU.

    python tools/bench_many_centres.py [--reps 20] [--out file.json]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from empanada_amd import _hip  # noqa: E402


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def blob_heat_map(D, size, n_blobs, gen):
    """n_blobs Gaussian bumps (sigma 2) of random height per slice: what a centre head looks like"""
    hm = torch.zeros((D, 1, size, size), device='cuda')
    for d in range(D):
        spots = torch.randperm(size * size, generator=gen, device='cuda')[:n_blobs]
        hm[d].view(-1)[spots] = torch.rand(n_blobs, generator=gen, device='cuda') * 0.5 + 0.5
    r = torch.arange(-6, 7, device='cuda', dtype=torch.float32)
    g = torch.exp(-r * r / 8.0)
    hm = F.conv2d(hm, g.view(1, 1, -1, 1), padding=(6, 0))
    hm = F.conv2d(hm, g.view(1, 1, 1, -1), padding=(0, 6))
    return hm[:, 0].contiguous()


def nearest_centre(ctr, h, w, chunk=4096):
    """(h*w, 2) coordinates of the centre nearest to every pixel"""
    yy, xx = torch.meshgrid(torch.arange(h, device='cuda'), torch.arange(w, device='cuda'), indexing='ij')
    pix = torch.stack([yy.reshape(-1), xx.reshape(-1)], dim=1).float()
    c = ctr.float()
    out = torch.empty((h * w, 2), device='cuda')
    for s in range(0, h * w, chunk):
        out[s:s + chunk] = c[torch.cdist(pix[s:s + chunk], c).argmin(dim=1)]
    return out, pix


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    _hip.require_gpu()
    gen = torch.Generator(device='cuda')
    gen.manual_seed(1)
    res = {'reps': args.reps, 'find_centers': [], 'group_pixels': []}

    # ---- detection: the price of the bitmap pass, against the kernel of the default path
    for D in (1, 16, 64):
        hm = blob_heat_map(D, 1024, 3000, gen)
        idx_a, cnt_a = _hip.find_centers(hm, 0.1, 7, cap=4096)
        idx_b, cnt_b = _hip.find_centers_ws(hm, 0.1, 7, 4096)
        assert torch.equal(cnt_a, cnt_b) and int(cnt_a.max()) <= 4096
        for d in range(D):
            assert torch.equal(idx_a[d, :int(cnt_a[d])], idx_b[d, :int(cnt_a[d])])
        t_old = timed(lambda: _hip.find_centers(hm, 0.1, 7, cap=4096), args.reps)
        t_new = timed(lambda: _hip.find_centers_ws(hm, 0.1, 7, 4096), args.reps)
        t_new_max = timed(lambda: _hip.find_centers_ws(hm, 0.1, 7, _hip.CENTER_LIMIT), args.reps)
        row = {'D': D, 'size': 1024, 'centres_per_slice': float(cnt_a.float().mean()),
               'emp_find_centers_ms_per_slice': t_old / D, 'emp_find_centers_ws_ms_per_slice': t_new / D,
               'emp_find_centers_ws_cap65535_ms_per_slice': t_new_max / D}
        res['find_centers'].append(row)
        print(json.dumps(row), flush=True)

    # ---- grouping at large K, 512^2 coarse heads
    h = w = 512
    D = 4
    for K in (4096, 16384, 65535):
        flat = torch.stack([torch.randperm(h * w, generator=gen, device='cuda')[:K].sort().values for _ in range(D)])
        idx = flat.int().contiguous()
        cnt = torch.full((D,), K, dtype=torch.int32, device='cuda')
        offs = {}
        structured = []
        for d in range(D):
            near, pix = nearest_centre(torch.stack([flat[d] // w, flat[d] % w], dim=1), h, w)
            o = (near - pix) * 4 + torch.randn((h * w, 2), generator=gen, device='cuda') * 0.5
            structured.append(o.t().reshape(2, h, w))
        offs['structured'] = torch.stack(structured).contiguous()
        offs['random'] = (torch.randn((D, 2, h, w), generator=gen, device='cuda') * 4 * 150).contiguous()
        for family, off in offs.items():
            t = timed(lambda: _hip.group_pixels(idx, cnt, off, 4), max(args.reps // 4, 3), warmup=1)
            row = {'K': K, 'family': family, 'D': D, 'size': 512, 'step': 4, 'emp_group_pixels_ms_per_slice': t / D}
            res['group_pixels'].append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
