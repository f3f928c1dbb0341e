"""Times of down-sampled inference (profiles/downsample.md).  Needs the GPU.

(a) feeder: device-event time of DeviceVolume.batch for the three planes of a size^3 uint8 volume at f = 1 (the
    existing emp_slices_to_input, the yardstick) and f = 2, 4 (emp_slices_to_input_scaled): ms per call of `slices`
    slices, algorithmic bytes/s (source bytes read once + fp32 bytes written) and ns per OUTPUT pixel (padded).
(b) driver: infer_volume on a synthetic size^3 volume with the MitoNet configuration (PanopticDeepLabPR / ResNet-50,
    synthesised weights, Render engine, median 3) at f = 1, 2, 4: wall time of the second call, Mvox/s of the
    full-resolution volume, peak allocated memory.

    python tools/bench_downsample.py feeder [--size 1024] [--slices 64] [--reps 10]
    python tools/bench_downsample.py driver [--size 512] [--axes xy,xz,yz] [--factors 1,2,4]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from empanada_amd import _hip  # noqa: E402
from empanada_amd.data import DeviceVolume  # noqa: E402

NORMS = dict(mean=0.508979, std=0.148561)
MITO = dict(encoder='resnet50', num_classes=1, stage4_stride=16, decoder_channels=256, low_level_stages=[1],
            low_level_channels_project=[32], atrous_rates=[2, 4, 6], aspp_channels=None, aspp_dropout=0.5,
            ins_decoder=True, ins_ratio=0.5)
ENGINE = dict(thing_list=[1], label_divisor=20000, stuff_area=64, void_label=0, nms_threshold=0.1, nms_kernel=7,
              confidence_thr=0.3, padding_factor=16, coarse_boundaries=True, median_kernel_size=3)


def timed(fn, reps, warmup=2):
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


def feeder(args):
    size, n = args.size, args.slices
    gen = torch.Generator(device='cuda')
    gen.manual_seed(1)
    vol = torch.randint(0, 256, (size, size, size), dtype=torch.uint8, device='cuda', generator=gen)
    rows = []
    for f in (1, 2, 4):
        dv = DeviceVolume(vol, NORMS['mean'], NORMS['std'], 16, 'cuda', scale=f)
        for axis in ('xy', 'xz', 'yz'):
            hp, wp = dv.padded_shape(axis)
            out = torch.empty((n, 1, hp, wp), dtype=torch.float32, device='cuda')
            ms = timed(lambda: dv.batch(axis, 0, n, out=out), args.reps)
            h, w = dv.plane_shape(axis)
            nbytes = n * h * w + 4 * out.numel()
            row = {'f': f, 'axis': axis, 'slices': n, 'plane': [h, w], 'output': [hp, wp], 'ms_per_call': ms,
                   'GB_per_s': nbytes / ms / 1e6, 'ns_per_output_pixel': ms * 1e6 / out.numel()}
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def driver(args):
    from empanada_amd import synthetic as SY
    from empanada_amd.inference.driver import infer_volume
    from empanada_amd.inference.engines import PanopticDeepLabRenderEngine3d
    from empanada_amd.models import PanopticDeepLabPR, prepare_for_inference, synthesize_weights
    model = synthesize_weights(PanopticDeepLabPR(**MITO))
    with torch.no_grad():                                  # as bench.py: logits of O(5)
        for head in (model.semantic_head, model.ins_center, model.ins_xy):
            head.head[1].weight.mul_(0.1)
    engine = PanopticDeepLabRenderEngine3d(prepare_for_inference(model, 'cuda'), **ENGINE)
    vol = SY.em_volume((args.size,) * 3, seed=7)
    axes = tuple(args.axes.split(','))
    rows = []
    for f in (int(v) for v in args.factors.split(',')):
        dv = DeviceVolume(vol, NORMS['mean'], NORMS['std'], 16, 'cuda', scale=f)
        times = []
        for _ in range(2):                                 # the first call warms up (library plans, workspaces)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            res = infer_volume(engine, dv, norms=NORMS, labels=[1], axes=axes, downsample_f=f)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        row = {'f': f, 'size': args.size, 'axes': list(axes), 'warmup_s': times[0], 'wall_s': times[1],
               'Mvox_per_s': args.size ** 3 / times[1] / 1e6,
               'peak_allocated_GiB': torch.cuda.max_memory_allocated() / 2 ** 30,
               'instances': int(res['instances'][1]),
               'labelled_share': float((res['volumes'][1].view(torch.int32) != 0).float().mean())}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del res, dv
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('what', choices=['feeder', 'driver'])
    ap.add_argument('--size', type=int, default=None)
    ap.add_argument('--slices', type=int, default=64)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--axes', default='xy,xz,yz')
    ap.add_argument('--factors', default='1,2,4')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    _hip.require_gpu()
    if args.size is None:
        args.size = 1024 if args.what == 'feeder' else 512
    rows = feeder(args) if args.what == 'feeder' else driver(args)
    if args.out:
        with open(args.out, 'w') as fh:
            json.dump({'what': args.what, 'size': args.size, 'rows': rows}, fh, indent=1)


if __name__ == '__main__':
    main()
