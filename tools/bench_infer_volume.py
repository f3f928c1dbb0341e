"""Wall time of the one-call API, infer_volume, with and without pipeline=VolumePipeline(...)
(profiles/infer_volume_pipeline.md).  Needs the GPU.

A synthetic size^3 uint8 volume, the model bench.py names (synthesised weights, last layers damped as there), the
engine parameters of bench.py with max_centers=65535 (random weights can produce many maxima), results written to a
zarr store under /dev/shm.  Per path an engine of its own and `--warmup` untimed calls (library plans, the tuner search,
graph capture), one call for the peak memory, then `--repeats` timed calls with the paths alternating, each call between
two device synchronisations.  One JSON line.

    python tools/bench_infer_volume.py --size 512 [--model pdl_r50|mitonet_pr] [--axes xy,xz,yz] [--paths plain,pipeline]
                                       [--repeats 3] [--warmup 1] [--no-tune] [--no-graph] [--overlap auto|on|off]
                                       [--window-slices W|auto] [--pyramid L] [--compressor zlib] [--measure]

--measure times every path named a second time as '<path>+measure', the same call with measure=True (per-object table,
csrc/emp_measure.hip), on the same engine and in the same alternation: the path without it, which launches nothing new,
is the comparison (profiles/label_measure.md).

--window-slices streams every plane through windows of W slices (inference/windowed.py) on the paths named; the row then
holds the steps per plane and the bytes of head buffers held (profiles/windowed_planes.md).

--pyramid L adds L (2, 2, 2) levels of a multiscale pyramid to every call (inference/pyramid.py; the levels are pooled on
the device and written beside level 0), --compressor zlib writes every level as zlib streams made on the device; the
same command without them is the comparison (profiles/label_pyramid.md).

--split also times the forwards of the three planes alone (heads written in place, no post-processing) on the pipeline's
own code, so that a volume whose random heads make the post-processing dominate can be read.

--split 26 (or 6 / 18) also times every path with split_objects= of that connectivity, as '<path>+split', alternating
with the path without it, and records res['split'] of class 1: how many ids were disconnected, how many pieces got a
new id and how many were erased (profiles/label_components.md).

--fill also times every path with fill_holes=True, as '<path>+fill', alternating likewise, and records res['filled'] of
class 1: how many closed cavities there were, how many were filled, shared or too large (profiles/label_holes.md).
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from empanada_amd import _hip  # noqa: E402

NORMS = dict(mean=0.508979, std=0.148561)
MITO = dict(encoder='resnet50', num_classes=1, stage4_stride=16, decoder_channels=256, low_level_stages=[1],
            low_level_channels_project=[32], atrous_rates=[2, 4, 6], aspp_channels=None, aspp_dropout=0.5,
            ins_decoder=True, ins_ratio=0.5)
ENGINE = dict(thing_list=[1], label_divisor=20000, stuff_area=64, void_label=0, nms_threshold=0.1, nms_kernel=7,
              confidence_thr=0.3, median_kernel_size=7, padding_factor=16, max_centers=65535)


def build_engine(name):
    from empanada_amd.inference import engines as EN
    from empanada_amd.models import PanopticDeepLab, PanopticDeepLabPR, prepare_for_inference, synthesize_weights
    if name == 'pdl_r50':
        model = PanopticDeepLab(encoder='resnet50', num_classes=1)
    else:
        model = PanopticDeepLabPR(**MITO)
    model = synthesize_weights(model)
    with torch.no_grad():                                  # as bench.py: logits of O(5)
        for head in (model.semantic_head, model.ins_center, model.ins_xy):
            head.head[1].weight.mul_(0.1)
    model = prepare_for_inference(model, 'cuda')
    if name == 'pdl_r50':
        return EN.PanopticDeepLabEngine3d(model, **ENGINE)
    return EN.PanopticDeepLabRenderEngine3d(model, coarse_boundaries=True, **ENGINE)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, res


def forwards_only(pipe, dv, axes, repeats):
    """the forwards of all planes through the pipeline's own code (VolumePipeline.forwards_only), nothing else"""
    times = []
    for _ in range(repeats + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pipe.forwards_only(dv, axes)
        times.append(time.perf_counter() - t0)
    return times[1:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--model', default='pdl_r50', choices=['pdl_r50', 'mitonet_pr'])
    ap.add_argument('--axes', default='xy,xz,yz', help="comma list of planes; 'xy' alone = stack mode")
    ap.add_argument('--paths', default='plain,pipeline')
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--batch-pixels', type=int, default=32 << 20)
    ap.add_argument('--no-tune', action='store_true')
    ap.add_argument('--load-tune', default=None, help='per-site choices (json) instead of the live search')
    ap.add_argument('--save-tune', default=None)
    ap.add_argument('--no-graph', action='store_true')
    ap.add_argument('--overlap', default='auto', choices=['auto', 'on', 'off'])
    ap.add_argument('--split', nargs='?', const='forwards', default=None, choices=['forwards', '6', '18', '26'],
                    help="bare: also time the forwards alone; 6 / 18 / 26: also time every path with split_objects= of "
                         "that connectivity, as '<path>+split', and report what the split found")
    ap.add_argument('--fill', action='store_true',
                    help="also time every path with fill_holes=True, as '<path>+fill', and report res['filled'] of class 1")
    ap.add_argument('--window-slices', default=None, help="slices per window, or 'auto'; default: whole planes")
    ap.add_argument('--pyramid', type=int, default=None, help='levels of a (2, 2, 2) label pyramid to add')
    ap.add_argument('--compressor', default=None, choices=['zlib'])
    ap.add_argument('--measure', action='store_true', help="also time every path with measure=True, as '<path>+measure'")
    ap.add_argument('--out', default=None, help='write the JSON line to this file as well')
    args = ap.parse_args()
    _hip.require_gpu()
    from empanada_amd import synthetic as SY
    from empanada_amd.data import DeviceVolume
    from empanada_amd.inference.driver import infer_volume
    from empanada_amd.inference.pipeline import VolumePipeline
    from empanada_amd.zarr_utils import ZarrV2Group

    axes = tuple(args.axes.split(','))
    paths = args.paths.split(',')
    dv = DeviceVolume(SY.em_volume((args.size,) * 3, seed=7), NORMS['mean'], NORMS['std'], 16, 'cuda')
    base = '/dev/shm' if os.path.isdir('/dev/shm') else tempfile.gettempdir()
    store = tempfile.mkdtemp(prefix='emp_infer_volume_', dir=base)
    kw = dict(norms=NORMS, labels=[1], axes=axes, class_names={1: 'mito'}, out=ZarrV2Group(store))
    if args.window_slices is not None:
        kw['window_slices'] = 'auto' if args.window_slices == 'auto' else int(args.window_slices)
    if args.pyramid is not None:
        kw['pyramid'] = args.pyramid
    if args.compressor is not None:
        kw['compressor'] = args.compressor
    row = {'size': args.size, 'model': args.model, 'axes': list(axes), 'batch_pixels': args.batch_pixels,
           'window_slices': kw.get('window_slices'), 'pyramid': args.pyramid, 'compressor': args.compressor,
           'device': torch.cuda.get_device_name(0), 'repeats': args.repeats, 'warmup': args.warmup}
    split_objects = int(args.split) if args.split not in (None, 'forwards') else None
    row['split_objects'] = split_objects
    fns, pipe, last = {}, None, {}
    try:
        # one engine per path: the plain path keeps every call site on its default, as a caller without pipeline= has it,
        # while the pipeline tunes its own engine's sites.  Per path: warm-up calls, one call for the peak memory; then
        # the timed calls of the paths ALTERNATE, so that whatever else the host and the device do hits both alike
        for path in list(paths):
            engine = build_engine(args.model)
            if path == 'plain':
                call = lambda e=engine, **more: infer_volume(e, dv, batch_pixels=args.batch_pixels, **kw, **more)
            else:
                tune = False if args.no_tune else (args.load_tune or True)
                pipe = VolumePipeline(engine, tune=tune, graph=not args.no_graph,
                                      overlap={'auto': 'auto', 'on': True, 'off': False}[args.overlap],
                                      batch_pixels=args.batch_pixels)
                call = lambda e=engine, **more: infer_volume(e, dv, pipeline=pipe, **kw, **more)
            fns[path] = call
            names = [path]
            if args.measure:
                fns[path + '+measure'] = lambda c=call: c(measure=True)
                names.append(path + '+measure')
            if split_objects is not None:
                fns[path + '+split'] = lambda c=call: c(split_objects=split_objects)
                names.append(path + '+split')
            if args.fill:
                fns[path + '+fill'] = lambda c=call: c(fill_holes=True)
                names.append(path + '+fill')
            paths[paths.index(path):paths.index(path) + 1] = names
            for name in names:
                warm = [round(timed(fns[name])[0], 3) for _ in range(args.warmup)]
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats()
                before = torch.cuda.memory_allocated()
                timed(fns[name])
                row[name] = {'warmup_s': warm, 'seconds': [],
                             'peak_allocated_GiB': round(torch.cuda.max_memory_allocated() / 2 ** 30, 3),
                             'allocated_before_call_GiB': round(before / 2 ** 30, 3)}
        for _ in range(args.repeats):
            for path in paths:
                t, last[path] = timed(fns[path])
                row[path]['seconds'].append(round(t, 4))
        for path in paths:
            times, res = row[path]['seconds'], last[path]
            row[path].update({'median_s': sorted(times)[len(times) // 2],
                              'spread_s': round(max(times) - min(times), 4),
                              'Mvox_per_s': round(args.size ** 3 / sorted(times)[len(times) // 2] / 1e6, 2),
                              'instances': int(res['instances'][1]),
                              'object_rows': None if 'objects' not in res else int(res['objects'][1].shape[0]),
                              'split': res.get('split', {}).get(1),
                              'filled': res.get('filled', {}).get(1),
                              'windows': res.get('windows'), 'head_bytes': res.get('head_bytes'),
                              'labelled_share': round(float((res['volumes'][1].view(torch.int32) != 0).float().mean()), 5)})
        if pipe is not None:
            row['pipeline']['pipeline'] = last['pipeline']['pipeline']
            if args.save_tune:
                pipe.save_tune(args.save_tune)
            if args.split == 'forwards':
                row['pipeline']['forwards_only_s'] = [round(t, 4) for t in forwards_only(pipe, dv, axes, args.repeats)]
            pipe.close()
        if 'plain' in row and 'pipeline' in row:
            row['speedup'] = round(row['plain']['median_s'] / row['pipeline']['median_s'], 3)
            a, b = last['plain']['volumes'][1].view(torch.int32), last['pipeline']['volumes'][1].view(torch.int32)
            # the two engines differ in their call sites' implementations (rounding), so the labels may differ a little
            row['voxels_labelled_differently'] = round(float(((a != 0) != (b != 0)).float().mean()), 6)
    finally:
        shutil.rmtree(store, ignore_errors=True)
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
