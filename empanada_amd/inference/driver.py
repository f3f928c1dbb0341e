"""Volume-level driver of the whole-stack path: what scripts/pdl_inference3d.py:110-233 does slice by slice --
for every plane: model -> engine -> RLE -> forward / backward matching -> trackers -> filters; then the consensus over
the planes (orthoplane mode) or the single plane's trackers (stack mode); then `fill_volume` into a zarr dataset per
class -- as ONE call that keeps the volume, the head tensors of a plane and every run table resident in HBM.

    engine = PanopticDeepLabRenderEngine3d(model, **engine_params)          # any of the four engines
    result = infer_volume(engine, volume_u8, norms=desc['norms'], labels=desc['labels'],
                          class_names=desc['class_names'], out=ZarrV2Group('out.zarr'))

With torch.distributed initialised (one process per GPU, backend 'nccl') every rank calls it with the same volume: the
slices of every plane are split into contiguous blocks over the ranks and each rank writes its own z-slab
(empanada_amd/inference/sharded.py).  Results are identical to the per-slice protocol on the same head tensors
(tests/test_pipeline_gpu.py).  bench.py times a pipeline of its own on planted heads (tuned sites, graph replay, two
streams); the product's form of that is `pipeline=VolumePipeline(engine)` (empanada_amd/inference/pipeline.py), which
computes the same volumes as the plain call (tests/test_volume_pipeline_gpu.py) and is timed by
tools/bench_infer_volume.py.
"""
import numpy as np
import torch

from .. import _hip
from ..data import DeviceVolume
from ..zarr_utils import ZarrV2Group
from . import pyramid as pyr
from . import sharded, windowed
from .engines import logits_to_prob

__all__ = ['infer_volume']

_AXES = {'xy': 0, 'xz': 1, 'yz': 2}
_HEADS = (('sem', 'sem_logits'), ('ctr_hmp', 'ctr_hmp'), ('offsets', 'offsets'))


# ---------------------------------------------------------------- the facts of a plane, shared with inference/pipeline.py
def slices_per_call(dv, axis, batch_pixels):
    """batch_pixels counts OUTPUT pixels: with a down-sampling volume (dv.scale = f > 1) the semantic head comes out at
    f x the padded input, so batch_pixels keeps bounding the memory"""
    hp, wp = dv.padded_shape(axis)
    return max(1, batch_pixels // (hp * wp * dv.scale ** 2))


def model_args(engine, steps):
    """extra positional arguments of the model's forward: (render_steps, interpolate_ins) for the PointRend ("render")
    engines, none for the plain ones"""
    return (steps, not engine.coarse_boundaries) if hasattr(engine, 'coarse_boundaries') else ()


def model_classes(model, dv, axis, margs):
    """channels of the semantic head: what the model says, or what it returns for one slice"""
    c = int(getattr(model, 'num_classes', 0))
    if not c:
        with torch.no_grad():
            x = dv.batch(axis, 0, 1).to(next(model.parameters()).dtype)
            c = int(model(x, *margs)['sem_logits'].shape[1])
    return c


def plane_head_shapes(engine, dv, axis, classes):
    """per-slice shapes of the plane's heads at the padded size (the reference pads every slice to a multiple of
    padding_factor and crops the labels, engines.py:351-394); n slices of them are (n,) + shape"""
    render = hasattr(engine, 'coarse_boundaries')
    return windowed.head_shapes(*dv.padded_shape(axis), classes, dv.scale if render else 1,
                                render and bool(engine.coarse_boundaries))


def write_heads(o, views):
    """the three heads of one model call, each written once into its (slices,) + shape fp32 view: a head the model left at
    quarter resolution (`deferred_up4`) is up-sampled into it, the semantic logits become probabilities on the way"""
    deferred = o.get('deferred_up4', ())
    for name, key in _HEADS:
        t, view = o[key], views[name]
        up = key in deferred
        if tuple(view.shape[:2] if up else view.shape) != tuple(t.shape[:2] if up else t.shape):
            raise RuntimeError(f"head {key}: the model returned {tuple(t.shape)}, the plane buffer holds "
                               f"{tuple(view.shape)}")
        if up:
            _hip.upsample_bilinear_prob(t, view.shape[2:], out=view, prob=name == 'sem')
        elif name != 'sem':
            view.copy_(t)
        elif t.dtype == torch.float32:
            _hip.logits_to_prob(t, out=view)
        else:
            view.copy_(logits_to_prob(t))


@torch.no_grad()
def forward_heads(model, margs, dv, axis, lo, hi, per, bufs, at=0):
    """slices [lo, hi) of the plane through the model in calls of `per`, on the current stream; the heads of slice s go to
    bufs[name][at + s - lo].  A GraphedForward's static input, once captured, is filled by the slice feeder itself"""
    hp, wp = dv.padded_shape(axis)
    dtype = next(model.parameters()).dtype
    static = getattr(model, 'input_buffer', None)
    for s in range(lo, hi, per):
        e = min(hi, s + per)
        x = dv.batch(axis, s, e, out=static((e - s, 1, hp, wp), args=margs) if static else None)
        if x.dtype != dtype:
            x = x.to(dtype)
        # the model's own outputs are not kept past this line: the next call's activations find that memory free
        write_heads(model(x.contiguous(memory_format=torch.channels_last), *margs),
                    {k: v[at + s - lo:at + e - lo] for k, v in bufs.items()})


def dataset_names(labels, class_names):
    return {c: f"{(class_names or {}).get(c, c)}_pred" for c in labels}


def open_datasets(out, labels, thing_list, class_names, shape3d, rank, world, group, compressor=None, levels=()):
    """{class: the '<class name>_pred' array of `out`, or None without one}: uint32 for thing classes, uint8 for stuff,
    chunks (1, Y, X) (pdl_inference3d.py:225-233); rank 0 creates them before any rank opens one.  compressor='zlib':
    created with {"id": "zlib", "level": 1} (the reference's datasets are compressed too, :228-233).  levels: the plan of
    a pyramid (pyramid.plan) -- rank 0 also creates '<class name>_pred_s<l>' for level l = 1 .. with the level's shape
    and the dtype, chunking and compressor of level 0, before the same barrier; open_level_datasets opens them"""
    if out is None:
        return {c: None for c in labels}
    names = dataset_names(labels, class_names)
    extra = {} if compressor is None else {'compressor': {'id': 'zlib', 'level': 1}}
    if rank == 0:
        for c in labels:
            for l, shape in enumerate([shape3d] + [lv['shape'] for lv in levels]):
                out.create_dataset(names[c] + (f"_s{l}" if l else ""), shape=shape,
                                   dtype=np.uint32 if c in thing_list else np.uint8, overwrite=True,
                                   chunks=(1, None, None), **extra)
    if world > 1:
        torch.distributed.barrier(group=group)
    return {c: out[names[c]] for c in labels}


def open_level_datasets(out, labels, class_names, levels):
    """{class: [the '<class name>_pred_s<l>' array of level l = 1 .., or None without `out`]}, after open_datasets"""
    names = dataset_names(labels, class_names)
    return {c: [None if out is None else out[f"{names[c]}_s{l}"] for l in range(1, len(levels) + 1)] for c in labels}


def pyramid_levels(pyramid, shape3d, world):
    """infer_volume's `pyramid` argument -> the plan (pyramid.plan) of every rank's z-slab, before any GPU work: a
    ValueError for a bad value or for a slab that a level's cells would straddle, on every rank alike"""
    return pyr.check_ranks(shape3d, pyr.normalize(pyramid), sharded.shard_bounds(int(shape3d[0]), world))


def _update_attrs(out, attrs):
    """`attrs` into the attributes of `out` beside what is there already; an `out` without attributes gets none"""
    if isinstance(out, ZarrV2Group):
        out.update_attrs(attrs)
    elif hasattr(out, 'attrs'):
        out.attrs.update(attrs)


def _write_tables(out, group, arrays, rows, attrs):
    """What the stages that store tables share.  The group's first rank creates one dataset per entry of
    arrays[key] = {dataset name: numpy array}, one chunk along the rows, writes the arrays that have rows and merges
    `attrs` into the attributes of `out`.  A store that cannot hold a zero-row array fails the creation: with
    rows[key] == 0 the key is left out instead, with rows it is an error.  Returns the set of keys left out, the same on
    every rank: the broadcast also tells the other ranks that the datasets are there to be opened."""
    rank, world = sharded._world(group)
    left_out = set()
    if rank == 0:
        for key, named in arrays.items():
            try:
                for name, a in named.items():
                    ds = out.create_dataset(name, shape=a.shape, dtype=a.dtype, overwrite=True,
                                            chunks=(max(a.shape[0], 1),) + tuple(a.shape[1:]))
                    if a.shape[0]:
                        ds[...] = a
            except Exception:
                if rows[key]:
                    raise
                left_out.add(key)
        _update_attrs(out, attrs)
    if world > 1:
        flag = [sorted(left_out, key=str)]
        src = 0 if group is None else torch.distributed.get_global_rank(group, 0)
        torch.distributed.broadcast_object_list(flag, src=src, group=group)
        left_out = set(flag[0])
    return left_out


def write_multiscales(out, labels, class_names, levels):
    """one OME-NGFF `multiscales` entry per class into the attributes of `out` (rank 0, after its levels are written):
    entries of other names are kept, one of the same name is replaced; an `out` without attributes gets none"""
    names = dataset_names(labels, class_names)
    cum = [(1, 1, 1)] + [lv['factor'] for lv in levels]
    new = [pyr.multiscales(names[c], [names[c]] + [f"{names[c]}_s{l}" for l in range(1, len(cum))], cum) for c in labels]
    if not isinstance(out, ZarrV2Group) and not hasattr(out, 'attrs'):
        return
    mine = {e['name'] for e in new}
    kept = [e for e in out.attrs.get('multiscales', []) if not (isinstance(e, dict) and e.get('name') in mine)]
    _update_attrs(out, {'multiscales': kept + new})


def host_slab(vol, thing):
    """a labelled device slab as the numpy array write_slab takes"""
    return vol.view(torch.int32).cpu().numpy().view(np.uint32) if thing else vol.cpu().numpy()


def result(vols, z_range, counts, datasets, windows=None, head_bytes=0, pipeline=None, compressed=None, pyramid=None):
    """infer_volume's result; windows ({axis: steps}): a windowed call, which also reports the head buffers it held;
    compressed ({class: bytes}): a call with compressor='zlib'; pyramid: a call with pyramid=, the keys it adds"""
    res = {'volumes': vols, 'z_range': z_range, 'instances': counts, 'datasets': datasets}
    if compressed is not None:
        res['compressed_bytes'] = compressed
    if pyramid is not None:
        res.update(pyramid)
    if windows is not None:
        res.update(windows=windows, head_bytes=int(head_bytes))
    if pipeline is not None:
        res['pipeline'] = pipeline
    return res


# ---------------------------------------------------------------------------------------------- the plain call's planes
@torch.no_grad()
def _plane_heads(engine, dv, axis, lo, hi, batch_pixels, render_steps):
    """model forward over slices [lo, hi) of one plane -> resident {'sem' probabilities, 'ctr_hmp', 'offsets'} at the
    padded size, every model call writing its slices of the three buffers"""
    margs = model_args(engine, render_steps)
    shapes = plane_head_shapes(engine, dv, axis, model_classes(engine.model, dv, axis, margs))
    heads = {k: torch.empty((hi - lo,) + s, dtype=torch.float32, device=dv.vol.device) for k, s in shapes.items()}
    forward_heads(engine.model, margs, dv, axis, lo, hi, slices_per_call(dv, axis, batch_pixels), heads)
    return heads


def _check_windows(window_slices, mem_budget, pipeline, world):
    """argument errors of the window switch, before any GPU work"""
    w = window_slices
    if w is not None and w != 'auto' and (isinstance(w, bool) or not isinstance(w, (int, np.integer)) or w < 1):
        raise ValueError(f"window_slices must be None, a positive number of slices or 'auto', got {w!r}")
    if mem_budget is not None:
        if isinstance(mem_budget, bool) or not isinstance(mem_budget, (int, np.integer)) or mem_budget < 1:
            raise ValueError(f"mem_budget must be a positive number of bytes, got {mem_budget!r}")
        if pipeline is not None:
            raise ValueError(f"mem_budget={mem_budget} given together with a pipeline: with pipeline= the pipeline's own "
                             "mem_budget serves window_slices='auto'")
    if w is not None and world > 1:
        raise ValueError(f"window_slices={w!r} with {world} ranks: windows within a rank's block are not built yet "
                         "(the hand-over across ranks stays as it is); leave window_slices=None")
    return w if w is None or w == 'auto' else int(w)


def _check_compressor(compressor, out):
    """argument errors of the compressed output, before any GPU work"""
    if compressor is None:
        return
    if compressor != 'zlib':
        raise ValueError(f"compressor must be None (raw chunks) or 'zlib', got {compressor!r}")
    if out is None:
        raise ValueError("compressor='zlib' without out=: there is nothing to compress, the volumes stay on the device")
    if not isinstance(out, ZarrV2Group):
        raise ValueError(f"compressor='zlib' needs out= to be a ZarrV2Group (the streams are written as its chunk files), "
                         f"got {type(out).__name__}")


def _check_ground_truth(ground_truth, labels, shape3d):
    """argument errors of the scoring, before any GPU work"""
    if ground_truth is None:
        return
    for c, gt in ground_truth.items():
        if c not in labels:
            raise ValueError(f"ground_truth has class {c!r}, the labels are {labels}")
        if tuple(gt.shape) != tuple(shape3d):
            raise ValueError(f"ground_truth[{c!r}] is {tuple(gt.shape)}, the volume {tuple(shape3d)}")


def _scored(res, ground_truth, thing_list, group):
    """the result with 'scores': each rank's slab of every class that has a ground truth against the same z-range of
    it, the overlap tables added over the ranks"""
    if ground_truth is not None:
        from ..evaluation import volume_scores
        z0, z1 = res['z_range']
        res['scores'] = {c: volume_scores(gt[z0:z1], res['volumes'][c], instances=c in thing_list, group=group)
                         for c, gt in ground_truth.items()}
    return res


def _check_measure(measure):
    """infer_volume's `measure` argument -> None or the voxel spacing (sz, sy, sx), before any GPU work"""
    if measure is None:
        return None
    if measure is True:
        return (1.0, 1.0, 1.0)
    bad = ValueError(f"measure must be None, True or a voxel spacing (sz, sy, sx) of three positive numbers, got {measure!r}")
    if isinstance(measure, (bool, np.bool_, str, bytes)):
        raise bad
    try:
        values = list(measure)
    except TypeError:
        raise bad from None
    import numbers
    if len(values) != 3 or any(isinstance(v, (bool, np.bool_)) or not isinstance(v, numbers.Real) for v in values):
        raise bad
    spacing = tuple(float(v) for v in values)
    if not all(np.isfinite(v) and v > 0 for v in spacing):
        raise bad
    return spacing


def object_dataset_names(labels, class_names):
    return {c: f"{(class_names or {}).get(c, c)}_objects" for c in labels}


_neighbour_slices = sharded.neighbour_slices


def _check_split(split_objects):
    """infer_volume's `split_objects` argument -> None or the connectivity, before any GPU work"""
    if split_objects is None:
        return None
    if isinstance(split_objects, (bool, np.bool_)) or not isinstance(split_objects, (int, np.integer)) \
            or int(split_objects) not in (6, 18, 26):
        raise ValueError(f"split_objects must be None or a connectivity of 6, 18 or 26, got {split_objects!r}")
    return int(split_objects)


def _repairing(finish, thing_list, stats, step):
    """`finish` with a repair of the thing classes behind it, before anything else reads the volumes: for every thing
    class, step(c, the class's slab made contiguous, z0, counts) returns the slab to keep and the repair's stats, which
    `stats` receives as {class: stats}; a step that changes the number of objects writes counts[c]"""
    def repaired_finish(planes):
        vols, (z0, z1), counts = finish(planes)
        counts = dict(counts)
        for c in vols:
            if c in thing_list:
                slab = vols[c] if vols[c].is_contiguous() else vols[c].contiguous()
                vols[c], stats[c] = step(c, slab, int(z0), counts)
        return vols, (z0, z1), counts

    return repaired_finish


def _splitting(finish, connectivity, thing_list, min_size, min_span, group, stats):
    """`finish` with the repair behind it: every thing class's slab goes through components.split_volume in place, with
    the call's min_size / min_span judged per piece, before anything reads the volumes; the counts become the objects
    that remain and `stats` receives {class: split_volume's stats}"""
    if connectivity is None:
        return finish
    from ..components import split_volume

    def split(c, slab, z0, counts):
        _, done = split_volume(slab, connectivity, min_size, min_span, group=group, z_base=z0)
        counts[c] = done['objects_out']
        return slab, done

    return _repairing(finish, thing_list, stats, split)


def _check_morph(morph):
    """infer_volume's `morph` argument -> None or (op, r2, sampling), before any GPU work"""
    from ..morphology import check
    return check(morph)


def _morphing(finish, morph, thing_list, shape3d, group, recount, stats):
    """`finish` with the morphology behind it: every thing class's slab is replaced by morphology.morph_volume's before
    anything else reads the volumes, and `stats` receives {class: morph_volume's stats}.  recount: an erosion or an
    opening can take an object's last voxel, so the counts become the distinct labels that remain (the rows of the
    measured table) -- unless split_objects, which runs next, counts anyway"""
    if morph is None:
        return finish
    from ..measurements import gather_tables
    from ..morphology import morph_volume
    op, r2, sampling = morph

    def morphed(c, slab, z0, counts):
        vol, done = morph_volume(slab, shape3d, op, r2, sampling, group=group, z_base=z0)
        if recount and op in ('erode', 'open'):
            below, above = _neighbour_slices(vol, group)
            table = gather_tables(_hip.measure_labels(vol, below=below, above=above, z_base=z0), group)
            counts[c] = int(table.shape[0])
        return vol, done

    return _repairing(finish, thing_list, stats, morphed)


def _check_separate(separate):
    """infer_volume's `separate` argument -> None or (r2, min_core, sampling), before any GPU work"""
    from ..separation import check
    return check(separate)


def _separating(finish, separate, thing_list, shape3d, group, recount, stats):
    """`finish` with the separation behind it: every thing class's slab goes through separation.separate_volume in
    place, after the morphology and before anything else reads the volumes, and `stats` receives {class:
    separate_volume's stats}.  recount: every piece that got a new label is one object more, so the counts grow by
    'pieces_added' -- unless split_objects, which runs next, counts anyway"""
    if separate is None:
        return finish
    from ..separation import separate_volume
    r2, min_core, sampling = separate

    def separated(c, slab, z0, counts):
        _, done = separate_volume(slab, shape3d, r2, min_core, sampling, group=group, z_base=z0)
        if recount:
            counts[c] = int(counts[c]) + done['pieces_added']
        return slab, done

    return _repairing(finish, thing_list, stats, separated)


def _check_fill(fill_holes):
    """infer_volume's `fill_holes` argument -> (wanted, cap in voxels or None), before any GPU work"""
    if fill_holes is None:
        return False, None
    if fill_holes is True:
        return True, None
    if isinstance(fill_holes, (bool, np.bool_)) or not isinstance(fill_holes, (int, np.integer)) or int(fill_holes) < 1:
        raise ValueError("fill_holes must be None, True or a positive number of voxels (the largest cavity to fill), "
                         f"got {fill_holes!r}")
    return True, int(fill_holes)


def _filling(finish, wanted, max_voxels, thing_list, shape3d, group, stats):
    """`finish` with the filling behind it: every thing class's slab goes through holes.fill_volume in place before
    anything reads the volumes; objects only grow, so the counts stay, and `stats` receives {class: fill_volume's stats}"""
    if not wanted:
        return finish
    from ..holes import fill_volume

    def filled(c, slab, z0, counts):
        _, done = fill_volume(slab, shape3d, max_voxels, group=group, z_base=z0)
        return slab, done

    return _repairing(finish, thing_list, stats, filled)


def _measured(res, spacing, labels, class_names, out, group):
    """the result with 'objects': every rank measures its slab of every class (_hip.measure_labels, z_base = z0) with the
    neighbouring ranks' end slices standing for what lies outside it, the tables are merged over the ranks, and rank 0
    writes one '<class name>_objects' dataset per class"""
    if spacing is None:
        return res
    from ..measurements import COLUMNS, gather_tables
    z0 = int(res['z_range'][0])
    objects = {}
    for c in labels:
        slab = res['volumes'][c].contiguous()
        below, above = _neighbour_slices(slab, group)
        objects[c] = gather_tables(_hip.measure_labels(slab, below=below, above=above, z_base=z0), group).cpu().numpy()
    res['objects'] = objects
    res['object_spacing'] = spacing
    if out is None:
        return res
    names = object_dataset_names(labels, class_names)
    assert all(t.dtype == np.int64 for t in objects.values())
    missing = _write_tables(out, group, {c: {names[c]: objects[c]} for c in labels},
                            {c: objects[c].shape[0] for c in labels},
                            {'objects': {'columns': list(COLUMNS), 'spacing': list(spacing)}})
    res['object_datasets'] = {c: None if c in missing else out[names[c]] for c in labels}
    return res


def _check_shapes(shapes):
    """infer_volume's `shapes` argument -> None or the voxel spacing (sz, sy, sx), before any GPU work"""
    from ..shapes import check
    return check(shapes)


def shape_dataset_names(labels, class_names):
    return {c: f"{(class_names or {}).get(c, c)}_shapes" for c in labels}


def _shaped(res, spacing, labels, class_names, out, group):
    """the result with 'shapes': every rank takes the shape sums of its slab of every class (_hip.shape_labels, z_base =
    z0) with the neighbouring ranks' end slices standing for what lies outside it, the tables are merged over the ranks,
    and rank 0 writes one '<class name>_shapes' dataset per class"""
    if spacing is None:
        return res
    from ..shapes import COLUMNS, gather_tables
    z0 = int(res['z_range'][0])
    tables = {}
    for c in labels:
        slab = res['volumes'][c].contiguous()
        below, above = _neighbour_slices(slab, group)
        tables[c] = gather_tables(_hip.shape_labels(slab, below=below, above=above, z_base=z0), group).cpu().numpy()
    res['shapes'] = tables
    res['shape_spacing'] = spacing
    if out is None:
        return res
    names = shape_dataset_names(labels, class_names)
    missing = _write_tables(out, group, {c: {names[c]: tables[c]} for c in labels},
                            {c: tables[c].shape[0] for c in labels},
                            {'shapes': {'columns': list(COLUMNS), 'spacing': list(spacing)}})
    res['shape_datasets'] = {c: None if c in missing else out[names[c]] for c in labels}
    return res


def _check_mesh(mesh):
    """infer_volume's `mesh` argument -> None or the number of smoothing iterations, before any GPU work"""
    from ..meshes import check
    return check(mesh)


def mesh_dataset_names(classes, class_names):
    return {c: {k: f"{(class_names or {}).get(c, c)}_mesh_{k}" for k in ('vertices', 'quads', 'objects')} for c in classes}


def _meshed(res, iterations, thing_list, shape3d, class_names, out, group):
    """the result with 'meshes': every rank emits its slab of every thing class (meshes.mesh_volume, z_base = z0) with
    the neighbouring ranks' end slices, every rank finishes the same whole mesh, and rank 0 writes three datasets per
    class"""
    if iterations is None:
        return res
    from ..meshes import OBJECT_COLUMNS, mesh_volume
    z0 = int(res['z_range'][0])
    classes = [c for c in res['volumes'] if c in thing_list]
    meshes = {}
    for c in classes:
        m = mesh_volume(res['volumes'][c], group, z0, int(shape3d[0]), iterations)
        meshes[c] = {k: v.cpu().numpy() for k, v in m.items()}
    res['meshes'] = meshes
    if out is None:
        return res
    names = mesh_dataset_names(classes, class_names)
    missing = _write_tables(out, group, {c: {names[c][k]: a for k, a in meshes[c].items()} for c in classes},
                            {c: meshes[c]['objects'].shape[0] for c in classes},
                            {'meshes': {'axes': 'zyx', 'object_columns': list(OBJECT_COLUMNS),
                                        'iterations': int(iterations)}})
    res['mesh_datasets'] = {c: None if c in missing else {k: out[names[c][k]] for k in names[c]} for c in classes}
    return res


def _check_skeleton(skeleton):
    """infer_volume's `skeleton` argument -> None or (r_cap, cap, sampling), before any GPU work"""
    from ..skeletons import check
    return check(skeleton)


SKELETON_KEYS = ('vertices', 'radius2', 'degree', 'edges', 'objects')


def skeleton_dataset_names(classes, class_names):
    return {c: {k: f"{(class_names or {}).get(c, c)}_skeleton_{k}" for k in SKELETON_KEYS} for c in classes}


def _skeletonized(res, skeleton, thing_list, shape3d, class_names, out, group):
    """the result with 'skeletons': the ranks thin every thing class in lock-step (skeletons.skeleton_volume, z0 = the
    slab's first slice), every rank finishes the same whole graph, and rank 0 writes five datasets per class"""
    if skeleton is None:
        return res
    from ..skeletons import OBJECT_COLUMNS, skeleton_volume
    r_cap, cap, sampling = skeleton
    z0 = int(res['z_range'][0])
    classes = [c for c in res['volumes'] if c in thing_list]
    skeletons = {}
    for c in classes:
        s = skeleton_volume(res['volumes'][c], group, z0, int(shape3d[0]), cap, sampling)
        skeletons[c] = {k: s[k].cpu().numpy() for k in SKELETON_KEYS}
    res['skeletons'] = skeletons
    if out is None:
        return res
    names = skeleton_dataset_names(classes, class_names)
    missing = _write_tables(out, group, {c: {names[c][k]: a for k, a in skeletons[c].items()} for c in classes},
                            {c: skeletons[c]['objects'].shape[0] for c in classes},
                            {'skeletons': {'axes': 'zyx', 'object_columns': list(OBJECT_COLUMNS), 'r_cap': float(r_cap),
                                           'sampling': [int(a) for a in sampling]}})
    res['skeleton_datasets'] = {c: None if c in missing else {k: out[names[c][k]] for k in names[c]} for c in classes}
    return res


def _check_contacts(contacts, labels, thing_list):
    """infer_volume's `contacts` argument -> None or (r2, sampling, the class pairs in sorted order), before any GPU work"""
    from ..contacts import check
    checked = check(contacts)
    if checked is None:
        return None
    r2, sampling, pairs = checked
    if pairs is None:
        pairs = [(c, c) for c in labels if c in thing_list] + [(c1, c2) for c1 in labels for c2 in labels if c1 != c2]
    for ca, cb in pairs:
        for c in (ca, cb):
            if c not in labels:
                raise ValueError(f"contacts: pairs name class {c!r}, the labels are {labels}")
    return r2, sampling, sorted(set(pairs), key=lambda p: (labels.index(p[0]), labels.index(p[1])))


def contact_dataset_names(pairs, class_names):
    name = lambda c: (class_names or {}).get(c, c)
    return {p: f"{name(p[0])}_{name(p[1])}_contacts" for p in pairs}


def _contacted(res, contacts, class_names, out, group):
    """the result with 'contacts': the ranks walk the class pairs in the same order; for each, every rank reads the
    contact table of its slab of A (_hip.label_contacts, z_base = z0) against its slab of B with B's halo slices from the
    ranks next to it (sharded.neighbour_slabs), the tables are merged over the ranks, and rank 0 writes one
    '<class a name>_<class b name>_contacts' dataset per pair"""
    if contacts is None:
        return res
    from ..contacts import COLUMNS, gather_tables, halo_slices
    r2, sampling, pairs = contacts
    z0 = int(res['z_range'][0])
    halo = halo_slices(r2, sampling)
    slabs = {c: res['volumes'][c].contiguous() for c in {c for p in pairs for c in p}}
    tables = {}
    for ca, cb in pairs:
        below, above = sharded.neighbour_slabs(slabs[cb], halo, group)
        table = _hip.label_contacts(slabs[ca], None if ca == cb else slabs[cb], r2, sampling, below=below, above=above,
                                    z_base=z0)
        tables[(ca, cb)] = gather_tables(table, group).cpu().numpy()
    res['contacts'] = tables
    res['contact_params'] = {'r2': int(r2), 'sampling': tuple(int(a) for a in sampling)}
    if out is None:
        return res
    names = contact_dataset_names(pairs, class_names)
    assert all(t.dtype == np.int64 for t in tables.values())
    missing = _write_tables(out, group, {p: {names[p]: tables[p]} for p in pairs},
                            {p: tables[p].shape[0] for p in pairs},
                            {'contacts': {'columns': list(COLUMNS), 'r2': int(r2), 'sampling': [int(a) for a in sampling],
                                          'pairs': [[ca, cb] for ca, cb in pairs]}})
    res['contact_datasets'] = {p: None if p in missing else out[names[p]] for p in pairs}
    return res


def _check_thickness(thickness):
    """infer_volume's `thickness` argument -> None or (r_cap, cap, sampling), before any GPU work"""
    from ..thickness import check
    return check(thickness)


def thickness_dataset_names(classes, class_names):
    return {c: f"{(class_names or {}).get(c, c)}_thickness" for c in classes}


def _thickened(res, thickness, thing_list, shape3d, class_names, out, group):
    """The result with 'thickness' and 'thickness_maps': every rank computes the map of its slab of every thing class
    with halo slices from the ranks next to it (thickness.thickness_volume) and the tables are merged over the ranks.
    With `out`, rank 0 creates one '<class name>_thickness' dataset per class -- uint16, the labels' shape, chunks
    (1, Y, X), always raw chunks: write_slab_device takes 1- and 4-byte items only, and a 2-byte device deflate is not
    built -- every rank writes its slab of it, and rank 0 writes the '<class name>_thickness_table' datasets"""
    if thickness is None:
        return res
    from ..thickness import COLUMNS, thickness_volume
    r_cap, cap, sampling = thickness
    rank, world = sharded._world(group)
    z0 = int(res['z_range'][0])
    classes = [c for c in res['volumes'] if c in thing_list]
    tables, maps = {}, {}
    for c in classes:
        stats = {}
        maps[c], table = thickness_volume(res['volumes'][c], group, cap, sampling, info=stats)
        tables[c] = {'table': table.cpu().numpy(), 'capped': int(stats['capped'])}
    res['thickness'] = tables
    res['thickness_maps'] = maps
    res['thickness_params'] = {'r_cap': float(r_cap), 'cap': int(cap), 'sampling': tuple(int(a) for a in sampling)}
    if out is None:
        return res
    names = thickness_dataset_names(classes, class_names)
    if rank == 0:
        for c in classes:
            out.create_dataset(names[c], shape=tuple(int(s) for s in shape3d), dtype=np.uint16, overwrite=True,
                               chunks=(1, None, None))
    if world > 1:
        torch.distributed.barrier(group=group)
    for c in classes:
        if maps[c].shape[0]:
            out[names[c]].write_slab(z0, maps[c].view(torch.int16).cpu().numpy().view(np.uint16))
    missing = _write_tables(out, group, {c: {names[c] + '_table': tables[c]['table']} for c in classes},
                            {c: tables[c]['table'].shape[0] for c in classes},
                            {'thickness': {'columns': list(COLUMNS), 'r_cap': float(r_cap), 'cap': int(cap),
                                           'sampling': [int(a) for a in sampling],
                                           'map': 'squared radius, diameter = 2 sqrt'}})
    res['thickness_datasets'] = {c: {'map': out[names[c]], 'table': None if c in missing else out[names[c] + '_table']}
                                 for c in classes}
    return res


@torch.no_grad()
def _plane_windowed(engine, dv, axis, n, batch_pixels, render_steps, params, window_slices, mem_budget, info):
    """one plane through windowed.windowed_panoptic_stack: the model forward of _plane_heads is the `fill`"""
    per = slices_per_call(dv, axis, batch_pixels)
    margs = model_args(engine, render_steps)
    shapes = plane_head_shapes(engine, dv, axis, model_classes(engine.model, dv, axis, margs))
    m = int(params['median_kernel_size']) // 2
    budget = mem_budget
    if window_slices == 'auto' and budget is None:
        budget = torch.cuda.mem_get_info(dv.vol.device)[0] - 4 * n * shapes['sem'][1] * shapes['sem'][2]   # less `pan`
    sem_bytes = 4 * int(np.prod(shapes['sem']))
    plan = windowed.plan_windows(n, per, m, window_slices, windowed.bytes_per_slice(shapes), budget, sem_bytes)

    def fill(lo, hi, bufs, at):
        forward_heads(engine.model, margs, dv, axis, lo, hi, per, bufs, at)

    step = {}
    pan = windowed.windowed_panoptic_stack(fill, plan, shapes, device=dv.vol.device, info=step, **params)
    info['windows'][axis] = step['windows']
    info['head_bytes'] = max(info['head_bytes'], step['head_bytes'])
    return pan


def infer_volume(engine, volume, *, norms, labels, axes=('xy', 'xz', 'yz'), merge_iou_thr=0.25, merge_ioa_thr=0.25,
                 min_size=500, min_span=4, pixel_vote_thr=2, cluster_iou_thr=0.75, bypass=False, class_names=None,
                 out=None, batch_pixels=None, render_steps=2, group=None, downsample_f=1, pipeline=None,
                 window_slices=None, mem_budget=None, ground_truth=None, compressor=None, pyramid=None,
                 measure=None, split_objects=None, fill_holes=None, morph=None, separate=None, mesh=None,
                 skeleton=None, contacts=None, thickness=None, shapes=None):
    """3D panoptic inference of a (D, H, W) uint8 volume (numpy array, tensor or DeviceVolume) with a 3d engine.

    axes: ('xy',) = stack mode, ('xy', 'xz', 'yz') = orthoplane mode with consensus (pdl_inference3d.py:92-96).
    labels: all class ids; engine.thing_list says which are instance classes.  out: ZarrV2Group (or anything with the
    same create_dataset) -- one dataset '<class name>_pred' per class, uint32 for thing classes and uint8 for stuff,
    chunks (1, Y, X) (pdl_inference3d.py:225-233); rank 0 creates them, every rank writes its slab.
    downsample_f: the script's -downsample-f (pdl_inference3d.py:50,154,169,178), a power of two: every slice is shrunk
    in-plane by f before the model sees it (DeviceVolume(scale=f)), the semantic head is rendered with log2 f more
    PointRend steps, the instance cells are enlarged by f more, and the labels come out at the full (D, H, W).  Needs
    a Render engine; a DeviceVolume passed in must have been built with scale=f.
    pipeline: a VolumePipeline built for this engine (inference/pipeline.py): the same result through tuned call sites,
    graph replay, heads written in place and two streams; its own batch_pixels sizes the model calls (passing another
    value here as well is an error).  The result gains 'pipeline': what ran.
    batch_pixels: output pixels per model call; None = 32 Mi pixels, or the pipeline's value with pipeline=.
    window_slices: None = the heads of a whole plane are resident before its post-processing starts (4 (C + 3) bytes per
    voxel of the plane); an integer W or 'auto' = the plane streams through windows of W slices
    (inference/windowed.py): W + m slices of heads (m = ks // 2) and the plane's uint32 labels are all that is resident,
    the volumes are the same.  W is rounded down to a multiple of the slices per model call; 'auto' takes the whole
    plane when it fits into mem_budget bytes (None: the free device memory) and the largest window that does otherwise.
    The result gains 'windows': {axis: steps} and 'head_bytes': bytes of head buffers held.  Not with several ranks.
    ground_truth: {class: (D, H, W) integer labels} for any of `labels` (numpy array, tensor, or anything sliceable along
    z such as a zarr array): once the volumes exist every rank scores its z-slab against the same slab of the ground
    truth (evaluation.volume_scores: overlap table on the device, added over the ranks) and the result gains
    'scores': {class: {'IoU', 'F1_50', 'F1_75', 'Precision_50', 'Precision_75', 'Recall_50', 'Recall_75', 'PQ', 'n_gt',
    'n_pred', 'n_matched'}} for thing classes and {'IoU'} for stuff classes -- the numbers scripts/evaluate3d.py:204-218
    prints.  None: no new key, nothing else changes.
    compressor: None = the datasets hold raw chunks; 'zlib' = they are created with {"id": "zlib", "level": 1} and every
    rank's slab of every class is made zlib streams on the device (ZarrV2Array.write_slab_device), so only compressed
    bytes cross to the host and reach the disk, and no CPU compresses; needs out= to be a ZarrV2Group.  The result
    gains 'compressed_bytes': {class: bytes this rank wrote}.  The volumes and what the datasets read back are the same.
    pyramid: None = level 0 only; an integer L (1..8) = L more levels, each the level below pooled by (2, 2, 2); a
    sequence of factor triples of 1s and 2s = one level per triple ((1, 2, 2) for thick serial sections).  A level's
    voxel is the most frequent label of its cell, the largest among equally frequent ones (inference/pyramid.py,
    _hip.pool_labels), computed on the device from the resident slab: uint32 for thing classes, uint8 for stuff.  With
    out=, level l of a class is the dataset '<class name>_pred_s<l>' with the dtype, chunking and compressor of level
    0, and the group's attributes gain one OME-NGFF 0.4 `multiscales` entry per class.  Every rank pools its own
    z-slab, so a slab must be aligned to every level's cumulative z-factor (ValueError otherwise, on every rank,
    before any work: fewer ranks, fewer levels or (1, 2, 2) levels).  The result gains 'pyramid': {class: [the rank's
    slab of level 1, ...]}, 'pyramid_z_ranges': [(z0, z1) of the rank per level], 'pyramid_datasets': {class: [array or
    None, ...]} and, with a compressor, 'pyramid_compressed_bytes': {class: [bytes per level]}.
    measure: None = no table, nothing else changes; True, or a voxel spacing (sz, sy, sx) of three positive numbers = once
    the volumes exist every rank measures its z-slab of every class on the device (_hip.measure_labels; the table is
    defined in include/emp_hip.h, E2) with the end slices of the ranks next to it standing for what lies outside the
    slab, and the tables are merged over the ranks.  The result gains 'objects': {class: (n, 14) int64 numpy table of
    the WHOLE volume, the same on every rank, one row per label ascending: measurements.COLUMNS} -- at most one row
    (label 1) for a stuff class -- and 'object_spacing': the spacing (True: (1, 1, 1)), which measurements.derive
    turns into volumes, centroids, boxes and surface areas.  With out=, rank 0 writes one dataset
    '<class name>_objects' per class (int64, (n, 14), one raw chunk), the group's attributes gain 'objects':
    {'columns', 'spacing'} beside what they hold, and the result gains 'object_datasets': {class: array, or None where
    the store cannot hold the zero-row table of a class without objects}.
    split_objects: None = the volumes as the consensus (or the stack's tracks) painted them, where an instance id need not
    be one piece; 6, 18 or 26 = every thing class's slab is split into its connected components of that connectivity on
    the device (components.split_volume; include/emp_hip.h, E3) before anything else reads it: the largest piece of an
    id keeps the id, every further piece gets a new id above the largest, and every piece on its own must pass
    min_size / min_span or is erased.  Datasets, compressed output, pyramid, scores and measurements see the repaired
    labels; stuff classes stay as they are.  'instances' become the objects that remain and the result gains 'split':
    {class: {'objects_in', 'objects_split', 'pieces_added', 'pieces_removed', 'objects_out'}}, the same on every rank.
    fill_holes: None = the volumes as they are; True = in every thing class's slab every closed cavity -- a 6-connected
    component of background voxels that does not reach the border of the volume -- whose wall carries ONE label is
    painted with that label on the device (holes.fill_volume; include/emp_hip.h, E4), right after split_objects and
    before anything else reads the slab; a positive integer fills only the cavities of at most that many voxels.  A
    cavity walled by two or more labels (a gap between touching objects, the shell around a nested object) is left.
    Datasets, compressed output, pyramid, scores and measurements see the filled labels; stuff classes stay as they
    are and 'instances' do not change.  The result gains 'filled': {class: {'cavities', 'filled', 'voxels_filled',
    'shared', 'too_large'}}, the same on every rank.
    morph: None = the volumes as they are; (op, r) or (op, r, (az, ay, ax)) = one morphological operation on every thing
    class's slab on the device (morphology.morph_volume; include/emp_hip.h, E5) BEFORE split_objects and fill_holes, so
    that an opening cuts a thin bridge and the split then separates and judges the pieces, and a closing's new cavities
    get filled.  op: 'erode' (a voxel keeps its label where every other label, background included, is farther than
    r), 'dilate' (a background voxel takes the nearest label within r, the largest among equally near; labelled voxels
    stay), 'open' (erode, then dilate: every label opened by itself) or 'close' (dilate, then erode, originals kept).
    r: the radius in the units of the sampling (az, ay, ax), integer voxel pitches in 1 .. 16, (1, 1, 1) by default
    ((3, 1, 1) for thick sections): exact Euclidean balls, 1 = the 6-neighbourhood, sqrt(2) the 18- and sqrt(3) the
    26-neighbourhood, up to sqrt(65534).  The volume's faces do not erode.  With several ranks every rank fetches the
    few slices of its neighbours that the ball reaches.  Datasets, compressed output, pyramid, scores and measurements
    see the new labels; stuff classes stay as they are.  After 'erode' and 'open', 'instances' become the labels that
    remain.  The result gains 'morph': {class: {'op', 'r2', 'sampling', 'voxels_removed', 'voxels_added'}}, the same on
    every rank.
    separate: None = the volumes as they are, where two objects that touch carry one id; r, (r, min_core) or (r, min_core,
    (az, ay, ax)) = every thing class's slab goes through separation.separate_volume on the device (include/emp_hip.h,
    E6) AFTER morph and BEFORE split_objects and fill_holes: every label is eroded by the exact Euclidean ball of radius
    r (read as morph reads it, in the units of the sampling), the cores that remain are labelled, and a label with two
    or more cores of at least min_core voxels (default 1) is divided among them -- every voxel goes to the core that
    reaches it first along 6-connected paths inside the object, the later-numbered core among equally near ones.  The
    largest piece keeps the id and every further piece gets a new id above the class's largest; no surface moves, no
    voxel is lost or added, and every other label stays exactly as it is.  A voxel of a divided object that no core
    reaches keeps the id; split_objects, which runs next, judges such crumbs and every new piece by min_size /
    min_span.  With several ranks every rank exchanges one end slice of the growth's state per side and round.
    Datasets, compressed output, pyramid, scores and measurements see the new labels; stuff classes stay as they are.
    'instances' grow by the pieces added and the result gains 'separated': {class: {'r2', 'min_core', 'sampling',
    'objects_in', 'objects_separated', 'pieces_added', 'voxels_moved', 'sweeps'}}, the same on every rank.
    mesh: None = no mesh, no new key, no launch; True, or a non-negative integer n = once the volumes are final (after
    morph, separate, split_objects and fill_holes, where measure runs) every thing class gets one welded, outward-
    oriented quad mesh of its objects' exposed voxel faces, built on the device (meshes.mesh_volume; include/emp_hip.h,
    E7): every rank emits its slab with the end slices of the ranks next to it, and every rank finishes the same whole
    mesh.  n > 0 adds n Taubin smoothing iterations on the device; every object is smoothed by itself, so touching
    objects may drift apart or overlap by a fraction of a voxel.  The result gains 'meshes': {class: {'vertices':
    (nv, 3) in zyx order, int32 lattice corners (True, 0) or float32 (n > 0), 'quads': (nq, 4) int32 vertex indices,
    'objects': (n, 5) int64 rows of label, v_begin, v_end, q_begin, q_end, ascending by label -- the rows of measure's
    table, whose columns 11..13 count the same faces}} as numpy arrays (meshes.triangles, meshes.object_mesh and
    meshes.write_obj read them).  With out=, rank 0 writes '<class name>_mesh_vertices', '<class name>_mesh_quads'
    and '<class name>_mesh_objects', the group's attributes gain 'meshes': {'axes': 'zyx', 'object_columns',
    'iterations'}, and the result gains 'mesh_datasets': {class: {'vertices', 'quads', 'objects'}, or None where the
    store cannot hold the zero-row arrays of a class without objects}.  A volume of more than 2^32 lattice corners
    (about 1624^3), or a mesh of 2^31 vertices or quads, is a ValueError.
    skeleton: None = no skeleton, no new key, no launch; True, r_cap or (r_cap, (az, ay, ax)) (skeletons.check; r_cap,
    default 64, is the largest radius reported, in the units of the sampling) = once the volumes are final, where mesh
    and measure run, every thing class is thinned to the centrelines of its objects on the device -- topological
    thinning that keeps 1-D isthmuses, by sub-fields (skeletons.skeleton_volume; include/emp_hip.h, E8) -- with the
    ranks in lock-step, one end slice of state exchanged per side and pass.  An object with a cavity keeps a closed
    shell around it, so fill_holes= belongs in front.  The result gains 'skeletons': {class: {'vertices': (nv, 3) int32
    zyx, 'radius2': (nv,) int32 capped squared distance to the object's surface in the final volume, 'degree': (nv,)
    int32, 'edges': (ne, 2) int32, 'objects': (n, 8) int64 rows of label, v_begin, v_end, e_begin, e_end, isolated,
    ends, junctions}} as numpy arrays (skeletons.derive, skeletons.object_skeleton and skeletons.write_obj read them).
    With out=, rank 0 writes '<class name>_skeleton_vertices', '_radius2', '_degree', '_edges' and '_objects', the
    group's attributes gain 'skeletons': {'axes': 'zyx', 'object_columns', 'r_cap', 'sampling'}, and the result gains
    'skeleton_datasets' as 'mesh_datasets'.  A volume above 2^32 voxels is a ValueError.
    contacts: None = no table, no new key, no launch; r, (r, (az, ay, ax)) or (r, (az, ay, ax), pairs) (contacts.check; r is
    the radius in the units of the sampling, integer voxel pitches in 1 .. 16, (1, 1, 1) by default; the ball may reach
    4 voxels along the finest axis) = once the volumes are final, where measure, mesh and skeleton run, every pair of
    classes (ca, cb) gets the table of the contact sites between the objects of ca and those of cb, read on the device
    (_hip.label_contacts; include/emp_hip.h, E9): a voxel of object a is a contact voxel of (a, b) when a voxel of b lies
    within r of it, every partner within r counting, not only the nearest.  pairs: a list of (class_a, class_b) from
    `labels` (an unknown class is a ValueError before any work); by default (c, c) for every thing class -- the
    instances of one class among each other -- and (c1, c2) for every ordered pair of distinct classes, stuff classes
    included (a thing class against a semantic class is the main use).  The ranks walk the pairs in the same order;
    every rank reads its z-slab of ca against its slab of cb with the few slices of cb that the ball reaches in the
    ranks next to it, and the tables are merged over the ranks.  The result gains 'contacts': {(ca, cb): (n, 10) int64
    numpy table of the WHOLE volume, the same on every rank, one row per ordered pair of labels (a, b) ascending:
    contacts.COLUMNS -- a, b, voxels, min_d2, sum_z, sum_y, sum_x, faces_z, faces_y, faces_x} and 'contact_params':
    {'r2', 'sampling'}, which contacts.derive turns into distances, centroids and shared areas.  With out=, rank 0 writes
    one dataset '<class a name>_<class b name>_contacts' per pair (int64, (n, 10), one raw chunk), the group's
    attributes gain 'contacts': {'columns', 'r2', 'sampling', 'pairs'}, and the result gains 'contact_datasets': {(ca,
    cb): array, or None where the store cannot hold a zero-row table}.
    thickness: None = no map, no new key, no launch; True (r_cap = 32), r_cap or (r_cap, (az, ay, ax)) (thickness.check;
    r_cap is the largest radius reported, >= 1 in the units of the integer sampling, cap = floor(r_cap^2) <= 65535) = once
    the volumes are final, where measure, mesh, skeleton and contacts run, every thing class gets its local thickness,
    computed on the device (_hip.label_thickness; include/emp_hip.h, E10): T2(p) is the squared radius, capped at cap,
    of the largest ball that fits the object and covers p -- not the one centred on p -- so the diameter at p is 2
    sqrt(T2(p)), with the voxel-centre bias of the edt (a line one voxel wide reads 2).  Every rank fetches 2
    (isqrt(cap - 1) // az) slices per side from the ranks next to it, so the map is that of the undivided volume.  The
    result gains 'thickness': {class: {'table': (m, 3) int64 numpy of the WHOLE volume, the same on every rank, rows
    (label, t2, voxels) ascending -- thickness.COLUMNS; thickness.derive and thickness.histogram read it --, 'capped':
    voxels of the whole volume whose distance reached the cap; 0 means the map is the uncapped one}},
    'thickness_maps': {class: the rank's (z1 - z0, Y, X) uint16 device slab of T2} and 'thickness_params': {'r_cap',
    'cap', 'sampling'}.  With out=, rank 0 creates one dataset '<class name>_thickness' per class (uint16, the labels'
    shape, chunks (1, Y, X)) and every rank writes its slab of it -- always raw chunks, whatever `compressor` says:
    write_slab_device takes 1- and 4-byte items only and a 2-byte device deflate is not built --, rank 0 writes the table
    as '<class name>_thickness_table' (int64, (m, 3), one raw chunk), the group's attributes gain 'thickness':
    {'columns', 'r_cap', 'cap', 'sampling', 'map': 'squared radius, diameter = 2 sqrt'}, and the result gains
    'thickness_datasets': {class: {'map': array, 'table': array, or None where the store cannot hold a zero-row table}}.
    shapes: None = no table, no new key, no launch; True, or a voxel spacing (sz, sy, sx) of three positive numbers = once
    the volumes are final, where measure runs, every rank takes the shape sums of its z-slab of every class on the device
    (_hip.shape_labels; include/emp_hip.h, E11) with the end slices of the ranks next to it, and the tables are merged
    over the ranks.  The result gains 'shapes': {class: (n, 26) int64 numpy table of the WHOLE volume, the same on every
    rank, one row per label ascending: shapes.COLUMNS} -- at most one row (label 1) for a stuff class -- and
    'shape_spacing': the spacing (True: (1, 1, 1)), which shapes.derive takes to turn the sums into a Crofton surface
    area, sphericity, the Euler number and the inertia ellipsoid.  The number of tunnels it reports holds for objects that
    are one 26-connected piece without cavities: ask for split_objects=26 and fill_holes=True.  With out=, rank 0 writes
    one dataset '<class name>_shapes' per class (int64, (n, 26), one raw chunk), the group's attributes gain 'shapes':
    {'columns', 'spacing'}, and the result gains 'shape_datasets': {class: array, or None where the store cannot hold a
    zero-row table}.
    Returns {'volumes': {class: the rank's (z1 - z0, Y, X) device slab}, 'z_range': (z0, z1),
             'instances': {class: number of instances kept}, 'datasets': {class: array or None}}."""
    rank, world = sharded._world(group)
    window_slices = _check_windows(window_slices, mem_budget, pipeline, world)
    _check_compressor(compressor, out)
    spacing = _check_measure(measure)
    connectivity = _check_split(split_objects)
    fill_wanted, fill_cap = _check_fill(fill_holes)
    morph = _check_morph(morph)
    separate = _check_separate(separate)
    mesh_iterations = _check_mesh(mesh)
    skeleton = _check_skeleton(skeleton)
    thickness = _check_thickness(thickness)
    shape_spacing = _check_shapes(shapes)
    levels = None
    if pyramid is not None:
        levels = pyramid_levels(pyramid, tuple(volume.shape), world)[rank]
    labels = list(labels)
    thing_list = list(engine.thing_list)
    contacts = _check_contacts(contacts, labels, thing_list)
    div = engine.label_divisor
    factor = int(getattr(engine, 'padding_factor', 16))
    f = downsample_f
    if isinstance(f, bool) or not isinstance(f, (int, np.integer)) or f < 1 or f & (f - 1):
        raise ValueError(f"downsample_f must be a power of two >= 1, got {downsample_f!r}")
    f = int(f)
    if f > 1 and not hasattr(engine, 'coarse_boundaries'):
        raise ValueError("downsample_f > 1 needs a Render engine (PanopticDeepLabRenderEngine3d: model(x, render_steps, "
                         "interpolate_ins) and `upsampling`); the plain engines cannot render the labels back to full "
                         f"resolution, got {type(engine).__name__}")
    if pipeline is not None:
        pipeline.check(engine, axes, batch_pixels)
    elif batch_pixels is None:
        batch_pixels = 32 * 1024 * 1024
    if isinstance(volume, DeviceVolume):
        dv = volume
        if dv.scale != f:
            raise ValueError(f"the DeviceVolume was built with scale={dv.scale}, downsample_f={f}")
    else:
        dv = DeviceVolume(volume, norms['mean'], norms['std'], factor, next(engine.model.parameters()).device, scale=f)
    steps = render_steps + f.bit_length() - 1
    shape3d = dv.shape
    _check_ground_truth(ground_truth, labels, shape3d)
    params = dict(thing_list=thing_list, label_divisor=div, stuff_area=engine.stuff_area, void_label=engine.void_label,
                  nms_threshold=engine.nms_threshold, nms_kernel=engine.nms_kernel,
                  confidence_thr=engine.confidence_thr, median_kernel_size=getattr(engine, 'ks', 1),
                  coarse_boundaries=bool(getattr(engine, 'coarse_boundaries', False)),
                  max_centers=getattr(engine, 'max_centers', None), upsampling=f)
    if len(axes) == 1:
        assert axes[0] == 'xy', "stack mode runs along z (axes=('xy',))"

    def track(pan, axis, base):
        h, w = dv.plane_shape(axis)
        return sharded.track_plane(pan[:, :h, :w].contiguous(), axis, shape3d, labels, thing_list, div, merge_iou_thr,
                                   merge_ioa_thr, inst_base=base, group=group)

    def finish(planes):
        if len(axes) == 1:
            # stack mode: the plane's own trackers are the result (pdl_inference3d.py:222-223)
            return sharded.plane_volume(planes['xy'], labels, thing_list, min_size, min_span, group=group)
        cons, vols, zs = sharded.consensus_volume(planes, shape3d, labels, thing_list, pixel_vote_thr, cluster_iou_thr,
                                                  bypass, min_size, min_span, group=group)
        return vols, zs, {c: int(cons[c].alive.sum()) for c in labels}

    morphed = {}
    finish = _morphing(finish, morph, thing_list, shape3d, group, connectivity is None, morphed)
    separated = {}
    finish = _separating(finish, separate, thing_list, shape3d, group, connectivity is None, separated)
    split = {}
    finish = _splitting(finish, connectivity, thing_list, min_size, min_span, group, split)
    filled = {}
    finish = _filling(finish, fill_wanted, fill_cap, thing_list, shape3d, group, filled)

    def done(res):
        if morph is not None:
            res['morph'] = morphed
        if separate is not None:
            res['separated'] = separated
        if connectivity is not None:
            res['split'] = split
        if fill_wanted:
            res['filled'] = filled
        res = _measured(_scored(res, ground_truth, thing_list, group), spacing, labels, class_names, out, group)
        res = _meshed(res, mesh_iterations, thing_list, shape3d, class_names, out, group)
        res = _skeletonized(res, skeleton, thing_list, shape3d, class_names, out, group)
        res = _contacted(res, contacts, class_names, out, group)
        res = _thickened(res, thickness, thing_list, shape3d, class_names, out, group)
        return _shaped(res, shape_spacing, labels, class_names, out, group)

    if pipeline is not None:
        res = pipeline.run(dv, axes=axes, labels=labels, thing_list=thing_list, params=params, steps=steps, group=group,
                           track=track, finish=finish, class_names=class_names, out=out, window_slices=window_slices,
                           compressor=compressor, levels=levels)
        return done(res)
    planes, base = {}, 0
    windows = {'windows': {}, 'head_bytes': 0}
    for axis in axes:
        n = dv.n_slices(axis)
        if window_slices is not None:
            pan = _plane_windowed(engine, dv, axis, n, batch_pixels, steps, params, window_slices, mem_budget, windows)
        else:
            b = sharded.shard_bounds(n, world)
            lo, hi = int(b[rank]), int(b[rank + 1])
            heads = _plane_heads(engine, dv, axis, lo, hi, batch_pixels, steps)
            pan = sharded.sharded_panoptic_stack(heads['sem'], heads['ctr_hmp'], heads['offsets'], group=group, **params)
            del heads
        planes[axis] = track(pan, axis, base)
        base += planes[axis].n_inst
        del pan
    vols, (z0, z1), counts = finish(planes)
    datasets = open_datasets(out, labels, thing_list, class_names, shape3d, rank, world, group, compressor, levels or ())
    compressed = None if compressor is None else {}
    if out is not None:
        for c in labels:
            if compressor is None:
                datasets[c].write_slab(z0, host_slab(vols[c], c in thing_list))
            else:
                compressed[c] = datasets[c].write_slab_device(z0, vols[c].contiguous())[1]
    extra = None
    if levels is not None:
        extra = {'pyramid': {c: pyr.build(vols[c].contiguous(), [lv['pool'] for lv in levels]) for c in labels},
                 'pyramid_z_ranges': [lv['z_range'] for lv in levels],
                 'pyramid_datasets': open_level_datasets(out, labels, class_names, levels)}
        if compressor is not None:
            extra['pyramid_compressed_bytes'] = {c: [] for c in labels}
        for c in labels if out is not None else ():
            for lv, slab, ds in zip(levels, extra['pyramid'][c], extra['pyramid_datasets'][c]):
                if compressor is None:
                    ds.write_slab(lv['z_range'][0], host_slab(slab, c in thing_list))
                else:
                    extra['pyramid_compressed_bytes'][c].append(ds.write_slab_device(lv['z_range'][0], slab)[1])
        if out is not None and rank == 0:
            write_multiscales(out, labels, class_names, levels)
    return done(result(vols, (z0, z1), counts, datasets, compressed=compressed, pyramid=extra,
                       **(windows if window_slices is not None else {})))
