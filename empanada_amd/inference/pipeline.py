"""The fast path of `infer_volume`: what outlives one volume -- the tuned call sites, the captured forward graphs, the
two streams, the plane buffers, the pinned write buffers -- held by one `VolumePipeline` per engine and reused.

    pipe = VolumePipeline(engine, tune=True, graph=True, overlap='auto', batch_pixels=32 << 20)
    res = infer_volume(engine, volume, norms=..., labels=..., out=..., pipeline=pipe)       # every other argument as usual

What it changes against the plain call (driver._plane_heads + the serial plane loop), never the result:
  * tune: every FusedConvBNAct site picks its fastest implementation once (models.tune_fused_convs), on the first plane
    shape seen and a quarter of a call's slices; with several ranks only rank 0 searches and the others adopt its choice;
  * graph: the forward of a batch is captured once per input shape (models.graphed.GraphedForward) and replayed; the
    slice feeder writes into the graph's static input; a model that is not fp32 is never captured;
  * heads in place: one resident buffer per head and plane; every batch writes its slices [s, e) exactly once -- the x4
    up-sampling of a DeepLab head is deferred out of the model (`defer_up4`) and finished, fused with logits_to_prob for
    the semantic head, by emp_upsample_bilinear_prob straight into the buffer;
  * overlap: forwards on one stream, everything downstream of a plane's forward on another, two sets of plane buffers;
    'auto' falls back to one set and serial planes when two planes' heads do not fit;
  * writing: the labelled slab goes to the zarr array through SlabWriter (pinned buffer, asynchronous copy, chunk files
    written by a pool while the next class is copied); with infer_volume(..., compressor='zlib') the slab is made zlib
    streams on the post stream first (ZarrV2Array.write_slab_device) and only those bytes are copied and written; with
    infer_volume(..., pyramid=) every class's level slabs are pooled on the post stream (inference/pyramid.py) and go
    the same way, each level through a writer and a pinned buffer of its own, keyed (class, level).
With infer_volume(..., window_slices=) the planes stream through windows of slices (inference/windowed.py) and the two
sets of buffers alternate per step of a plane instead of per plane (_run_windowed).
What a plane is -- slices per model call, the model's arguments, head shapes, the loop that writes every batch's heads,
the datasets -- is driver.py's and the plain call's too; run() holds what surrounds the two walks.
"""
import contextlib
import json
import os

import numpy as np
import torch

from ..zarr_utils import SlabWriter, ZarrV2Array
from . import driver, pyramid, sharded, windowed

__all__ = ['VolumePipeline']


def _stacked(n, shapes):
    """per-slice head shapes -> the shapes of n slices"""
    return {k: (n,) + tuple(v) for k, v in shapes.items()}


def _sites(model):
    from ..models.panoptic_deeplab import FusedConvBNAct
    return [(n, m) for n, m in model.named_modules() if isinstance(m, FusedConvBNAct)]


class VolumePipeline:
    """State of the fast path for ONE engine; pass it to `infer_volume(..., pipeline=)`.

    tune: False = leave every site's impl as it is; True = tune_fused_convs once; a collection of implementation names =
          the same with `allow=`; a path = load {module name: impl} from that JSON file (what save_tune and
          `bench.py --save-tune` write).
    graph: replay the forward as a HIP graph (fp32 models only; anything else runs eagerly).
    overlap: True / False / 'auto' (two sets of plane buffers if they fit into `mem_budget` bytes, or into the free
          device memory when mem_budget is None).
    batch_pixels: output pixels per model call, as infer_volume's own argument (which must then be left out or equal).
    model_args: extra positional arguments of the model's forward; None = what the engine's kind implies
          ((render_steps, interpolate_ins) for the Render engines)."""

    def __init__(self, engine, tune=True, graph=True, overlap='auto', batch_pixels=32 << 20, model_args=None,
                 mem_budget=None):
        if overlap not in (True, False, 'auto'):
            raise ValueError(f"overlap must be True, False or 'auto', got {overlap!r}")
        if isinstance(batch_pixels, bool) or int(batch_pixels) < 1:
            raise ValueError(f"batch_pixels must be a positive number of pixels, got {batch_pixels!r}")
        if isinstance(tune, (str, os.PathLike)):
            if not os.path.isfile(tune):
                raise ValueError(f"tune={os.fspath(tune)!r}: no such file of per-site choices")
        elif not isinstance(tune, bool):
            tune = tuple(tune)
            if not all(isinstance(t, str) for t in tune):
                raise ValueError(f"tune must be a bool, a path or a collection of implementation names, got {tune!r}")
        self.engine = engine
        self.model = engine.model
        self.tune = tune
        self.graph = bool(graph)
        self.overlap = overlap
        self.batch_pixels = int(batch_pixels)
        self.model_args = None if model_args is None else tuple(model_args)
        self.mem_budget = None if mem_budget is None else int(mem_budget)
        self._tuned = tune is False
        self._graphed = None
        self._streams = None
        self._store = [None, None]                    # flat fp32 storage of the two sets of plane buffers
        self._writers = {}
        self._zpool = None                            # compressor='zlib': the writer threads ...
        self._zbufs = {}                              # ... and one pinned buffer of compressed bytes per class (and level)

    # ------------------------------------------------------------------------------------------ checks, before GPU work
    def _param(self):
        return next(self.model.parameters())

    def check(self, engine, axes, batch_pixels=None):
        """ValueError for what this pipeline cannot serve; nothing here touches the GPU"""
        if engine is not self.engine:
            raise ValueError("pipeline= was built for another engine: a VolumePipeline holds the tuned sites and the "
                             "captured graphs of ONE engine's model")
        p = self._param()
        if p.device.type != 'cuda':
            raise ValueError(f"pipeline= needs the engine's model on the GPU (it is on {p.device}): graphs, streams and "
                             "the fused head kernel have no host form")
        if batch_pixels is not None and int(batch_pixels) != self.batch_pixels:
            raise ValueError(f"batch_pixels={batch_pixels} given together with a pipeline built for batch_pixels="
                             f"{self.batch_pixels}: with pipeline= the pipeline's own value sizes the model calls")
        if self.tune is not False and not self._tuned and p.dtype != torch.float32:
            raise ValueError(f"tune={self.tune!r} with a {p.dtype} model: only the fp32 call sites have implementations "
                             "to choose from")
        for axis in axes:
            if axis not in ('xy', 'xz', 'yz'):
                raise ValueError(f"unknown plane {axis!r}")

    # ------------------------------------------------------------------------------------------ tuning
    def tuned_counts(self):
        counts = {}
        for _, m in _sites(self.model):
            counts[m.impl] = counts.get(m.impl, 0) + 1
        return counts

    def save_tune(self, path):
        """the per-site choices as {module name: impl} (the format `tune=<path>` and bench.py --load-tune read)"""
        with open(path, 'w') as fh:
            json.dump({n: m.impl for n, m in _sites(self.model)}, fh, indent=1)

    @torch.no_grad()
    def _tune_once(self, shape, margs, group):
        """shape: (slices per call, hp, wp) of the first plane.  Only rank 0 searches: a slice's logits must not depend
        on the rank that computed it"""
        if self._tuned:
            return
        rank, world = sharded._world(group)
        sites = _sites(self.model)
        if rank == 0:
            if isinstance(self.tune, (str, os.PathLike)):
                with open(self.tune) as fh:
                    choice = json.load(fh)
                for n, m in sites:
                    m.impl = choice.get(n, m.impl)
            else:
                from ..models import tune_fused_convs
                per, hp, wp = shape
                x = torch.rand((max(1, per // 4), 1, hp, wp), device=self._param().device)
                tune_fused_convs(self.model, x.contiguous(memory_format=torch.channels_last),
                                 allow=None if self.tune is True else self.tune, model_args=margs)
        if world > 1:
            import torch.distributed as dist
            box = [{n: m.impl for n, m in sites} if rank == 0 else None]
            dist.broadcast_object_list(box, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
            for n, m in sites:
                m.impl = box[0].get(n, m.impl)
        self._tuned = True

    # ------------------------------------------------------------------------------------------ buffers
    @staticmethod
    def _elems(shapes):
        return sum(-(-int(np.prod(s)) // 64) * 64 for s in shapes.values())

    def _reserve(self, k, need, device):
        """set k's flat allocation, grown on the caller's stream before any work of this volume is queued (the last
        volume's work on both streams is ordered before it: run() ends with the caller's stream waiting for them)"""
        if self._store[k] is None or self._store[k].numel() < need or self._store[k].device != device:
            self._store[k] = None
            self._store[k] = torch.empty((need,), dtype=torch.float32, device=device)

    def _views(self, k, shapes):
        """the three head buffers of a plane: views of set k's allocation"""
        out, at = {}, 0
        for name, s in shapes.items():
            n = int(np.prod(s))
            out[name] = self._store[k][at:at + n].view(s)
            at += -(-n // 64) * 64
        return out

    def _held(self):
        """bytes of the flat allocations"""
        return 4 * sum(s.numel() for s in self._store if s is not None)

    def _available(self, dev):
        """bytes a planner without a mem_budget may use: free, cached by the allocator, held by this pipeline already"""
        free, _ = torch.cuda.mem_get_info(dev)
        return free + torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev) + self._held()

    def _fits(self, plane_elems, dv, out_bytes):
        """overlap='auto': two planes' heads + the resident volume + the labelled slabs against the budget"""
        two = 4 * sum(sorted(plane_elems)[-2:])
        if self.mem_budget is not None:
            return two + dv.vol.numel() + out_bytes <= self.mem_budget
        return two + out_bytes <= self._available(dv.vol.device)   # the volume is resident already: it is not in `free`

    # ------------------------------------------------------------------------------------------ the forward
    def _margs(self, steps):
        """extra positional arguments of the model's forward"""
        return self.model_args if self.model_args is not None else driver.model_args(self.engine, steps)

    def _model(self):
        """(what a forward calls, whether it replays graphs): a model that is not fp32 is never captured"""
        graph = self.graph and self._param().dtype == torch.float32
        if graph and self._graphed is None:
            from ..models.graphed import GraphedForward
            # up to two batch sizes per plane and three planes per volume shape: room for a few shapes, so that
            # alternating between volumes does not evict and re-capture; res['pipeline']['captures'] counts what a call cost
            self._graphed = GraphedForward(self.model, warmup=1, max_graphs=24, clone_outputs=False)
        return (self._graphed if graph else self.model), graph

    @contextlib.contextmanager
    def _deferring(self):
        """while the pipeline runs, the x4 up-sampling of the heads leaves the model (driver.write_heads finishes it): only
        on the fp32 GPU path of a model that offers it"""
        defer = (self._param().dtype == torch.float32 and hasattr(self.model, 'defer_up4')
                 and bool(getattr(self.model, 'hip_ops', False)))
        try:
            if defer:
                self.model.defer_up4 = True
            yield
        finally:
            if defer:
                self.model.defer_up4 = False

    def forwards_only(self, dv, axes=('xy', 'xz', 'yz'), render_steps=2):
        """For measurements: the forwards of all planes exactly as run() queues them (same arguments, batches, graph
        replay, heads written in place into set 0), without any post-processing; blocks until they are done.  Call it
        after a run() on the same volume, so that tuning and captures are out of the way."""
        margs = self._margs(render_steps + dv.scale.bit_length() - 1)
        model, _ = self._model()
        classes = driver.model_classes(self.model, dv, axes[0], margs)
        with self._deferring():
            for axis in axes:
                n = dv.n_slices(axis)
                shapes = _stacked(n, driver.plane_head_shapes(self.engine, dv, axis, classes))
                self._reserve(0, self._elems(shapes), dv.vol.device)
                driver.forward_heads(model, margs, dv, axis, 0, n, driver.slices_per_call(dv, axis, self.batch_pixels),
                                     self._views(0, shapes))
        torch.cuda.synchronize(dv.vol.device)

    # ------------------------------------------------------------------------------------------ the volume
    def run(self, dv, *, axes, labels, thing_list, params, steps, group, track, finish, class_names, out,
            window_slices=None, compressor=None, levels=None):
        """Called by infer_volume after its own argument checks.  track(pan, axis, base) and finish(planes) are the
        driver's own plane and volume steps, so both paths share them.  The loops over planes (_run_planes) or over the
        steps of every plane (_run_windowed, window_slices=) plan and allocate first and hand back their `walk`; all
        around it is here: streams, the forward to call, the waits on entry and exit, the volume step, writing, the
        result."""
        dev = dv.vol.device
        rank, world = sharded._world(group)
        margs = self._margs(steps)
        plan = []                                         # (axis, the rank's slices [lo, hi), slices per model call)
        for axis in axes:
            b = sharded.shard_bounds(dv.n_slices(axis), world)
            plan.append((axis, int(b[rank]), int(b[rank + 1]), driver.slices_per_call(dv, axis, self.batch_pixels)))
        self._tune_once((plan[0][3],) + tuple(dv.padded_shape(axes[0])), margs, group)
        classes = driver.model_classes(self.model, dv, axes[0], margs)
        shapes = [driver.plane_head_shapes(self.engine, dv, axis, classes) for axis in axes]
        if window_slices is None:
            out_bytes = int(np.prod(dv.shape)) // world * sum(4 if c in thing_list else 1 for c in labels)
            walk, overlap = self._run_planes(dv, plan, shapes, margs, params, group, track, out_bytes)
        else:
            walk, overlap = self._run_windowed(dv, plan, shapes, margs, params, track, window_slices)
        if self._streams is None or self._streams[0].device != dev:
            self._streams = (torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev))
        fwd, post = self._streams
        model, graph = self._model()
        captured = self._graphed.captures if graph else 0

        cur = torch.cuda.current_stream(dev)
        fwd.wait_stream(cur)                              # the volume's upload, whatever the caller queued before
        post.wait_stream(cur)
        with self._deferring(), torch.cuda.stream(post):
            planes, windows, hist_bytes = walk(model, fwd, post)
            vols, (z0, z1), counts = finish(planes)
            slabs = None                                  # pyramid=: every class's level slabs, pooled on the post stream
            if levels is not None:
                slabs = {c: pyramid.build(vols[c].contiguous(), [lv['pool'] for lv in levels]) for c in labels}
            datasets, compressed, extra = self._write(out, vols, z0, labels, thing_list, class_names, dv.shape, rank,
                                                      world, group, post, compressor, levels, slabs)
        cur.wait_stream(post)
        cur.wait_stream(fwd)
        for v in list(vols.values()) + [s for lst in (slabs or {}).values() for s in lst]:
            v.record_stream(cur)                          # allocated on the post stream, handed to the caller's
        head_bytes = self._held() + hist_bytes
        pipe = {'tuned': self.tuned_counts(), 'graph': bool(graph), 'overlap': bool(overlap), 'head_bytes': int(head_bytes)}
        if windows is not None:
            pipe['windows'] = windows
        pipe['captures'] = (self._graphed.captures - captured) if graph else 0
        return driver.result(vols, (z0, z1), counts, datasets, windows, head_bytes, pipe, compressed, extra)

    def _run_planes(self, dv, plan, shapes, margs, params, group, track, out_bytes):
        """Whole planes: the two sets of head buffers alternate per plane, the forward of plane i + 2 is queued as soon as
        plane i's heads have been read.  Returns (walk, overlap); walk(model, fwd, post) runs on the post stream and
        returns (planes, None, 0)."""
        shapes = [_stacked(hi - lo, sh) for (_, lo, hi, _), sh in zip(plan, shapes)]
        elems = [self._elems(s) for s in shapes]
        overlap = self.overlap
        if overlap == 'auto':
            overlap = self._fits(elems, dv, out_bytes)
        overlap = bool(overlap) and len(plan) > 1
        nsets = 2 if overlap else 1
        if not overlap:
            self._store[1] = None
        for k in range(nsets):
            self._reserve(k, max(elems[k::nsets]), dv.vol.device)

        def walk(model, fwd, post):
            bufs = [None] * len(plan)
            done = [torch.cuda.Event() for _ in plan]     # forward of plane i complete
            free = [torch.cuda.Event() for _ in plan]     # post-processing of plane i has read its heads

            def launch(i):
                axis, lo, hi, per = plan[i]
                with torch.cuda.stream(fwd):
                    if i >= nsets:
                        fwd.wait_event(free[i - nsets])   # this set's buffers are still being read until then
                    bufs[i] = self._views(i % nsets, shapes[i])
                    driver.forward_heads(model, margs, dv, axis, lo, hi, per, bufs[i])
                    done[i].record(fwd)

            planes, base = {}, 0
            for i in range(min(nsets, len(plan))):
                launch(i)
            for i, (axis, _, _, _) in enumerate(plan):
                if bufs[i] is None:
                    launch(i)
                post.wait_event(done[i])
                h = bufs[i]
                pan = sharded.sharded_panoptic_stack(h['sem'], h['ctr_hmp'], h['offsets'], group=group, **params)
                free[i].record(post)
                if overlap and i + nsets < len(plan):
                    launch(i + nsets)                     # queued behind `free`, ahead of this plane's host work
                planes[axis] = track(pan, axis, base)
                base += planes[axis].n_inst
                del pan
            return planes, None, 0
        return walk, overlap

    def _run_windowed(self, dv, plan, shapes, margs, params, track, window_slices):
        """Every plane streamed through windows of slices (inference/windowed.py; one rank).  The two sets of head
        buffers alternate per STEP instead of per plane: the forward of step k + 1 runs on the forward stream while the
        post stream labels step k; with overlap off, one set and strict alternation.  The carry copy and the median
        are ordinary launches on the two streams, outside the captured forward, under the same events that order the
        sets.  'auto' plans with the pipeline's mem_budget (None: the free device memory), halved when two sets are
        held.  Returns (walk, overlap); walk(model, fwd, post) returns (planes, {axis: steps}, bytes of history)."""
        dev = dv.vol.device
        ks = int(params['median_kernel_size'])
        budget = self.mem_budget
        if budget is None:                                # less the largest plane's labels
            budget = max(0, self._available(dev) - 4 * max(n * sh['sem'][1] * sh['sem'][2]
                                                           for (_, _, n, _), sh in zip(plan, shapes)))
        nsets = 1 if self.overlap is False else 2
        while True:
            chunks = [windowed.plan_windows(n, per, ks // 2, window_slices, windowed.bytes_per_slice(sh), budget // nsets,
                                            4 * int(np.prod(sh['sem']))) for (_, _, n, per), sh in zip(plan, shapes)]
            lay = [windowed.plane_layout(c, ks) for c in chunks]
            elems = [self._elems(_stacked(cap, sh)) for (_, _, cap), sh in zip(lay, shapes)]
            if nsets == 1 or self.overlap is True or window_slices == 'auto' or 8 * max(elems) <= budget:
                break
            nsets = 1                                     # overlap='auto' and two sets of these windows do not fit
        overlap = nsets == 2
        if any(borrow for _, borrow, _ in lay):
            nsets = 2                                     # windows shorter than the filter borrow their halo from a second set
        if nsets == 1:
            self._store[1] = None
        for k in range(nsets):
            self._reserve(k, max(elems), dev)

        def walk(model, fwd, post):
            last_read = {}                                # set -> event: the last post-processing that read it
            planes, base, steps, hist_bytes = {}, 0, {}, 0
            for (axis, _, _, per), sh, c in zip(plan, shapes, chunks):
                def fill(lo, hi, bufs, at, axis=axis, per=per):
                    driver.forward_heads(model, margs, dv, axis, lo, hi, per, bufs, at)

                P = windowed.WindowedPlane(fill, c, sh, device=dev, sets=nsets,
                                           alloc=lambda i, shp: self._views(i, shp), **params)
                K = len(P.steps)
                done = [torch.cuda.Event() for _ in range(K)]
                ahead = 1 if (overlap and not P.borrow) else 0
                f = 0
                for k in range(K):
                    while f <= min(K - 1, P.needs(k) + ahead):
                        with torch.cuda.stream(fwd):
                            if f % len(P.sets) in last_read:
                                fwd.wait_event(last_read[f % len(P.sets)])
                            P.forward(f)
                            done[f].record(fwd)
                        f += 1
                    post.wait_event(done[P.needs(k)])
                    P.post(k)
                    ev = torch.cuda.Event()
                    ev.record(post)
                    last_read[k % len(P.sets)] = ev
                    if P.borrow:
                        last_read[(k + 1) % len(P.sets)] = ev
                steps[axis] = K
                hist_bytes = max(hist_bytes, 0 if P.hist is None else P.hist.numel() * 4)
                planes[axis] = track(P.pan, axis, base)
                base += planes[axis].n_inst
                del P
            return planes, steps, hist_bytes
        return walk, overlap

    # ------------------------------------------------------------------------------------------ writing
    def _writer(self, c, array, z0, shape, dtype):
        """one SlabWriter (pool + pinned buffer) per key c -- a class, or (class, level) for a pyramid's levels -- and slab
        shape, kept across volumes: pinning is slow"""
        key = (c, tuple(shape), dtype)
        w = self._writers.get(key)
        if w is None:
            for k in [k for k in self._writers if k[0] == c]:
                self._writers.pop(k).close()
            w = self._writers[key] = SlabWriter(array, z0, shape, dtype, buffers=1)
        w.retarget(array, z0)
        return w

    def _pinned(self, c, nbytes):
        """the pinned buffer for compressed bytes of key c (a class, or (class, level)): sized by what a slab actually
        took, and only ever grown"""
        buf = self._zbufs.get(c)
        if buf is None or buf.numel() < nbytes:
            buf = self._zbufs[c] = torch.empty((max(nbytes, 1),), dtype=torch.uint8).pin_memory()
        return buf

    @staticmethod
    def _jobs(datasets, vols, z0, labels, levels, slabs, level_sets):
        """what a volume writes, as (key, class, array, first slice, slab): level 0 of every class under the class itself
        as key, level l of a pyramid under (class, l) -- the keys of the writers and of the pinned buffers, so that the
        levels of one class, whose slab shapes differ, do not evict one another"""
        jobs = [(c, c, datasets[c], z0, vols[c]) for c in labels]
        for c in labels if levels is not None else ():
            for l, (lv, slab, ds) in enumerate(zip(levels, slabs[c], level_sets[c]), start=1):
                jobs.append(((c, l), c, ds, lv['z_range'][0], slab))
        return jobs

    def _write_compressed(self, jobs):
        """compressor='zlib': every slab is encoded on the post stream (the current one), its compressed bytes are copied
        into its key's pinned buffer, and the chunk files are written by the pool while the next slab is encoded.
        Returns {key: bytes written}"""
        if self._zpool is None:
            from concurrent.futures import ThreadPoolExecutor
            self._zpool = ThreadPoolExecutor(max_workers=4)
        pending, compressed = [], {}
        for key, _, arr, zs, slab in jobs:
            futures, compressed[key] = arr.write_slab_device(zs, slab.contiguous(), self._zpool,
                                                             host=lambda n, key=key: self._pinned(key, n))
            pending += futures
        for f in pending:
            f.result()
        return compressed

    def _write(self, out, vols, z0, labels, thing_list, class_names, shape3d, rank, world, group, post, compressor=None,
               levels=None, slabs=None):
        """the datasets, {class: compressed bytes} or None, and the result keys of a pyramid (levels: the rank's plan,
        slabs: {class: its level slabs}) or None"""
        datasets = driver.open_datasets(out, labels, thing_list, class_names, shape3d, rank, world, group, compressor,
                                        levels or ())
        extra = level_sets = None
        if levels is not None:
            level_sets = driver.open_level_datasets(out, labels, class_names, levels)
            extra = {'pyramid': slabs, 'pyramid_z_ranges': [lv['z_range'] for lv in levels],
                     'pyramid_datasets': level_sets}
        jobs = self._jobs(datasets, vols, z0, labels, levels, slabs, level_sets) if out is not None else []
        compressed = None
        if compressor is not None:
            nbytes = self._write_compressed(jobs)
            compressed = {c: nbytes[c] for c in labels}
            if levels is not None:
                extra['pyramid_compressed_bytes'] = {c: [nbytes[(c, l)] for l in range(1, len(levels) + 1)]
                                                     for c in labels}
        else:
            used = []
            for key, c, arr, zs, slab in jobs:
                thing = c in thing_list
                if isinstance(arr, ZarrV2Array):
                    w = self._writer(key, arr, zs, slab.shape, torch.int32 if thing else torch.uint8)
                    w.next_buffer().copy_(slab.view(torch.int32) if thing else slab, non_blocking=True)
                    post.synchronize()                    # the post stream only
                    w.submit()                            # chunk files by the pool, while the next slab is copied
                    used.append(w)
                else:
                    arr.write_slab(zs, driver.host_slab(slab, thing))
            for w in used:
                w.drain()
        if levels is not None and out is not None and rank == 0:
            driver.write_multiscales(out, labels, class_names, levels)
        return datasets, compressed, extra

    def close(self):
        for w in self._writers.values():
            w.close()
        self._writers = {}
        if self._zpool is not None:
            self._zpool.shutdown()
        self._zpool, self._zbufs = None, {}
