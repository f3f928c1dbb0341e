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
    written by a pool while the next class is copied).
With infer_volume(..., window_slices=) the planes stream through windows of slices (inference/windowed.py) and the two
sets of buffers alternate per step of a plane instead of per plane (_run_windowed).
"""
import json
import os

import numpy as np
import torch

from .. import _hip
from ..zarr_utils import SlabWriter, ZarrV2Array
from . import sharded, windowed
from .engines import logits_to_prob

__all__ = ['VolumePipeline']

_HEADS = (('sem', 'sem_logits'), ('ctr_hmp', 'ctr_hmp'), ('offsets', 'offsets'))


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
    def _head_shapes(self, dv, axis, n, render, coarse, classes):
        """the padded head shapes sharded_panoptic_stack takes for n slices of the plane"""
        hp, wp = dv.padded_shape(axis)
        f = dv.scale if render else 1
        ins = (hp // 4, wp // 4) if (render and coarse) else (hp, wp)
        return {'sem': (n, classes, hp * f, wp * f), 'ctr_hmp': (n, 1) + ins, 'offsets': (n, 2) + ins}

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

    def _fits(self, plane_elems, dv, out_bytes):
        """overlap='auto': two planes' heads + the resident volume + the labelled slabs against the budget"""
        two = 4 * sum(sorted(plane_elems)[-2:])
        if self.mem_budget is not None:
            return two + dv.vol.numel() + out_bytes <= self.mem_budget
        free, _ = torch.cuda.mem_get_info(dv.vol.device)
        cached = torch.cuda.memory_reserved(dv.vol.device) - torch.cuda.memory_allocated(dv.vol.device)
        held = 4 * sum(s.numel() for s in self._store if s is not None)
        return two + out_bytes <= free + cached + held        # the volume is resident already: it is not in `free`

    # ------------------------------------------------------------------------------------------ one plane's forward
    @torch.no_grad()
    def _forward(self, model, dv, axis, lo, hi, per, margs, bufs):
        """slices [lo, hi) of the plane through the model, on the current (forward) stream; every batch writes its slices
        of the three head buffers once"""
        hp, wp = dv.padded_shape(axis)
        graphed = model is self._graphed
        for s in range(lo, hi, per):
            e = min(hi, s + per)
            buf = model.input_buffer((e - s, 1, hp, wp), args=margs) if graphed else None
            x = dv.batch(axis, s, e, out=buf)
            if x.dtype != self._param().dtype:
                x = x.to(self._param().dtype)
            o = model(x.contiguous(memory_format=torch.channels_last), *margs)
            deferred = o.get('deferred_up4', ())
            for name, key in _HEADS:
                t, view = o[key], bufs[name][s - lo:e - lo]
                if key in deferred:
                    if tuple(view.shape[:2]) != tuple(t.shape[:2]):
                        raise RuntimeError(f"head {key}: the model returned {tuple(t.shape)}, the plane buffer holds "
                                           f"{tuple(view.shape)}")
                    _hip.upsample_bilinear_prob(t, view.shape[2:], out=view, prob=name == 'sem')
                    continue
                if tuple(view.shape) != tuple(t.shape):
                    raise RuntimeError(f"head {key}: the model returned {tuple(t.shape)}, the plane buffer holds "
                                       f"{tuple(view.shape)}")
                if name != 'sem':
                    view.copy_(t)
                elif t.dtype == torch.float32:
                    _hip.logits_to_prob(t, out=view)
                else:
                    view.copy_(logits_to_prob(t))

    def _margs(self, steps):
        """extra positional arguments of the model's forward"""
        if self.model_args is not None:
            return self.model_args
        if hasattr(self.engine, 'coarse_boundaries'):
            return (steps, not self.engine.coarse_boundaries)
        return ()

    def _per(self, dv, axis):
        """slices per model call: batch_pixels counts OUTPUT pixels (a down-sampling volume renders scale x the input)"""
        hp, wp = dv.padded_shape(axis)
        return max(1, self.batch_pixels // (hp * wp * dv.scale ** 2))

    def _defers(self):
        """the x4 up-sampling of the heads leaves the model only on the fp32 GPU path of a model that offers it"""
        return (self._param().dtype == torch.float32 and hasattr(self.model, 'defer_up4')
                and bool(getattr(self.model, 'hip_ops', False)))

    @torch.no_grad()
    def forwards_only(self, dv, axes=('xy', 'xz', 'yz'), render_steps=2):
        """For measurements: the forwards of all planes exactly as run() queues them (same arguments, batches, graph
        replay, heads written in place into set 0), without any post-processing; blocks until they are done.  Call it
        after a run() on the same volume, so that tuning and captures are out of the way."""
        render = hasattr(self.engine, 'coarse_boundaries')
        coarse = bool(getattr(self.engine, 'coarse_boundaries', False))
        margs = self._margs(render_steps + dv.scale.bit_length() - 1)
        graph = self.graph and self._param().dtype == torch.float32 and self._graphed is not None
        model = self._graphed if graph else self.model
        classes = int(self.model.num_classes)
        defer = self._defers()
        try:
            if defer:
                self.model.defer_up4 = True
            for axis in axes:
                n = dv.n_slices(axis)
                shapes = self._head_shapes(dv, axis, n, render, coarse, classes)
                self._reserve(0, self._elems(shapes), dv.vol.device)
                self._forward(model, dv, axis, 0, n, self._per(dv, axis), margs, self._views(0, shapes))
        finally:
            if defer:
                self.model.defer_up4 = False
        torch.cuda.synchronize(dv.vol.device)

    # ------------------------------------------------------------------------------------------ the volume
    def run(self, dv, *, axes, labels, thing_list, params, steps, group, track, finish, class_names, out,
            window_slices=None):
        """Called by infer_volume after its own argument checks.  track(pan, axis, base) and finish(planes) are the
        driver's own plane and volume steps, so both paths share them.  window_slices: see _run_windowed."""
        if window_slices is not None:
            return self._run_windowed(dv, axes=axes, labels=labels, thing_list=thing_list, params=params, steps=steps,
                                      track=track, finish=finish, class_names=class_names, out=out,
                                      window_slices=window_slices)
        engine = self.engine
        dev = dv.vol.device
        rank, world = sharded._world(group)
        render = hasattr(engine, 'coarse_boundaries')
        coarse = bool(getattr(engine, 'coarse_boundaries', False))
        margs = self._margs(steps)
        fp32 = self._param().dtype == torch.float32
        classes = int(getattr(self.model, 'num_classes', 0)) or None
        plan = []
        for axis in axes:
            b = sharded.shard_bounds(dv.n_slices(axis), world)
            lo, hi = int(b[rank]), int(b[rank + 1])
            hp, wp = dv.padded_shape(axis)
            per = self._per(dv, axis)
            plan.append((axis, lo, hi, per, hp, wp))
        self._tune_once((plan[0][3], plan[0][4], plan[0][5]), margs, group)
        if classes is None:                               # a model that does not say: ask it on one slice
            with torch.no_grad():
                classes = int(self.model(dv.batch(plan[0][0], 0, 1).to(self._param().dtype), *margs)['sem_logits'].shape[1])
        shapes = [self._head_shapes(dv, a, hi - lo, render, coarse, classes) for a, lo, hi, _, _, _ in plan]
        elems = [self._elems(s) for s in shapes]
        out_bytes = int(np.prod(dv.shape)) // world * sum(4 if c in thing_list else 1 for c in labels)
        overlap = self.overlap
        if overlap == 'auto':
            overlap = self._fits(elems, dv, out_bytes)
        overlap = bool(overlap) and len(plan) > 1
        nsets = 2 if overlap else 1
        if not overlap:
            self._store[1] = None
        for k in range(nsets):
            self._reserve(k, max(elems[k::nsets]), dev)
        head_bytes = 4 * sum(s.numel() for s in self._store if s is not None)
        if self._streams is None or self._streams[0].device != dev:
            self._streams = (torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev))
        fwd, post = self._streams
        graph = self.graph and fp32
        if graph and self._graphed is None:
            from ..models.graphed import GraphedForward
            # up to two batch sizes per plane and three planes per volume shape: room for a few shapes, so that
            # alternating between volumes does not evict and re-capture; res['pipeline']['captures'] counts what a call cost
            self._graphed = GraphedForward(self.model, warmup=1, max_graphs=24, clone_outputs=False)
        model = self._graphed if graph else self.model
        defer = self._defers()
        captured = self._graphed.captures if graph else 0

        cur = torch.cuda.current_stream(dev)
        fwd.wait_stream(cur)                              # the volume's upload, whatever the caller queued before
        post.wait_stream(cur)
        bufs = [None] * len(plan)
        done = [torch.cuda.Event() for _ in plan]         # forward of plane i complete
        free = [torch.cuda.Event() for _ in plan]         # post-processing of plane i has read its heads

        def launch(i):
            axis, lo, hi, per, _, _ = plan[i]
            with torch.cuda.stream(fwd):
                if i >= nsets:
                    fwd.wait_event(free[i - nsets])       # this set's buffers are still being read until then
                bufs[i] = self._views(i % nsets, shapes[i])
                self._forward(model, dv, axis, lo, hi, per, margs, bufs[i])
                done[i].record(fwd)

        planes, base = {}, 0
        try:
            if defer:
                self.model.defer_up4 = True
            for i in range(min(nsets, len(plan))):
                launch(i)
            with torch.cuda.stream(post):
                for i, (axis, lo, hi, _, _, _) in enumerate(plan):
                    if bufs[i] is None:
                        launch(i)
                    post.wait_event(done[i])
                    h = bufs[i]
                    pan = sharded.sharded_panoptic_stack(h['sem'], h['ctr_hmp'], h['offsets'], group=group, **params)
                    free[i].record(post)
                    if overlap and i + nsets < len(plan):
                        launch(i + nsets)                 # queued behind `free`, ahead of this plane's host work
                    planes[axis] = track(pan, axis, base)
                    base += planes[axis].n_inst
                    del pan
                vols, (z0, z1), counts = finish(planes)
                datasets = self._write(out, vols, z0, labels, thing_list, class_names, dv.shape, rank, world, group, post)
        finally:
            if defer:
                self.model.defer_up4 = False
        cur.wait_stream(post)
        cur.wait_stream(fwd)
        for v in vols.values():
            v.record_stream(cur)                          # allocated on the post stream, handed to the caller's
        return {'volumes': vols, 'z_range': (z0, z1), 'instances': counts, 'datasets': datasets,
                'pipeline': {'tuned': self.tuned_counts(), 'graph': bool(graph), 'overlap': bool(overlap),
                             'head_bytes': int(head_bytes),
                             'captures': (self._graphed.captures - captured) if graph else 0}}

    # ------------------------------------------------------------------------------------------ the volume, in windows
    def _run_windowed(self, dv, *, axes, labels, thing_list, params, steps, track, finish, class_names, out,
                      window_slices):
        """run() with every plane streamed through windows of slices (inference/windowed.py; one rank).  The two sets of
        head buffers alternate per STEP instead of per plane: the forward of step k + 1 runs on the forward stream
        while the post stream labels step k; with overlap off, one set and strict alternation.  The carry copy and the
        median are ordinary launches on the two streams, outside the captured forward, under the same events that
        order the sets.  'auto' plans with the pipeline's mem_budget (None: the free device memory), halved when two
        sets are held."""
        engine, dev = self.engine, dv.vol.device
        render = hasattr(engine, 'coarse_boundaries')
        coarse = bool(getattr(engine, 'coarse_boundaries', False))
        margs = self._margs(steps)
        fp32 = self._param().dtype == torch.float32
        ks = int(params['median_kernel_size'])
        m = ks // 2
        geo = [(axis, dv.n_slices(axis), self._per(dv, axis)) + tuple(dv.padded_shape(axis)) for axis in axes]
        self._tune_once((geo[0][2], geo[0][3], geo[0][4]), margs, None)
        classes = int(getattr(self.model, 'num_classes', 0))
        if not classes:                                   # a model that does not say: ask it on one slice
            with torch.no_grad():
                classes = int(self.model(dv.batch(geo[0][0], 0, 1).to(self._param().dtype), *margs)['sem_logits'].shape[1])
        shapes = [windowed.head_shapes(hp, wp, classes, dv.scale if render else 1, render and coarse)
                  for _, _, _, hp, wp in geo]
        budget = self.mem_budget
        if budget is None:
            free, _ = torch.cuda.mem_get_info(dev)
            cached = torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)
            held = 4 * sum(s.numel() for s in self._store if s is not None)
            budget = max(0, free + cached + held - 4 * max(n * sh['sem'][1] * sh['sem'][2]
                                                           for (_, n, _, _, _), sh in zip(geo, shapes)))
        nsets = 1 if self.overlap is False else 2
        while True:
            plans = [windowed.plan_windows(n, per, m, window_slices, windowed.bytes_per_slice(sh), budget // nsets,
                                           4 * int(np.prod(sh['sem']))) for (_, n, per, _, _), sh in zip(geo, shapes)]
            lay = [windowed.plane_layout(p, ks) for p in plans]
            elems = [self._elems({k: (cap,) + tuple(v) for k, v in sh.items()}) for (_, _, cap), sh in zip(lay, shapes)]
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
        if self._streams is None or self._streams[0].device != dev:
            self._streams = (torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev))
        fwd, post = self._streams
        graph = self.graph and fp32
        if graph and self._graphed is None:
            from ..models.graphed import GraphedForward
            self._graphed = GraphedForward(self.model, warmup=1, max_graphs=24, clone_outputs=False)
        model = self._graphed if graph else self.model
        defer = self._defers()
        captured = self._graphed.captures if graph else 0

        cur = torch.cuda.current_stream(dev)
        fwd.wait_stream(cur)
        post.wait_stream(cur)
        last_read = {}                                    # set -> event: the last post-processing that read it
        planes, base, counts_w, hist_bytes = {}, 0, {}, 0
        try:
            if defer:
                self.model.defer_up4 = True
            with torch.cuda.stream(post):
                for (axis, n, per, hp, wp), sh, plan in zip(geo, shapes, plans):
                    def fill(lo, hi, bufs, at, axis=axis, per=per):
                        self._forward(model, dv, axis, lo, hi, per, margs,
                                      {k: v[at:at + hi - lo] for k, v in bufs.items()})

                    P = windowed.WindowedPlane(fill, plan, sh, device=dev, sets=nsets,
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
                    counts_w[axis] = K
                    hist_bytes = max(hist_bytes, 0 if P.hist is None else P.hist.numel() * 4)
                    planes[axis] = track(P.pan, axis, base)
                    base += planes[axis].n_inst
                    del P
                vols, (z0, z1), counts = finish(planes)
                datasets = self._write(out, vols, z0, labels, thing_list, class_names, dv.shape, 0, 1, None, post)
        finally:
            if defer:
                self.model.defer_up4 = False
        cur.wait_stream(post)
        cur.wait_stream(fwd)
        for v in vols.values():
            v.record_stream(cur)
        head_bytes = 4 * sum(s.numel() for s in self._store if s is not None) + hist_bytes
        return {'volumes': vols, 'z_range': (z0, z1), 'instances': counts, 'datasets': datasets,
                'windows': counts_w, 'head_bytes': int(head_bytes),
                'pipeline': {'tuned': self.tuned_counts(), 'graph': bool(graph), 'overlap': bool(overlap),
                             'head_bytes': int(head_bytes), 'windows': counts_w,
                             'captures': (self._graphed.captures - captured) if graph else 0}}

    # ------------------------------------------------------------------------------------------ writing
    def _writer(self, c, array, z0, shape, dtype):
        """one SlabWriter (pool + pinned buffer) per class and slab shape, kept across volumes: pinning is slow"""
        key = (c, tuple(shape), dtype)
        w = self._writers.get(key)
        if w is None:
            for k in [k for k in self._writers if k[0] == c]:
                self._writers.pop(k).close()
            w = self._writers[key] = SlabWriter(array, z0, shape, dtype, buffers=1)
        w.retarget(array, z0)
        return w

    def _write(self, out, vols, z0, labels, thing_list, class_names, shape3d, rank, world, group, post):
        datasets = {c: None for c in labels}
        if out is None:
            return datasets
        names = {c: f"{(class_names or {}).get(c, c)}_pred" for c in labels}
        if rank == 0:
            for c in labels:
                out.create_dataset(names[c], shape=shape3d, dtype=np.uint32 if c in thing_list else np.uint8,
                                   overwrite=True, chunks=(1, None, None))
        if world > 1:
            torch.distributed.barrier(group=group)
        used = []
        for c in labels:
            arr = datasets[c] = out[names[c]]
            thing = c in thing_list
            if isinstance(arr, ZarrV2Array):
                w = self._writer(c, arr, z0, vols[c].shape, torch.int32 if thing else torch.uint8)
                w.next_buffer().copy_(vols[c].view(torch.int32) if thing else vols[c], non_blocking=True)
                post.synchronize()                        # the post stream only
                w.submit()                                # chunk files by the pool, while the next class is copied
                used.append(w)
            else:
                host = vols[c].view(torch.int32).cpu().numpy().view(np.uint32) if thing else vols[c].cpu().numpy()
                arr.write_slab(z0, host)
        for w in used:
            w.drain()
        return datasets

    def close(self):
        for w in self._writers.values():
            w.close()
        self._writers = {}
