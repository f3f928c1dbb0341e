"""Planes that stream through windows of slices: the head tensors of a plane need not be resident at once.

Everything downstream of the heads is per slice except the recursive median, and that recursion can be cut at any
slice and resumed bit for bit from the last m = ks // 2 FILTERED slices and the next m RAW ones
(emp_median_harden_window; sharded.median_handover does the same across ranks).  So a plane is walked in windows of W
slices: the model fills a window's heads, the post-processing labels it into the plane's resident uint32 `pan`, and
only m slices of heads and the m-slice history survive a step.  The result is identical to the whole-plane path
(sharded.sharded_panoptic_stack on all heads), tests/test_windowed_gpu.py.

    plan = plan_windows(n, per, m, window_slices)                  # pure Python: the forward chunks of the plane
    pan = windowed_panoptic_stack(fill, plan, shapes, device=..., **engine_params)

The lag scheme (every window at least as long as the filter): the post-processing runs m slices behind the forward.
One set of head buffers holds W + m slices; a step's view is [m carried raw slices | the chunk just filled]; its body
is all of the view but the last m slices, which are its halo and, copied to the front, the next step's carry.  The
first step has no history, the last no halo and takes everything left.
Windows shorter than the filter (W < ks, more than one of them) cannot give the first step ks slices in W + m: there
two sets of W slices alternate, a step's body is its whole chunk and its halo the first m slices of the next set.
"""
import torch

from .. import _hip
from .postprocess import centers_batched

__all__ = ['plan_windows', 'head_shapes', 'plane_layout', 'WindowedPlane', 'windowed_panoptic_stack']

HEADS = ('sem', 'ctr_hmp', 'offsets')


def _count(what, v, least):
    if isinstance(v, bool) or not isinstance(v, int) or v < least:
        raise ValueError(f"{what} must be an integer >= {least}, got {v!r}")
    return v


def plan_windows(n_slices, per, m, window_slices, bytes_per_slice=None, budget=None, sem_bytes=0):
    """The forward chunks [(lo, hi), ...] of a plane of n_slices slices; pure Python.
    per: slices per model call; m = ks // 2: the median's reach.
    window_slices: None = one chunk (the whole plane); an integer W, rounded DOWN to a multiple of `per` so that every
    model call sees the slices it sees in the unwindowed run (a W below `per` shrinks the calls to W instead); 'auto' =
    the whole plane when n_slices * bytes_per_slice fits into `budget` bytes, else the largest multiple of `per` with
    (W + m) * bytes_per_slice + m * sem_bytes <= budget (the head buffers of the lag scheme and the history).
    Every chunk but the last has the same length; a last chunk shorter than m is merged into the one before it."""
    n = _count('n_slices', n_slices, 1)
    per = _count('per', per, 1)
    m = _count('m', m, 0)
    ks = 2 * m + 1
    if n < ks:
        raise ValueError(f"a plane of {n} slices is shorter than the median kernel (ks={ks})")
    if window_slices is None:
        return [(0, n)]
    if isinstance(window_slices, str):
        if window_slices != 'auto':
            raise ValueError(f"window_slices must be None, a positive integer or 'auto', got {window_slices!r}")
        bps = _count('bytes_per_slice', bytes_per_slice, 1)
        budget = _count('budget', budget, 0)
        if n * bps <= budget:
            return [(0, n)]
        W = ((budget - m * _count('sem_bytes', sem_bytes, 0)) // bps - m) // per * per
        if W < per:
            raise ValueError(f"not even one model call of {per} slices fits: ({per} + {m}) slices of {bps} bytes and "
                             f"{m} slices of {sem_bytes} bytes of history against a budget of {budget} bytes")
    else:
        W = _count('window_slices', window_slices, 1)
        if W >= n:
            return [(0, n)]
        if W >= per:
            W = W // per * per
    if W < m:
        raise ValueError(f"windows of {W} slices are shorter than the median's reach m={m} (ks={ks}, {per} slices per "
                         "model call)")
    if W >= n:
        return [(0, n)]
    chunks = [(lo, min(n, lo + W)) for lo in range(0, n, W)]
    if chunks[-1][1] - chunks[-1][0] < m:
        chunks[-2:] = [(chunks[-2][0], n)]
    return chunks


def head_shapes(hp, wp, classes, scale=1, coarse=False):
    """per-slice shapes of the three heads for a (hp, wp) padded model input: the semantic head comes out `scale` x
    larger (down-sampled inference), the instance heads at 1/4 with coarse boundaries"""
    ins = (hp // 4, wp // 4) if coarse else (hp, wp)
    return {'sem': (classes, hp * scale, wp * scale), 'ctr_hmp': (1,) + ins, 'offsets': (2,) + ins}


def bytes_per_slice(shapes):
    n = 0
    for s in shapes.values():
        n += 4 * s[0] * s[1] * s[2]
    return n


def plane_layout(plan, ks):
    """(steps, borrow, cap) of a plane: the (lo, hi) the forwards fill, whether the windows are shorter than the filter
    (no carry: the halo is borrowed from the next set), and the slices one set of head buffers holds"""
    m = ks // 2
    plan = [(int(lo), int(hi)) for lo, hi in plan]
    n = plan[-1][1]
    if plan[0][0] != 0 or any(a[1] != b[0] for a, b in zip(plan, plan[1:])) or any(hi <= lo for lo, hi in plan):
        raise ValueError(f"the plan's chunks must be contiguous from 0: {plan}")
    if n < ks or any(hi - lo < m for lo, hi in plan):
        raise ValueError(f"every chunk needs >= m={m} slices and the plane >= ks={ks}: {plan}")
    W = plan[0][1] - plan[0][0]
    borrow = len(plan) > 1 and W < ks
    if not borrow and len(plan) > 1 and plan[-1][1] - plan[-1][0] > W:
        lo, hi = plan[-1]                           # a merged last chunk is filled in two steps: W + m slices hold it
        plan[-1:] = [(lo, lo + W), (lo + W, hi)]
    cap = max(hi - lo for lo, hi in plan) + (m if (len(plan) > 1 and not borrow) else 0)
    return plan, borrow, cap


class WindowedPlane:
    """One plane's walk: forward(k) fills step k's heads, post(k) labels what the step can label.  post(k) needs the
    forwards up to needs(k); with several buffer sets forward(k) writes set k % sets, which post(k - sets) was the last
    to read (and, in the lag scheme, reads the tail of set (k - 1) % sets).  windowed_panoptic_stack is the serial
    driver; VolumePipeline runs the two on two streams.
    alloc(i, {name: shape}) -> {name: fp32 tensor}: where set i's head buffers come from (default torch.empty)."""

    def __init__(self, fill, plan, shapes, *, device, thing_list, label_divisor=1000, stuff_area=64, void_label=0,
                 nms_threshold=0.1, nms_kernel=7, confidence_thr=0.5, median_kernel_size=3, coarse_boundaries=True,
                 n_classes=None, max_centers=None, upsampling=1, sets=1, alloc=None):
        self.fill = fill
        self.ks = int(median_kernel_size)
        self.m = self.ks // 2
        self.steps, self.borrow, cap = plane_layout(plan, self.ks)
        n = self.steps[-1][1]
        if alloc is None:
            def alloc(i, shp):
                return {k: torch.empty(v, dtype=torch.float32, device=device) for k, v in shp.items()}
        nsets = min(max(int(sets), 2 if self.borrow else 1), len(self.steps))
        self.sets = [alloc(i, {k: (cap,) + tuple(shapes[k]) for k in HEADS}) for i in range(nsets)]
        self.hist = None
        self.filled = [0] * len(self.steps)
        C, H, Wd = shapes['sem']
        self.pan = torch.empty((n, H, Wd), dtype=torch.int32, device=device).view(torch.uint32)
        self.thing_list = list(thing_list)
        self.step = 4 if coarse_boundaries else 1
        self.up = int(upsampling)
        self.n_classes = n_classes if n_classes is not None else max(2 if C == 1 else C, max(self.thing_list) + 1)
        self.centers = (nms_threshold, nms_kernel, max_centers)
        self.fuse = (label_divisor, stuff_area, void_label)
        self.thr = confidence_thr

    def head_bytes(self):
        """bytes of head buffers this plane holds: the sets and the history"""
        t = [b for s in self.sets for b in s.values()] + ([self.hist] if self.hist is not None else [])
        return sum(x.numel() * x.element_size() for x in t)

    def needs(self, k):
        """post(k) may run once forward(needs(k)) has"""
        return min(k + 1, len(self.steps) - 1) if self.borrow else k

    def forward(self, k):
        lo, hi = self.steps[k]
        S = self.sets[k % len(self.sets)]
        at = 0
        if k > 0 and not self.borrow:
            at = self.m
            if at:
                prev, end = self.sets[(k - 1) % len(self.sets)], self.filled[k - 1]
                for name in HEADS:                  # the carry: end >= 2m, so within one set the two ranges are disjoint
                    S[name][:at].copy_(prev[name][end - at:end])
        self.fill(lo, hi, S, at)
        self.filled[k] = at + hi - lo

    def post(self, k):
        m, ks = self.m, self.ks
        lo, hi = self.steps[k]
        S = self.sets[k % len(self.sets)]
        last = k == len(self.steps) - 1
        n = self.filled[k]
        if self.borrow:
            D, first = n, lo
            halo = None if last else self.sets[(k + 1) % len(self.sets)]['sem'][:m]
        else:
            D, first = (n if last else n - m), hi - n
            halo = None if last else S['sem'][D:D + m]
        prob = S['sem'][:D]
        if ks == 1:
            sem = _hip.median_harden_window(prob, 1, self.thr)
        elif (k == 0 and not last and D == m) or (last and k > 0 and D == m):
            # a chunk of exactly m slices at either end of the axis passes through raw
            sem = _hip.median_harden_window(prob, 1, self.thr)
            if k == 0:
                self.hist = prob.clone()
        elif last:
            sem = _hip.median_harden_window(prob, ks, self.thr, hist=self.hist if k else None)
        elif self.hist is None:
            sem, self.hist = _hip.median_harden_window(prob, ks, self.thr, halo=halo, want_tail=True)
        else:
            sem, _ = _hip.median_harden_window(prob, ks, self.thr, hist=self.hist if k else None, halo=halo,
                                               tail_out=self.hist)
        idx, cnt = centers_batched(S['ctr_hmp'][:D], *self.centers)
        ids = _hip.group_pixels(idx, cnt, S['offsets'][:D], self.step,
                                sem=sem if (self.step == 1 and self.up == 1) else None, thing_list=self.thing_list)
        label_divisor, stuff_area, void_label = self.fuse
        _hip.fuse_panoptic(sem, ids, idx.shape[1], self.n_classes, self.thing_list, label_divisor, stuff_area, void_label,
                           up=self.step * self.up, out=self.pan[first:first + D])


def windowed_panoptic_stack(fill, plan, shapes, *, device, info=None, **params):
    """The plane-level step sharded_panoptic_stack is for a whole block, window by window.
    fill(lo, hi, bufs, at): writes the heads of slices [lo, hi) into bufs['sem' | 'ctr_hmp' | 'offsets'][at:at + hi - lo]
    (fp32, (slices,) + shapes[name]); plan: plan_windows' chunks; shapes: per-slice head shapes (head_shapes); params:
    sharded_panoptic_stack's.  Returns pan (n, H, W) uint32, identical to sharded_panoptic_stack on the plane's heads.
    info: a dict that receives 'windows' (steps run) and 'head_bytes' (bytes of head buffers held)."""
    plane = WindowedPlane(fill, plan, shapes, device=device, **params)
    f = 0
    for k in range(len(plane.steps)):
        while f <= plane.needs(k):
            plane.forward(f)
            f += 1
        plane.post(k)
    if info is not None:
        info['windows'] = len(plane.steps)
        info['head_bytes'] = plane.head_bytes()
    return plane.pan
