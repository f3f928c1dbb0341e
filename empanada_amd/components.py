"""Split disconnected objects: host logic over the component tables of _hip.label_components (include/emp_hip.h, E3).

The consensus paints an instance wherever the votes put it and a stack-mode track may join slices that merely overlap,
so an instance id need not be one piece; users of the reference repair that afterwards with cc3d.connected_components
and cc3d.dust on a CPU.  Here the voxel passes run on the device (csrc/emp_components.hip) and everything in this
module works on O(#components) tables: joining the components of z-blocks and of the ranks' slabs across their seams
(`seam_pairs`, `merge_blocks`), deciding which piece keeps the label, which gets a new one and which is erased
(`plan`), and the whole repair of one class (`split_volume`).  All but split_volume runs on the CPU.
"""
import numpy as np
import torch

from .tables import _host, bits, merge_seamed

__all__ = ['COLUMNS', 'merge_blocks', 'seam_pairs', 'plan', 'merged_table', 'split_volume']

COLUMNS = ('label', 'voxels', 'first', 'z0', 'y0', 'x0', 'z1', 'y1', 'x1')
_SHIFTS = {6: [(0, 0)],
           18: [(0, 0), (-1, 0), (1, 0), (0, -1), (0, 1)],
           26: [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]}
_MAX_LABEL = 2 ** 32 - 1


def _check_connectivity(connectivity):
    if isinstance(connectivity, bool) or connectivity not in _SHIFTS:
        raise ValueError(f"connectivity must be 6, 18 or 26, got {connectivity!r}")
    return int(connectivity)


def _wide(t):
    """an integer plane as a non-negative int64 tensor (the bits of int32 / uint32 are taken as they are)"""
    if not isinstance(t, torch.Tensor):
        a = np.asarray(t)
        if a.dtype in (np.int32, np.uint32):
            return torch.from_numpy(np.ascontiguousarray(a).view(np.uint32).astype(np.int64))
        return torch.from_numpy(a.astype(np.int64))
    t = bits(t)
    return t.long() & 0xffffffff if t.dtype == torch.int32 else t.long()


def seam_pairs(lab_a, ids_a, lab_b, ids_b, connectivity):
    """The provisional ids that touch across a seam: (H, W) planes `a` (the last slice of one block, z) and `b` (the
    first slice of the next, z + 1) with their original labels and the ids painted over them (0 = background).  Voxel
    a[y, x] is a neighbour of b[y + dy, x + dx] for the 1, 5 or 9 in-plane shifts that connectivity 6, 18 or 26 allows
    beside the step along z; a pair (id_a, id_b) is collected where both labels are equal and non-zero.  Returns the
    distinct pairs as an (m, 2) int64 array, ascending -- a tensor on the planes' device for tensors, numpy for numpy."""
    shifts = _SHIFTS[_check_connectivity(connectivity)]
    as_numpy = not isinstance(lab_a, torch.Tensor)
    la, ia, lb, ib = (_wide(t) for t in (lab_a, ids_a, lab_b, ids_b))
    if not (la.dim() == 2 and la.shape == ia.shape == lb.shape == ib.shape):
        raise ValueError(f"seam_pairs: four (H, W) planes of one shape expected, got {tuple(la.shape)}, "
                         f"{tuple(ia.shape)}, {tuple(lb.shape)}, {tuple(ib.shape)}")
    H, W = la.shape
    found = []
    for dy, dx in shifts:
        ya, yb = slice(max(0, -dy), H - max(0, dy)), slice(max(0, dy), H - max(0, -dy))
        xa, xb = slice(max(0, -dx), W - max(0, dx)), slice(max(0, dx), W - max(0, -dx))
        a, b = la[ya, xa], lb[yb, xb]
        hit = (a == b) & (a != 0)
        if hit.any():
            found.append(torch.stack([ia[ya, xa][hit], ib[yb, xb][hit]], dim=1))
    pairs = torch.unique(torch.cat(found), dim=0) if found else torch.zeros((0, 2), dtype=torch.int64, device=la.device)
    return pairs.cpu().numpy() if as_numpy else pairs


def merge_blocks(tables, seams, return_index=False):
    """The component table of a volume from the tables of its z-blocks (or of the ranks' slabs), each labelled by
    itself with its own z_base.  Provisional id p = 1 + row in the concatenation of `tables`; `seams` is a list of
    (m, 2) arrays of provisional ids that touch across a border (seam_pairs).  Ids joined by any chain of pairs become
    one component: voxels added, `first` and the box minima the minimum, the box maxima the maximum; the result is
    renumbered ascending by `first`, so it equals the table of the undivided volume.  Union-find on the host
    (scipy.sparse.csgraph).  numpy in, numpy out; with any tensor among the tables the result is a tensor on its
    device.  return_index: also the (n_provisional,) int64 map from p - 1 to the row of the merged table."""
    def same_label(rows, pairs):
        if len(pairs) and (rows[pairs[:, 0] - 1, 0] != rows[pairs[:, 1] - 1, 0]).any():
            raise ValueError("merge_blocks: a seam joins components of different labels")

    # the label is the same all over a component, so its minimum is the label
    return merge_seamed(tables, seams, len(COLUMNS), first=2, sums=[1], mins=[0, 2, 3, 4, 5], maxs=[6, 7, 8],
                        check=same_label, return_index=return_index)


def plan(table, min_size=None, min_span=None):
    """What becomes of every component: (lut, stats).  lut[k] (uint32 numpy, one per row of `table`) is the label that
    component k is painted with, 0 = erased.  Per original label, ascending: its components are ordered by (voxels
    descending, first ascending); the first keeps the label and every further one gets a new label max label + 1, + 2,
    ... in that order.  Every component, the first included, is judged on its own by the rules of the reference's
    filters (inference/filters.py:9-43): erased if voxels < min_size or if any of z1 - z0, y1 - y0, x1 - x0 is < min_span.
    New labels go to survivors only, so the labels stay dense above the old maximum.  stats: 'objects_in' (distinct
    labels), 'objects_split' (labels of more than one component), 'pieces_added' (new labels handed out),
    'pieces_removed' (components erased), 'objects_out' (components that remain).  A new label above 2^32 - 1 is a
    ValueError."""
    t = _host(table).reshape(-1, len(COLUMNS))
    n = len(t)
    lut = np.zeros(n, np.uint32)
    if n == 0:
        return lut, dict(objects_in=0, objects_split=0, pieces_added=0, pieces_removed=0, objects_out=0)
    if t[:, 0].min() < 1 or t[:, 0].max() > _MAX_LABEL:
        raise ValueError(f"plan: labels outside 1 .. {_MAX_LABEL}")
    keep = np.ones(n, bool)
    if min_size is not None:
        keep &= t[:, 1] >= min_size
    if min_span is not None:
        keep &= ((t[:, 6:9] - t[:, 3:6]) >= min_span).all(axis=1)
    order = np.lexsort((t[:, 2], -t[:, 1], t[:, 0]))          # by label, then voxels descending, then first
    lab = t[order, 0]
    head = np.ones(n, bool)
    head[1:] = lab[1:] != lab[:-1]
    extra = ~head & keep[order]                               # survivors that need a new label, in hand-out order
    top = int(t[:, 0].max())
    n_new = int(extra.sum())
    if top + n_new > _MAX_LABEL:
        raise ValueError(f"plan: {n_new} new labels above the largest label {top} would pass {_MAX_LABEL}")
    value = np.where(head, lab, 0)
    value[extra] = top + 1 + np.arange(n_new)
    value[~keep[order]] = 0
    lut[order] = value.astype(np.uint32)
    counts = np.diff(np.append(np.flatnonzero(head), n))
    stats = dict(objects_in=int(head.sum()), objects_split=int((counts > 1).sum()), pieces_added=n_new,
                 pieces_removed=int((~keep).sum()), objects_out=int(keep.sum()))
    return lut, stats


def merged_table(lc, connectivity, group=None, who="merged_table"):
    """The component table of the volume whose consecutive z-slabs the ranks of `group` hold, from every rank's own
    _hip.label_components result `lc`: (table, mine).  The ranks gather their tables and exchange their end slices --
    labels and provisional ids, as the measurements exchange theirs (sharded.neighbour_slices) -- each finds the pairs
    that touch across the seam below it, and every rank computes the same merged table; mine[k] is the row of this
    rank's component k in it.  A single rank: (lc.table, None)."""
    from .inference import sharded
    rank, world = sharded._world(group)
    if world == 1:
        return lc.table, None
    slab = lc.slab
    dev = slab.device
    tables = sharded._gather_var(lc.table, group)
    base = sum(int(t.shape[0]) for t in tables[:rank])
    if sum(int(t.shape[0]) for t in tables) > _MAX_LABEL:
        raise ValueError(f"{who}: the ranks' provisional components do not fit 32-bit ids")
    H, W = int(slab.shape[1]), int(slab.shape[2])
    ends = torch.zeros((2 if slab.shape[0] else 0, H, W), dtype=torch.uint32, device=dev)
    if slab.shape[0] and lc.n:
        ids = base + 1 + torch.arange(lc.n, dtype=torch.int64, device=dev)
        ends = torch.stack([lc.paint_slice(ids, z).view(torch.int32) for z in (0, int(slab.shape[0]) - 1)])
        ends = ends.view(torch.uint32)
    below_lab, _ = sharded.neighbour_slices(slab, group)
    below_ids, _ = sharded.neighbour_slices(ends, group)
    if below_lab is not None and slab.shape[0]:
        seam = seam_pairs(below_lab, below_ids, slab[0], ends[0], connectivity)
    else:
        seam = torch.zeros((0, 2), dtype=torch.int64, device=dev)
    seams = sharded._gather_var(seam.contiguous(), group)
    table, index = merge_blocks(tables, seams, return_index=True)
    return table, index[base:base + lc.n]


def split_volume(slab, connectivity=26, min_size=None, min_span=None, group=None, z_base=0, out=None):
    """The repair of one class: every label of `slab` -- a rank's (d, H, W) device slab of a volume whose slices
    [z_base, z_base + d) it holds, uint8 or int32 / uint32 -- is split into its connected components and `plan` decides
    what each is painted with; returns (volume, stats), stats being plan's.  out=None paints the slab itself in place
    (only the runs whose value changes are written); any other `out` as LabelComponents.paint takes it.  With `group`
    the ranks hold consecutive z-slabs of ONE volume: every rank labels its own slab, the ranks gather their tables and
    exchange their end slices -- labels and provisional ids, as the measurements exchange theirs
    (sharded.neighbour_slices) -- each finds the pairs that touch across the seam below it, and every rank computes the
    same merged table and the same plan and paints its own slab.  A rank without slices takes part with an empty slab."""
    from . import _hip
    connectivity = _check_connectivity(connectivity)
    lc = _hip.label_components(slab, connectivity, z_base=z_base)
    dev = slab.device
    table, mine = merged_table(lc, connectivity, group, "split_volume")
    lut, stats = plan(table, min_size, min_span)
    lut = torch.from_numpy(lut.astype(np.int64)).to(dev)
    if mine is not None:
        lut = lut[mine]
    return lc.paint(lut, out=slab if out is None else out), stats
