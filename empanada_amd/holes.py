"""Fill enclosed holes in objects: host logic over the cavity tables of _hip.label_holes (include/emp_hip.h, E4).

MitoNet-style models leave cavities inside objects -- cristae, matrix granules, voxels where the planes' votes disagree
-- and users of the reference fill them afterwards on a CPU with scipy.ndimage.binary_fill_holes, object by object.
Here the voxel passes run on the device (csrc/emp_holes.hip) and everything in this module works on O(#cavities)
tables: joining the cavities of z-blocks and of the ranks' slabs across their seams (`merge_blocks`, with the pairs of
components.seam_pairs over the zero voxels), deciding which cavity is filled with which label (`plan`), and the whole
repair of one class (`fill_volume`).  All but fill_volume runs on the CPU.
"""
import numpy as np
import torch

from .components import _host, seam_pairs
from .tables import bits, merge_seamed

__all__ = ['COLUMNS', 'NO_LABEL', 'merge_blocks', 'plan', 'fill_volume']

COLUMNS = ('voxels', 'first', 'z0', 'y0', 'x0', 'z1', 'y1', 'x1', 'lab_min', 'lab_max')
NO_LABEL = 2 ** 32                   # lab_min of a cavity without a surveyed wall label (its lab_max is 0)


def merge_blocks(tables, seams, return_index=False):
    """The cavity table of a volume from the tables of its z-blocks (or of the ranks' slabs), each labelled by itself
    with its own z_base and its true neighbour slices.  Provisional id p = 1 + row in the concatenation of `tables`;
    `seams` is a list of (m, 2) arrays of provisional ids that touch across a border: components.seam_pairs(a == 0,
    ids_a, b == 0, ids_b, 6).  Ids joined by any chain of pairs become one cavity: voxels added, `first`, the box minima
    and lab_min the minimum, the box maxima and lab_max the maximum -- except that a cavity with any piece that touches
    an x or y border (lab_max == 0, see E4) reports (NO_LABEL, 0), as the undivided volume does.  The result is
    renumbered ascending by `first`, so it equals the table of the undivided volume.  Union-find on the host
    (scipy.sparse.csgraph).  numpy in, numpy out; with any tensor among the tables the result is a tensor on its
    device.  return_index: also the (n_provisional,) int64 map from p - 1 to the row of the merged table."""
    def border(rows, index, out):
        hit = np.zeros(len(out), bool)
        hit[index[rows[:, 9] == 0]] = True
        out[hit, 8], out[hit, 9] = NO_LABEL, 0

    return merge_seamed(tables, seams, len(COLUMNS), first=1, sums=[0], mins=[1, 2, 3, 4, 8], maxs=[5, 6, 7, 9],
                        fixup=border, return_index=return_index)


def _is_zero(plane):
    """the zero voxels of an integer plane as a bool tensor (torch compares few uint32 tensors)"""
    return bits(plane) == 0


def _check_cap(max_voxels, what='max_voxels'):
    if max_voxels is None:
        return None
    if isinstance(max_voxels, (bool, np.bool_)) or not isinstance(max_voxels, (int, np.integer)) or max_voxels < 1:
        raise ValueError(f"{what} must be None or a positive integer, got {max_voxels!r}")
    return int(max_voxels)


def plan(table, shape3d, max_voxels=None):
    """What becomes of every cavity: (lut, stats).  lut[k] (uint32 numpy, one per row of `table`) is the label that
    cavity k is painted with, 0 = left as it is.  A cavity is closed when its box keeps clear of all six faces of the
    WHOLE volume `shape3d` = (D, H, W): z0, y0, x0 > 0 and z1 < D, y1 < H, x1 < W.  A closed cavity is filled with L
    when its wall labels are exactly {L} (lab_min == lab_max) and, with a cap, voxels <= max_voxels.  stats: 'cavities'
    (the closed ones), 'filled', 'voxels_filled', 'shared' (closed, two or more wall labels: left), 'too_large'
    (closed, one wall label, above the cap: left)."""
    t = _host(table).reshape(-1, len(COLUMNS))
    max_voxels = _check_cap(max_voxels)
    if len(shape3d) != 3 or any(int(s) < 0 for s in shape3d):
        raise ValueError(f"plan: shape3d must be (D, H, W), got {shape3d!r}")
    size = np.asarray([int(s) for s in shape3d], np.int64)
    closed = (t[:, 2:5] > 0).all(axis=1) & (t[:, 5:8] < size).all(axis=1)
    if (closed & (t[:, 9] == 0)).any():
        raise ValueError("plan: a closed cavity without a wall label: the table is not that of this shape")
    single = closed & (t[:, 8] == t[:, 9])
    fill = single if max_voxels is None else single & (t[:, 0] <= max_voxels)
    lut = np.where(fill, t[:, 8], 0).astype(np.uint32)
    stats = dict(cavities=int(closed.sum()), filled=int(fill.sum()), voxels_filled=int(t[fill, 0].sum()),
                 shared=int((closed & ~single).sum()), too_large=int((single & ~fill).sum()))
    return lut, stats


def fill_volume(slab, shape3d, max_voxels=None, group=None, z_base=0):
    """The repair of one class: every closed cavity of the volume `shape3d` = (D, H, W) that one label alone walls is
    painted with that label, in place, in `slab` -- a rank's (d, H, W) device slab holding the volume's slices [z_base,
    z_base + d), uint8 or int32 / uint32; returns (slab, stats), stats being plan's.  Only voxels of filled cavities are
    written.  With `group` the ranks hold consecutive z-slabs of ONE volume: every rank labels its own slab with the
    neighbouring ranks' end slices standing for what lies outside it, the ranks gather their tables and exchange their
    end slices -- labels and provisional ids (sharded.neighbour_slices) -- each finds the pairs that touch across the
    seam below it, and every rank computes the same merged table and the same plan and paints its own slab.  A rank
    without slices takes part with an empty slab."""
    from . import _hip
    from .inference import sharded
    max_voxels = _check_cap(max_voxels)
    rank, world = sharded._world(group)
    dev = slab.device
    if world == 1:
        lh = _hip.label_holes(slab, z_base=z_base)
        table, mine = lh.table, None
    else:
        below, above = sharded.neighbour_slices(slab, group)
        lh = _hip.label_holes(slab, below=below, above=above, z_base=z_base)
        tables = sharded._gather_var(lh.table, group)
        base = sum(int(t.shape[0]) for t in tables[:rank])
        if sum(int(t.shape[0]) for t in tables) > 0xffffffff:
            raise ValueError("fill_volume: the ranks' provisional cavities do not fit 32-bit ids")
        H, W = int(slab.shape[1]), int(slab.shape[2])
        ends = torch.zeros((2 if slab.shape[0] else 0, H, W), dtype=torch.uint32, device=dev)
        if slab.shape[0] and lh.n:
            ids = base + 1 + torch.arange(lh.n, dtype=torch.int64, device=dev)
            ends = torch.stack([lh.paint_slice(ids, z).view(torch.int32) for z in (0, int(slab.shape[0]) - 1)])
            ends = ends.view(torch.uint32)
        below_ids, _ = sharded.neighbour_slices(ends, group)
        if below is not None and slab.shape[0]:
            seam = seam_pairs(_is_zero(below), below_ids, _is_zero(slab[0]), ends[0], 6)
        else:
            seam = torch.zeros((0, 2), dtype=torch.int64, device=dev)
        seams = sharded._gather_var(seam.contiguous(), group)
        table, index = merge_blocks(tables, seams, return_index=True)
        mine = index[base:base + lh.n]
    lut, stats = plan(table, shape3d, max_voxels)
    lut = torch.from_numpy(lut.astype(np.int64)).to(dev)
    if mine is not None:
        lut = lut[mine]
    lh.paint(lut)
    return slab, stats
