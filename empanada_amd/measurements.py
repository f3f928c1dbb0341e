"""Per-object measurements of a labelled volume: voxels, bounding box, centroid and surface area of every label.

The reference stops at the labelled volume (scripts/pdl_inference3d.py:225-233); its trackers carry boxes and runs per
plane only (inference/tracker.py:61-123).  The table is defined in include/emp_hip.h (E2) and read on the device by
_hip.measure_labels (csrc/emp_measure.hip), slab by slab, rank by rank: one row of 14 int64 per distinct non-zero label,
ascending by label, the columns being COLUMNS.  Columns 1 and 8..13 are sums and 2..7 minima / maxima of integers, so
tables of the z-blocks of a volume -- each measured with its true neighbour slices -- merge into the table of the whole
(`merge_tables`), whatever the partition and the order.  `derive` turns a table into physical quantities on the host.
"""
import numpy as np
import torch

from .tables import (_labels_to_device, bits, gather_keyed, merge_keyed, volume_device, volume_slabs,
                     volume_table)

__all__ = ['COLUMNS', 'merge_tables', 'gather_tables', 'volume_measurements', 'derive']

COLUMNS = ('label', 'voxels', 'z0', 'y0', 'x0', 'z1', 'y1', 'x1', 'sum_z', 'sum_y', 'sum_x',
           'faces_z', 'faces_y', 'faces_x')
_SUM = [1, 8, 9, 10, 11, 12, 13]
_MIN = [2, 3, 4]
_MAX = [5, 6, 7]


def merge_tables(tables):
    """Merge of measurement tables ((n, 14) int64 each, of a volume's z-blocks or of the ranks' slabs): one row per
    distinct label, ascending by label, columns 1 and 8..13 added, 2..4 the minimum and 5..7 the maximum.  numpy in,
    numpy out; with any torch tensor among them the result is a torch table on that tensor's device.  No tables, or
    empty ones, give a (0, 14) table.  Integer sums, minima and maxima: exact whatever the order."""
    return merge_keyed(tables, len(COLUMNS), [0], _SUM, _MIN, _MAX)


def gather_tables(table, group=None):
    """The ranks' tables merged: every rank of `group` passes the table of its own slab and receives the table of all of
    them (one count all-gather + one padded all-gather, as the overlap tables travel in evaluation.gather_overlaps).
    Without an initialised process group the table comes back merged with itself, i.e. sorted."""
    return gather_keyed(table, len(COLUMNS), merge_tables, group)


def volume_measurements(labels, *, slab_rows=None, group=None):
    """The measurement table of a label volume (D, H, W) as an (n, 14) int64 numpy array: `labels` is a numpy array, a
    tensor or anything that has a shape and can be sliced along axis 0 (a ZarrV2Array, say).  Every slab of slab_rows
    slices goes to the device (host data is uploaded slab by slab, so the volume need not be resident as a whole) and
    through _hip.measure_labels together with the slices next to it, which stand for what lies outside the slab;
    slab_rows=None takes a device tensor whole and host data in slabs of about 2^27 voxels.  With `group` the ranks'
    tables are merged too -- every rank passes a volume of its own and all receive the merge; ranks that hold the
    z-slabs of ONE volume must hand each slab its neighbour slices themselves (_hip.measure_labels' below / above, as
    infer_volume does) and then call gather_tables."""
    from . import _hip
    _hip.require_gpu()
    if len(labels.shape) != 3:
        raise ValueError(f"volume_measurements: labels must be (D, H, W), got {tuple(labels.shape)}")
    dev, resident = volume_device(labels)
    tables, below = [], None
    for z, z1, _, hi in volume_slabs("volume_measurements", labels.shape, slab_rows, resident, halo=1):
        # one upload covers the slab and the slice above it; the slice below is kept from the slab before
        part = _labels_to_device(labels[z:hi], dev)
        slab = part[:z1 - z]
        above = part[z1 - z] if hi > z1 else None
        if slab.numel():
            tables.append(_hip.measure_labels(slab, below=below, above=above, z_base=z))
        if slab.shape[0]:                   # a copy of one slice, so that the slab itself can go (as int32: same bits)
            below = bits(slab[-1]).clone().view(slab.dtype)
        del part, slab, above
    return volume_table(tables, len(COLUMNS), merge_tables, gather_tables, group, dev)


def derive(table, spacing=(1.0, 1.0, 1.0)):
    """Physical quantities of a measurement table ((n, 14) int64, numpy or torch) for a voxel of `spacing` = (sz, sy, sx);
    no GPU is needed.  Returns a dict of numpy arrays:
        label         table[:, 0]
        voxels        table[:, 1]
        volume        voxels * sz * sy * sx                                          (float64)
        centroid      (n, 3): (sum_z, sum_y, sum_x) / voxels, in voxel indices       (float64 division)
        bbox          (n, 6): z0, y0, x0, z1, y1, x1 (the upper ends exclusive)      (int64)
        surface_area  faces_z * sy * sx + faces_y * sz * sx + faces_x * sz * sy      (float64)
    The products are formed left to right as written.  surface_area is the area of the exposed voxel faces (the
    "crack" area): exact, and additive over blocks and ranks, but it overestimates a smooth surface -- by up to 1.5 x
    for a sphere -- so no sphericity is derived from it."""
    if isinstance(table, torch.Tensor):
        table = table.cpu().numpy()
    t = np.asarray(table, dtype=np.int64).reshape(-1, len(COLUMNS))
    try:
        sz, sy, sx = (float(s) for s in spacing)
    except (TypeError, ValueError):
        raise ValueError(f"derive: spacing must be three positive numbers (sz, sy, sx), got {spacing!r}") from None
    if not all(np.isfinite(s) and s > 0 for s in (sz, sy, sx)):
        raise ValueError(f"derive: spacing must be three positive numbers (sz, sy, sx), got {spacing!r}")
    voxels = t[:, 1]
    return {'label': t[:, 0].copy(),
            'voxels': voxels.copy(),
            'volume': voxels * sz * sy * sx,
            'centroid': t[:, 8:11] / voxels[:, None].astype(np.float64),
            'bbox': t[:, 2:8].copy(),
            'surface_area': t[:, 11] * sy * sx + t[:, 12] * sz * sx + t[:, 13] * sz * sy}
