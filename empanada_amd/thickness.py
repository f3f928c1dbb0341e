"""Local thickness of the labelled objects: how thick an object is, and where (include/emp_hip.h, E10).

The diameter distribution tells swollen mitochondria from constricted ones, tubules differ from sheets by their
thickness and a constriction site is a local minimum of it: every morphometric study of organelles reports it.  Users
of the reference get it on a CPU afterwards, from ImageJ / BoneJ "Local Thickness" or an edt per object.  Here the map
is computed on the device (_hip.label_thickness, csrc/emp_label_thick.hip), slab by slab, rank by rank: T2(p) is the
largest capped squared distance d2(q) (_hip.label_edt's) among the voxels q whose ball |p - q|^2 < d2(q) covers p -- the
largest inscribed ball that COVERS the voxel (Hildebrand and Ruegsegger), not the one centred on it.  The diameter is
2 sqrt(T2) in units of the sampling; it carries the voxel-centre bias of the edt (a line one voxel wide reads 2, as
ImageJ's plug-in does) and nothing corrects for it.  The cap is part of the definition: a ball whose true radius
exceeds it is shrunk to it and covers less, so the result for a cap is not the uncapped one clamped -- 'capped', the
number of voxels with d2 == cap, says whether it bit (0: the result is the uncapped one).

The table is the exact sparse histogram of the map per object: rows (label, t2, voxels) ascending by (label, t2), the
label as an unsigned 32-bit value.  The voxel counts of the z-blocks of a volume -- each computed with its
halo_slices() true neighbour slices per side -- add up to the table of the whole (`merge_tables`), whatever the
partition.  `derive` and `histogram` turn a table into diameters on the host.

Not built: a masked or calibrated thickness that removes the voxel bias, thickness of the background ("separation"),
radii above sqrt(65535), compressed output of the uint16 map, a pyramid of the map.
"""
import math

import numpy as np
import torch

from .tables import _labels_to_device, gather_keyed, merge_keyed, volume_device, volume_slabs, volume_table

__all__ = ['COLUMNS', 'R_CAP', 'check', 'halo_slices', 'merge_tables', 'gather_tables', 'thickness_volume', 'derive',
           'histogram', 'volume_thickness']

COLUMNS = ('label', 't2', 'voxels')
R_CAP = 32
CAP_MAX = 65535


def check(thickness):
    """infer_volume's `thickness` argument -> None or (r_cap, cap, sampling).  thickness: None, True (r_cap = 32, sampling
    (1, 1, 1)), r_cap, or (r_cap, (az, ay, ax)).  r_cap is the largest radius reported, a real number >= 1 in the units
    of the sampling, read as skeletons.check reads it: cap = floor(r_cap^2 + 1e-9) must lie in 1 .. 65535.  The sampling
    is three integers in 1 .. 16.  Everything else is a ValueError."""
    from .morphology import check_cap
    return check_cap("thickness", thickness, R_CAP, at_least=1, cap_max=CAP_MAX)


def halo_slices(cap, sampling=(1, 1, 1)):
    """slices of its neighbours that a z-slab needs on either side: 2 h with h = floor(sqrt(cap - 1)) // az -- the map of
    the slab needs d2 on h slices, and that d2 needs labels on h more"""
    return 2 * (math.isqrt(int(cap) - 1) // int(sampling[0]))


def merge_tables(tables):
    """Merge of thickness tables ((m, 3) int64 each, of a volume's z-blocks or of the ranks' slabs): one row per distinct
    (label, t2), ascending by (label, t2) with the label as an unsigned 32-bit value, the voxels added.  numpy in, numpy
    out; with any torch tensor among them the result is a torch table on that tensor's device.  No tables, or empty
    ones, give a (0, 3) table."""
    return merge_keyed(tables, len(COLUMNS), [0, 1], [2])


def gather_tables(table, group=None):
    """The ranks' tables merged: every rank of `group` passes the table of its own slab and receives the table of all of
    them (one count all-gather + one padded all-gather, as contacts.gather_tables).  Without an initialised process
    group the table comes back merged with itself, i.e. sorted."""
    return gather_keyed(table, len(COLUMNS), merge_tables, group)


def thickness_volume(slab, group=None, cap=R_CAP * R_CAP, sampling=(1, 1, 1), info=None):
    """The thickness of ONE volume whose consecutive z-slabs the ranks of `group` hold: (t2, table).  t2 is the map of
    the rank's own slab, (d, H, W) uint16 on its device; table is that of the WHOLE volume, (m, 3) int64 on the device,
    the same on every rank.  Every rank fetches halo_slices() slices per side from the ranks next to it
    (sharded.neighbour_slabs), so the map equals the slab of the undivided volume's.  A rank without slices takes part.
    info: a dict that receives _hip.label_thickness' counts, 'capped' summed over the ranks."""
    from . import _hip
    from .inference import sharded
    if not slab.is_contiguous():
        slab = slab.contiguous()
    below, above = sharded.neighbour_slabs(slab, halo_slices(cap, sampling), group)
    stats = {} if info is None else info
    t2, table = _hip.label_thickness(slab, cap, sampling, below=below, above=above, info=stats)
    stats['capped'] = int(sharded._all_reduce_sum(np.asarray([stats['capped']], np.int64), group)[0])
    return t2, gather_tables(table, group)


def _rows(table):
    if isinstance(table, torch.Tensor):
        table = table.cpu().numpy()
    t = np.asarray(table, dtype=np.int64).reshape(-1, len(COLUMNS))
    return merge_tables([t])                                   # sorted by (label, t2), one row per pair


def _unit(unit):
    try:
        unit = float(unit)
    except (TypeError, ValueError):
        unit = float('nan')
    if not (np.isfinite(unit) and unit > 0):
        raise ValueError("thickness: unit must be a positive number")
    return unit


def derive(table, unit=1.0):
    """Per object of a thickness table ((m, 3) int64, numpy or torch), the diameter 2 sqrt(t2) * unit -- one unit of the
    sampling is `unit` long (nm, say) -- over its voxels; no GPU is needed.  Returns a dict of numpy arrays, one entry per
    label ascending: 'label', 'voxels' (int64) and, float64, 'mean', 'std' (of the population, as numpy.std), 'min',
    'median' (as numpy.median of the voxels' values: the mean of the two middle ones for an even count) and 'max'."""
    unit = _unit(unit)
    t = _rows(table)
    labels, first = np.unique(t[:, 0], return_index=True)
    n = len(labels)
    out = {'label': labels, 'voxels': np.zeros(n, np.int64)}
    for k in ('mean', 'std', 'min', 'median', 'max'):
        out[k] = np.zeros(n, np.float64)
    ends = list(first[1:]) + [len(t)]
    for i, (a, b) in enumerate(zip(first, ends)):
        diam = 2.0 * np.sqrt(t[a:b, 1].astype(np.float64)) * unit          # ascending, as t2 is
        w = t[a:b, 2]
        total = int(w.sum())
        cum = np.cumsum(w)
        mean = float((diam * w).sum() / total)
        lo = diam[np.searchsorted(cum, (total - 1) // 2 + 1)]
        hi = diam[np.searchsorted(cum, total // 2 + 1)]
        out['voxels'][i] = total
        out['mean'][i] = mean
        out['std'][i] = math.sqrt(max(float((w * (diam - mean) ** 2).sum() / total), 0.0))
        out['min'][i] = diam[0]
        out['median'][i] = 0.5 * (lo + hi)
        out['max'][i] = diam[-1]
    return out


def histogram(table, edges, unit=1.0):
    """Voxel counts per diameter bin and object: {'label': the labels ascending, 'counts': (labels, len(edges) - 1)
    int64}.  edges: ascending bin edges of the diameter 2 sqrt(t2) * unit, read as numpy.histogram reads them (a bin
    holds its left edge, the last one its right edge too); voxels outside the edges are not counted."""
    unit = _unit(unit)
    edges = np.asarray(edges, dtype=np.float64).reshape(-1)
    if len(edges) < 2 or not np.all(np.isfinite(edges)) or np.any(np.diff(edges) <= 0):
        raise ValueError(f"histogram: edges must be at least two ascending finite numbers, got {edges!r}")
    t = _rows(table)
    labels, inv = np.unique(t[:, 0], return_inverse=True)
    counts = np.zeros((len(labels), len(edges) - 1), np.int64)
    diam = 2.0 * np.sqrt(t[:, 1].astype(np.float64)) * unit
    b = np.searchsorted(edges, diam, side='right') - 1
    b[diam == edges[-1]] = len(edges) - 2
    ok = (b >= 0) & (b < len(edges) - 1)
    np.add.at(counts, (inv.reshape(-1)[ok], b[ok]), t[ok, 2])
    return {'label': labels, 'counts': counts}


def volume_thickness(labels, *, r_cap=R_CAP, sampling=(1, 1, 1), slab_rows=None, group=None, out=None):
    """The thickness of a label volume (D, H, W) that is already there: (t2, table, capped).  `labels` is a numpy array,
    a tensor or anything that has a shape and can be sliced along axis 0 (a ZarrV2Array, say).  r_cap and sampling are
    read as `check` reads them.  Every slab of slab_rows slices goes to the device together with halo_slices() slices on
    either side (host data is uploaded slab by slab, so the volume need not be resident as a whole) and through
    _hip.label_thickness; slab_rows=None takes a device tensor whole and host data in slabs of about 2^27 voxels.  t2 is
    the (D, H, W) uint16 map as a numpy array, or `out` -- anything of that shape that takes out[z0:z1] = array -- when
    one is given; table is the (m, 3) int64 numpy table and capped the number of voxels with d2 == cap.  With `group`
    the tables and capped are merged too: every rank passes a volume of its own; ranks that hold the z-slabs of ONE
    volume call thickness_volume instead."""
    from . import _hip
    from .inference import sharded
    _, cap, sampling = check((r_cap, sampling))
    if len(labels.shape) != 3:
        raise ValueError(f"volume_thickness: labels must be (D, H, W), got {tuple(labels.shape)}")
    shape = tuple(int(s) for s in labels.shape)
    if out is not None and tuple(out.shape) != shape:
        raise ValueError(f"volume_thickness: out is {tuple(out.shape)}, labels {shape}")
    _hip.require_gpu()
    dev, resident = volume_device(labels)
    t2 = np.zeros(shape, np.uint16) if out is None else out
    tables, capped = [], 0
    for z, z1, lo, hi in volume_slabs("volume_thickness", shape, slab_rows, resident, halo_slices(cap, sampling)):
        ext = _labels_to_device(labels[lo:hi], dev)             # one upload covers the slab and its halo on both sides
        core = ext[z - lo:z1 - lo]
        if core.numel():
            stats = {}
            part, table = _hip.label_thickness(core, cap, sampling, below=ext[:z - lo] if z > lo else None,
                                               above=ext[z1 - lo:] if hi > z1 else None, info=stats)
            t2[z:z1] = part.view(torch.int16).cpu().numpy().view(np.uint16)
            tables.append(table)
            capped += stats['capped']
        del ext, core
    capped = int(sharded._all_reduce_sum(np.asarray([capped], np.int64), group)[0])
    return t2, volume_table(tables, len(COLUMNS), merge_tables, gather_tables, group, dev), capped
