"""Separate touching objects: erosion cores regrown by geodesic growth (include/emp_hip.h, E6).

Two objects that touch come out of the consensus under one id.  split_objects= only separates pieces that are already
disconnected and an opening changes every surface, so users of the reference erode the object, label the cores that
remain and grow them back inside the original object -- a watershed on the binary mask -- on a CPU.  Here the voxel
passes run on the device (_hip.label_erode, _hip.label_components, _hip.label_grow) and this module holds what is
left: reading the `separate` argument (`check`), deciding on O(#cores) tables which piece keeps the label and which
gets a new one (`plan`), and the whole repair of one class's slab, several ranks included (`separate_volume`).
"""
import numbers

import numpy as np
import torch

__all__ = ['check', 'plan', 'grow_volume', 'separate_volume']

_MAX_LABEL = 2 ** 32 - 1


def _check_min_core(min_core):
    if isinstance(min_core, (bool, np.bool_)) or not isinstance(min_core, numbers.Integral) or min_core < 1:
        raise ValueError(f"separate: min_core must be an integer >= 1, got {min_core!r}")
    return int(min_core)


def check(separate):
    """infer_volume's `separate` argument -> None or (r2, min_core, sampling).  separate: None, r, (r, min_core) or
    (r, min_core, (az, ay, ax)).  r, a real radius in the units of the sampling, and the sampling, three integers in
    1 .. 16 (default (1, 1, 1)), are read exactly as morphology.check reads an erosion's: r2 = floor(r^2 + 1e-9) in
    min(sampling)^2 .. 65534.  min_core, an integer >= 1 (default 1), is the smallest core in voxels that counts as a
    seed -- the role seed_thres plays in the reference.  Everything else is a ValueError."""
    from . import morphology
    if separate is None:
        return None
    if isinstance(separate, (tuple, list)):
        if len(separate) not in (2, 3):
            raise ValueError(f"separate must be None, r, (r, min_core) or (r, min_core, (az, ay, ax)), got {separate!r}")
        r, min_core, pitch = separate[0], _check_min_core(separate[1]), tuple(separate[2:])
    else:
        r, min_core, pitch = separate, 1, ()
    if isinstance(r, (str, bytes)):
        raise ValueError(f"separate must be None, r, (r, min_core) or (r, min_core, (az, ay, ax)), got {separate!r}")
    r2, sampling = morphology.check_radius("separate", r, *pitch)
    return r2, min_core, sampling


def plan(pieces, top, max_label=_MAX_LABEL):
    """What every piece is painted with: (lut, stats).  pieces: rows of (label, seed id, voxels), the pieces that the
    growth made of the candidate labels; the seed ids are 1 .. n, each once.  top: the class's largest label over all
    ranks.  lut (uint32 numpy, n + 1 entries, entry 0 unused) holds the label per seed id.  Per label, ascending, the
    pieces are ordered by (voxels descending, seed id ascending); the first keeps the label and every further piece gets
    top + 1, top + 2, ... in that order: components.plan's rule with the class's maximum in place of the table's.
    stats: 'objects_separated' (distinct labels among the pieces), 'pieces_added' (new labels handed out) and
    'voxels_moved' (the voxels of the pieces that got one).  A new label above max_label (2^32 - 1; 255 for a uint8
    slab) is a ValueError."""
    p = np.asarray(pieces, dtype=np.int64).reshape(-1, 3)
    n = len(p)
    if isinstance(top, (bool, np.bool_)) or not isinstance(top, numbers.Integral) or not 0 <= top <= _MAX_LABEL:
        raise ValueError(f"plan: top must be an integer in 0 .. {_MAX_LABEL}, got {top!r}")
    lut = np.zeros(n + 1, np.uint32)
    if n == 0:
        return lut, dict(objects_separated=0, pieces_added=0, voxels_moved=0)
    if sorted(p[:, 1].tolist()) != list(range(1, n + 1)):
        raise ValueError(f"plan: the seed ids must be 1 .. {n}, each once")
    if p[:, 0].min() < 1 or p[:, 0].max() > top:
        raise ValueError(f"plan: labels outside 1 .. top = {int(top)}")
    if p[:, 2].min() < 0:
        raise ValueError("plan: negative voxel counts")
    order = np.lexsort((p[:, 1], -p[:, 2], p[:, 0]))           # by label, then voxels descending, then seed id
    lab = p[order, 0]
    head = np.ones(n, bool)
    head[1:] = lab[1:] != lab[:-1]
    n_new = int((~head).sum())
    if int(top) + n_new > max_label:
        raise ValueError(f"plan: {n_new} new labels above the largest label {int(top)} would pass {max_label}")
    value = lab.copy()
    value[~head] = int(top) + 1 + np.arange(n_new)
    lut[p[order, 1]] = value.astype(np.uint32)
    stats = dict(objects_separated=int(head.sum()), pieces_added=n_new, voxels_moved=int(p[order, 2][~head].sum()))
    return lut, stats


def _seeds(table, min_core):
    """(seed id per row of the merged core table, 0 = no seed; label per seed id) -- a label is a candidate if it has
    two or more cores of at least min_core voxels, and its cores of that size become seeds, numbered from 1 ascending
    by the core's first voxel (the table's own order)"""
    t = table.cpu().numpy() if isinstance(table, torch.Tensor) else np.asarray(table)
    t = t.reshape(-1, 9)
    big = t[:, 1] >= min_core
    labels, counts = np.unique(t[big, 0], return_counts=True)
    seed = big & np.isin(t[:, 0], labels[counts >= 2])
    ids = np.zeros(len(t), np.int64)
    ids[seed] = 1 + np.arange(int(seed.sum()))
    return ids, t[seed, 0]


def grow_volume(slab, seeds, group=None, neighbours=None):
    """_hip.label_grow of a rank's (d, H, W) slab and seeds where the ranks of `group` hold consecutive z-slabs of ONE
    volume: the LabelGrow of this rank's part of the undivided volume's growth.  Every rank grows its own slab, then
    each round exchanges one end slice of state per side (sharded.neighbour_slices on the 64-bit keys), sweeps on with
    them (LabelGrow.resume) and all ranks reduce whether any key fell: they stop together after a round in which none
    did.  neighbours: the slab's (below, above) label slices if the caller has fetched them already."""
    from . import _hip
    from .inference import sharded
    grown = _hip.label_grow(slab, seeds)
    if sharded._world(group)[1] == 1:
        return grown
    lab_below, lab_above = sharded.neighbour_slices(slab, group) if neighbours is None else neighbours
    while True:
        key_below, key_above = sharded.neighbour_slices(grown.state, group)
        fell = grown.resume(None if lab_below is None or key_below is None else (lab_below, key_below),
                            None if lab_above is None or key_above is None else (lab_above, key_above))
        if int(sharded._all_reduce_sum(np.asarray([int(fell)], np.int64), group)[0]) == 0:
            return grown


def separate_volume(slab, shape3d, r2, min_core=1, sampling=(1, 1, 1), connectivity=6, group=None, z_base=0):
    """The repair of one class: (slab, stats).  slab: a rank's (d, H, W) device slab holding the slices [z_base,
    z_base + d) of the volume `shape3d` = (D, H, W), uint8 or int32 / uint32, contiguous; it is painted in place.  r2,
    min_core, sampling: what `check` returns.  The steps: 1. the erosion E of the slab by the ball of squared radius r2
    (_hip.label_erode, the ranks' halos from sharded.neighbour_slabs); 2. the cores, E's components of `connectivity`
    (_hip.label_components, the table merged over the ranks by components.merged_table); 3. a label with two or more
    cores of at least min_core voxels is a candidate and those cores become seeds, numbered from 1 by first voxel; every
    other label gets no seed and stays exactly as it is -- without a candidate on any rank the slab is returned as it
    is and no growth is launched; 4. the seeds grow back inside their label (_hip.label_grow); with `group` the ranks
    hold consecutive z-slabs of ONE volume, exchange one end slice of state per side and round (sharded.neighbour_slices)
    and stop together when no rank's keys fell; 5. the pieces' exact sizes (_hip.measure_labels of the owners, summed
    over the ranks); 6. `plan`, then the paint in place.  A voxel of a candidate label that no seed reaches -- a crumb
    without a core of its own -- keeps the label; split_objects=, which runs next in infer_volume, deals with it.  A new
    label that the slab's dtype cannot hold is a ValueError before anything is painted.  stats: {'r2', 'min_core',
    'sampling', 'objects_in' (distinct labels), 'objects_separated' (candidate labels), 'pieces_added', 'voxels_moved'
    (voxels whose label changed), 'sweeps' (summed over the ranks)}, the same on every rank.  A rank without slices takes
    part with an empty slab."""
    from . import _hip, components, morphology
    from .inference import sharded
    from .measurements import gather_tables
    sampling = morphology.check_sampling("morph", sampling)
    min_core = _check_min_core(min_core)
    connectivity = components._check_connectivity(connectivity)
    if len(shape3d) != 3 or any(int(s) < 0 for s in shape3d):
        raise ValueError(f"separate_volume: shape3d must be (D, H, W), got {shape3d!r}")
    r2, z_base = int(r2), int(z_base)
    dev = slab.device
    below, above = sharded.neighbour_slabs(slab, morphology.halo_slices('erode', r2, sampling), group)
    eroded = _hip.label_erode(slab, r2, sampling, below=below, above=above)
    del below, above
    cores = _hip.label_components(eroded, connectivity, z_base=z_base)
    table, mine = components.merged_table(cores, connectivity, group, "separate_volume")
    ids, seed_labels = _seeds(table, min_core)
    lab_below, lab_above = sharded.neighbour_slices(slab, group)
    whole = gather_tables(_hip.measure_labels(slab, below=lab_below, above=lab_above, z_base=z_base), group)
    top = int(whole[-1, 0]) if whole.shape[0] else 0
    stats = dict(r2=r2, min_core=min_core, sampling=sampling, objects_in=int(whole.shape[0]), objects_separated=0,
                 pieces_added=0, voxels_moved=0, sweeps=0)
    n_seeds = len(seed_labels)
    if n_seeds == 0:
        return slab, stats
    core_ids = torch.from_numpy(ids).to(dev)
    seeds = cores.paint(core_ids if mine is None else core_ids[mine], dtype=torch.uint32)
    del cores, eroded
    grown = grow_volume(slab, seeds, group, (lab_below, lab_above))
    del seeds
    sizes = np.zeros(n_seeds + 1, np.int64)
    if slab.numel():
        owned = _hip.measure_labels(grown.owners())[:, :2].cpu().numpy()
        sizes[owned[:, 0]] = owned[:, 1]
    sizes = sharded._all_reduce_sum(sizes, group)
    pieces = np.stack([seed_labels, 1 + np.arange(n_seeds), sizes[1:]], axis=1)
    lut, planned = plan(pieces, top, 255 if slab.dtype == torch.uint8 else _MAX_LABEL)
    grown.paint(lut, out=slab)
    stats.update(planned, sweeps=int(sharded._all_reduce_sum(np.asarray([grown.sweeps], np.int64), group)[0]))
    return slab, stats
