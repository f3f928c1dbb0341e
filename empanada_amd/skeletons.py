"""Skeletons of the labelled objects (include/emp_hip.h, E8).

Length, branching and thickness along the centreline are what organelle morphometry -- mitochondrial network analysis
above all -- reports; users of the reference get them from kimimaro or skimage.morphology.skeletonize, object by object
on the host.  Here the thinning, the graph and the radius run on the device (_hip.label_thin / LabelThin,
_hip.label_graph, _hip.graph_finish, _hip.label_edt) and this module holds what is left: reading the `skeleton` argument
(`check`), the thinning and the skeleton of one class over several ranks (`thin_volume`, `skeleton_volume`) and what a
user does with the arrays (`derive`, `object_skeleton`, `write_obj`).

A skeleton is a dict of five arrays: 'vertices' (nv, 3) int32 in zyx order, the voxels that the thinning leaves,
ascending by (label, z, y, x); 'degree' (nv,) int32, the number of 26-neighbours of the vertex's label; 'radius2' (nv,)
the capped squared Euclidean distance of the vertex to the nearest voxel outside its object in the ORIGINAL volume, in
units of the sampling (a value at the cap means "at least r_cap"); 'edges' (ne, 2) int32 with i < j, one per pair of
26-adjacent vertices of one label; and 'objects' (n, 8) int64 rows of OBJECT_COLUMNS, ascending by label.

The thinning is topological: per label the 26-components, cavities and tunnels of the object are those of its
skeleton.  A solid with a cavity therefore keeps a closed shell around it: run fill_holes= first.  It is not
idempotent -- thinning a skeleton again eats its curves from their ends.

Not built: pruning of short branches, SWC / neuroglancer precomputed skeletons, surface (2-D isthmus) skeletons and
anisotropic thinning (the sampling is used for the radius only; the thinning is on the voxel lattice).
"""
import numpy as np

__all__ = ['OBJECT_COLUMNS', 'R_CAP', 'check', 'thin_volume', 'skeleton_volume', 'derive', 'object_skeleton',
           'write_obj']

OBJECT_COLUMNS = ('label', 'v_begin', 'v_end', 'e_begin', 'e_end', 'isolated', 'ends', 'junctions')
R_CAP = 64
CAP_MAX = 65535


def check(skeleton):
    """infer_volume's `skeleton` argument -> None or (r_cap, cap, sampling).  skeleton: None, True (r_cap = 64, sampling
    (1, 1, 1)), r_cap, or (r_cap, (az, ay, ax)).  r_cap is the largest radius reported, a positive real in the units of
    the sampling, read as morphology.check reads a radius: cap = floor(r_cap^2 + 1e-9) must lie in 1 .. 65535.  The
    sampling is three integers in 1 .. 16.  Everything else is a ValueError."""
    from .morphology import check_cap
    return check_cap("skeleton", skeleton, R_CAP, cap_max=CAP_MAX)


def thin_volume(slab, group=None, z_base=0, info=None):
    """The skeleton S of ONE volume whose consecutive z-slabs the ranks of `group` hold: the rank's part of it, a new
    (d, H, W) tensor of the slab's dtype.  The ranks run the mark step and the eight passes in lock-step; before each
    of them every rank fetches ONE end slice of state per side from the ranks next to it (sharded.neighbour_slices on
    the uint8 state; the labels' end slices are fetched once), the deleted count is summed once per iteration and all
    ranks stop together.  A rank without slices takes part.  More than max(volume's shape) + 2 iterations is a
    RuntimeError.  info: a dict that receives LabelThin's counts."""
    from . import _hip
    from .inference import sharded
    if not slab.is_contiguous():
        slab = slab.contiguous()
    world = sharded._world(group)[1]
    if world == 1:
        return _hip.label_thin(slab, z_base=int(z_base), info=info)
    thin = _hip.LabelThin(slab, int(z_base), info=info)
    lab_below, lab_above = sharded.neighbour_slices(slab, group)

    def halo():
        st_below, st_above = sharded.neighbour_slices(thin.state, group)
        return (None if lab_below is None else (lab_below, st_below),
                None if lab_above is None else (lab_above, st_above))

    dims = sharded._all_reduce_sum(np.asarray([slab.shape[0]], np.int64), group)
    limit = max(int(dims[0]), int(slab.shape[1]), int(slab.shape[2])) + 2
    while True:
        thin.mark(*halo())
        for s in range(8):
            thin.run_pass(s, *halo())
        fresh = int(sharded._all_reduce_sum(np.asarray([thin.deleted()], np.int64), group)[0])
        if fresh == 0:
            break
        if thin.iterations >= limit:
            raise RuntimeError(f"thin_volume: not settled after {limit} iterations")
    if info is not None:
        info['voxels_deleted'] = thin.voxels_deleted
    return thin.paint()


def skeleton_volume(slab, group=None, z0=0, depth=None, cap=R_CAP * R_CAP, sampling=(1, 1, 1), info=None):
    """The skeleton of ONE volume whose consecutive z-slabs the ranks of `group` hold: {'vertices', 'degree', 'radius2',
    'edges', 'objects'} as device tensors, the whole skeleton and the same on every rank.  slab: the rank's (d, H, W)
    slab on the device, uint8 or int32 / uint32; z0: its first slice; depth: the volume's depth (None: z0 + d, a single
    rank's whole volume).  thin_volume thins it; every rank emits the vertices and edges of its part of S with the end
    slices of the ranks next to it (sharded.neighbour_slices), reads the capped squared distance of the ORIGINAL slab
    (_hip.label_edt with `cap` and `sampling`, the halo from morphology.halo_slices / sharded.neighbour_slabs) at its
    vertices, the records are all-gathered in rank order -- which is z order -- and every rank finishes the same graph;
    the radius travels with the sorted permutation."""
    import torch
    from . import _hip
    from .inference import sharded
    from .morphology import halo_slices
    d, H, W = (int(s) for s in slab.shape)
    z0 = int(z0)
    depth = z0 + d if depth is None else int(depth)
    if not slab.is_contiguous():
        slab = slab.contiguous()
    stats = {} if info is None else info
    skel = thin_volume(slab, group, z0, info=stats)
    below, above = sharded.neighbour_slices(skel, group)
    (vkeys, vdeg), (ekeys, ecodes) = _hip.label_graph(skel, below=below, above=above, z_base=z0, depth=depth)
    lo, hi = sharded.neighbour_slabs(slab, halo_slices('erode', max(int(cap) - 1, 0), sampling), group)
    edt = _hip.label_edt(slab, sampling, int(cap), below=lo, above=hi)
    at = (vkeys & 0xffffffff) - z0 * H * W
    # torch indexes few uint16 tensors: the bits are gathered as int16 and widened
    radius2 = (edt.view(torch.int16).reshape(-1)[at].to(torch.int32) & 0xffff) if vkeys.numel() else \
        torch.zeros((0,), dtype=torch.int32, device=slab.device)
    if sharded._world(group)[1] > 1:
        vkeys, vdeg, radius2, ekeys, ecodes = (torch.cat(sharded._gather_var(t, group))
                                               for t in (vkeys, vdeg, radius2, ekeys, ecodes))
    vertices, degree, edges, objects, order = _hip.graph_finish((vkeys, vdeg), (ekeys, ecodes), (depth, H, W))
    return {'vertices': vertices, 'degree': degree, 'radius2': radius2[order.long()], 'edges': edges,
            'objects': objects}


def _objects(skel):
    return np.asarray(skel['objects']).reshape(-1, len(OBJECT_COLUMNS))


def derive(skel, spacing=(1, 1, 1)):
    """Per object, in float64 on the host: {'label', 'length', 'ends', 'junctions', 'isolated', 'mean_radius',
    'max_radius'}, arrays with one entry per row of skel['objects'].  length: the sum of the Euclidean lengths of the
    object's edges with the voxel pitch `spacing` (z, y, x).  26-adjacent voxels around a junction form small cliques
    (triangles of mutually adjacent voxels), so the edge sum overestimates the length there, by up to a voxel diagonal
    per junction.  The radii are sqrt(radius2), in the units of the sampling the skeleton was made with; a radius at the
    cap means "at least r_cap"."""
    spacing = np.asarray(spacing, dtype=np.float64)
    if spacing.shape != (3,) or not np.all(np.isfinite(spacing)) or np.any(spacing <= 0):
        raise ValueError(f"derive: spacing must be three positive numbers (z, y, x), got {spacing!r}")
    objects = _objects(skel)
    v = np.asarray(skel['vertices']).reshape(-1, 3).astype(np.float64) * spacing
    e = np.asarray(skel['edges']).reshape(-1, 2)
    r = np.sqrt(np.asarray(skel['radius2'], dtype=np.float64).reshape(-1))
    if len(e) and (e.min() < 0 or e.max() >= len(v)):
        raise ValueError("derive: an edge points outside the vertices")
    seg = np.sqrt(((v[e[:, 1]] - v[e[:, 0]]) ** 2).sum(1)) if len(e) else np.zeros(0)
    n = len(objects)
    out = {'label': objects[:, 0].copy(), 'length': np.zeros(n), 'ends': objects[:, 6].copy(),
           'junctions': objects[:, 7].copy(), 'isolated': objects[:, 5].copy(), 'mean_radius': np.zeros(n),
           'max_radius': np.zeros(n)}
    for i, (_, v0, v1, e0, e1) in enumerate(objects[:, :5]):
        out['length'][i] = seg[e0:e1].sum()
        if v1 > v0:
            out['mean_radius'][i] = r[v0:v1].mean()
            out['max_radius'][i] = r[v0:v1].max()
    return out


def object_skeleton(skel, label):
    """one object of a skeleton: (vertices, degree, radius2, edges) with the indices rebased to the object's first
    vertex.  A label that the skeleton does not hold is a KeyError."""
    objects = _objects(skel)
    row = np.searchsorted(objects[:, 0], label)
    if row == len(objects) or objects[row, 0] != label:
        raise KeyError(f"object_skeleton: the skeleton holds no object with label {label!r}")
    _, v0, v1, e0, e1 = (int(v) for v in objects[row, :5])
    return (np.asarray(skel['vertices'])[v0:v1], np.asarray(skel['degree'])[v0:v1], np.asarray(skel['radius2'])[v0:v1],
            np.asarray(skel['edges'])[e0:e1] - v0)


def write_obj(path, skel, label=None):
    """A plain Wavefront OBJ of the skeleton, or of one object of it: 'v x y z' lines -- the vertices' columns reversed,
    as meshes.write_obj writes them -- and 'l a b' lines with 1-based indices.  With label=None the objects follow each
    other as 'o <label>' groups."""
    if label is None:
        vertices, edges = np.asarray(skel['vertices']).reshape(-1, 3), np.asarray(skel['edges']).reshape(-1, 2)
        groups = [(int(r[0]), int(r[3]), int(r[4])) for r in _objects(skel)]
    else:
        vertices, _, _, edges = object_skeleton(skel, label)
        groups = [(int(label), 0, len(edges))]
    with open(path, 'w') as f:
        f.write(f"# {len(vertices)} vertices, {len(edges)} edges, x y z\n")
        np.savetxt(f, vertices[:, ::-1], fmt='v %d %d %d')
        for name, e0, e1 in groups:
            f.write(f"o {name}\n")
            np.savetxt(f, edges[e0:e1].astype(np.int64) + 1, fmt='l %d %d')
