"""Surface meshes of the labelled objects (include/emp_hip.h, E7).

People look at the objects of a 3D EM segmentation as surfaces and export them to Blender, VAST, webKnossos or MeshLab;
users of the reference get them from skimage.measure.marching_cubes or zmesh, object by object on the host.  Here the
voxel passes, the sorts, the indexing and the smoothing run on the device (_hip.label_mesh, _hip.mesh_finish,
_hip.mesh_smooth) and this module holds what is left: reading the `mesh` argument (`check`), the mesh of one class over
several ranks (`mesh_volume`) and what a user does with the arrays (`triangles`, `object_mesh`, `write_obj`).

A mesh is a dict of three arrays: 'vertices' (nv, 3) in zyx order -- int32 corners of the voxel lattice, or float32 once
smoothed --, 'quads' (nq, 4) int32 indices into the vertices, wound counter-clockwise seen from outside in the (z, y, x)
frame, and 'objects' (n, 5) int64 rows of (label, v_begin, v_end, q_begin, q_end), ascending by label (OBJECT_COLUMNS).
The surface is the "crack" surface of the voxels: exact, closed, and as blocky as they are.  Where two voxels of one
object meet only along an edge or at a corner they share the vertices there, so such an edge carries four quads.

Not built: marching cubes / surface nets, simplification, splitting non-manifold edges, volumes above the limit of 2^32
lattice corners (about 1624^3), and neuroglancer's precomputed mesh format.
"""
import numbers

import numpy as np

__all__ = ['OBJECT_COLUMNS', 'check', 'mesh_volume', 'triangles', 'object_mesh', 'write_obj']

OBJECT_COLUMNS = ('label', 'v_begin', 'v_end', 'q_begin', 'q_end')


def check(mesh):
    """infer_volume's `mesh` argument -> None or the number of smoothing iterations.  mesh: None, True (no smoothing)
    or a non-negative integer (Taubin iterations).  Everything else is a ValueError."""
    if mesh is None:
        return None
    if mesh is True:
        return 0
    if isinstance(mesh, (bool, np.bool_)) or not isinstance(mesh, numbers.Integral) or mesh < 0:
        raise ValueError(f"mesh must be None, True or a non-negative number of smoothing iterations, got {mesh!r}")
    return int(mesh)


def mesh_volume(slab, group=None, z0=0, depth=None, iterations=0):
    """The mesh of ONE volume whose consecutive z-slabs the ranks of `group` hold: {'vertices', 'quads', 'objects'} as
    device tensors, the whole mesh and the same on every rank.  slab: the rank's (d, H, W) slab on the device, uint8 or
    int32 / uint32; z0: its first slice; depth: the volume's depth (None: z0 + d, a single rank's whole volume).  Each
    rank emits the keys and quads of its slab with the end slices of the ranks next to it standing for what lies outside
    it (sharded.neighbour_slices), the rank whose slab ends the volume also owns the last corner plane, keys and quads
    are all-gathered in rank order -- which is z order -- and every rank finishes the same mesh.  iterations > 0: Taubin
    smoothing on the device, float32 vertices."""
    from . import _hip
    from .inference import sharded
    if isinstance(iterations, (bool, np.bool_)) or not isinstance(iterations, numbers.Integral) or iterations < 0:
        raise ValueError(f"mesh_volume: iterations must be a non-negative integer, got {iterations!r}")
    d = int(slab.shape[0])
    depth = int(z0) + d if depth is None else int(depth)
    if not slab.is_contiguous():
        slab = slab.contiguous()
    below, above = sharded.neighbour_slices(slab, group)
    keys, (qkeys, qdirs) = _hip.label_mesh(slab, below=below, above=above, z_base=int(z0), depth=depth,
                                          top=int(z0) + d == depth)
    if sharded._world(group)[1] > 1:
        import torch
        keys, qkeys, qdirs = (torch.cat(sharded._gather_var(t, group)) for t in (keys, qkeys, qdirs))
    vertices, quads, objects = _hip.mesh_finish(keys, (qkeys, qdirs), (depth,) + tuple(slab.shape[1:]))
    if iterations:
        vertices = _hip.mesh_smooth(vertices, quads, iterations)
    return {'vertices': vertices, 'quads': quads, 'objects': objects}


def triangles(quads):
    """(2 nq, 3): every quad (v0, v1, v2, v3) as the triangles (v0, v1, v2), (v0, v2, v3), same winding"""
    q = np.asarray(quads)
    if q.ndim != 2 or q.shape[1] != 4:
        raise ValueError(f"triangles: quads must be (nq, 4), got {q.shape}")
    return q[:, [0, 1, 2, 0, 2, 3]].reshape(-1, 3)


def object_mesh(mesh, label):
    """one object of a mesh: (vertices, quads) with the indices rebased to the object's first vertex.  A label that the
    mesh does not hold is a KeyError."""
    objects = np.asarray(mesh['objects']).reshape(-1, len(OBJECT_COLUMNS))
    row = np.searchsorted(objects[:, 0], label)
    if row == len(objects) or objects[row, 0] != label:
        raise KeyError(f"object_mesh: the mesh holds no object with label {label!r}")
    _, v0, v1, q0, q1 = (int(v) for v in objects[row])
    return np.asarray(mesh['vertices'])[v0:v1], np.asarray(mesh['quads'])[q0:q1] - v0


def write_obj(path, mesh, label=None):
    """A plain Wavefront OBJ of the mesh, or of one object of it: 'v x y z' lines -- the vertices' columns reversed --
    and 'f a b c d' lines with 1-based indices.  Swapping z and x mirrors the frame, so every face is written as (v0,
    v3, v2, v1): counter-clockwise seen from outside in the right-handed x y z frame that viewers assume.  With
    label=None the objects follow each other as 'o <label>' groups."""
    if label is None:
        vertices, quads = np.asarray(mesh['vertices']), np.asarray(mesh['quads'])
        groups = [(int(r[0]), int(r[3]), int(r[4])) for r in np.asarray(mesh['objects']).reshape(-1, len(OBJECT_COLUMNS))]
    else:
        vertices, quads = object_mesh(mesh, label)
        groups = [(int(label), 0, len(quads))]
    fmt = '%d' if np.issubdtype(vertices.dtype, np.integer) else '%.9g'
    with open(path, 'w') as f:
        f.write(f"# {len(vertices)} vertices, {len(quads)} quads, x y z\n")
        np.savetxt(f, vertices[:, ::-1], fmt='v ' + ' '.join([fmt] * 3))
        for name, q0, q1 in groups:
            f.write(f"o {name}\n")
            np.savetxt(f, quads[q0:q1][:, [0, 3, 2, 1]].astype(np.int64) + 1, fmt='f %d %d %d %d')
