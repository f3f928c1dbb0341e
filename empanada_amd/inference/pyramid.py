"""Multiscale label pyramid of infer_volume's output: what a viewer (napari, neuroglancer, any OME-NGFF reader) needs
beside the full-resolution labels.  Level l is level l - 1 pooled by a factor triple of 1s and 2s with the mode of every
cell (_hip.pool_labels, csrc/emp_pool.hip: labels cannot be averaged), on the device, while the labelled slab is still
resident -- the reference writes level 0 only and leaves the rest to a CPU pass over the files.

    factors = normalize(3)                                  # [(2, 2, 2)] * 3; [(1, 2, 2), (2, 2, 2)] for thick sections
    levels = plan(shape3d, factors, z0, z1)                 # shapes, cumulative factors, the rank's z-range per level
    slabs = build(slab, factors)                            # the rank's slab of every level, on the current stream
    group.update_attrs({'multiscales': [multiscales('mito_pred', paths, cum_factors)]})

Every rank pools its own z-slab only.  That is exact as long as no cell straddles two ranks, which `plan` checks; a
halo exchange between ranks is deliberately not built (as windows across ranks were not when windowing landed)."""
import numbers

__all__ = ['normalize', 'plan', 'check_ranks', 'build', 'multiscales', 'MAX_LEVELS']

MAX_LEVELS = 8


def _triple(t):
    try:
        t = tuple(t)
    except TypeError:
        return None
    if len(t) != 3 or any(isinstance(v, bool) or not isinstance(v, numbers.Integral) or v not in (1, 2) for v in t):
        return None
    return tuple(int(v) for v in t) if max(t) == 2 else None


def normalize(pyramid):
    """infer_volume's `pyramid` argument as a list of factor triples (fz, fy, fx): None -> []; an integer L, 1 <= L <=
    MAX_LEVELS -> L times (2, 2, 2); a sequence of triples of 1s and 2s, each with at least one 2, as it is.
    ValueError for anything else."""
    if pyramid is None:
        return []
    if isinstance(pyramid, numbers.Integral) and not isinstance(pyramid, bool):
        if not 1 <= pyramid <= MAX_LEVELS:
            raise ValueError(f"pyramid={pyramid!r}: the number of levels must be between 1 and {MAX_LEVELS}")
        return [(2, 2, 2)] * int(pyramid)
    if not isinstance(pyramid, (str, bytes)):
        try:
            levels = [_triple(t) for t in pyramid]
        except TypeError:
            levels = [None]
        if levels and len(levels) <= MAX_LEVELS and all(t is not None for t in levels):
            return levels
    raise ValueError(f"pyramid must be None, a number of (2, 2, 2) levels between 1 and {MAX_LEVELS}, or a sequence of at "
                     f"most {MAX_LEVELS} factor triples of 1s and 2s with at least one 2 each, got {pyramid!r}")


def plan(shape3d, factors, z0, z1):
    """Levels 1 .. len(factors) of a (Z, Y, X) volume for the rank that owns the z-slab [z0, z1): a list of
    {'shape': the level's array shape (ceilings: a level is pooled from the level below, not from level 0),
     'factor': the cumulative factor (Fz, Fy, Fx), 'z_range': the rank's slices [z0 / Fz, ceil(z1 / Fz)) of it,
     'pool': the level's own triple}.
    The rank pools its own slab only, so no cell may straddle two ranks: z0 % Fz == 0, and z1 % Fz == 0 unless z1 is
    the volume's end -- a ValueError otherwise."""
    Z = int(shape3d[0])
    z0, z1 = int(z0), int(z1)
    shape, cum, out = tuple(int(s) for s in shape3d), (1, 1, 1), []
    for l, f in enumerate(factors, start=1):
        shape = tuple(-(-s // v) for s, v in zip(shape, f))
        cum = tuple(c * v for c, v in zip(cum, f))
        Fz = cum[0]
        if z0 % Fz or (z1 % Fz and z1 != Z):
            raise ValueError(f"pyramid: the rank slab z = [{z0}, {z1}) of {Z} slices is not aligned to level {l}, whose "
                             f"cumulative z-factor is {Fz}: a cell would straddle two ranks.  The call works with fewer "
                             "ranks, with fewer levels, or with (1, 2, 2) levels, which do not pool along z")
        out.append({'shape': shape, 'factor': cum, 'z_range': (z0 // Fz, -(-z1 // Fz)), 'pool': tuple(f)})
    return out


def check_ranks(shape3d, factors, bounds):
    """`plan` for the slabs [bounds[r], bounds[r + 1]) of ALL ranks, so that every rank raises alike; returns the plans"""
    return [plan(shape3d, factors, int(a), int(b)) for a, b in zip(bounds[:-1], bounds[1:])]


def build(slab, factors):
    """the level slabs 1 .. len(factors) of a labelled (n, Y, X) device slab by repeated _hip.pool_labels, on the current
    stream; a level is pooled from the level below"""
    from .. import _hip
    out = []
    for f in factors:
        slab = _hip.pool_labels(slab, f)
        out.append(slab)
    return out


def multiscales(name, paths, cum_factors):
    """the OME-NGFF 0.4 `multiscales` entry of one label image: paths[l] is the dataset of level l (level 0 first),
    cum_factors[l] its cumulative factor (Fz, Fy, Fx), (1, 1, 1) for level 0.  Coordinates are in level-0 voxels (the
    voxel size is not known here, so the axes carry no unit): a level's voxel is F voxels wide and its centre sits
    (F - 1) / 2 voxels past the centre of the first level-0 voxel it covers"""
    datasets = []
    for path, F in zip(paths, cum_factors):
        tf = [{'type': 'scale', 'scale': [float(v) for v in F]}]
        if any(v != 1 for v in F):
            tf.append({'type': 'translation', 'translation': [(v - 1) / 2 for v in F]})
        datasets.append({'path': path, 'coordinateTransformations': tf})
    return {'version': '0.4', 'name': name, 'type': 'mode',
            'axes': [{'name': a, 'type': 'space'} for a in 'zyx'], 'datasets': datasets}
