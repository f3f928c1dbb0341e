"""Label morphology: exact Euclidean erode, dilate, open and close of a labelled volume (include/emp_hip.h, E5).

The consensus paints an object wherever enough planes agree, so its surfaces carry one-voxel spikes, pits and thin
bridges; users of the reference clean them afterwards on a CPU with scipy.ndimage.binary_opening / binary_closing object
by object.  Here the voxel passes run on the device (csrc/emp_label_morph.hip, _hip.label_erode / label_dilate) and this
module holds what is left: reading the `morph` argument (`check`) and the whole operation on one class's slab, compound
operations and several ranks included (`morph_volume`).

    erode    a voxel keeps its label where its distance to every other label, background included, exceeds r
    dilate   a zero voxel takes the nearest label within r (the largest among equally near); labelled voxels stay
    open     dilate(erode(L)): a voxel that the erosion of label l took can only come back as l, because the ball around
             an eroded voxel of m lies inside m -- the binary opening of every label by itself
    close    where(L != 0, L, erode(dilate(L))): the originals are kept, since the erosion would bite them where two
             objects touch
"""
import math
import numbers

import numpy as np
import torch

from .tables import bits

__all__ = ['OPS', 'check', 'check_sampling', 'check_radius', 'check_cap', 'halo_slices', 'morph_volume']

OPS = ('erode', 'dilate', 'open', 'close')
R2_MAX = 65534


def check_sampling(who, sampling):
    """a voxel pitch (az, ay, ax), three integers in 1 .. 16, for the reader `who`"""
    try:
        vals = tuple(sampling)
    except TypeError:
        vals = None
    if vals is None or len(vals) != 3 or any(isinstance(a, (bool, np.bool_)) or not isinstance(a, numbers.Integral)
                                             or not 1 <= a <= 16 for a in vals):
        raise ValueError(f"{who}: the sampling must be three integers (az, ay, ax) in 1 .. 16, got {sampling!r}")
    return tuple(int(a) for a in vals)


def _is_real(r):
    return not isinstance(r, (bool, np.bool_)) and isinstance(r, numbers.Real) and math.isfinite(r)


def check_radius(who, r, sampling=(1, 1, 1)):
    """A real radius r in the units of the sampling -> (r2, sampling) for the reader `who`: r2 = floor(r^2 + 1e-9) must
    lie in min(sampling)^2 .. 65534.  The sampling is read once r is known to be a positive real number."""
    if not _is_real(r) or r <= 0:
        raise ValueError(f"{who}: the radius must be a positive real number, got {r!r}")
    sampling = check_sampling(who, sampling)
    r = float(r)
    if r * r > R2_MAX + 1:
        raise ValueError(f"{who}: the radius {r!r} is above sqrt({R2_MAX})")
    r2 = int(math.floor(r * r + 1e-9))
    if r2 > R2_MAX:
        raise ValueError(f"{who}: the radius {r!r} is above sqrt({R2_MAX})")
    if r2 < min(sampling) ** 2:
        raise ValueError(f"{who}: the radius {r!r} is below the smallest pitch of {sampling}: the ball is a point")
    return r2, sampling


def check_cap(who, arg, r_default, at_least=None, cap_max=65535):
    """infer_volume's `skeleton` / `thickness` argument -> None or (r_cap, cap, sampling) for the reader `who`.  arg:
    None, True (r_default, sampling (1, 1, 1)), r_cap, or (r_cap, (az, ay, ax)).  r_cap is a real number >= at_least
    (None: any positive one) and cap = floor(r_cap^2 + 1e-9), as check_radius reads a radius, must lie in 1 .. cap_max."""
    if arg is None:
        return None
    sampling = (1, 1, 1)
    if arg is True:
        r = r_default
    elif isinstance(arg, (tuple, list)):
        if len(arg) != 2:
            raise ValueError(f"{who} must be None, True, r_cap or (r_cap, (az, ay, ax)), got {arg!r}")
        r = arg[0]
        sampling = check_sampling(who, arg[1])
    else:
        r = arg
    if not _is_real(r) or (r <= 0 if at_least is None else r < at_least):
        raise ValueError(f"{who}: r_cap must be a " + ("positive real number" if at_least is None else
                                                        f"real number >= {at_least}") + f", got {r!r}")
    r = float(r)
    cap = int(math.floor(r * r + 1e-9)) if r * r <= cap_max + 1 else cap_max + 1
    if not 1 <= cap <= cap_max:
        raise ValueError(f"{who}: r_cap = {r!r} gives cap = r_cap^2 outside 1 .. {cap_max}")
    return r, cap, sampling


def check(morph):
    """infer_volume's `morph` argument -> None or (op, r2, sampling).  morph: None, (op, r) or (op, r, (az, ay, ax)) with
    op one of OPS, r a real radius in the units of the sampling and the sampling three integers in 1 .. 16 (default
    (1, 1, 1)).  r2 = floor(r^2 + 1e-9): 1 gives the 6-neighbourhood, sqrt(2) the 18- and sqrt(3) the 26-neighbourhood.
    r2 must lie in min(sampling)^2 .. 65534 -- below that the ball is a point.  Everything else is a ValueError."""
    if morph is None:
        return None
    if not isinstance(morph, (tuple, list)) or len(morph) not in (2, 3):
        raise ValueError(f"morph must be None, (op, r) or (op, r, (az, ay, ax)), got {morph!r}")
    op = morph[0]
    if not isinstance(op, str) or op not in OPS:
        raise ValueError(f"morph: the operation must be one of {OPS}, got {op!r}")
    return (op,) + check_radius("morph", *morph[1:])


def halo_slices(op, r2, sampling=(1, 1, 1)):
    """slices of its neighbours that a z-slab needs on either side: floor(sqrt(r2)) // az for erode and dilate, twice
    that for the compound operations"""
    one = math.isqrt(int(r2)) // int(sampling[0])
    return one if op in ('erode', 'dilate') else 2 * one


def morph_volume(slab, shape3d, op, r2, sampling=(1, 1, 1), group=None, z_base=0):
    """One operation on one class: (new_slab, stats).  slab: a rank's (d, H, W) device slab holding the slices [z_base,
    z_base + d) of the volume `shape3d` = (D, H, W), uint8 or int32 / uint32, contiguous; it is not written.  op, r2,
    sampling: what `check` returns.  With `group` the ranks hold consecutive z-slabs of ONE volume and every rank
    fetches halo_slices() slices of its neighbours (sharded.neighbour_slabs), so its new slab is its part of the
    single-rank result; a rank without slices takes part with an empty slab.  The compound operations run their first
    step on the slab extended by those slices -- what the second step reads of the first step's result then lies a
    one-step halo inside it -- and keep the core.  stats: {'op', 'r2', 'sampling', 'voxels_removed', 'voxels_added'}:
    the voxels that lost their label and the zero voxels that gained one, summed over the ranks, exact integers."""
    from . import _hip
    from .inference import sharded
    if op not in OPS:
        raise ValueError(f"morph_volume: the operation must be one of {OPS}, got {op!r}")
    sampling = check_sampling("morph", sampling)
    if len(shape3d) != 3 or any(int(s) < 0 for s in shape3d):
        raise ValueError(f"morph_volume: shape3d must be (D, H, W), got {shape3d!r}")
    r2 = int(r2)
    below, above = sharded.neighbour_slabs(slab, halo_slices(op, r2, sampling), group)
    if op == 'erode':
        new = _hip.label_erode(slab, r2, sampling, below=below, above=above)
    elif op == 'dilate':
        new = _hip.label_dilate(slab, r2, sampling, below=below, above=above)
    else:
        parts = [p for p in (below, slab, above) if p is not None]
        ext = slab if len(parts) == 1 else torch.cat([bits(p) for p in parts]).view(slab.dtype)
        lo = 0 if below is None else int(below.shape[0])
        first, second = (_hip.label_erode, _hip.label_dilate) if op == 'open' else (_hip.label_dilate, _hip.label_erode)
        new = second(first(ext, r2, sampling), r2, sampling)[lo:lo + int(slab.shape[0])]
        if op == 'close':
            new = torch.where(bits(slab) != 0, bits(slab), bits(new)).view(slab.dtype)
        new = new.contiguous()
    # an erosion or an opening only takes voxels and a dilation or a closing only gives them: two counts say how many
    change = int(torch.count_nonzero(bits(new))) - int(torch.count_nonzero(bits(slab)))
    assert change <= 0 if op in ('erode', 'open') else change >= 0
    moved = np.asarray([max(-change, 0), max(change, 0)], np.int64)
    moved = sharded._all_reduce_sum(moved, group)
    return new, dict(op=op, r2=r2, sampling=sampling, voxels_removed=int(moved[0]), voxels_added=int(moved[1]))
