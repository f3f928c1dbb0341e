"""Contact sites between labelled objects: which objects touch or lie within a distance of each other, over how much of
their surface, and where (include/emp_hip.h, E9).

Mitochondria-ER contact sites within 10-30 nm, the instances of one class that abut, the number of partners of an
organelle: the questions a multi-class segmentation is made for.  Users of the reference answer them on a CPU afterwards,
object pair by object pair, with scipy.ndimage.distance_transform_edt or a dilation per object.  Here the table is read
on the device (_hip.label_contacts, csrc/emp_label_contacts.hip), slab by slab, rank by rank: one row of 10 int64 per
ordered pair (a, b) with at least one contact voxel, ascending by (a, b), the columns being COLUMNS.  Columns 2 and 4..9
are sums and column 3 a minimum of integers, and every contact voxel belongs to the one block that owns it, so tables of
the z-blocks of a volume -- each read with B's true halo slices -- merge into the table of the whole (`merge_tables`),
whatever the partition and the order.  `derive` and `partners` turn a table into physical quantities on the host.

Not built: radii above a ring of 4 voxels (_hip.CONTACT_MAX_HALO), geodesic proximity, connected components per contact
site (the table is per pair), a painted contact-voxel volume, contacts against a ground truth, annotation export.
"""
import math
import numbers

import numpy as np
import torch

from .morphology import check_sampling
from .tables import _labels_to_device, gather_keyed, merge_keyed, volume_device, volume_slabs, volume_table

__all__ = ['COLUMNS', 'MAX_HALO', 'check', 'halo_slices', 'merge_tables', 'gather_tables', 'volume_contacts', 'derive',
           'partners']

COLUMNS = ('a', 'b', 'voxels', 'min_d2', 'sum_z', 'sum_y', 'sum_x', 'faces_z', 'faces_y', 'faces_x')
MAX_HALO = 4
_SUM = [2, 4, 5, 6, 7, 8, 9]
_MIN = [3]


def _radius(r, sampling):
    """r2 = floor(r^2 + 1e-9) of a real radius, inside what the kernel's ring takes"""
    if isinstance(r, (bool, np.bool_)) or not isinstance(r, numbers.Real) or not math.isfinite(r) or r <= 0:
        raise ValueError(f"contacts: the radius must be a positive real number, got {r!r}")
    r = float(r)
    if r > 16 * (MAX_HALO + 1):
        raise ValueError(f"contacts: the radius {r!r} reaches more than {MAX_HALO} voxels")
    r2 = int(math.floor(r * r + 1e-9))
    if r2 < min(sampling) ** 2:
        raise ValueError(f"contacts: the radius {r!r} is below the smallest pitch of {sampling}: the ball is a point")
    if math.isqrt(r2) // min(sampling) > MAX_HALO:
        raise ValueError(f"contacts: the radius {r!r} at sampling {sampling} reaches {math.isqrt(r2) // min(sampling)} "
                         f"voxels, more than {MAX_HALO}")
    return r2


def check(contacts):
    """infer_volume's `contacts` argument -> None or (r2, sampling, pairs or None).  contacts: None, r, (r, (az, ay, ax))
    or (r, (az, ay, ax), pairs) with r a real radius in the units of the sampling, the sampling three integers in 1 .. 16
    (default (1, 1, 1)) and pairs a list of (class_a, class_b).  r2 = floor(r^2 + 1e-9), as morphology.check reads a
    radius; min(sampling)^2 <= r2 and isqrt(r2) // min(sampling) <= 4.  Everything else is a ValueError."""
    if contacts is None:
        return None
    sampling, pairs = (1, 1, 1), None
    if isinstance(contacts, (tuple, list)):
        if len(contacts) not in (2, 3):
            raise ValueError("contacts must be None, r, (r, (az, ay, ax)) or (r, (az, ay, ax), pairs), got "
                             f"{contacts!r}")
        r = contacts[0]
        sampling = check_sampling("contacts", contacts[1])
        if len(contacts) == 3:
            raw = contacts[2]
            if isinstance(raw, (str, bytes)) or not isinstance(raw, (tuple, list)) or len(raw) == 0:
                raise ValueError(f"contacts: pairs must be a non-empty list of (class_a, class_b), got {raw!r}")
            pairs = []
            for p in raw:
                if isinstance(p, (str, bytes)) or not isinstance(p, (tuple, list)) or len(p) != 2:
                    raise ValueError(f"contacts: pairs must be a list of (class_a, class_b), got {p!r} in it")
                if tuple(p) not in pairs:
                    pairs.append(tuple(p))
    else:
        r = contacts
    return _radius(r, sampling), sampling, pairs


def halo_slices(r2, sampling=(1, 1, 1)):
    """slices of B that a z-slab of A needs on either side: floor(sqrt(r2)) // az"""
    return math.isqrt(int(r2)) // int(sampling[0])


def merge_tables(tables):
    """Merge of contact tables ((n, 10) int64 each, of a volume's z-blocks or of the ranks' slabs): one row per distinct
    (a, b), ascending by (a, b) as unsigned 32-bit values, columns 2 and 4..9 added and column 3 the minimum.  numpy in,
    numpy out; with any torch tensor among them the result is a torch table on that tensor's device.  No tables, or empty
    ones, give a (0, 10) table.  Integer sums and minima: exact whatever the order."""
    return merge_keyed(tables, len(COLUMNS), [0, 1], _SUM, _MIN)


def gather_tables(table, group=None):
    """The ranks' tables merged: every rank of `group` passes the table of its own slab and receives the table of all of
    them (one count all-gather + one padded all-gather, as measurements.gather_tables).  Without an initialised process
    group the table comes back merged with itself, i.e. sorted."""
    return gather_keyed(table, len(COLUMNS), merge_tables, group)


def volume_contacts(a, b=None, *, r, sampling=(1, 1, 1), slab_rows=None, group=None):
    """The contact table of label volumes (D, H, W) that are already there, as an (n, 10) int64 numpy array: `a` and `b`
    are numpy arrays, tensors or anything that has a shape and can be sliced along axis 0 (a ZarrV2Array, say); b=None is
    the same-volume case.  r: the radius in the units of the sampling, read as `check` reads it.  Every slab of slab_rows
    slices of A goes to the device together with the same slices of B and B's halo_slices() slices on either side (host
    data is uploaded slab by slab, so the volumes need not be resident as a whole) and through _hip.label_contacts;
    slab_rows=None takes device tensors whole and host data in slabs of about 2^27 voxels.  With `group` the ranks' tables
    are merged too -- every rank passes volumes of its own and all receive the merge; ranks that hold the z-slabs of ONE
    volume must hand each slab B's halo themselves (_hip.label_contacts' below / above, as infer_volume does) and then
    call gather_tables."""
    from . import _hip
    sampling = check_sampling("contacts", sampling)
    r2 = _radius(r, sampling)
    if len(a.shape) != 3:
        raise ValueError(f"volume_contacts: a must be (D, H, W), got {tuple(a.shape)}")
    if b is not None and tuple(b.shape) != tuple(a.shape):
        raise ValueError(f"volume_contacts: b is {tuple(b.shape)}, a is {tuple(a.shape)}")
    _hip.require_gpu()
    dev, resident = volume_device(a, b)
    tables = []
    for z, z1, lo, hi in volume_slabs("volume_contacts", a.shape, slab_rows, resident, halo_slices(r2, sampling)):
        # one upload covers B's slab and its halo on both sides; A's slab is a view of it in the same-volume case
        ext = _labels_to_device((a if b is None else b)[lo:hi], dev)
        ext = ext if ext.is_contiguous() else ext.contiguous()
        core = ext[z - lo:z1 - lo]
        below = ext[:z - lo] if z > lo else None
        above = ext[z1 - lo:] if hi > z1 else None
        if core.numel():
            if b is None:
                tables.append(_hip.label_contacts(core, None, r2, sampling, below=below, above=above, z_base=z))
            else:
                slab = _labels_to_device(a[z:z1], dev)
                slab = slab if slab.is_contiguous() else slab.contiguous()
                tables.append(_hip.label_contacts(slab, core, r2, sampling, below=below, above=above, z_base=z))
                del slab
        del ext, core, below, above
    return volume_table(tables, len(COLUMNS), merge_tables, gather_tables, group, dev)


def derive(table, sampling=(1, 1, 1), unit=1.0):
    """Physical quantities of a contact table ((n, 10) int64, numpy or torch) read with voxel pitch `sampling` = (az, ay,
    ax), one unit of which is `unit` long (nm, say); no GPU is needed.  Returns a dict of numpy arrays:
        a, b          table[:, 0], table[:, 1]
        voxels        table[:, 2]
        min_distance  sqrt(min_d2) * unit                                                 (float64)
        centroid      (n, 3): (sum_z, sum_y, sum_x) / voxels, in voxel indices            (float64 division)
        area          (faces_z * ay * ax + faces_y * az * ax + faces_x * az * ay) * unit^2
    area is that of the voxel faces a shares with b (the "crack" area), exact and additive over blocks and ranks; it
    overestimates a smooth interface as measurements.derive's surface area does."""
    if isinstance(table, torch.Tensor):
        table = table.cpu().numpy()
    t = np.asarray(table, dtype=np.int64).reshape(-1, len(COLUMNS))
    try:
        az, ay, ax = (float(s) for s in sampling)
        unit = float(unit)
    except (TypeError, ValueError):
        raise ValueError(f"derive: sampling must be three positive numbers and unit one, got {sampling!r}, {unit!r}") from None
    if not all(np.isfinite(s) and s > 0 for s in (az, ay, ax, unit)):
        raise ValueError(f"derive: sampling must be three positive numbers and unit one, got {sampling!r}, {unit!r}")
    voxels = t[:, 2]
    return {'a': t[:, 0].copy(), 'b': t[:, 1].copy(), 'voxels': voxels.copy(),
            'min_distance': np.sqrt(t[:, 3].astype(np.float64)) * unit,
            'centroid': t[:, 4:7] / voxels[:, None].astype(np.float64),
            'area': (t[:, 7] * ay * ax + t[:, 8] * az * ax + t[:, 9] * az * ay) * unit * unit}


def partners(table):
    """Per label a of a contact table: {'a': the distinct a ascending, 'partners': the number of distinct b of each,
    'min_d2': the smallest min_d2 over its rows}, numpy int64 arrays; no GPU is needed."""
    if isinstance(table, torch.Tensor):
        table = table.cpu().numpy()
    t = np.asarray(table, dtype=np.int64).reshape(-1, len(COLUMNS))
    labels, inv = np.unique(t[:, 0], return_inverse=True)
    inv = inv.reshape(-1)
    count = np.zeros(len(labels), np.int64)
    near = np.full(len(labels), np.iinfo(np.int64).max, np.int64)
    # one row per (a, b): the rows of a are its distinct partners
    np.add.at(count, inv, 1)
    np.minimum.at(near, inv, t[:, 3])
    return {'a': labels, 'partners': count, 'min_d2': near}
