"""What the tables of the labelled-volume stages share: one merge of keyed tables, one gather over the ranks,
one merge across seams and one walk over the slabs of a volume that is already there.

A stage table is (n, n_col) int64 with one row per key -- a label, or a pair of values below 2^32 -- and columns that add,
take the minimum or take the maximum, so the tables of z-blocks, of slabs and of ranks merge exactly, whatever the
partition and the order.  measurements, contacts, thickness and evaluation say which columns do what; components and
holes, whose rows are joined by seam pairs instead of a key, do the same for `merge_seamed`.
"""
import numpy as np
import torch

__all__ = ['bits', 'merge_keyed', 'gather_keyed', 'merge_seamed', 'volume_device', 'volume_slabs',
           'volume_table']

_I64 = np.iinfo(np.int64)


def bits(t):
    """a uint32 tensor as int32, the same bits: torch compares and copies few uint32 tensors"""
    return t.view(torch.int32) if t.dtype == torch.uint32 else t


def merge_keyed(tables, n_col, keys, sums=(), mins=(), maxs=()):
    """Merge of (n, n_col) int64 tables: one row per distinct key, ascending, the columns `sums` added, `mins` the
    minimum and `maxs` the maximum.  keys: one column, ordered as int64, or two whose values lie in 0 .. 2^32 - 1,
    ordered by (k0, k1) as unsigned values.  numpy in, numpy out; with any torch tensor among the tables the result is
    a torch table on that tensor's device, made there.  No tables, or empty ones, give a (0, n_col) table."""
    tables = list(tables)
    keys, sums, mins, maxs = list(keys), list(sums), list(mins), list(maxs)
    if any(isinstance(t, torch.Tensor) for t in tables):
        dev = next(t.device for t in tables if isinstance(t, torch.Tensor))
        rows = torch.cat([torch.as_tensor(t).to(dev).reshape(-1, n_col).long() for t in tables])
        if rows.shape[0] == 0:
            return rows
        if len(keys) == 2:
            # the values are below 2^32: the upper one reaches the sign bit only from 2^31 on, which the flip keeps in order
            key = ((rows[:, keys[0]] << 32) | rows[:, keys[1]]) ^ (-1 << 63)
        else:
            key = rows[:, keys[0]]
        uniq, inv = torch.unique(key, return_inverse=True)                  # ascending
        out = torch.zeros((uniq.shape[0], n_col), dtype=torch.int64, device=dev)
        if len(keys) == 2:
            uniq = uniq ^ (-1 << 63)
            out[:, keys[0]] = (uniq >> 32) & 0xffffffff
            out[:, keys[1]] = uniq & 0xffffffff
        else:
            out[:, keys[0]] = uniq
        for cols, how, start in ((sums, 'sum', 0), (mins, 'amin', _I64.max), (maxs, 'amax', _I64.min)):
            if cols:
                acc = torch.full((uniq.shape[0], len(cols)), start, dtype=torch.int64, device=dev)
                acc.scatter_reduce_(0, inv[:, None].expand(-1, len(cols)), rows[:, cols].contiguous(), how)
                out[:, cols] = acc
        return out
    parts = [np.asarray(t, dtype=np.int64).reshape(-1, n_col) for t in tables]
    rows = np.concatenate(parts) if parts else np.zeros((0, n_col), np.int64)
    if len(rows) == 0:
        return rows
    if len(keys) == 2:
        key = (rows[:, keys[0]].astype(np.uint64) << np.uint64(32)) | rows[:, keys[1]].astype(np.uint64)
    else:
        key = rows[:, keys[0]]
    uniq, inv = np.unique(key, return_inverse=True)
    inv = inv.reshape(-1)
    out = np.zeros((len(uniq), n_col), np.int64)
    if len(keys) == 2:
        out[:, keys[0]] = (uniq >> np.uint64(32)).astype(np.int64)
        out[:, keys[1]] = (uniq & np.uint64(0xffffffff)).astype(np.int64)
    else:
        out[:, keys[0]] = uniq
    _reduce_rows(out, inv, rows, sums, mins, maxs)
    return out


def _reduce_rows(out, index, rows, sums, mins, maxs):
    """rows[i] added / minimised / maximised into out[index[i]], column by column (numpy)"""
    out[:, mins] = _I64.max
    out[:, maxs] = _I64.min
    for cols, op in ((sums, np.add), (mins, np.minimum), (maxs, np.maximum)):
        for c in cols:
            op.at(out[:, c], index, rows[:, c])


def gather_keyed(table, n_col, merge, group=None):
    """The ranks' tables merged: every rank of `group` passes the (n, n_col) table of its own share and receives
    `merge` of all of them (one count all-gather + one padded all-gather, sharded._gather_var).  numpy in, numpy out.
    Without an initialised process group the table comes back merged with itself, i.e. sorted."""
    from .inference import sharded
    if sharded._world(group)[1] == 1:
        return merge([table])
    was_numpy = not isinstance(table, torch.Tensor)
    t = torch.as_tensor(table).reshape(-1, n_col).long()
    merged = merge(sharded._gather_var(t, group))
    return merged.cpu().numpy() if was_numpy else merged


def _host(t):
    """a table or pair list as an int64 numpy array"""
    if isinstance(t, torch.Tensor):
        t = t.cpu().numpy()
    return np.asarray(t, dtype=np.int64)


def merge_seamed(tables, seams, n_col, first, sums=(), mins=(), maxs=(), check=None, fixup=None, return_index=False):
    """The table of a volume from the (n, n_col) tables of its z-blocks (or of the ranks' slabs) whose rows are joined
    across the seams.  Provisional id p = 1 + row in the concatenation of `tables`; `seams` is a list of (m, 2) arrays
    of provisional ids that touch across a border.  Ids joined by any chain of pairs become one row: the columns `sums`
    added, `mins` (the column `first` among them) the minimum and `maxs` the maximum; the result is renumbered
    ascending by `first`.  Union-find on the host (scipy.sparse.csgraph).  check(rows, pairs) may refuse the seams and
    fixup(rows, index, out) amend the merged rows, both on the host.  numpy in, numpy out; with any tensor among the
    tables the result is a tensor on its device.  return_index: also the (n_provisional,) int64 map from p - 1 to the
    row of the merged table."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    tables = list(tables)
    dev = next((t.device for t in tables if isinstance(t, torch.Tensor)), None)
    parts = [_host(t).reshape(-1, n_col) for t in tables]
    rows = np.concatenate(parts) if parts else np.zeros((0, n_col), np.int64)
    n = len(rows)
    pairs = [_host(s).reshape(-1, 2) for s in seams]
    pairs = np.concatenate(pairs) if pairs else np.zeros((0, 2), np.int64)
    if len(pairs) and (pairs.min() < 1 or pairs.max() > n):
        raise ValueError(f"merge_blocks: seam ids outside 1 .. {n}")
    if check is not None:
        check(rows, pairs)
    if n == 0:
        out, index = rows, np.zeros((0,), np.int64)
    else:
        graph = coo_matrix((np.ones(len(pairs), np.int8), (pairs[:, 0] - 1, pairs[:, 1] - 1)), shape=(n, n))
        m, grp = connected_components(graph, directed=False)
        lead = np.full(m, _I64.max, np.int64)
        np.minimum.at(lead, grp, rows[:, first])
        rank = np.empty(m, np.int64)
        rank[np.argsort(lead, kind='stable')] = np.arange(m)
        index = rank[grp]
        out = np.zeros((m, n_col), np.int64)
        _reduce_rows(out, index, rows, list(sums), list(mins), list(maxs))
        if fixup is not None:
            fixup(rows, index, out)
    if dev is not None:
        out, index = torch.from_numpy(out).to(dev), torch.from_numpy(index).to(dev)
    return (out, index) if return_index else out


# ----------------------------------------------------------------------------- a volume that is already there, slab by slab
_SLAB_VOXELS = 1 << 27        # host volumes are uploaded in slabs of about this many voxels (512 MiB of uint32)


def _labels_to_device(x, dev):
    """one slab of labels as a contiguous uint8 or uint32 tensor on `dev`; any integer type whose values fit 32 bits"""
    if isinstance(x, torch.Tensor):
        if x.dtype == torch.bool:
            x = x.to(torch.uint8)
        if x.dtype not in (torch.uint8, torch.int32, torch.uint32):
            if x.is_floating_point() or x.is_complex():
                raise ValueError(f"volume_scores: labels must be integers, got {x.dtype}")
            x = x.to(torch.int64)
            if x.numel() and (int(x.min()) < 0 or int(x.max()) >= 2 ** 32):
                raise ValueError("volume_scores: labels must lie in 0 .. 2^32 - 1")
            x = x.to(torch.int32)                                       # keeps the low 32 bits
        return x.to(dev).contiguous()
    a = np.asarray(x)
    if a.dtype == np.bool_:
        a = a.astype(np.uint8)
    if a.dtype.kind not in 'iu':
        raise ValueError(f"volume_scores: labels must be integers, got {a.dtype}")
    if a.dtype == np.uint8:
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    if a.dtype != np.uint32:
        if a.size and (int(a.min()) < 0 or int(a.max()) >= 2 ** 32):
            raise ValueError("volume_scores: labels must lie in 0 .. 2^32 - 1")
        a = a.astype(np.uint32)
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(dev).view(torch.uint32)


def volume_device(*volumes):
    """(device, resident): the volumes' device if every one of them (None apart) is a tensor on a GPU -- then they are
    resident and taken whole by default -- and the current GPU otherwise"""
    volumes = [v for v in volumes if v is not None]
    resident = all(isinstance(v, torch.Tensor) and v.is_cuda for v in volumes)
    return (volumes[0].device if resident else torch.device('cuda', torch.cuda.current_device())), resident


def volume_slabs(who, shape, slab_rows, resident, halo=0, what="slices"):
    """The slabs of a volume of `shape` in which a volume_* function walks it: a list of (z, z1, lo, hi), the slab's
    own indices [z, z1) along axis 0 and, with `halo` more on either side as far as the volume goes, [lo, hi).
    slab_rows=None takes a resident volume whole and any other in slabs of about 2^27 voxels."""
    n = int(shape[0])
    if slab_rows is None:
        per_row = int(np.prod(shape[1:], dtype=np.int64))
        slab_rows = max(n, 1) if resident else max(1, _SLAB_VOXELS // max(per_row, 1))
    elif isinstance(slab_rows, bool) or not isinstance(slab_rows, (int, np.integer)) or slab_rows < 1:
        raise ValueError(f"{who}: slab_rows must be a positive number of {what}, got {slab_rows!r}")
    slab_rows = int(slab_rows)
    return [(z, min(n, z + slab_rows), max(0, z - halo), min(n, z + slab_rows + halo)) for z in range(0, n, slab_rows)]


def volume_table(tables, n_col, merge, gather, group, dev):
    """the end of such a walk: the slabs' tables merged -- none is an empty table on `dev` -- then gathered over the
    ranks of `group`, as a numpy array"""
    table = merge(tables) if tables else torch.zeros((0, n_col), dtype=torch.int64, device=dev)
    return gather(table, group).cpu().numpy()
