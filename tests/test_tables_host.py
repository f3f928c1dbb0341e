"""CPU: what the stage tables share (empanada_amd/tables.py) -- the keyed merge against a dictionary merge in Python
integers, the gather over ranks under gloo, the seam merge on blocks of volumes small enough to write their tables out by
hand -- and the readers of a radius, a cap and a sampling, each under its caller's name."""
import itertools
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from empanada_amd import components, contacts, evaluation, holes, measurements, morphology, separation, skeletons
from empanada_amd import tables as TB
from empanada_amd import thickness
from test_components_host import components_ref
from test_holes_host import holes_ref
from test_scores_host import _free_port

KEY_VALUES = [0, 1, 2, 7, 300, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1]
ROWS = (0, 1, 5, 40)
DATA = 2 ** 50                              # sums of coordinates and faces stay far below 2^63; negative values included
# n_col, keys, sums, mins, maxs: measurements, contacts, thickness
LAYOUTS = {'measure': (14, [0], [1, 8, 9, 10, 11, 12, 13], [2, 3, 4], [5, 6, 7]),
           'contacts': (10, [0, 1], [2, 4, 5, 6, 7, 8, 9], [3], []),
           'thickness': (3, [0, 1], [2], [], [])}
MERGES = {'measure': measurements.merge_tables, 'contacts': contacts.merge_tables, 'thickness': thickness.merge_tables}


def random_tables(n_col, keys, seed):
    """tables of 0, 1, 5 and 40 rows; the 5-row one holds the keys on either side of the sign bit of 32 bits"""
    rng = np.random.default_rng(seed)
    out = []
    for n in ROWS:
        t = rng.integers(-DATA, DATA, size=(n, n_col), dtype=np.int64)
        t[:, keys] = rng.choice(KEY_VALUES, size=(n, len(keys)))
        if n == 5:
            t[:2, keys[0]] = [2 ** 31, 2 ** 31 - 1]
        out.append(t)
    return out


def brute_merge(tables, n_col, keys, sums, mins, maxs):
    """a dict keyed by the key tuple, Python integers added / minimised / maximised; ascending by the key tuple"""
    acc = {}
    for t in tables:
        for row in np.asarray(t).reshape(-1, n_col).tolist():
            k = tuple(row[c] for c in keys)
            if k not in acc:
                acc[k] = list(row)
                continue
            old = acc[k]
            for c in sums:
                old[c] = old[c] + row[c]
            for c in mins:
                old[c] = min(old[c], row[c])
            for c in maxs:
                old[c] = max(old[c], row[c])
    rows = [acc[k] for k in sorted(acc)]
    return np.asarray(rows, dtype=np.int64).reshape(-1, n_col)


def as_numpy(t):
    return t.numpy() if isinstance(t, torch.Tensor) else t


def assert_unsigned_order(table, keys):
    """ascending by the keys as unsigned values: 2^31 after 2^31 - 1"""
    k = [tuple(r) for r in table[:, keys].tolist()]
    assert k == sorted(k) and len(set(k)) == len(k)
    lead = table[:, keys[0]].tolist()
    assert 2 ** 31 in lead and 2 ** 31 - 1 in lead
    assert lead.index(2 ** 31) > max(i for i, v in enumerate(lead) if v == 2 ** 31 - 1)


@pytest.mark.parametrize('kind', ['numpy', 'torch'])
@pytest.mark.parametrize('name', sorted(LAYOUTS))
def test_merge_keyed_equals_a_dictionary_merge(name, kind):
    n_col, keys, sums, mins, maxs = LAYOUTS[name]
    for seed in range(3):
        tabs = random_tables(n_col, keys, seed)
        expected = brute_merge(tabs, n_col, keys, sums, mins, maxs)
        if kind == 'torch':
            tabs = [torch.from_numpy(t) for t in tabs]
        got = TB.merge_keyed(tabs, n_col, keys, sums, mins, maxs)
        assert isinstance(got, torch.Tensor) == (kind == 'torch')
        got = as_numpy(got)
        assert got.dtype == np.int64 and got.shape == expected.shape
        np.testing.assert_array_equal(got, expected)
        assert_unsigned_order(got, keys)
        np.testing.assert_array_equal(as_numpy(MERGES[name](tabs)), expected)          # the stage's own name for it


@pytest.mark.parametrize('kind', ['numpy', 'torch'])
def test_merge_overlaps_equals_a_dictionary_merge(kind):
    for seed in range(3):
        tabs = random_tables(3, [0, 1], seed)
        expected = brute_merge(tabs, 3, [0, 1], [2], [], [])
        parts = [(t[:, :2].copy(), t[:, 2].copy()) for t in tabs]
        if kind == 'torch':
            parts = [(torch.from_numpy(p), torch.from_numpy(c)) for p, c in parts]
        pairs, counts = evaluation.merge_overlaps(parts)
        assert isinstance(pairs, torch.Tensor) == isinstance(counts, torch.Tensor) == (kind == 'torch')
        assert pairs.is_contiguous() if kind == 'torch' else pairs.flags['C_CONTIGUOUS']
        pairs, counts = as_numpy(pairs), as_numpy(counts)
        assert pairs.dtype == counts.dtype == np.int64 and pairs.shape == (len(expected), 2)
        np.testing.assert_array_equal(pairs, expected[:, :2])
        np.testing.assert_array_equal(counts, expected[:, 2])
        assert_unsigned_order(pairs, [0, 1])


@pytest.mark.parametrize('name', sorted(LAYOUTS))
def test_merge_keyed_mixed_empty_doubled_permuted(name):
    n_col, keys, sums, mins, maxs = LAYOUTS[name]
    tabs = random_tables(n_col, keys, 7)
    once = TB.merge_keyed(tabs, n_col, keys, sums, mins, maxs)
    # a numpy / torch mix returns a tensor
    mixed = TB.merge_keyed([tabs[0], torch.from_numpy(tabs[1]), tabs[2], torch.from_numpy(tabs[3])], n_col, keys, sums,
                           mins, maxs)
    assert isinstance(mixed, torch.Tensor) and mixed.dtype == torch.int64
    np.testing.assert_array_equal(mixed.numpy(), once)
    # none, or only empty ones
    for empties in ([], [np.zeros((0, n_col), np.int64)] * 2, [np.zeros(0, np.int64)]):
        got = TB.merge_keyed(empties, n_col, keys, sums, mins, maxs)
        assert isinstance(got, np.ndarray) and got.shape == (0, n_col) and got.dtype == np.int64
    got = TB.merge_keyed([torch.zeros((0, n_col), dtype=torch.int32)], n_col, keys, sums, mins, maxs)
    assert isinstance(got, torch.Tensor) and tuple(got.shape) == (0, n_col) and got.dtype == torch.int64
    # a table merged with itself: the sums double, minima and maxima stay
    twice = TB.merge_keyed([once, once], n_col, keys, sums, mins, maxs)
    np.testing.assert_array_equal(twice[:, sums], 2 * once[:, sums])
    rest = keys + mins + maxs
    np.testing.assert_array_equal(twice[:, rest], once[:, rest])
    # any order of the tables
    for order in itertools.permutations(range(len(tabs))):
        np.testing.assert_array_equal(TB.merge_keyed([tabs[i] for i in order], n_col, keys, sums, mins, maxs), once)


# ------------------------------------------------------------------------------------------------ over the ranks
def _contacts_merge(tabs):
    return TB.merge_keyed(tabs, *LAYOUTS['contacts'])


def test_gather_keyed_without_a_process_group_merges_the_table_with_itself():
    n_col, keys = LAYOUTS['contacts'][:2]
    table = np.concatenate(random_tables(n_col, keys, 11))
    got = TB.gather_keyed(table, n_col, _contacts_merge)
    assert isinstance(got, np.ndarray)
    np.testing.assert_array_equal(got, _contacts_merge([table]))
    got = TB.gather_keyed(torch.from_numpy(table), n_col, _contacts_merge)
    assert isinstance(got, torch.Tensor)
    np.testing.assert_array_equal(got.numpy(), _contacts_merge([table]))


def _worker(rank, world, port, q):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        n_col, keys = LAYOUTS['contacts'][:2]
        if rank == 0:
            table = np.concatenate(random_tables(n_col, keys, 11))
        else:                                                            # an empty share, and a tensor beside a numpy table
            table = torch.zeros((0, n_col), dtype=torch.int64)
        got = TB.gather_keyed(table, n_col, _contacts_merge)
        q.put((rank, type(got).__name__, np.asarray(got)))
    finally:
        dist.destroy_process_group()


def test_gather_keyed_under_gloo_with_an_empty_rank():
    n_col, keys = LAYOUTS['contacts'][:2]
    expected = _contacts_merge(random_tables(n_col, keys, 11))
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = [q.get(timeout=180) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert sorted((g[0], g[1]) for g in got) == [(0, 'ndarray'), (1, 'Tensor')]
    for _, _, table in got:
        np.testing.assert_array_equal(table, expected)


# ------------------------------------------------------------------------------------------------ across seams
NO = holes.NO_LABEL
# (4, 2, 3): label 1 runs through the seam between z = 1 and z = 2; label 2 is two pieces that never meet
COMPONENT_VOLUME = np.array([[[1, 1, 0], [0, 0, 2]],
                             [[1, 0, 0], [0, 0, 2]],
                             [[1, 0, 3], [0, 0, 0]],
                             [[0, 0, 3], [0, 0, 2]]], np.uint32)
#                  label voxels first z0 y0 x0 z1 y1 x1
COMPONENT_WHOLE = [[1, 4, 0, 0, 0, 0, 3, 1, 2],
                   [2, 2, 5, 0, 1, 2, 2, 2, 3],
                   [3, 2, 14, 2, 0, 2, 4, 1, 3],
                   [2, 1, 23, 3, 1, 2, 4, 2, 3]]
COMPONENT_BLOCKS = ([[1, 3, 0, 0, 0, 0, 2, 1, 2],                # slices 0, 1
                     [2, 2, 5, 0, 1, 2, 2, 2, 3]],
                    [[1, 1, 12, 2, 0, 0, 3, 1, 1],               # slices 2, 3 with z_base 2
                     [3, 2, 14, 2, 0, 2, 4, 1, 3],
                     [2, 1, 23, 3, 1, 2, 4, 2, 3]])


def _cavity_volume():
    """(4, 3, 5) of label 7 with a 9 at (0, 1, 3): cavity P = (1, 1, 1), (2, 1, 1), (2, 1, 0) reaches the x border in
    its upper piece only; cavity Q = (1, 1, 3), (2, 1, 3) is closed and sees the 9 from its lower piece only"""
    v = np.full((4, 3, 5), 7, np.uint32)
    v[0, 1, 3] = 9
    for z, y, x in ((1, 1, 1), (2, 1, 1), (2, 1, 0), (1, 1, 3), (2, 1, 3)):
        v[z, y, x] = 0
    return v


#               voxels first z0 y0 x0 z1 y1 x1 lab_min lab_max
CAVITY_WHOLE = [[3, 21, 1, 1, 0, 3, 2, 2, NO, 0],
                [2, 23, 1, 1, 3, 3, 2, 4, 7, 9]]
CAVITY_BLOCKS = ([[1, 21, 1, 1, 1, 2, 2, 2, 7, 7],               # slices 0, 1
                  [1, 23, 1, 1, 3, 2, 2, 4, 7, 9]],
                 [[2, 35, 2, 1, 0, 3, 2, 2, NO, 0],              # slices 2, 3 with z_base 2
                  [1, 38, 2, 1, 3, 3, 2, 4, 7, 7]])


def test_the_hand_written_tables_are_those_of_the_definition():
    v = COMPONENT_VOLUME
    np.testing.assert_array_equal(components_ref(v, 6)[0], COMPONENT_WHOLE)
    np.testing.assert_array_equal(components_ref(v[:2], 6)[0], COMPONENT_BLOCKS[0])
    np.testing.assert_array_equal(components_ref(v[2:], 6, z_base=2)[0], COMPONENT_BLOCKS[1])
    v = _cavity_volume()
    np.testing.assert_array_equal(holes_ref(v), CAVITY_WHOLE)
    np.testing.assert_array_equal(holes_ref(v[:2], above=v[2]), CAVITY_BLOCKS[0])
    np.testing.assert_array_equal(holes_ref(v[2:], below=v[1], z_base=2), CAVITY_BLOCKS[1])


@pytest.mark.parametrize('kind', ['numpy', 'torch'])
@pytest.mark.parametrize('merge, blocks, seams, whole, index', [
    (components.merge_blocks, COMPONENT_BLOCKS, [[[1, 3]]], COMPONENT_WHOLE, [0, 1, 0, 2, 3]),
    (components.merge_blocks, COMPONENT_BLOCKS[::-1], [[], [[4, 1]]], COMPONENT_WHOLE, [0, 2, 3, 0, 1]),
    (holes.merge_blocks, CAVITY_BLOCKS, [[[1, 3]], [[4, 2]]], CAVITY_WHOLE, [0, 1, 0, 1]),
    (holes.merge_blocks, CAVITY_BLOCKS[::-1], [[[3, 1], [2, 4]]], CAVITY_WHOLE, [0, 1, 0, 1]),
], ids=['components', 'components-upper-first', 'holes', 'holes-upper-first'])
def test_merge_seamed_gives_the_table_of_the_undivided_volume(merge, blocks, seams, whole, index, kind):
    if kind == 'torch':
        blocks = [torch.tensor(b, dtype=torch.int64) for b in blocks]
    got, got_index = merge(blocks, seams, return_index=True)
    assert isinstance(got, torch.Tensor) == isinstance(got_index, torch.Tensor) == (kind == 'torch')
    assert got.dtype == got_index.dtype == (torch.int64 if kind == 'torch' else np.int64)
    np.testing.assert_array_equal(as_numpy(got), whole)
    np.testing.assert_array_equal(as_numpy(got_index), index)
    np.testing.assert_array_equal(as_numpy(merge(blocks, seams)), whole)


def test_merge_seamed_layouts_and_errors():
    # the two layouts straight through merge_seamed, without the stages' own check and fix-up
    got = TB.merge_seamed(COMPONENT_BLOCKS, [[[1, 3]]], 9, first=2, sums=[1], mins=[0, 2, 3, 4, 5], maxs=[6, 7, 8])
    np.testing.assert_array_equal(got, COMPONENT_WHOLE)
    got = TB.merge_seamed(CAVITY_BLOCKS, [[[1, 3], [2, 4]]], 10, first=1, sums=[0], mins=[1, 2, 3, 4, 8], maxs=[5, 6, 7, 9])
    np.testing.assert_array_equal(got[1], CAVITY_WHOLE[1])
    np.testing.assert_array_equal(got[0], CAVITY_WHOLE[0][:8] + [7, 7])       # what holes' fix-up is there to amend
    # no blocks, no rows
    got, index = TB.merge_seamed([], [], 9, first=2, return_index=True)
    assert got.shape == (0, 9) and got.dtype == np.int64 and index.shape == (0,)
    # seam ids outside 1 .. n, for both stages
    for merge, blocks in ((components.merge_blocks, COMPONENT_BLOCKS), (holes.merge_blocks, CAVITY_BLOCKS)):
        n = sum(len(b) for b in blocks)
        for bad in ([[0, 1]], [[1, n + 1]]):
            with pytest.raises(ValueError) as e:
                merge(blocks, [bad])
            assert str(e.value) == f"merge_blocks: seam ids outside 1 .. {n}"
    with pytest.raises(ValueError) as e:
        components.merge_blocks(COMPONENT_BLOCKS, [[[1, 4]]])
    assert str(e.value) == "merge_blocks: a seam joins components of different labels"


# ------------------------------------------------------------------------------------------------ the readers
def _morph(r, s):
    return morphology.check(('erode', r, s))


def _separate(r, s):
    return separation.check((r, 1, s))


def _contacts(r, s):
    return contacts.check((r, s))


def _skeleton(r, s):
    return skeletons.check((r, s))


def _thickness(r, s):
    return thickness.check((r, s))


@pytest.mark.parametrize('check, who, bad_radius', [
    (_morph, 'morph', "morph: the radius must be a positive real number, got -1"),
    (_separate, 'separate', "separate: the radius must be a positive real number, got -1"),
    (_contacts, 'contacts', "contacts: the radius must be a positive real number, got -1"),
    (_skeleton, 'skeleton', "skeleton: r_cap must be a positive real number, got -1"),
    (_thickness, 'thickness', "thickness: r_cap must be a real number >= 1, got -1"),
], ids=['morph', 'separate', 'contacts', 'skeleton', 'thickness'])
def test_every_reader_reports_under_its_own_name(check, who, bad_radius):
    for sampling in ((1, 1, 17), (1, 1), (True, 1, 1), 1):
        with pytest.raises(ValueError) as e:
            check(2, sampling)
        assert str(e.value) == f"{who}: the sampling must be three integers (az, ay, ax) in 1 .. 16, got {sampling!r}"
    with pytest.raises(ValueError) as e:
        check(-1, (1, 1, 1))
    assert str(e.value) == bad_radius
    assert check(2, (2, 1, 1)) is not None


def test_the_bounds_that_differ_between_the_readers():
    with pytest.raises(ValueError) as e:                                 # a positive r_cap: its cap refuses it
        skeletons.check(0.5)
    assert str(e.value) == "skeleton: r_cap = 0.5 gives cap = r_cap^2 outside 1 .. 65535"
    with pytest.raises(ValueError) as e:
        thickness.check(0.5)
    assert str(e.value) == "thickness: r_cap must be a real number >= 1, got 0.5"
    with pytest.raises(ValueError) as e:
        thickness.check(300)
    assert str(e.value) == "thickness: r_cap = 300.0 gives cap = r_cap^2 outside 1 .. 65535"
    for who, check in (('skeleton', skeletons.check), ('thickness', thickness.check)):
        with pytest.raises(ValueError) as e:
            check((1, 2, 3))
        assert str(e.value) == f"{who} must be None, True, r_cap or (r_cap, (az, ay, ax)), got (1, 2, 3)"
    with pytest.raises(ValueError) as e:
        separation.check((300, 1))
    assert str(e.value) == "separate: the radius 300.0 is above sqrt(65534)"
    with pytest.raises(ValueError) as e:
        morphology.check(('erode', 1, (2, 2, 2)))
    assert str(e.value) == "morph: the radius 1.0 is below the smallest pitch of (2, 2, 2): the ball is a point"
