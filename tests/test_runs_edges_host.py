"""CPU: the two references behind tests/test_runs_edges_gpu.py (the oracle modules and the plain numpy / pure-Python
statement written there) agree on every input of that module -- so that a wrong reference cannot hide a wrong kernel,
and so that the inputs and references are exercised where there is no GPU.  Nothing here is slower than about a second;
no reference had to be kept out of the GPU module for its run time."""
import numpy as np
import pytest

import test_runs_edges_gpu as E


def test_row_run_references_agree():
    n = 0
    for W in E.ROW_WIDTHS:
        pats = E.row_patterns(W, *E.ROW_DH)
        assert len(pats) == 10
        for name, pan in pats.items():
            counts, st, ln, val = E.runs_refs(pan)
            E._same_tables(E.runs_numpy(pan), (counts, st, ln, val), f'runs_numpy W={W} {name}')
            assert ln.sum() == np.count_nonzero(pan) and (name != 'zero' or len(st) == 0)
            n += len(st)
    assert n > 10000
    full = E.runs_refs(E.row_patterns(1028)['full'])
    assert full[0].tolist() == [1] * 6 and full[2].tolist() == [1028] * 6
    assert E.runs_refs(E.row_patterns(65)['row_join'])[0].tolist() == [2] * 6


@pytest.mark.parametrize('shape', E.ROW_BIG, ids=lambda s: 'x'.join(map(str, s)))
def test_row_run_closed_form(shape):
    pan, exp = E.row_big_stack(*shape)
    assert pan.shape[0] * pan.shape[1] > 65536
    E._same_tables(E.runs_numpy(pan), exp, 'closed form against runs_numpy')
    E._same_tables(E.runs_scan(pan), exp, 'closed form against the row scan')


@pytest.mark.parametrize('name', list(E.LABEL_CASES))
def test_label_references_agree(name):
    pan, div, cc = E.LABEL_CASES[name]
    T = E.label_refs(pan, div, cc)
    assert T['c_area'].sum() == np.count_nonzero(pan)
    assert pan.shape[1] <= 40 and pan.shape[2] <= 70


def test_label_references_agree_high_class():
    pan, div = E.high_class_stack()
    for mask in (0b010, 0xffffffff):
        cc = [c for c in range(32) if (mask >> c) & 1]
        assert E.cc_mask_of(cc) == mask
        T = E.label_refs(pan, div, cc)
        assert (T['c_val'] == 335).sum() == 2              # one component per slice, whatever the mask
    assert E.cc_mask_of([1, 33, -1]) == 2
    E.label_refs(np.zeros((2, 3, 4), np.uint32), 1000, [1])
    E.label_refs(E.table_stack(), 1000, [1])
    E.label_refs(E.lift_stack(), 1000, [1])
    for Xl in (1, 7):
        E.label_refs(E.yz_stack(Xl), 1000, [1])


@pytest.mark.parametrize('name', list(E.OVERLAP_CASES))
def test_overlap_references_agree(name):
    T, trip = E.overlap_refs(E.OVERLAP_CASES[name], 1000, [1])
    assert all(t[2] > 0 for t in trip)
    if name in ('identical', 'shifted', 'empty_middle'):
        assert (sum(trip.values()) > 50) == (name != 'empty_middle')


def test_reduce_scan_sort_references_agree():
    for trip in E.REDUCE_INPUTS.values():
        E.reduce_refs(trip)
    for n in E.SCAN_N:
        x = E.scan_input(n)
        assert x.min(initial=0) >= -3 and x.max(initial=0) <= 3 and (n < 100 or x.min() < 0)
        E.scan_refs(x)
    keys = E.sort_input()
    assert (keys >> np.uint64(63)).any()
    for bits in ((40, 64), (0, 40), (0, 64), (63, 64)):
        order = E.sort_refs(keys, *bits)
        assert sorted(order.tolist()) == list(range(len(keys)))


def test_vote_references_agree():
    for name, (starts, ends, grp, n_groups, base) in E.VOTE_CASES.items():
        assert len(starts) == 0 or (starts.min() >= base and ends.max() < (1 << 40) and ends.max() - base <= E.VOTE_SPAN)
        for thr in E.VOTE_THR:
            out, off = E.vote_plain(starts, ends, grp, n_groups, thr, base)
            assert off[-1] == len(out) and len(off) == n_groups + 1
    out, off = E.vote_plain(*E.VOTE_CASES['mixed'][:4], 1)
    assert out[:3].tolist() == [[10, 31], [100, 200], [310, 320]] and off.tolist() == [0, 0, 3, 3, 3, 4, 4, 5, 5, 5]
    for thr in (2, 3):
        assert len(E.vote_lists_refs(E.vote_lists(), thr)) > 5


def test_pair_and_fill_references_agree():
    starts, lens, off = E.pair_instances()
    table = E.pair_table_refs(starts, lens, off)
    assert (table == table.T).all() and (np.diag(table) == [lens[off[i]:off[i + 1]].sum() for i in range(12)]).all()
    E.fill_refs(*E.fill_case_small())
    n, st, ln, order, ids = E.fill_case_small()
    E.fill_refs(n, st, ln, order, ids, vol=np.random.default_rng(43).integers(0, 2 ** 31, n).astype(np.uint32))
    n, st, ln, order, ids = E.fill_case_many()
    assert len(st) > 32768 and (ids == 0).any() and ids.max() < 2 ** 31
    E.fill_refs(n, st, ln, order, ids)


def test_box_and_rle_references_agree():
    for nd in (2, 3):
        for nb in E.BOX_NB:
            a, b = E.boxes_input(5, nd, 0), E.boxes_input(nb, nd, 1)
            b[:min(nb, 5)] = a[:min(nb, 5)]
            exp = E.box_pairs_refs(a, b)
            assert nb == 1 or len(exp) > 3
            assert nb == 1 or (((b[:, nd:] - b[:, :nd]) < 0).any() and (b < 0).any())       # inverted, negative
    assert len(E.box_pairs_refs(E.boxes_input(6, 2, 2), E.boxes_input(300, 2, 3))) > 20
    starts, runs = E.rle_case()
    idx = E.rle_decode_refs(starts, runs)
    assert (np.diff(idx) > 0).all()
    E.rle_encode_refs(idx)


def test_track_references_agree():
    pan = E.lift_stack()
    D, H, W = pan.shape
    T = E.label_refs(pan, 1000, [1])
    for axis, slice0, inst_base in E.LIFT_GEOM:
        Y, X = (H, W) if axis == 0 else (D + slice0 + 2, W)
        for comp_inst in E.lift_insts(T['n_comp']).values():
            E.lift_refs(axis, T, comp_inst, H, W, Y, X, slice0, inst_base)
    for tw, X, y0, x0, inst_base in E.TILE_GEOM:
        for comp_inst in E.lift_insts(T['n_comp']).values():
            E.tile_refs(T, comp_inst, tw, X, y0, x0, inst_base)
    for Xl, X, x0 in E.YZ_GEOM:
        before, after = E.yz_refs(E.yz_volume(Xl), X, x0, 1000)
        assert (len(after[0]) < len(before[0])) == (Xl == X)        # rows touch only when the slab is the whole row
    key, ln = E.sort_chain_input()
    assert len(E.sort_chain_refs(key, ln, False)[0]) == len(key)
    assert len(E.sort_chain_refs(key, ln, True)[0]) == 14
    key, ln = E.clip_input()
    for lo, hi in E.CLIP_INTERVALS:
        E.clip_refs(key, ln, lo, hi)


WORK_N = [0, 1, 2047, 2048, 2049, 100000]
# recorded from the library before the layouts were moved onto the shared workspace carver.  The three byte counts
# are taken without the radix sort's own workspace (it depends on the rocPRIM version, and its query answers -1 where
# rocPRIM cannot size itself without a device; either way it is added into the total as it is)
WORK_SIZES = {
    'emp_scan_tmp_elems': [2, 2, 2, 2, 3, 50],
    'emp_track_work_elems': [6, 6, 4098, 4100, 4103, 200052],
    'emp_rle_encode_work_elems': [3, 5, 4097, 4099, 4102, 200051],
    'emp_runs_label_work_elems': [200, 200, 20480, 20484, 32776, 1186484],
    'emp_track_sort_work_bytes': [1792, 1792, 65792, 66048, 67328, 3200768],
    'emp_triplets_reduce_work_bytes': [1792, 1792, 65792, 66048, 67328, 3200768],
    'emp_vote_work_bytes': [2560, 2560, 180480, 181248, 182784, 8801280],
}


def test_work_sizes_unchanged():
    """a rewritten layout cannot silently shrink a workspace: every size query answers what it always did"""
    from empanada_amd import _hip
    _hip.load()
    q = _hip.query
    sort_items = {'emp_track_sort_work_bytes': lambda n: n, 'emp_triplets_reduce_work_bytes': lambda n: n,
                  'emp_vote_work_bytes': lambda n: 2 * max(n, 1)}
    for name, want in WORK_SIZES.items():
        got = [q(name, n) - (q('emp_sort_work_bytes', sort_items[name](n)) if name in sort_items else 0)
               for n in WORK_N]
        assert got == want, name
