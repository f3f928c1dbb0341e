"""CPU: the per-object measurement table (include/emp_hip.h, E2) -- the checker the GPU tests compare the kernel with,
on cases counted by hand; measurements.merge_tables and derive; the argument checks of the ABI and of
infer_volume(measure=), none of which needs a GPU.

The checker `measure_ref` is a numpy restatement of the definition that shares nothing with the kernel: the array is
zero-padded by one voxel on every side, `below` / `above` go into the z pads, the centre is compared with its six
shifted copies, and the columns are accumulated per label with np.add.at / np.minimum.at / np.maximum.at."""
import ctypes

import numpy as np
import pytest
import torch

N_COL = 14


# ------------------------------------------------------------------------------------------------------ the checker
def measure_ref(lab, below=None, above=None, z_base=0):
    """(D, H, W) unsigned labels -> the (n, 14) int64 table of the definition"""
    lab = np.asarray(lab)
    D, H, W = lab.shape
    pad = np.zeros((D + 2, H + 2, W + 2), np.int64)
    pad[1:-1, 1:-1, 1:-1] = lab
    if below is not None:
        pad[0, 1:-1, 1:-1] = below
    if above is not None:
        pad[-1, 1:-1, 1:-1] = above
    c = pad[1:-1, 1:-1, 1:-1]
    fz = (c != pad[:-2, 1:-1, 1:-1]).astype(np.int64) + (c != pad[2:, 1:-1, 1:-1])
    fy = (c != pad[1:-1, :-2, 1:-1]).astype(np.int64) + (c != pad[1:-1, 2:, 1:-1])
    fx = (c != pad[1:-1, 1:-1, :-2]).astype(np.int64) + (c != pad[1:-1, 1:-1, 2:])
    z, y, x = np.nonzero(c)
    labels, inv = np.unique(c[z, y, x], return_inverse=True)
    inv = inv.reshape(-1)
    out = np.zeros((len(labels), N_COL), np.int64)
    out[:, 0] = labels
    out[:, 2:5] = np.iinfo(np.int64).max
    out[:, 5:8] = np.iinfo(np.int64).min
    zg = z + z_base
    np.add.at(out[:, 1], inv, 1)
    for col, v in ((2, zg), (3, y), (4, x)):
        np.minimum.at(out[:, col], inv, v)
    for col, v in ((5, zg + 1), (6, y + 1), (7, x + 1)):
        np.maximum.at(out[:, col], inv, v)
    for col, v in ((8, zg), (9, y), (10, x), (11, fz[z, y, x]), (12, fy[z, y, x]), (13, fx[z, y, x])):
        np.add.at(out[:, col], inv, v)
    return out


def test_the_checker_on_cases_counted_by_hand():
    one = np.zeros((3, 3, 3), np.uint8)
    one[1, 2, 0] = 7
    assert measure_ref(one, z_base=5).tolist() == [[7, 1, 6, 2, 0, 7, 3, 1, 6, 2, 0, 2, 2, 2]]
    cube = np.full((2, 2, 2), 3, np.uint32)
    assert measure_ref(cube).tolist() == [[3, 8, 0, 0, 0, 2, 2, 2, 4, 4, 4, 8, 8, 8]]
    pair = np.array([[[4, 9]]], np.uint32)                   # the shared face counts for both
    assert measure_ref(pair).tolist() == [[4, 1, 0, 0, 0, 1, 1, 1, 0, 0, 0, 2, 2, 2], [9, 1, 0, 0, 1, 1, 1, 2, 0, 0, 1, 2, 2, 2]]
    same = np.array([[[4, 4]]], np.uint32)
    assert measure_ref(same).tolist() == [[4, 2, 0, 0, 0, 1, 1, 2, 0, 0, 1, 4, 4, 2]]
    v = np.array([[[5]]], np.uint8)
    assert measure_ref(v, below=np.array([[5]]))[0, 11:].tolist() == [1, 2, 2]
    assert measure_ref(v, below=np.array([[6]]))[0, 11:].tolist() == [2, 2, 2]
    assert measure_ref(v, below=np.array([[5]]), above=np.array([[5]]))[0, 11:].tolist() == [0, 2, 2]
    assert measure_ref(np.zeros((2, 2, 2), np.uint8)).shape == (0, N_COL)
    top = np.array([[[0xFFFFFFFF, 0x80000000]]], np.uint32)  # labels are unsigned
    assert measure_ref(top)[:, 0].tolist() == [0x80000000, 0xFFFFFFFF]


def test_the_checker_is_additive_over_z_blocks():
    from empanada_amd import measurements as M
    rng = np.random.default_rng(5)
    lab = rng.integers(0, 4, size=(6, 5, 7)).astype(np.uint32)
    whole = measure_ref(lab)
    for cut in (1, 3, 5):
        parts = [measure_ref(lab[:cut], above=lab[cut]), measure_ref(lab[cut:], below=lab[cut - 1], z_base=cut)]
        np.testing.assert_array_equal(M.merge_tables(parts), whole)
        blind = [measure_ref(lab[:cut]), measure_ref(lab[cut:], z_base=cut)]
        assert (M.merge_tables(blind) != whole).any()


# ------------------------------------------------------------------------------------------------------ the host module
def test_columns():
    from empanada_amd import measurements as M
    assert M.COLUMNS == ('label', 'voxels', 'z0', 'y0', 'x0', 'z1', 'y1', 'x1', 'sum_z', 'sum_y', 'sum_x',
                         'faces_z', 'faces_y', 'faces_x')


def test_merge_tables():
    from empanada_amd import measurements as M
    a = np.array([[5, 2, 0, 3, 4, 1, 5, 6, 0, 7, 9, 2, 4, 4], [3, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 2, 2, 2]], np.int64)
    b = np.array([[5, 1, 3, 0, 5, 4, 1, 8, 3, 0, 5, 2, 2, 2], [2 ** 32 - 1, 4, 9, 9, 9, 10, 10, 13, 36, 36, 42, 2, 2, 2]],
                 np.int64)
    want = [[3, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 2, 2, 2], [5, 3, 0, 0, 4, 4, 5, 8, 3, 7, 14, 4, 6, 6],
            [2 ** 32 - 1, 4, 9, 9, 9, 10, 10, 13, 36, 36, 42, 2, 2, 2]]
    got = M.merge_tables([a, b])
    assert isinstance(got, np.ndarray) and got.dtype == np.int64 and got.tolist() == want
    assert M.merge_tables([b, a]).tolist() == want and M.merge_tables([a[:1], b, a[1:]]).tolist() == want
    assert M.merge_tables([a, np.zeros((0, N_COL), np.int64)]).tolist() == sorted(a.tolist())
    for tables in ([torch.from_numpy(a), torch.from_numpy(b)], [a, torch.from_numpy(b)], [torch.from_numpy(a), b]):
        got = M.merge_tables(tables)
        assert isinstance(got, torch.Tensor) and got.dtype == torch.int64 and got.tolist() == want
    for empty in ([], [np.zeros((0, N_COL), np.int64)], [np.zeros((0, N_COL), np.int64)] * 2):
        got = M.merge_tables(empty)
        assert isinstance(got, np.ndarray) and got.shape == (0, N_COL) and got.dtype == np.int64
    got = M.merge_tables([torch.zeros((0, N_COL), dtype=torch.int64)])
    assert isinstance(got, torch.Tensor) and tuple(got.shape) == (0, N_COL)
    assert M.gather_tables(a).tolist() == sorted(a.tolist())              # no process group: merged with itself


def test_derive_exact_values():
    from empanada_amd import measurements as M
    t = np.array([[3, 7, 1, 2, 3, 4, 6, 9, 15, 22, 40, 10, 12, 14], [9, 1, 0, 0, 0, 1, 1, 1, 0, 0, 0, 2, 2, 2]], np.int64)
    sz, sy, sx = 40.0, 8.0, 4.0
    for table in (t, torch.from_numpy(t)):
        d = M.derive(table, (sz, sy, sx))
        assert sorted(d) == ['bbox', 'centroid', 'label', 'surface_area', 'volume', 'voxels']
        assert d['label'].tolist() == [3, 9] and d['voxels'].tolist() == [7, 1]
        assert (d['volume'] == t[:, 1] * sz * sy * sx).all() and d['volume'].tolist() == [8960.0, 1280.0]
        assert d['centroid'].shape == (2, 3) and d['centroid'].dtype == np.float64
        assert (d['centroid'] == t[:, 8:11] / t[:, 1:2]).all()
        assert d['centroid'][0].tolist() == [15 / 7, 22 / 7, 40 / 7]
        assert d['bbox'].tolist() == [[1, 2, 3, 4, 6, 9], [0, 0, 0, 1, 1, 1]]
        assert (d['surface_area'] == t[:, 11] * sy * sx + t[:, 12] * sz * sx + t[:, 13] * sz * sy).all()
        assert d['surface_area'].tolist() == [10 * 32.0 + 12 * 160.0 + 14 * 320.0, 2 * 32.0 + 2 * 160.0 + 2 * 320.0]
    unit = M.derive(t)
    assert unit['volume'].tolist() == [7.0, 1.0] and unit['surface_area'].tolist() == [36.0, 6.0]
    empty = M.derive(np.zeros((0, N_COL), np.int64))
    assert empty['centroid'].shape == (0, 3) and empty['bbox'].shape == (0, 6) and empty['volume'].shape == (0,)
    for bad in ((1, 1), (1, 0, 1), (1, -2, 1), (1, float('nan'), 1), (1, float('inf'), 1), 3.0, 'abc'):
        with pytest.raises(ValueError, match='spacing'):
            M.derive(t, bad)


# ------------------------------------------------------------------------------------------------------ the ABI
def test_abi_argument_checks_without_gpu():
    """every check returns before any launch: -1, and text in emp_last_error()"""
    from empanada_amd import _hip
    lib = _hip.load()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)                                 # a non-null, 16-byte aligned address that is never read
    p -= p % 16
    p += 16
    big = 1 << 20

    def refused(rc, word):
        assert rc == -1
        msg = lib.emp_last_error()
        assert word in msg, msg

    count, measure = lib.emp_label_measure_count, lib.emp_label_measure
    assert lib.emp_label_measure_count_work_bytes(10) > 0 and lib.emp_label_measure_work_bytes(10) > 0
    refused(count(None, 4, 2, 3, 5, p, big, p, None), b'null')
    refused(count(p, 4, 2, 3, 5, None, big, p, None), b'null')
    refused(count(p, 4, 2, 3, 5, p, big, None, None), b'null')
    refused(count(p, 2, 2, 3, 5, p, big, p, None), b'uint8')
    refused(count(p, 4, 2, 3, 0, p, big, p, None), b'shape')
    refused(count(p, 4, 2, 0, 5, p, big, p, None), b'shape')
    refused(count(p, 4, -1, 3, 5, p, big, p, None), b'shape')
    refused(count(p, 1, 2, 1 << 15, 1 << 15, p, big, p, None), b'2^31')             # 2^31 voxels: one too many
    refused(count(p, 4, 1 << 11, 1 << 10, 1 << 10, p, big, p, None), b'2^31')
    refused(count(p, 4, 1 << 40, 1 << 40, 1 << 40, p, big, p, None), b'2^31')       # no overflow in the check itself
    refused(count(p + 2, 4, 2, 3, 5, p, big, p, None), b'misaligned')
    refused(count(p, 4, 2, 3, 5, p, lib.emp_label_measure_count_work_bytes(6) - 1, p, None), b'workspace')

    def m(lab=p, item=4, D=2, H=3, W=5, below=None, above=None, z_base=0, offs=p, n_runs=4, work=p, wb=big, out=p, n_out=p):
        return measure(lab, item, D, H, W, below, above, z_base, offs, n_runs, work, wb, out, n_out, None)

    refused(m(lab=None), b'null')
    refused(m(offs=None), b'null')
    refused(m(n_out=None), b'null')
    refused(m(work=None), b'null')
    refused(m(out=None), b'null')
    refused(m(item=2), b'uint8')
    refused(m(W=0), b'shape')
    refused(m(D=1 << 11, H=1 << 10, W=1 << 10), b'2^31')
    refused(m(lab=p + 1), b'misaligned')
    refused(m(below=p + 3), b'misaligned')
    refused(m(above=p + 2), b'misaligned')
    refused(m(z_base=-1), b'z_base')
    refused(m(n_runs=-1), b'n_runs')
    refused(m(n_runs=31), b'n_runs')                          # more runs than voxels
    refused(m(wb=lib.emp_label_measure_work_bytes(4) - 1), b'workspace')
    refused(m(wb=0), b'workspace')


def test_signatures_match_the_issue():
    from empanada_amd import _hip
    for name in ('emp_label_measure_count_work_bytes', 'emp_label_measure_count', 'emp_label_measure_work_bytes',
                 'emp_label_measure'):
        assert name in _hip.SIGNATURES
    assert len(_hip.SIGNATURES['emp_label_measure_count'][1]) == 9
    assert len(_hip.SIGNATURES['emp_label_measure'][1]) == 15


# ------------------------------------------------------------------------------------------------------ the wrappers
def test_measure_labels_refuses_operands_before_a_launch():
    from empanada_amd import _hip
    host = torch.zeros((2, 3, 4), dtype=torch.uint8)
    with pytest.raises(ValueError, match='GPU'):
        _hip.measure_labels(host)


class _NoModel:
    """an engine whose model must never be reached"""
    thing_list = [1]
    label_divisor = 1000

    @property
    def model(self):
        raise AssertionError("infer_volume touched the model before it checked `measure`")


@pytest.mark.parametrize('bad', [False, np.True_, (1.0, 2.0), (1, 2, 3, 4), (1.0, 0.0, 1.0), (1.0, -1.0, 1.0),
                                 (1.0, float('nan'), 1.0), (1.0, float('inf'), 1.0), (True, 1, 1), ('1', 1, 1), 'abc', 3.0,
                                 {'z': 1}], ids=repr)
def test_infer_volume_refuses_bad_measure_values(bad):
    from empanada_amd.inference.driver import infer_volume
    vol = np.zeros((4, 8, 8), np.uint8)
    with pytest.raises(ValueError, match='measure'):
        infer_volume(_NoModel(), vol, norms=dict(mean=0.5, std=0.1), labels=[1], measure=bad)


def test_check_measure_accepts():
    from empanada_amd.inference.driver import _check_measure
    assert _check_measure(None) is None
    assert _check_measure(True) == (1.0, 1.0, 1.0)
    assert _check_measure((40, 8.0, np.float32(8))) == (40.0, 8.0, 8.0)
    assert _check_measure(np.array([2.0, 1.0, 1.0])) == (2.0, 1.0, 1.0)
