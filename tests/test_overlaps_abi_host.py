"""CPU: argument checks of the overlap-table entry points (csrc/emp_overlaps.hip) and of their Python wrapper.  Every
refusal comes back as EMP_EINVAL before any launch, so it can be asked for without a GPU; the pointers handed over are
host buffers that are never read."""
import ctypes

import numpy as np
import pytest
import torch

EINVAL = -1
INT32_MAX = 2 ** 31 - 1


@pytest.fixture(scope='module')
def lib():
    from empanada_amd import _hip
    return _hip.load()


@pytest.fixture(scope='module')
def buf():
    b = ctypes.create_string_buffer(1 << 16)
    return ctypes.addressof(b), b


def test_count_refuses_bad_arguments(lib, buf):
    a, _ = buf
    need = lib.emp_label_overlaps_count_work_bytes(8)
    assert 0 < need <= 1 << 16
    good = dict(gt=a, gb=4, pred=a, pb=1, R=8, W=16, work=a, wb=need, offs=a)

    def call(**kw):
        v = {**good, **kw}
        return lib.emp_label_overlaps_count(v['gt'], v['gb'], v['pred'], v['pb'], v['R'], v['W'], v['work'], v['wb'],
                                            v['offs'], None)

    for kw, word in ((dict(gt=None), b'null'), (dict(pred=None), b'null'), (dict(work=None), b'null'),
                     (dict(offs=None), b'null'), (dict(R=-1), b'shape'), (dict(W=0), b'shape'), (dict(W=-3), b'shape'),
                     (dict(gb=2), b'uint8'), (dict(pb=8), b'uint8'), (dict(wb=need - 1), b'workspace'),
                     (dict(wb=0), b'workspace'), (dict(gt=a + 2), b'misaligned'),
                     (dict(R=2 ** 16, W=2 ** 15, wb=1 << 40), b'2^31'),          # 2^31 voxels: one too many
                     (dict(R=1, W=2 ** 31, wb=1 << 40), b'2^31'), (dict(R=2 ** 40, W=2 ** 40, wb=1 << 62), b'2^31')):
        assert call(**kw) == EINVAL, kw
        assert word in lib.emp_last_error(), (kw, lib.emp_last_error())


def test_table_refuses_bad_arguments(lib, buf):
    a, _ = buf
    need = lib.emp_label_overlaps_work_bytes(10)
    assert 0 < need <= 1 << 16
    assert lib.emp_label_overlaps_work_bytes(1000) > need
    good = dict(gt=a, gb=1, pred=a, pb=4, R=8, W=16, offs=a, n=10, work=a, wb=need, pairs=a, counts=a, n_out=a)

    def call(**kw):
        v = {**good, **kw}
        return lib.emp_label_overlaps(v['gt'], v['gb'], v['pred'], v['pb'], v['R'], v['W'], v['offs'], v['n'], v['work'],
                                      v['wb'], v['pairs'], v['counts'], v['n_out'], None)

    for kw, word in ((dict(gt=None), b'null'), (dict(pred=None), b'null'), (dict(offs=None), b'null'),
                     (dict(n_out=None), b'null'), (dict(work=None), b'null'), (dict(pairs=None), b'null'),
                     (dict(counts=None), b'null'), (dict(R=-1), b'shape'), (dict(W=0), b'shape'),
                     (dict(gb=3), b'uint8'), (dict(n=-1), b'n_spans'), (dict(n=8 * 16 + 1), b'n_spans'),
                     (dict(wb=need - 1), b'workspace'), (dict(wb=0), b'workspace'),
                     (dict(R=2 ** 16, W=2 ** 15), b'2^31'), (dict(pred=a + 1), b'misaligned')):
        assert call(**kw) == EINVAL, kw
        assert word in lib.emp_last_error(), (kw, lib.emp_last_error())


def test_the_voxel_limit_of_one_call_is_what_the_wrapper_splits_at(lib, buf):
    from empanada_amd import _hip
    assert _hip.OVERLAP_MAX_VOXELS == INT32_MAX
    a, _ = buf
    # the largest shapes inside the limit pass the shape check and are stopped by the next one (the workspace)
    for R, W in ((1, INT32_MAX), (INT32_MAX, 1), (2 ** 16, 2 ** 15 - 1)):
        assert lib.emp_label_overlaps_count(a, 1, a, 1, R, W, a, 0, a, None) == EINVAL
        assert b'workspace' in lib.emp_last_error()


def test_wrapper_needs_a_gpu_and_device_tensors():
    from empanada_amd import _hip
    g = torch.ones((4, 8), dtype=torch.int32)
    if not torch.cuda.is_available():
        with pytest.raises(_hip.HipError):
            _hip.label_overlaps(g, g)
        from empanada_amd import evaluation as EV
        with pytest.raises(_hip.HipError):
            EV.volume_scores(np.ones((2, 3, 4), np.uint8), np.ones((2, 3, 4), np.uint8))
