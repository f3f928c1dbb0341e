"""CPU: the entry points and the limit parsing behind more than 4096 centres per slice (emp_find_centers_ws,
EMP_MAX_CENTERS).  The argument checks return before any launch, so they run on a builder without a GPU."""
import pytest


def test_new_entry_points_validate_before_any_launch():
    from empanada_amd import _hip
    lib = _hip.load()
    assert _hip.CENTER_LIMIT == 65535 and _hip.MAX_CENTERS == 4096
    # (hmp, D, h, w, thr, k, cap, work, out_idx, out_count, stream); 16 stands in for an aligned non-null pointer
    assert lib.emp_find_centers_ws(16, 1, 8, 8, 0.1, 3, 65536, 16, 16, 16, None) == -1
    assert b'65535' in lib.emp_last_error()
    assert lib.emp_find_centers_ws(16, 1, 8, 8, 0.1, 3, 0, 16, 16, 16, None) == -1
    assert lib.emp_find_centers_ws(None, 1, 8, 8, 0.1, 3, 16, 16, 16, 16, None) == -1
    assert b'null' in lib.emp_last_error()
    assert lib.emp_find_centers_ws(16, 1, 8, 8, 0.1, 3, 16, None, 16, 16, None) == -1
    assert lib.emp_find_centers_ws(16, 1, 8, 8, 0.1, 99, 16, 16, 16, 16, None) == -1
    assert b'nms kernel' in lib.emp_last_error()
    # the bitmap: one bit per pixel and slice
    small = lib.emp_find_centers_work_elems(1, 8, 8, 16)
    mid = lib.emp_find_centers_work_elems(1, 300, 300, 65535)
    big = lib.emp_find_centers_work_elems(1, 1024, 1024, 65535)
    assert 0 < small < mid < big
    assert mid * 32 >= 300 * 300 and big == 1024 * 1024 // 32
    assert lib.emp_find_centers_work_elems(4, 1024, 1024, 65535) == 4 * big
    assert lib.emp_find_centers_work_elems(1, 0, 8, 16) == 0
    # grouping: the uint16 ceiling holds, the old one is gone (the call below fails on its step, after the cap check)
    assert lib.emp_group_pixels(16, 16, 65536, 16, 1, 8, 8, 1, None, 0, 16, 16, None) == -1
    assert b'65535' in lib.emp_last_error()
    assert lib.emp_group_pixels(16, 16, 65535, 16, 1, 8, 8, 3, None, 0, 16, 16, None) == -1
    assert b'step' in lib.emp_last_error()


def test_max_centres_from_argument_and_environment(monkeypatch):
    from empanada_amd import _hip
    from empanada_amd.inference.postprocess import resolve_max_centers
    monkeypatch.delenv('EMP_MAX_CENTERS', raising=False)
    assert resolve_max_centers() == 4096
    assert resolve_max_centers(None) == 4096
    monkeypatch.setenv('EMP_MAX_CENTERS', '65535')
    assert resolve_max_centers() == 65535
    assert resolve_max_centers(100) == 100          # an explicit argument wins over the environment
    monkeypatch.setenv('EMP_MAX_CENTERS', '1')
    assert resolve_max_centers() == 1
    for bad in ('0', '70000', 'abc', '-5', '4096.0'):
        monkeypatch.setenv('EMP_MAX_CENTERS', bad)
        with pytest.raises(_hip.HipError, match='EMP_MAX_CENTERS'):
            resolve_max_centers()
    monkeypatch.delenv('EMP_MAX_CENTERS')
    for bad in (0, 65536, -1, 4096.0, '4096', True):
        with pytest.raises(_hip.HipError, match='max_centers'):
            resolve_max_centers(bad)
    assert resolve_max_centers(65535) == 65535


def test_engines_keep_the_limit():
    import torch
    from empanada_amd.inference import engines as EN
    model = torch.nn.Linear(1, 1)
    for cls in (EN.PanopticDeepLabEngine, EN.PanopticDeepLabEngine3d, EN.PanopticDeepLabRenderEngine,
                EN.PanopticDeepLabRenderEngine3d):
        assert cls(model, thing_list=[1]).max_centers is None
        eng = cls(model, thing_list=[1], max_centers=65535)
        assert eng.max_centers == 65535
        assert eng._stack_params()['max_centers'] == 65535
