"""CPU: the window planning of inference/windowed.py, the argument checks of emp_median_harden_window (they return before
any launch) and the argument errors of infer_volume's window switch (raised before any GPU work)."""
import itertools
import types

import numpy as np
import pytest


# ----------------------------------------------------------------------------- plan_windows
def _plan(*a, **kw):
    from empanada_amd.inference.windowed import plan_windows
    return plan_windows(*a, **kw)


def test_plan_examples():
    assert _plan(23, 4, 3, 8) == [(0, 8), (8, 16), (16, 23)]
    assert _plan(23, 4, 3, 10) == [(0, 8), (8, 16), (16, 23)]                  # 10 rounds down to 8
    assert _plan(24, 4, 3, 3) == [(lo, lo + 3) for lo in range(0, 24, 3)]       # W < per: calls of 3
    assert _plan(17, 4, 3, 8) == [(0, 8), (8, 17)]                             # a last chunk of 1 < m is merged
    assert _plan(23, 4, 3, 23) == [(0, 23)]
    assert _plan(23, 4, 3, 64) == [(0, 23)]
    assert _plan(23, 4, 3, None) == [(0, 23)]


def test_plan_calls_shrink_below_per():
    chunks = _plan(23, 4, 3, 3)
    assert chunks[0] == (0, 3) and all(hi - lo == 3 for lo, hi in chunks[:-1]) and chunks[-1][1] == 23
    assert chunks[-1][1] - chunks[-1][0] >= 3                                   # 23 = 7 * 3 + 2: the 2 are merged


def test_plan_auto():
    bps, m = 1000, 3
    assert _plan(23, 4, m, 'auto', bytes_per_slice=bps, budget=23 * bps) == [(0, 23)]
    assert _plan(23, 4, m, 'auto', bytes_per_slice=bps, budget=(8 + m) * bps) == [(0, 8), (8, 16), (16, 23)]
    assert _plan(23, 4, m, 'auto', bytes_per_slice=bps, budget=(8 + m) * bps + m * 400 - 1, sem_bytes=400) \
        == [(0, 4), (4, 8), (8, 12), (12, 16), (16, 20), (20, 23)]            # the history counts
    with pytest.raises(ValueError, match='not even one model call'):
        _plan(23, 4, m, 'auto', bytes_per_slice=bps, budget=(4 + m) * bps - 1)
    with pytest.raises(ValueError):
        _plan(23, 4, m, 'auto')                                                 # no sizes to plan with


def test_plan_errors_name_the_numbers():
    with pytest.raises(ValueError, match=r'6 slices.*ks=7'):
        _plan(6, 4, 3, 8)
    with pytest.raises(ValueError, match=r'2 slices.*m=3'):
        _plan(23, 1, 3, 2)
    for bad in (True, False, 0, -1, 'x', 2.5):
        with pytest.raises(ValueError):
            _plan(23, 4, 3, bad)


def test_plan_properties():
    for n, per, m, W in itertools.product((1, 7, 8, 23, 40), (1, 3, 4, 16), (0, 1, 3, 5), (1, 3, 4, 7, 8, 12, 40, 100)):
        if n < 2 * m + 1:
            with pytest.raises(ValueError):
                _plan(n, per, m, W)
            continue
        if W >= n:
            assert _plan(n, per, m, W) == [(0, n)]
            continue
        eff = W // per * per if W >= per else W
        if eff < m:
            with pytest.raises(ValueError):
                _plan(n, per, m, W)
            continue
        chunks = _plan(n, per, m, W)
        assert chunks[0][0] == 0 and chunks[-1][1] == n
        assert all(a[1] == b[0] for a, b in zip(chunks, chunks[1:]))
        assert all(hi - lo >= max(m, 1) for lo, hi in chunks)
        assert all(hi - lo == eff for lo, hi in chunks[:-1])                    # equal, and a multiple of per if W >= per
        if W >= per:
            assert all((hi - lo) % per == 0 for lo, hi in chunks[:-1])
        assert chunks[-1][1] - chunks[-1][0] < eff + max(m, 1)


# ----------------------------------------------------------------------------- the ABI's argument checks
def test_window_entry_rejects_bad_arguments_without_gpu():
    from empanada_amd import _hip
    lib = _hip.load()
    f = lib.emp_median_harden_window
    p = 4096                                                                    # never dereferenced: the checks come first

    def bad(word, *a):
        assert f(*a) == -1
        assert word in lib.emp_last_error(), lib.emp_last_error()

    bad(b'null', None, None, None, 4, 1, 16, 3, 0.5, p, None, None)            # prob
    bad(b'null', None, p, None, 4, 1, 16, 3, 0.5, None, None, None)            # out_sem
    bad(b'ks=4', None, p, None, 4, 1, 16, 4, 0.5, p, None, None)
    bad(b'ks=13', None, p, None, 40, 1, 16, 13, 0.5, p, None, None)
    bad(b'C=17', None, p, None, 4, 17, 16, 3, 0.5, p, None, None)
    bad(b'D=2', p, p, p, 2, 1, 16, 7, 0.5, p, None, None)                      # D < m
    bad(b'D=0', None, p, None, 0, 1, 16, 1, 0.5, p, None, None)
    bad(b'shorter than ks=7', None, p, None, 4, 1, 16, 7, 0.5, p, None, None)  # no hist, no halo, D < ks
    bad(b'shorter than ks=7', p, p, None, 3, 1, 16, 7, 0.5, p, None, None)     # 3 + 3 + 0 < 7
    bad(b'ks=1', p, p, None, 4, 1, 16, 1, 0.5, p, None, None)                  # ks = 1 with a hist pointer
    bad(b'ks=1', None, p, None, 4, 1, 16, 1, 0.5, p, p, None)                  # ... with a tail
    bad(b'LDS', None, p, None, 40, 15, 16, 11, 0.5, p, None, None)


# ----------------------------------------------------------------------------- infer_volume's window switch
def _stub_engine():
    return types.SimpleNamespace(thing_list=[1], label_divisor=1000, model=None)


def test_infer_volume_window_arguments_fail_before_gpu_work():
    from empanada_amd.inference.driver import infer_volume
    vol = np.zeros((8, 8, 8), np.uint8)
    kw = dict(norms=dict(mean=0.5, std=0.1), labels=[1])
    for bad in (0, -3, True, 'x', 2.5):
        with pytest.raises(ValueError, match='window_slices'):
            infer_volume(_stub_engine(), vol, window_slices=bad, **kw)
    with pytest.raises(ValueError, match='mem_budget'):
        infer_volume(_stub_engine(), vol, window_slices='auto', mem_budget=0, **kw)
    with pytest.raises(ValueError, match="pipeline's own"):
        infer_volume(_stub_engine(), vol, window_slices='auto', mem_budget=1 << 30, pipeline=object(), **kw)


def test_windows_with_several_ranks_are_refused(monkeypatch):
    from empanada_amd.inference import driver, sharded
    monkeypatch.setattr(sharded, '_world', lambda group=None: (0, 2))
    with pytest.raises(ValueError, match='not built yet'):
        driver.infer_volume(_stub_engine(), np.zeros((8, 8, 8), np.uint8), norms=dict(mean=0.5, std=0.1), labels=[1],
                            window_slices=4)
