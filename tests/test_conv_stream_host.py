"""The tile walk of the persistent conv kernel (emp_conv_stream.hip) through its host query emp_conv_stream_walk: every
(batch entry, tile) is visited exactly once, and a block only visits tiles of the contiguous eighth of the sequence that
its XCD (block & 7) owns.  No GPU needed."""
import ctypes

import pytest

# tiles per batch entry, batch entries, grid
CASES = [(3072, 1, 768), (3073, 1, 768), (4096, 1, 768), (32768, 1, 768), (3373, 1, 768), (1157, 1, 768),
         (86, 36, 768), (1024, 3, 768), (128, 36, 768),
         (5, 1, 8),            # fewer tiles than blocks
         (13, 3, 40),          # 39 tiles on 40 blocks
         (100, 1, 768),        # far fewer tiles than blocks
         (7, 7, 16), (1, 1, 8), (769, 1, 768)]


@pytest.fixture(scope='module')
def lib():
    from empanada_amd import _hip
    return _hip.load()


def _walk(lib, tiles, batch, grid, block):
    out = []
    e, t = ctypes.c_int64(-1), ctypes.c_int64(-1)
    step = 0
    while lib.emp_conv_stream_walk(tiles, batch, grid, block, step, ctypes.byref(e), ctypes.byref(t)):
        out.append((e.value, t.value))
        step += 1
        assert step <= tiles * batch
    # the valid steps are a prefix: nothing after the first refusal
    assert not lib.emp_conv_stream_walk(tiles, batch, grid, block, step + 1, ctypes.byref(e), ctypes.byref(t))
    return out


@pytest.mark.parametrize('tiles,batch,grid', CASES)
def test_walk_covers_every_tile_once(lib, tiles, batch, grid):
    total = tiles * batch
    chunk = (total + 7) // 8
    seen = set()
    counts = []
    for b in range(grid):
        units = _walk(lib, tiles, batch, grid, b)
        counts.append(len(units))
        last = -1
        for e, t in units:
            assert 0 <= e < batch and 0 <= t < tiles
            u = e * tiles + t
            assert (b & 7) * chunk <= u < min(((b & 7) + 1) * chunk, total), "tile outside the block's XCD chunk"
            assert u > last                      # a block's tiles ascend
            last = u
            assert (e, t) not in seen
            seen.add((e, t))
    assert len(seen) == total
    # blocks of one XCD differ by at most one tile
    for x in range(8):
        c = counts[x::8]
        assert max(c) - min(c) <= 1


def test_grid(lib):
    assert lib.emp_conv_stream_grid(3072, 1) == 768
    assert lib.emp_conv_stream_grid(86, 36) == 768
    assert lib.emp_conv_stream_grid(5, 1) == 8
    assert lib.emp_conv_stream_grid(13, 3) == 40
    assert lib.emp_conv_stream_grid(0, 1) == 0


def test_walk_rejects_bad_arguments(lib):
    e, t = ctypes.c_int64(), ctypes.c_int64()
    for args in [(0, 1, 8, 0, 0), (8, 0, 8, 0, 0), (8, 1, 12, 0, 0), (8, 1, 8, 8, 0), (8, 1, 8, -1, 0), (8, 1, 8, 0, -1)]:
        assert lib.emp_conv_stream_walk(*args, ctypes.byref(e), ctypes.byref(t)) == 0


def test_eligibility_is_a_host_query(lib):
    q = lib.emp_conv_stream_eligible
    assert q(1, 1 << 21, 256, 256, 1, 1, 1, 0, 1, 0, 0) == 1        # the heads' pointwise convolution at the bench's size
    assert q(1, 1 << 21, 256, 256, 1, 1, 1, 0, 1, 0, 1) == 0        # ... through the proj entry: not taken over
    assert q(1, 1 << 21, 256, 256, 3, 3, 1, 1, 1, 0, 0) == 0
    assert q(1, 1 << 21, 256, 256, 1, 1, 2, 0, 1, 0, 0) == 0
    assert q(1, 1 << 21, 256, 256, 1, 1, 1, 0, 1, 1, 0) == 0
    assert q(1, 1 << 21, 256, 64, 1, 1, 1, 0, 1, 0, 0) == 0
    assert q(1, 1 << 21, 256, 128, 1, 1, 1, 0, 1, 0, 0) == 0        # a weight-stationary shape stays where it is
    assert q(36, 8192, 64, 64, 1, 1, 1, 0, 0, 0, 0) == 0
