"""CPU: the cut of a slab into z-blocks that the labelled-volume stages of _hip.py share -- the voxels per call they were
asked for, the whole slices that makes, and the walk over the blocks with their true neighbour slices.  CPU tensors:
nothing here touches the GPU."""
import pytest
import torch


def test_z_blocks_walk_with_true_neighbours():
    from empanada_amd._hip import _z_blocks
    slab = torch.arange(5 * 2 * 3, dtype=torch.int32).reshape(5, 2, 3)
    below, above = torch.full((2, 3), -1, dtype=torch.int32), torch.full((2, 3), -2, dtype=torch.int32)
    blocks = list(_z_blocks(slab, below, above, 2))
    assert [(z0, z1) for z0, z1, _, _, _ in blocks] == [(0, 2), (2, 4), (4, 5)]
    for z0, z1, part, _, _ in blocks:
        assert part.data_ptr() == slab[z0].data_ptr() and tuple(part.shape) == (z1 - z0, 2, 3)     # views, no copies
        assert torch.equal(part, slab[z0:z1])
    los, his = [b[3] for b in blocks], [b[4] for b in blocks]
    assert los[0] is below and his[2] is above
    assert [t.data_ptr() for t in los[1:]] == [slab[1].data_ptr(), slab[3].data_ptr()]
    assert [t.data_ptr() for t in his[:2]] == [slab[2].data_ptr(), slab[4].data_ptr()]
    assert torch.equal(los[1], slab[1]) and torch.equal(los[2], slab[3])
    assert torch.equal(his[0], slab[2]) and torch.equal(his[1], slab[4])
    # no neighbour given: None at the ends, the slab's own slices inside
    blocks = list(_z_blocks(slab, None, None, 3))
    assert [(b[0], b[1]) for b in blocks] == [(0, 3), (3, 5)]
    assert blocks[0][3] is None and blocks[1][4] is None
    assert torch.equal(blocks[0][4], slab[3]) and torch.equal(blocks[1][3], slab[2])
    # one block holds everything; an empty slab has no block
    assert [(b[0], b[1], b[3] is below, b[4] is above) for b in _z_blocks(slab, below, above, 7)] == [(0, 5, True, True)]
    assert list(_z_blocks(slab[:0], below, above, 2)) == []


@pytest.mark.parametrize('bad', [True, 0, 1.5, 101])
def test_block_voxels_errors(bad):
    from empanada_amd._hip import _block_voxels
    with pytest.raises(ValueError) as e:
        _block_voxels("measure_labels", bad, 100)
    assert str(e.value) == f"measure_labels: block_voxels must lie in 1 .. 100, got {bad!r}"


def test_block_voxels_and_slices():
    import numpy as np
    from empanada_amd._hip import _block_slices, _block_voxels
    assert _block_voxels("label_holes", None, 100) == 100                         # None: the kernel's limit
    assert _block_voxels("label_holes", 1, 100) == 1 and _block_voxels("label_holes", 100, 100) == 100
    got = _block_voxels("label_holes", np.int64(7), 100)
    assert got == 7 and type(got) is int
    assert _block_slices("label_holes", 4, 5, 100) == 5
    assert _block_slices("label_holes", 4, 5, 99) == 4
    assert _block_slices("label_holes", 4, 5, 20) == 1                            # exactly one slice
    assert _block_slices("label_holes", 0, 5, 20) == 20                           # no voxels: nothing to divide by
    with pytest.raises(ValueError) as e:
        _block_slices("label_holes", 4, 5, 19)
    assert str(e.value) == ("label_holes: a single slice of 4 x 5 = 20 voxels exceeds the limit of 19 voxels per call; "
                            "there is no split within a slice")


def test_stage_texts_through_an_entry_point():
    """the helpers raise under the stage's own name, before anything asks for a GPU"""
    from empanada_amd import _hip
    slab = torch.zeros((2, 4, 5), dtype=torch.uint8)
    for bad in (True, 0, 1.5, 2 ** 31):
        with pytest.raises(ValueError) as e:
            _hip.label_components(slab, block_voxels=bad)
        assert str(e.value) == f"label_components: block_voxels must lie in 1 .. {2 ** 31 - 1}, got {bad!r}"
    with pytest.raises(ValueError, match="label_components: a single slice of 4 x 5 = 20 voxels exceeds the limit of 19"):
        _hip.label_components(slab, block_voxels=19)


@pytest.mark.parametrize('dtype', [torch.uint8, torch.uint32])
def test_z_stack_equals_a_concatenation_of_the_same_slices(dtype):
    """every (lo, hi) that _morph, label_contacts and label_thickness form: the halo of 2 slices under and over each
    block of 1, 2 or 5 slices of a slab of 5, with 1 slice of the caller's below it and 3 above"""
    import numpy as np
    from empanada_amd._hip import _z_stack
    D, halo, n_below, n_above = 5, 2, 1, 3
    whole = np.arange((n_below + D + n_above) * 2 * 3, dtype=np.int64).reshape(-1, 2, 3) + 7
    whole = whole.astype(np.uint8 if dtype == torch.uint8 else np.uint32)
    whole[-1] = whole.max() if dtype == torch.uint8 else 2 ** 32 - 1

    def tensor(a):
        a = np.ascontiguousarray(a)
        return torch.from_numpy(a) if dtype == torch.uint8 else torch.from_numpy(a.view(np.int32)).view(torch.uint32)

    def host(t):
        return t.numpy() if dtype == torch.uint8 else t.view(torch.int32).numpy().view(np.uint32)

    below, slab, above = tensor(whole[:n_below]), tensor(whole[n_below:n_below + D]), tensor(whole[n_below + D:])
    for per in (1, 2, 5):
        for z0 in range(0, D, per):
            z1 = min(D, z0 + per)
            for lo, hi in ((z0 - halo, z0), (z1, z1 + halo)):
                for lo_stack, hi_stack in ((below, above), (None, above), (below, None), (None, None)):
                    first = max(lo, -n_below if lo_stack is not None else 0)
                    last = min(hi, D + (n_above if hi_stack is not None else 0))
                    expected = np.concatenate([whole[n_below + z:n_below + z + 1] for z in range(first, last)] +
                                              [whole[:0]])
                    got, n = _z_stack(slab, lo, hi, lo_stack, hi_stack)
                    assert n == len(expected)
                    if n == 0:
                        assert got is None
                        continue
                    assert got.dtype == dtype and got.is_contiguous()
                    np.testing.assert_array_equal(host(got), expected)
                    if 0 <= lo and hi <= D:                                   # one part suffices: a view of the slab
                        assert got.data_ptr() == slab[lo].data_ptr()


def test_halo_blocks_refuse_a_block_exactly_above_the_limit():
    from empanada_amd._hip import _halo_blocks
    # 5 slices of 2 x 3 in blocks of 2 with 1 halo slice: 1 + 2 + 1, 1 + 2 + 1 and 1 + 1 + 0 slices with one slice below
    assert _halo_blocks("label_erode", 5, 2, 3, 2, 1, 1, 0, 24) == [(0, 2), (2, 4), (4, 5)]
    with pytest.raises(ValueError) as e:
        _halo_blocks("label_erode", 5, 2, 3, 2, 1, 1, 0, 23)
    assert str(e.value) == ("label_erode: a block of 2 slices of 2 x 3 with its halo slices is 24 voxels, above the limit "
                            "of 23 voxels per call")
    # without the caller's slice below, the first block has no halo under it: the second one is the first above the limit
    assert _halo_blocks("label_thickness", 5, 2, 3, 2, 1, 0, 0, 24) == [(0, 2), (2, 4), (4, 5)]
    with pytest.raises(ValueError, match="a block of 2 slices of 2 x 3 with its halo slices is 24 voxels, above the "
                                         "limit of 23"):
        _halo_blocks("label_thickness", 5, 2, 3, 2, 1, 0, 0, 23)
    assert _halo_blocks("label_thickness", 5, 2, 3, 5, 2, 1, 3, 48) == [(0, 5)]         # 1 + 5 + 2 slices
    with pytest.raises(ValueError, match="a block of 5 slices of 2 x 3 with its halo slices is 48 voxels"):
        _halo_blocks("label_thickness", 5, 2, 3, 5, 2, 1, 3, 47)
    assert _halo_blocks("label_edt", 0, 2, 3, 4, 1, 0, 0, 1) == []                      # an empty slab has no block


def test_one_table_and_the_small_checks():
    from empanada_amd import _hip
    merged = []

    def merge(tables):
        merged.append(len(tables))
        return 'merged'
    assert _hip._one_table([], 'empty', merge) == 'empty'
    assert _hip._one_table(['only'], 'empty', merge) == 'only'
    assert _hip._one_table(['a', 'b'], 'empty', merge) == 'merged' and merged == [2]
    assert _hip._dhw("label_mesh", torch.zeros((2, 4, 5))) == (2, 4, 5)
    with pytest.raises(ValueError) as e:
        _hip._dhw("label_graph", torch.zeros((4, 5)), "skel")
    assert str(e.value) == "label_graph: skel must be a (D, H, W) tensor, got (4, 5)"
    _hip._z_base("label_holes", 0)
    for bad in (True, -1, 1.0):
        with pytest.raises(ValueError) as e:
            _hip._z_base("label_holes", bad)
        assert str(e.value) == f"label_holes: z_base must be a non-negative integer, got {bad!r}"
