"""CPU: the hand-off tests' scene and expected work-item lists (tests/handoff_reference.py).

* ``piled_scene`` through the oracle's binning still gives the uneven load the GPU tests rely on (empty tiles, one-item
  tiles, a tile of 32 or more items at a work-item length of 64, in two-zone views a tile whose core and tail lists
  both split), so those tests cannot pass vacuously after someone edits the scene;
* ``work_items`` on hand-written range tables;
* the comparisons the GPU tests use reject the lists a broken builder would leave (a tail list's tile_item0 equal to
  the core list's, the empty tiles' items missing) and a ticket region that was not left zero.
"""
from __future__ import annotations

import numpy as np
import pytest

import handoff_reference as hr
from oracle import oracle as orc

# name: (W, H, tile, cutoff, core cutoff); the one-zone views are the fit path's (5 sigma)
VIEWS = {
    "112x80_t16_two_zones": (112, 80, 16, 7.0, 5.5),
    "112x80_t16_one_zone": (112, 80, 16, 5.0, 5.0),
    "112x80_t32_one_zone": (112, 80, 32, 5.0, 5.0),
    "200x120_t16_two_zones": (200, 120, 16, 7.0, 5.5),
}


def oracle_ranges(scene, W, H, tile, cutoff, core):
    view, proj = orc.orbit_cameras(4, W, H)[1]
    v = orc.make_view(view, proj, W, H, None, cutoff=cutoff, core_cutoff=core, tile=tile)
    rec, rect, counts = orc.preprocess(v, scene)
    return orc.bin_pairs(v, rec, rect, counts)[3]


@pytest.mark.parametrize("name", list(VIEWS))
def test_piled_scene_is_an_uneven_load(name):
    W, H, tile, cutoff, core = VIEWS[name]
    ranges = oracle_ranges(hr.piled_scene(), W, H, tile, cutoff, core)
    two = core < cutoff
    d = hr.assert_uneven(ranges, two)
    print(f"{name}: {d}")
    assert d["tiles"] == ((W + tile - 1) // tile) * ((H + tile - 1) // tile)
    assert d["longest"] <= 84  # the per-tile bar of the GPU tests is derived for tiles of at most 84 items
    # at the default work-item length (512 for these pair counts) the piled tile still splits
    assert hr.load_conditions(ranges, 512)["longest"] >= 4
    if not two:
        assert not hr.list_lengths(ranges)[1::2].any()


def test_piled_scene_is_seeded():
    a, b = hr.piled_scene(), hr.piled_scene()
    for x, y in zip(a.arrays(), b.arrays()):
        assert x.dtype == np.float32 and np.array_equal(x, y)
    assert a.means.shape == (5800, 3) and a.opacities.min() >= 0.02 and a.opacities.max() <= 0.32
    assert not np.array_equal(a.means, hr.piled_scene(6).means)


def test_work_items_hand_written():
    # 3 tiles at ch = 4: tile 0 core 9 pairs (chunks 4, 4, 1) and tail 4 pairs (an exact multiple: one chunk, no
    # empty one behind it); tile 1 empty; tile 2 tail only, 5 pairs
    ranges = [[0, 9], [20, 24], [0, 0], [0, 0], [0, 0], [24, 29]]
    items, num, item0 = hr.work_items(ranges, 4)
    assert items.tolist() == [[0, 0, 4, 0], [0, 4, 8, 1], [0, 8, 9, 2], [1, 20, 24, 0], [5, 24, 28, 0], [5, 28, 29, 1],
                              [2, 0, 0, 0]]
    assert num.tolist() == [7, 6]
    assert item0.tolist() == [0, 3, 6, 6, 4, 4]
    assert hr.tile_items(ranges, 4).tolist() == [4, 1, 2]


def test_work_items_all_empty():
    ranges = np.zeros((8, 2), np.int32)
    ranges[3] = (7, 7)  # an empty list stored with a non-zero start
    items, num, item0 = hr.work_items(ranges, 64)
    assert items.tolist() == [[0, 0, 0, 0], [2, 0, 0, 0], [4, 0, 0, 0], [6, 0, 0, 0]]
    assert num.tolist() == [4, 0]
    assert item0.tolist() == [0, 0, 1, 1, 2, 2, 3, 3]


def test_work_items_exact_multiples_and_one_pair():
    # ch = 64: 128 pairs = exactly two chunks; 64 = exactly one; 1 pair; an empty tile between non-empty ones
    ranges = [[0, 128], [0, 0], [128, 192], [300, 301], [0, 0], [0, 0], [192, 193], [301, 429]]
    items, num, item0 = hr.work_items(ranges, 64)
    assert items.tolist() == [[0, 0, 64, 0], [0, 64, 128, 1], [2, 128, 192, 0], [3, 300, 301, 0], [6, 192, 193, 0],
                              [7, 301, 365, 0], [7, 365, 429, 1], [4, 0, 0, 0]]
    assert num.tolist() == [8, 7]
    assert item0.tolist() == [0, 2, 2, 3, 7, 7, 4, 5]
    # every pair of every list is covered once, in order
    for v, (a, b) in enumerate(ranges):
        mine = items[(items[:, 0] == v) & (items[:, 2] > items[:, 1])]
        assert mine[:, 3].tolist() == list(range(len(mine)))
        assert (b == a and len(mine) == 0) or (mine[0, 1] == a and mine[-1, 2] == b and (mine[1:, 1] == mine[:-1, 2]).all())


def test_comparisons_reject_broken_lists():
    """The mutations a broken builder or consumer would leave, fed to the comparisons the GPU tests use."""
    W, H, tile, cutoff, core = VIEWS["112x80_t16_two_zones"]
    ranges = oracle_ranges(hr.piled_scene(), W, H, tile, cutoff, core)
    items, num, item0 = hr.work_items(ranges, 64)
    hr.compare_items(items, num, item0, ranges, 64)
    cap = np.concatenate([items, np.full((5, 4), -7, np.int32)])  # the buffer's unused capacity is not compared
    hr.compare_items(cap, num, item0, ranges, 64)
    # the tail chunks' first item taken for the core chunks' (tile_item0[2t + 1] = tile_item0[2t])
    bad0 = item0.copy()
    bad0[1::2] = item0[0::2]
    assert not np.array_equal(bad0, item0)
    with pytest.raises(AssertionError, match="tile_item0"):
        hr.compare_items(items, num, bad0, ranges, 64)
    # the empty tiles' items not written (the capacity's old contents instead), or not counted
    bad_items = items.copy()
    bad_items[num[1]:] = -7
    with pytest.raises(AssertionError, match="items"):
        hr.compare_items(bad_items, num, item0, ranges, 64)
    with pytest.raises(AssertionError, match="num_items"):
        hr.compare_items(items, np.asarray([num[1], num[1]], np.int32), item0, ranges, 64)
    # a chunk cut one pair short
    bad_items = items.copy()
    bad_items[0, 2] -= 1
    with pytest.raises(AssertionError, match="items"):
        hr.compare_items(bad_items, num, item0, ranges, 64)
    # a split tile's ticket left at its item count (no reset by the last arrival); a fan-in counter left raised
    tiles = len(ranges) // 2
    words = hr.ticket_words(tiles)
    ticket = np.zeros(words, np.int32)
    hr.assert_tickets_zero(ticket, tiles)
    t = int(np.argmax(hr.tile_items(ranges, 64)))
    ticket[t] = hr.tile_items(ranges, 64)[t]
    with pytest.raises(AssertionError, match=f"ticket of tile {t}"):
        hr.assert_tickets_zero(ticket, tiles)
    ticket[t] = 0
    ticket[hr.fan_offset(tiles) + 32 * 8] = 1
    with pytest.raises(AssertionError, match="fan-in counter 8"):
        hr.assert_tickets_zero(ticket, tiles)
