"""Reference for the work-item lists and the split-tile hand-offs (numpy only).

``piled_scene``: 5,800 Gaussians of which 3,500 sit in one pile at the origin, so that one tile's pair list is tens
of work items long at a work-item length of 64 while other tiles are empty or hold a single item: the uneven load the
cross-workgroup hand-offs (split-tile partial sums, the finished-tile fan-in, the column scan's fan-in) are tested
under.  ``work_items``: the list the builders must produce from the per-virtual-tile pair ranges, restated from the
comment above k_work_items in gr_hip.hip.
"""
from __future__ import annotations

import numpy as np

from oracle import oracle as orc

N_PILE, N_SPREAD, N_BROAD = 3500, 2000, 300


def piled_scene(seed: int = 5) -> orc.Scene:
    rng = np.random.default_rng(seed)
    pile = rng.normal(0.0, 0.03, (N_PILE, 3))
    spread = (rng.random((N_SPREAD, 3)) - 0.5) * 1.2
    broad = (rng.random((N_BROAD, 3)) - 0.5) * 0.8
    means = np.concatenate([pile, spread, broad])
    scales = np.concatenate([np.full((N_PILE, 3), 0.02), np.full((N_SPREAD, 3), 0.03), np.full((N_BROAD, 3), 0.12)])
    n = means.shape[0]
    perm = rng.permutation(n)
    means, scales = means[perm], scales[perm]
    colors = rng.random((n, 3))
    opacities = 0.02 + 0.3 * rng.random(n)
    return orc.Scene(means.astype(np.float32), scales.astype(np.float32), colors.astype(np.float32),
                     opacities.astype(np.float32))


def list_lengths(ranges) -> np.ndarray:
    """Pairs of each virtual tile's list (an empty list may be stored as any range with end <= start)."""
    r = np.asarray(ranges, np.int64).reshape(-1, 2)
    return np.maximum(r[:, 1] - r[:, 0], 0)


def chunks(lens, ch: int) -> np.ndarray:
    return (np.asarray(lens, np.int64) + ch - 1) // ch


def work_items(ranges, ch: int):
    """(items (num, 4) int32, num_items (2,) int32 = (all, non-empty), tile_item0 (2 tiles,) int32) for the pair
    ranges (2 tiles, 2) of the virtual tiles (2t: core list of tile t, 2t + 1: its tail list) at work-item length ch:
    the non-empty tiles in tile order, per tile its core chunks then its tail chunks, each [k0, min(k1, k0 + ch)) with
    its chunk index; then one (2t, 0, 0, 0) item per tile empty in both zones, in tile order.  tile_item0[v]: the first
    item of list v (an empty list of a non-empty tile: where it would start; an empty tile: its empty item, both)."""
    r = np.asarray(ranges, np.int64).reshape(-1, 2)
    assert r.shape[0] % 2 == 0 and ch > 0
    tiles = r.shape[0] // 2
    lens = list_lengths(r)
    items, empty = [], []
    tile_item0 = np.zeros(2 * tiles, np.int32)
    for t in range(tiles):
        if lens[2 * t] + lens[2 * t + 1] == 0:
            empty.append(t)
            continue
        for v in (2 * t, 2 * t + 1):
            tile_item0[v] = len(items)
            k0, k1 = (int(r[v, 0]), int(r[v, 1])) if lens[v] > 0 else (0, 0)
            for c in range((k1 - k0 + ch - 1) // ch):
                items.append((v, k0 + c * ch, min(k1, k0 + (c + 1) * ch), c))
    full = len(items)
    for t in empty:
        tile_item0[2 * t] = tile_item0[2 * t + 1] = len(items)
        items.append((2 * t, 0, 0, 0))
    return (np.asarray(items, np.int32).reshape(-1, 4), np.asarray([len(items), full], np.int32), tile_item0)


def compare_items(got_items, got_num, got_item0, ranges, ch: int) -> None:
    """Asserts that a builder's lists are the expected ones, word for word."""
    items, num, item0 = work_items(ranges, ch)
    np.testing.assert_array_equal(np.asarray(got_num).reshape(2), num, err_msg="num_items (all, non-empty)")
    np.testing.assert_array_equal(np.asarray(got_item0).reshape(-1), item0, err_msg="tile_item0")
    np.testing.assert_array_equal(np.asarray(got_items).reshape(-1, 4)[:num[0]], items, err_msg="items")


def tile_items(ranges, ch: int) -> np.ndarray:
    """Work items of each tile (both zones; an empty tile's one item counts)."""
    c = chunks(list_lengths(ranges), ch).reshape(-1, 2).sum(axis=1)
    return np.maximum(c, 1)


def load_conditions(ranges, ch: int = 64) -> dict:
    """What makes a view an uneven load, counted in tiles at work-item length ch: empty tiles, tiles of exactly one
    item, tiles of 32 or more items, tiles whose core and tail lists both split; and the longest tile's items."""
    lens = list_lengths(ranges).reshape(-1, 2)
    c = chunks(lens, ch)
    per = c.sum(axis=1)
    return {"pairs": int(lens.sum()), "tiles": int(lens.shape[0]), "empty": int((lens.sum(axis=1) == 0).sum()),
            "one_item": int((per == 1).sum()), "long": int((per >= 32).sum()), "longest": int(per.max()),
            "both_split": int(((c[:, 0] >= 2) & (c[:, 1] >= 2)).sum())}


FAN_STRIDE = 32  # ints between the fan-in counters (one 128-byte line each)


def fan_offset(tiles: int) -> int:
    """Int index of the first fan-in counter behind the ``tiles`` per-tile tickets (gr_hip.h gr_items_layout)."""
    return (tiles + 1 + FAN_STRIDE - 1) // FAN_STRIDE * FAN_STRIDE


def ticket_words(tiles: int) -> int:
    """Ints of the ticket region: the per-tile tickets, then nine lines of FAN_STRIDE."""
    return fan_offset(tiles) + 9 * FAN_STRIDE


def assert_tickets_zero(ticket, tiles: int) -> None:
    """Every per-tile ticket and each of the nine fan-in counters (eight shards, then the top counter) reads zero."""
    ticket = np.asarray(ticket).reshape(-1)
    assert ticket.shape[0] >= fan_offset(tiles) + 8 * FAN_STRIDE + 1
    bad = np.nonzero(ticket[:tiles])[0]
    assert bad.size == 0, f"ticket of tile {int(bad[0])} left at {int(ticket[bad[0]])} ({bad.size} tiles)"
    for k in range(9):
        v = int(ticket[fan_offset(tiles) + FAN_STRIDE * k])
        assert v == 0, f"fan-in counter {k} left at {v}"


def assert_uneven(ranges, two_zones: bool, ch: int = 64) -> dict:
    d = load_conditions(ranges, ch)
    assert d["empty"] >= 1 and d["one_item"] >= 1 and d["long"] >= 1, d
    if two_zones:
        assert d["both_split"] >= 1, d
    return d
