"""Host model of the TRIANGULAR workgroup -> tile map of the persistent INT8 GEMM kernels (oz2_gemm_common.hpp make_tile_map_tri /
map_tile_tri / map_tile with TileMapArgs.tri != 0; gemmul8_syrk), line for line with the device code, in the style of test_tile_map.py:
over the virtual workgroup ids 0 .. total-1 every (plane, tile-row, tile-column) of the triangle must come exactly once and nothing else
may come at all -- the walk has no skipped slots, so the producer and consumer waves of the kernel keep one loop.  No GPU needed."""
import pytest

from test_tile_map import magic, udivmod_magic


def make_tile_map_tri(T, tri):
    a = dict(T=T, tri=tri)
    a["tpp"] = T * (T + 1) // 2
    a["m_tpp"] = magic(a["tpp"])
    npairs = (T - 7) // 8 + 1 if T >= 7 else 0
    a["pr"] = 4 * T
    a["m_pr"] = magic(a["pr"])
    a["s_pairs"] = npairs * a["pr"]
    a["t0"] = 4 * npairs - 1 if npairs else 0
    a["th"] = T - a["t0"] - 4 * npairs
    a["m_th"] = magic(a["th"])
    return a


def map_trapezoid(q, h, a0, M):
    full = h * (a0 + 1)
    if q < full:
        if h == 4:
            return a0 + (q & 3), q >> 2
        c, r = udivmod_magic(q, h, M)
        return a0 + r, c
    d = q - full
    i = 1 + (d >= 1) + (d >= 3) + (d >= 6) + (d >= 10) + (d >= 15)
    return a0 + i, a0 + 1 + d - i * (i - 1) // 2


def map_tile_tri(rem, a):
    if rem < a["s_pairs"]:
        p, q = udivmod_magic(rem, a["pr"], a["m_pr"])
        ll = a["pr"] - 16 * p - 6
        if q < ll:
            return map_trapezoid(q, 4, a["T"] - 4 - 4 * p, 0)
        return map_trapezoid(q - ll, 4, 4 * p - 1, 0)
    return map_trapezoid(rem - a["s_pairs"], a["th"], a["t0"], a["m_th"])


def canonical(bid, nwg):
    """the XCD chunking at the head of map_tile (shared with the rectangular walk)"""
    xcd, idx = bid & 7, bid >> 3
    fc = (nwg >> 3) >> 5
    if idx < fc * 32:
        return (idx >> 5) * 256 + xcd * 32 + (idx & 31)
    rem = nwg - fc * 256
    q, r = rem >> 3, rem & 7
    return fc * 256 + (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + (idx - fc * 32)


def map_tile(bid, nwg, a):
    plane, rem = udivmod_magic(canonical(bid, nwg), a["tpp"], a["m_tpp"])
    tm, tn = map_tile_tri(rem, a)
    return (plane, tm, tn) if a["tri"] == 1 else (plane, tn, tm)


def test_the_middle_rows_are_at_most_seven():
    for T in list(range(1, 71)) + [130]:
        a = make_tile_map_tri(T, 1)
        assert 0 <= a["th"] <= 7 and (a["th"] > 0 or T >= 7), T


@pytest.mark.parametrize("tri", [1, 2])
@pytest.mark.parametrize("planes", [1, 2, 14])
def test_every_triangle_tile_exactly_once_and_nothing_else(tri, planes):
    for T in list(range(1, 71)) + [130]:
        a = make_tile_map_tri(T, tri)
        total = planes * T * (T + 1) // 2
        seen = [map_tile(vb, total, a) for vb in range(total)]
        want = {(p, tm, tn) for p in range(planes) for tm in range(T) for tn in range(T) if (tm >= tn if tri == 1 else tm <= tn)}
        assert len(seen) == len(set(seen)) == total, (T, planes)
        assert set(seen) == want, (T, planes)


def _canon_tiles(T, tri=1):
    a = make_tile_map_tri(T, tri)
    total = T * (T + 1) // 2
    return [map_tile_tri(c, a) for c in range(total)]


def test_groups_keep_the_panel_sharing_of_the_rectangle():
    """Inside the full columns of a 4-row group the order is the rectangle's (tile-row fastest): 32 consecutive tiles = 4 tile-rows x 8
    tile-columns = 12 panels, the rectangle's 8 x 4.  T = 64 (n = 16384): every aligned run of 32 canonical tiles -- an XCD's share of a chunk --
    lies in at most two groups; any 256 consecutive tiles lie in at most two pairs (16 tile-rows)."""
    tiles = _canon_tiles(64)
    a = make_tile_map_tri(64, 1)
    for p in range(8):
        a0 = 60 - 4 * p
        for c in range(0, a0 + 1 - 7, 8):
            run = [map_tile_tri(p * a["pr"] + 4 * c + i, a) for i in range(32)]
            assert {tm for tm, _ in run} == set(range(a0, a0 + 4)) and {tn for _, tn in run} == set(range(c, c + 8))
            assert [tm for tm, _ in run[:4]] == list(range(a0, a0 + 4))
    for s in range(0, len(tiles) - 31, 32):
        rows = {tm for tm, _ in tiles[s:s + 32]}
        assert len(rows) <= 8, (s, rows)
    for s in range(0, len(tiles) - 255):
        assert len({tm for tm, _ in tiles[s:s + 256]}) <= 16, s


def test_chunk_property_T64_256_consecutive_tiles_touch_at_most_8_tile_rows():
    """The check as the feature request states it, for the chunks of 256 the kernel runs at once (canonical tiles [256 c, 256 c + 256)): for
    T = 64 a pair of 4-row groups is 4 T = 256 tiles, so every chunk is one pair and touches 8 tile-rows (the first 7: tile-rows 0 .. 2 and
    60 .. 63; the last chunk is tile-row 31 alone).  This is the aligned reading: an UNALIGNED window of 256 consecutive tiles straddles two pairs and
    touches up to 16 tile-rows (asserted in test_groups_keep_the_panel_sharing_of_the_rectangle), and so do the aligned chunks of every T other than
    64: above it a pair is longer than a chunk, below it a chunk holds 256 / (4 T) pairs (T = 32, n = 8192: two pairs, 16 tile-rows)."""
    tiles = _canon_tiles(64)
    worst = [len({tm for tm, _ in tiles[c:c + 256]}) for c in range(0, len(tiles), 256)]
    print("tile-rows touched by the aligned chunks:", worst)
    assert worst == [7, 8, 8, 8, 8, 8, 8, 8, 1]
    assert max(worst) <= 8, worst
