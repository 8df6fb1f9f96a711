"""The last layer's scan range of a split call (medaka_amd/csrc/gru_split.hpp `plan_scan_ranges`, exported device-free as
`mdk_split_scan_ranges`; option "scan_split_trim"): runs without a GPU.  What the device side (rec_fused.hpp, `rng`) and the
certificate (scan_split.hpp k_split_verify) rely on, over the grid of shapes the plan itself is tested on:
  * every range lies inside the virtual window, and the four launch lengths around the chunk's midpoint are whole strips of 8;
  * a range contains the chunk's delivered columns and every layer-1 certificate column read from that chunk -- both points of
    both junctions it takes part in, as the warm and as the carried side;
  * a chunk that starts at a window's own end starts its scan there;
  * what the second launch finishes lies inside what the other direction covered in the first;
  * the longest range is core + margin (level 2) or core + 1.5 margin (level 1), up to the rounding to strips;
  * level 0 is the whole window, and the plan itself (`mdk_split_plan`) does not depend on any of this."""
import pytest
from hypothesis import given, settings, strategies as st

from medaka_amd import engine, lib

STRIP = 8


def check_ranges(B, T, share, mode, margin, trim):
    p = engine.split_plan(B, T, share, mode, margin)
    r = engine.split_scan_ranges(B, T, share, mode, margin, trim)
    S, Tv, G = p["chunks"], p["columns"], p["margin"]
    assert r["chunks"] == S
    if S == 1:
        assert r["trim"] == 0 and r["lo_fwd"] == [0] and r["lo_rev"] == [0] and r["hi_fwd"] == [T] and r["hi_rev"] == [T]
        return r
    assert r["trim"] == trim
    lead = G if trim == 1 else G // 2
    for k in range(S):
        s, a, b = p["start"][k], p["first"][k], p["last"][k]
        lo_f, hi_f, lo_r, hi_r, mid = (r[n][k] for n in ("lo_fwd", "hi_fwd", "lo_rev", "hi_rev", "mid"))
        if trim == 0:
            assert (lo_f, hi_f, lo_r, hi_r, mid) == (0, Tv, 0, Tv, Tv // 2 // STRIP * STRIP)
            continue
        # inside the virtual window; whole strips on either side of the midpoint, none of them empty
        assert 0 <= lo_f <= lo_r < mid < hi_f <= hi_r <= Tv, (k, r, p)
        for n in (mid - lo_f, hi_r - mid, hi_f - mid, mid - lo_r):
            assert n > 0 and n % STRIP == 0, (k, r, p)
        assert all(v % STRIP == 0 for v in (lo_f, hi_f, lo_r, hi_r, mid))      # ... hence also around the midpoint of any union of ranges
        # the delivered columns
        for lo, hi in ((lo_f, hi_f), (lo_r, hi_r)):
            assert lo <= a - s and b - s <= hi, (k, r, p)
        # a chunk that starts at a window end starts its scan there
        if k == 0:
            assert lo_f == 0 and lo_r == 0
        if k == S - 1:
            assert s + hi_r == T and s + hi_f == T
        # launch 2 finishes only columns that have the other direction's partial logits from launch 1
        assert lo_f <= lo_r and hi_f <= hi_r
        # the longest range: core + margin / 2 behind it + `lead` in front of it, rounded outwards to strips
        for lo, hi in ((lo_f, hi_f), (lo_r, hi_r)):
            assert hi - lo <= (b - a) + G // 2 + lead + 2 * (STRIP - 1), (k, r, p)
    if trim == 0:
        return r
    # layer-1 certificate columns (scan_split.hpp k_split_verify): junction j at a = first[j + 1]; direction 0 reads a - 1 and
    # a - 1 + G/2, direction 1 reads a and a - G/2, each from chunk j and from chunk j + 1
    for j in range(S - 1):
        a = p["first"][j + 1]
        for k in (j, j + 1):
            s = p["start"][k]
            for t in (a - 1, a - 1 + G // 2):
                assert r["lo_fwd"][k] <= t - s < r["hi_fwd"][k], (j, k, t, r, p)
            for t in (a, a - G // 2):
                assert r["lo_rev"][k] <= t - s < r["hi_rev"][k], (j, k, t, r, p)
        # the warm side has run at least `lead` columns (less the one the junction state sits on) when it is first compared
        assert (a - 1) - (p["start"][j + 1] + r["lo_fwd"][j + 1]) >= lead - 1
        assert (p["start"][j] + r["hi_rev"][j] - 1) - a >= lead - 1
    return r


@settings(max_examples=400, deadline=None)
@given(B=st.integers(1, 1200), T=st.integers(1, 40000), share=st.integers(1, 8), mode=st.integers(1, 16),
       margin=st.sampled_from([16, 32, 64, 128, 256, 512, 1024, 4096]), trim=st.sampled_from([1, 2]))
def test_range_properties(B, T, share, mode, margin, trim):
    check_ranges(B, T, share, mode, margin, trim)


@settings(max_examples=100, deadline=None)
@given(B=st.integers(1, 1200), T=st.integers(1, 40000), share=st.integers(1, 8), mode=st.integers(1, 16),
       margin=st.sampled_from([16, 32, 64, 128, 256, 512, 1024, 4096]))
def test_level_0_is_the_whole_window(B, T, share, mode, margin):
    check_ranges(B, T, share, mode, margin, 0)


def check_tiles(B, T, share, mode, margin, trim):
    """What the device runs (layout.hpp split_tile_range, exported as mdk_split_tile_ranges): a recurrence tile is 8 consecutive
    virtual windows (virtual window k * B + w = chunk k of window w) and takes the union of its chunks' ranges and the midpoint
    of that union.  Everything a chunk's own range guarantees must hold for every tile the chunk has windows in."""
    p = engine.split_plan(B, T, share, mode, margin)
    r = engine.split_scan_ranges(B, T, share, mode, margin, trim)
    tiles = engine.split_tile_ranges(B, T, share, mode, margin, trim)
    S, Tv, G = p["chunks"], p["columns"], p["margin"]
    nb = S * B
    assert len(tiles) == (nb + 7) // 8
    for t, (lo_f, hi_f, lo_r, hi_r, mid) in enumerate(tiles):
        chunks = sorted({w // B for w in range(8 * t, min(8 * t + 8, nb))})
        # the union over the tile's chunks, and the middle of the union of both directions, on a strip boundary
        assert lo_f == min(r["lo_fwd"][k] for k in chunks) and hi_f == max(r["hi_fwd"][k] for k in chunks), (t, tiles[t], r)
        assert lo_r == min(r["lo_rev"][k] for k in chunks) and hi_r == max(r["hi_rev"][k] for k in chunks), (t, tiles[t], r)
        assert mid == (lo_f + hi_r) // 2 // STRIP * STRIP
        if len(chunks) == 1:
            assert mid == r["mid"][chunks[0]]
        if S == 1:
            continue
        # both launches of both directions: whole strips, none empty, inside the window; launch 2 inside the other's launch 1
        assert 0 <= lo_f <= lo_r < mid < hi_f <= hi_r <= Tv, (t, tiles[t], p)
        for n in (mid - lo_f, hi_r - mid, hi_f - mid, mid - lo_r):
            assert n > 0 and n % STRIP == 0, (t, tiles[t], p)
        for k in chunks:
            s, a, b = p["start"][k], p["first"][k], p["last"][k]
            # every window of the tile gets its chunk's delivered columns finished in launch 2: reverse [lo_r, mid), forward [mid, hi_f)
            assert lo_r <= a - s and b - s <= hi_f, (t, k, tiles[t], p)
            # ... and its chunk's certificate columns scanned, in both roles
            for j in (k - 1, k):
                if 0 <= j < S - 1:
                    c = p["first"][j + 1]
                    for col in (c - 1, c - 1 + G // 2):
                        assert lo_f <= col - s < hi_f, (t, k, j, col, tiles[t], p)
                    for col in (c, c - G // 2):
                        assert lo_r <= col - s < hi_r, (t, k, j, col, tiles[t], p)
    return tiles


@settings(max_examples=300, deadline=None)
@given(B=st.integers(1, 1200), T=st.integers(1, 40000), share=st.integers(1, 8), mode=st.integers(1, 16),
       margin=st.sampled_from([16, 32, 64, 128, 256, 512, 1024, 4096]), trim=st.sampled_from([0, 1, 2]))
def test_tile_range_properties(B, T, share, mode, margin, trim):
    check_tiles(B, T, share, mode, margin, trim)


def _launches(B, T, margin, trim):
    """Steps of the two launches of the last layer: each lasts as long as its longest TILE."""
    tiles = check_tiles(B, T, 1, 1, margin, trim)
    first = max(max(mid - lo_f, hi_r - mid) for lo_f, hi_f, lo_r, hi_r, mid in tiles)
    second = max(max(hi_f - mid, mid - lo_r) for lo_f, hi_f, lo_r, hi_r, mid in tiles)
    return first, second


def test_headline_shape():
    """200 x 10 000 at margin 128: 5 chunks of 2256 columns, 25 tiles per chunk (no tile mixes chunks).  Both trims: chunk 0
    scans [0, 2064), the interior chunks [64, 2192), the last [192, 2256): 1064 + 1064 steps against 1128 + 1128; the trailing
    trim alone: 1128 + 1064."""
    r = check_ranges(200, 10000, 1, 1, 128, 2)
    assert [(r["lo_fwd"][k], r["hi_rev"][k]) for k in range(5)] == [(0, 2064)] + [(64, 2192)] * 3 + [(192, 2256)]
    assert r["lo_rev"] == r["lo_fwd"] and r["hi_fwd"] == r["hi_rev"]
    assert _launches(200, 10000, 128, 2) == (1064, 1064)
    assert _launches(200, 10000, 128, 1) == (1128, 1064)
    assert _launches(200, 10000, 128, 0) == (1128, 1128)
    # a model that needs a margin of 256
    assert _launches(200, 10000, 256, 2) == (1128, 1128)
    assert _launches(200, 10000, 256, 0) == (1256, 1256)


def test_tiles_that_mix_an_edge_chunk_bound_the_launch():
    """100 x 10 000 (the reference CLI's default batch): 10 chunks of 1264 columns, 12.5 tiles per chunk, so every other junction
    of the virtual batch lies inside a tile.  Interior chunks share one local range, but the edge chunks' windows are shifted
    (chunk 0 starts at its window's own end, the last chunk ends at it), and the tile that mixes an edge chunk with its
    neighbour runs the union.  Per chunk the trims would give 632 + 568 and 568 + 568 steps; the device runs:
      level 1: the tile of chunks 8 | 9 needs forward [0, 1264) around 632: 632 + 632 -- nothing saved on the longest tile;
      level 2: that tile needs [64, 1264) around 664, the tile of chunks 0 | 1 [0, 1192) around 592: 600 + 600."""
    r = check_ranges(100, 10000, 1, 1, 128, 2)
    per_chunk = (max(max(r["mid"][k] - r["lo_fwd"][k], r["hi_rev"][k] - r["mid"][k]) for k in range(10)),
                 max(max(r["hi_fwd"][k] - r["mid"][k], r["mid"][k] - r["lo_rev"][k]) for k in range(10)))
    assert per_chunk == (568, 568)
    assert _launches(100, 10000, 128, 0) == (632, 632)
    assert _launches(100, 10000, 128, 1) == (632, 632)
    assert _launches(100, 10000, 128, 2) == (600, 600)
    tiles = engine.split_tile_ranges(100, 10000, trim=1)
    assert tiles[12] == (0, 1192, 0, 1256, 624) and tiles[112] == (0, 1264, 64, 1264, 632) and tiles[13] == (0, 1192, 64, 1256, 624)


def test_the_plan_does_not_depend_on_the_trim():
    assert engine.split_plan(200, 10000) == {
        "chunks": 5, "columns": 2256, "margin": 128, "start": [0, 1872, 3872, 5872, 7744],
        "first": [0, 2000, 4000, 6000, 8000], "last": [2000, 4000, 6000, 8000, 10000]}


def test_bad_arguments_are_errors():
    for args in ((-1, 100, 1, 1, 128, 1), (1, 100, 1, 1, 100, 1), (1, 10000, 1, 1, 128, 3), (1, 10000, 1, 1, 128, -1)):
        with pytest.raises(lib.EngineError):
            engine.split_scan_ranges(*args)
    with pytest.raises(lib.EngineError):
        engine.split_tile_ranges(0, 100)
