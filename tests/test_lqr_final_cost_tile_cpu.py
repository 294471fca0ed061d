"""Bookkeeping of the rollout's cost tiles (lqr_mfma16x8.hip as restated in lqr_final_cost_tile_ref.py), no GPU: for every
horizon 0 .. 110 each of the T + 1 costs is written exactly once, from the row that holds its step, nothing is written beyond
T, the final cost rides in the last chunk as row tc, and the rows stay inside the chunk buffer."""

import pytest

import lqr_final_cost_tile_ref as ref

HORIZONS = range(0, 111)


@pytest.mark.parametrize("T", HORIZONS)
def test_every_cost_is_written_once(T):
    stores = ref.cost_stores(T)
    where = sorted(s[0] for s in stores)
    assert where == list(range(T + 1)), (T, "each of costs[0 .. T] once, nothing beyond T")
    chunk_of = ref.chunks(T)
    for idx, c, row, nt, i in stores:
        t0, tc, last = chunk_of[c]
        assert idx == t0 + row and row == ref.TILE * nt + i, (T, idx)
        assert 0 <= row <= ref.CHUNK, (T, row, "the buffer has CHUNK + 1 rows")
        # a stage cost comes from a row a rollout step completed, the final cost from row tc of the last chunk
        assert row < tc or (last and row == tc and idx == T), (T, idx, row)


@pytest.mark.parametrize("T", HORIZONS)
def test_loads_stay_inside_the_priced_rows(T):
    for t0, tc, last in ref.chunks(T):
        rows = tc + 1 if last else tc
        assert rows >= 1
        for nt, i, row, off in ref.chunk_cost_stores(rows):
            assert 0 <= row < rows <= ref.CHUNK + 1, (T, t0, row)
            assert off is None or off == row


@pytest.mark.parametrize("T", HORIZONS)
def test_the_final_row(T):
    c, row, nt, col = ref.final_row(T)
    t0, tc, last = ref.chunks(T)[c]
    assert last and row == tc == T - t0 and (nt, col) == divmod(row, ref.TILE)
    # the final cost sits in the LAST tile the chunk prices: that is the tile whose costs the NaN test reads
    assert nt == max(s[3] for s in ref.cost_stores(T) if s[1] == c)
    # the zeroed action part is read by no action store of the chunk and lies inside the buffer
    assert not set(ref.zeroed_floats(T)) & set(ref.action_floats_stored(T))
    assert max(ref.zeroed_floats(T)) < (ref.CHUNK + 1) * 26
    # only the last chunk prices an extra row; every chunk before it is full
    assert all(tc_ == ref.CHUNK and not l for _, tc_, l in ref.chunks(T)[:-1])
    assert sum(tc_ for _, tc_, _ in ref.chunks(T)) == T


@pytest.mark.parametrize("T", HORIZONS)
def test_tile_count(T):
    """One tile fewer than with a final pass of its own, except where row tc opens a tile (tc a multiple of 16): equal there."""
    _, tc, _, _ = ref.final_row(T)
    assert ref.tiles(T) == ref.tiles_separate_final_pass(T) - (0 if tc % ref.TILE == 0 else 1)


def test_headline_horizon():
    assert ref.tiles(50) == 4 and ref.tiles_separate_final_pass(50) == 5
    assert ref.final_row(50) == (0, 50, 3, 2)
