"""The cost bookkeeping of the matrix-core LQR rollout (lqr_mfma16x8.hip), restated in plain Python for the tests of the final
cost's tile (test_lqr_final_cost_tile_cpu.py, test_lqr_final_cost_tile_gpu.py).

The rollout works through the horizon in chunks of ``CHUNK`` steps.  Row r of the chunk buffer holds z = [x; u] of step
t0 + r; the buffer has ``CHUNK + 1`` rows, and row tc (tc: the steps of the chunk) holds the state the last step produced.
``chunk_costs(rows, out)`` prices rows [0, rows) sixteen at a time: tile nt, column i is row 16 nt + i, clamped to rows - 1 for
the load and guarded for the store.  The LAST chunk prices tc + 1 rows -- the final cost rides as row tc, with a zeroed action
part -- and every other chunk prices tc.

This is a model, kept in step with the kernel BY HAND: nothing derives it from the source.  ``CHUNK`` restates the default of the
macro ``TFMPC_LQR_TC`` (``kTC``), ``chunks`` the head of the kernel's chunk loop (``t0 == 0 || t0 < T``, ``last = T - t0 <= kTC``)
and ``chunk_cost_stores`` the tile loop and row guard of its ``chunk_costs``.  The CPU test therefore guards the bookkeeping as
designed; that the kernel follows it is what the GPU test checks, at the horizons where the two could part."""

CHUNK = 52      # kTC
TILE = 16       # columns of one matrix-core tile
N, M = 16, 8    # the tile grid: states, actions of a row


def chunks(T):
    """(t0, tc, last) of every pass of the chunk loop.  T = 0 runs it once with no step."""
    out, t0 = [], 0
    while t0 == 0 or t0 < T:
        last = T - t0 <= CHUNK
        out.append((t0, T - t0 if last else CHUNK, last))
        t0 += CHUNK
    return out


def chunk_cost_stores(rows):
    """What one ``chunk_costs(rows, out)`` does: [(tile, column, row loaded, offset stored into ``out`` or None)]."""
    ops = []
    nt = 0
    while nt * TILE < rows:
        for i in range(TILE):
            row = TILE * nt + i
            ops.append((nt, i, row if row < rows else rows - 1, row if row < rows else None))
        nt += 1
    return ops


def cost_stores(T):
    """Every store into the costs of one instance: [(index into costs[0 .. T], chunk, buffer row priced, tile, column)]."""
    out = []
    for c, (t0, tc, last) in enumerate(chunks(T)):
        for nt, i, row, off in chunk_cost_stores(tc + 1 if last else tc):
            if off is not None:
                out.append((t0 + off, c, row, nt, i))
    return out


def tiles(T):
    """Matrix-core tiles the costs of one instance take."""
    return sum(-(-(tc + 1 if last else tc) // TILE) for _, tc, last in chunks(T))


def tiles_separate_final_pass(T):
    """... when the final cost took a tile of its own behind the chunk loop."""
    return sum(-(-min(CHUNK, T - t0) // TILE) for t0 in range(0, T, CHUNK)) + 1


def final_row(T):
    """(chunk, buffer row, tile, column) of the final cost, and the lane that holds it for the NaN test (q = 0: lane == column)."""
    t0, tc, last = chunks(T)[-1]
    assert last and t0 + tc == T
    return len(chunks(T)) - 1, tc, tc // TILE, tc % TILE


def zeroed_floats(T):
    """Floats of the chunk buffer (row stride 26) the last chunk zeroes: the action part of row tc."""
    _, tc, _, _ = final_row(T)
    return [tc * 26 + N + a for a in range(M)]


def action_floats_stored(T):
    """Floats of the chunk buffer the last chunk's action stores read: rows 0 .. tc - 1, columns 16 .. 23."""
    _, tc, _, _ = final_row(T)
    return [r * 26 + N + a for r in range(tc) for a in range(M)]
