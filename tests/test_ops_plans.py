"""The host-side helpers that the ragged ops of dpmn_amd/ops.py share, without a GPU: the tile table (_tile_table) and the packing of one
call's arrays into one upload buffer (_pack, what _upload sends)."""
import numpy as np
import pytest


def _tiles_by_loops(sizes, tile_h, tile_w):
    rows, first = [], [0]
    for i, (h, w) in enumerate(sizes):
        for tr in range((h + tile_h - 1) // tile_h):
            for tc in range((w + tile_w - 1) // tile_w):
                rows.append((i, tr, tc))
        first.append(len(rows))
    return rows, first


@pytest.mark.parametrize("sizes, tile", [([(1, 1), (8, 32), (9, 33), (8, 33), (17, 32)], (8, 32)), ([(32, 32), (33, 1)], (32, 32)),
                                         ([(9, 33)], (8, 32)), ([(33, 1)], (32, 32))])
def test_tile_table_is_the_triple_loop(sizes, tile):
    from dpmn_amd import ops
    hs, ws = (np.array(v, np.int64) for v in zip(*sizes))
    tiles, first = ops._tile_table(hs, ws, *tile)
    rows, expected_first = _tiles_by_loops(sizes, *tile)
    assert tiles.dtype == np.int32 and tiles.shape == (len(rows), 3) and tiles.tolist() == [list(r) for r in rows]
    assert first.dtype == np.int64 and first.tolist() == expected_first
    counts = [-(-h // tile[0]) * -(-w // tile[1]) for h, w in sizes]
    assert first.tolist() == [sum(counts[:i]) for i in range(len(sizes) + 1)]


def test_tile_table_feeds_both_plans():
    from dpmn_amd import ops
    hs, ws = np.array([9, 1], np.int64), np.array([33, 70], np.int64)
    assert [tuple(t) for t in ops._region_tiles(hs, ws).tolist()] == _tiles_by_loops([(9, 33), (1, 70)], *ops.QUAD_TILE)[0] == \
        [(0, 0, 0), (0, 0, 1), (0, 1, 0), (0, 1, 1), (1, 0, 0), (1, 0, 1), (1, 0, 2)]
    assert ops.QUAD_TILE == (8, 32) and ops.DEGRADE_TILE == 32


def test_pack_puts_every_array_on_an_8_byte_boundary():
    from dpmn_amd import ops
    arrays = [np.arange(1, 4, dtype=np.int32), np.arange(10, 14, dtype=np.int64).reshape(2, 2), np.empty((0, 3), np.int32),
              np.arange(21, 26, dtype=np.int32), np.array([[1.5, -2.25, 3.0]], np.float32), np.array([7], np.int64)]
    buf, starts = ops._pack(*arrays)
    assert buf.dtype == np.int64 and buf.ndim == 1 and len(starts) == len(arrays)
    assert starts == [0, 2, 6, 6, 9, 11] and buf.size == 12      # words: 3 int32 -> 2, 4 int64 -> 4, none -> 0, 5 int32 -> 3, 3 fp32 -> 2, 1
    raw = buf.view(np.uint8)
    used = np.zeros(raw.size, bool)
    for a, at in zip(arrays, starts):
        assert (at * 8) % 8 == 0 and at * 8 + a.nbytes <= raw.size
        back = raw[at * 8:at * 8 + a.nbytes].view(a.dtype).reshape(a.shape)
        assert np.array_equal(back, a)
        assert not used[at * 8:at * 8 + a.nbytes].any()      # no two arrays share a byte
        used[at * 8:at * 8 + a.nbytes] = True
    assert int(used.sum()) == sum(a.nbytes for a in arrays) and not raw[~used].any()      # the gaps are zero
    # the layouts the kernels were written against: the arrays back to back, an odd int32 count rounded up to a word
    n = 5
    tiles = np.arange(n * 3, dtype=np.int32).reshape(n, 3)
    table = np.arange(18, dtype=np.int64).reshape(2, 9)
    buf, starts = ops._pack(table, tiles)
    old = np.zeros(18 + (n * 3 + 1) // 2, np.int64)
    old[:18] = table.reshape(-1)
    old[18:].view(np.int32)[:n * 3] = tiles.reshape(-1)
    assert starts == [0, 18] and np.array_equal(buf, old)
    buf, starts = ops._pack()
    assert buf.size == 0 and starts == []


def test_pack_refuses_other_dtypes_and_strided_arrays():
    from dpmn_amd import ops
    for bad in (np.zeros(3, np.float64), np.zeros(3, np.uint8), np.zeros((4, 4), np.int32)[:, ::2]):
        with pytest.raises(TypeError):
            ops._pack(bad)
