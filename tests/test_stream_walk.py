"""The streaming batch kernel's tile walk (ecx_stream_walk_probe runs the
kernel's own start/step code on the CPU): over all hardware blocks of a
launch, every (stripe, tile) of the batch is visited exactly once and
nothing outside it. CPU only."""
import numpy as np
import pytest

import ceph_amd

# (n_stripes, tiles per chunk)
SHAPES = [(1, 1), (1, 3), (5, 1), (5, 3), (800, 1), (800, 3)]


def _widths(S):
    # 1, 2, 3, S, one that does not divide S, one larger than S
    return sorted({1, 2, 3, S, 7, S + 9})


def _grids(n_tiles):
    # a single block, fewer blocks than XCDs, no multiple of 8, a multiple
    # of 8, a step that carries in every index, one block per tile
    g = {1, 3, 7, 13, 64, 1001, n_tiles - 1, n_tiles}
    return sorted(x for x in g if 1 <= x <= n_tiles)


def _visits(S, tpc, width, xcd, grid):
    seen = np.zeros((S, tpc), dtype=np.int64)
    for b in range(grid):
        v = ceph_amd.stream_walk_probe(S, tpc, width, xcd, grid, b)
        assert v.shape[1] == 2
        if len(v):
            assert v[:, 0].max() < S and v[:, 1].max() < tpc, (b, v)
            np.add.at(seen, (v[:, 0], v[:, 1]), 1)
    return seen


@pytest.mark.parametrize("xcd", [0, 1])
@pytest.mark.parametrize("S,tpc", SHAPES)
def test_every_tile_exactly_once(S, tpc, xcd):
    for width in _widths(S):
        for grid in _grids(S * tpc):
            seen = _visits(S, tpc, width, xcd, grid)
            assert (seen == 1).all(), (width, grid, np.argwhere(seen != 1)[:4])


def _order(S, tpc, width, xcd, grid):
    """Tiles in logical order: hardware blocks sorted by their first tile's
    number are the logical blocks 0..grid-1."""
    walks = [ceph_amd.stream_walk_probe(S, tpc, width, xcd, grid, b)
             for b in range(grid)]
    return walks


def test_width_ends_are_the_two_orders():
    S, tpc, grid = 5, 3, 4
    # width 1: tile in chunk fastest; width S: stripe fastest
    w1 = _order(S, tpc, 1, 0, grid)
    ws = _order(S, tpc, S, 0, grid)
    for b in range(grid):
        n = np.arange(b, S * tpc, grid)
        assert np.array_equal(w1[b], np.stack([n // tpc, n % tpc], axis=1))
        assert np.array_equal(ws[b], np.stack([n % S, n // S], axis=1))


def test_group_numbering():
    # (group, tile, stripe in group), last group narrower: S=5, W=2, tpc=3
    S, tpc, W = 5, 3, 2
    got = ceph_amd.stream_walk_probe(S, tpc, W, 0, 1, 0)
    want = [(g * W + s, t) for g in range(3) for t in range(tpc)
            for s in range(W) if g * W + s < S]
    assert [tuple(r) for r in got] == want


def test_xcd_mapping_is_contiguous_per_die():
    # blocks id, id + 8, id + 16, ... (one die) take consecutive runs of the
    # tile order; grid 21 is no multiple of 8, so dies 0..4 get 3 blocks and
    # dies 5..7 get 2
    S, tpc, grid = 800, 3, 21
    first = [ceph_amd.stream_walk_probe(S, tpc, 1, 1, grid, b)[0]
             for b in range(grid)]
    number = [int(s) * tpc + int(t) for s, t in first]  # width 1 numbering
    assert sorted(number) == list(range(grid))
    for die in range(8):
        run = number[die::8]
        assert run == list(range(run[0], run[0] + len(run))), (die, run)
    starts = [number[die] for die in range(8)]
    assert starts == sorted(starts)
    # a grid that is a multiple of 8: (id % 8) * (grid / 8) + id / 8
    grid = 24
    for b in range(grid):
        s, t = ceph_amd.stream_walk_probe(S, tpc, 1, 1, grid, b)[0]
        assert int(s) * tpc + int(t) == (b % 8) * (grid // 8) + b // 8


def test_probe_rejects_bad_arguments():
    for args in [(0, 1, 1, 0, 1, 0), (5, 0, 1, 0, 1, 0), (5, 3, 1, 0, 0, 0),
                 (5, 3, 1, 0, 4, 4)]:
        with pytest.raises(ceph_amd.EcError):
            ceph_amd.stream_walk_probe(*args)
