"""CPU tests (no GPU) of tiled detection's host layer: the tile grid and its properties, the numpy model of the merge against a
brute-force restatement, the merge groups, and the argument checks."""
import numpy as np
import pytest

from tests import tiles_model as tm

# (L, t, overlap): t == L, t > L, overlap == 0, L - t not a multiple of the step, a fraction, the bench's axes, step 1
AXES = [(64, 64, 16), (50, 64, 16), (100, 20, 0), (100, 30, 7), (96, 64, 32), (160, 64, 32), (37, 16, 5), (53, 21, 20), (3840, 640, 128),
        (2160, 640, 128), (101, 40, 0.25), (65, 64, 63), (17, 1, 0), (1, 1, 0)]


@pytest.mark.parametrize('L,t,overlap', AXES)
def test_axis_properties(L, t, overlap):
    from terran_amd import tiles
    other = 23
    grid = tiles.tile_grid(L, other, (t, 9), (overlap, 2))
    assert grid.dtype == np.int32 and grid.shape[1] == 2
    assert np.array_equal(grid, tm.tile_grid_model(L, other, (t, 9), (overlap, 2)))
    assert np.array_equal(tiles.tile_grid(other, L, (9, t), (2, overlap)), tm.tile_grid_model(other, L, (9, t), (2, overlap)))
    ys = np.unique(grid[:, 0])
    tt = min(t, L)
    px = tm.overlap_model(t, overlap)
    assert ys[0] == 0 and (ys >= 0).all() and (ys + tt <= L).all()                     # every origin lies inside the frame
    assert len(ys) == len(set(ys.tolist())) and (np.diff(ys) > 0).all()                # no duplicates, ascending
    covered = np.zeros(L, bool)
    for y in ys:
        covered[y:y + tt] = True
    assert covered.all()                                                              # every pixel is covered
    if len(ys) > 1:
        # every interval [a, a + n) with n <= overlap lies wholly inside at least one tile
        for n in range(1, px + 1):
            a = np.arange(0, L - n + 1)
            inside = (ys[:, None] <= a) & (a + n <= ys[:, None] + tt)
            assert inside.any(axis=0).all(), (n, a[~inside.any(axis=0)][:4])
    # the grid is the product of the axes, row-major
    xs = grid[:len(grid) // len(ys), 1]
    assert np.array_equal(grid, np.array([[y, x] for y in ys for x in xs], np.int32))


def test_grid_2d_and_scalar_arguments():
    from terran_amd import tiles
    g = tiles.tile_grid(96, 160, 64, 32)
    assert g.tolist() == [[y, x] for y in (0, 32) for x in (0, 32, 64, 96)]
    assert np.array_equal(g, tm.tile_grid_model(96, 160, 64, 32))
    assert np.array_equal(tiles.tile_grid(2160, 3840, 640, 0.2), tm.tile_grid_model(2160, 3840, 640, 0.2))
    assert len(tiles.tile_grid(2160, 3840, 640, 128)) == 32                              # 4 x 8: the bench's 1 024 tiles of 32 frames
    assert tiles.tile_grid(100, 100, 640, 128).tolist() == [[0, 0]]                      # a frame smaller than the tile: itself
    assert tiles.tile_shape(100, 300, 256) == (100, 256)


def random_case(rng, n_frames, n_groups, per_group, ties):
    """Groups of random candidates over a 200 x 200 frame, with zooms, origins, interior bits and (ties) repeated scores and boxes."""
    groups, first = [], 0
    frames = np.sort(rng.integers(0, n_frames, n_groups))
    for f in frames:
        count = int(rng.integers(0, per_group + 1))
        x0, y0 = rng.integers(0, 100, 2)
        groups.append(tm.group(int(f), first, count, ox=float(x0) + float(rng.choice([0.0, 0.25, 0.4])), oy=float(y0),
                               zoom=float(rng.choice([1.0, 1.3, 2.0, 0.5])), rect=(x0, y0, x0 + 100, y0 + 100), interior=int(rng.integers(0, 16))))
        first += count
    first += 2                                                                            # two rows in no group
    boxes = rng.uniform(0, 80, (first, 2))
    boxes = np.concatenate([boxes, boxes + rng.uniform(5, 50, (first, 2))], axis=1).astype(np.float32)
    scores = rng.uniform(0.3, 1.0, first).astype(np.float32)
    if ties:
        boxes = np.round(boxes / 8) * 8
        scores = (np.round(scores * 4) / 4).astype(np.float32)
    lm = rng.uniform(0, 100, (first, 5, 2)).astype(np.float32)
    return groups, boxes, lm, scores


@pytest.mark.parametrize('seed', range(12))
def test_merge_model_against_brute_force(seed):
    rng = np.random.default_rng(seed)
    n_frames = int(rng.integers(1, 4))
    groups, boxes, lm, scores = random_case(rng, n_frames, int(rng.integers(1, 7)), 12, ties=seed % 2 == 1)
    for metric in (0, 1):
        for edge in (0.0, 6.0):
            thr = float(rng.choice([0.2, 0.4, 0.5]))
            got = tm.merge_model(groups, n_frames, boxes, lm, scores, thr, metric, edge)
            want = tm.merge_brute(groups, n_frames, boxes, lm, scores, thr, metric, edge)
            for a, b, what in zip(got, want, ('counts', 'boxes', 'landmarks', 'scores', 'source')):
                assert a.dtype == b.dtype and np.array_equal(a, b), (seed, metric, edge, what)


def test_merge_model_threshold_is_strict():
    """[0,0,2,2] and [0,0,2,1] overlap by exactly 0.5: both stay at nms_thr = 0.5; [0,0,2,2] and [0,0,2,1.5] (0.75) do not."""
    lm = np.zeros((2, 5, 2), np.float32)
    g = [tm.group(0, 0, 2)]
    counts, *_ = tm.merge_model(g, 1, [[0, 0, 2, 2], [0, 0, 2, 1]], lm, [0.9, 0.8], 0.5)
    assert counts.tolist() == [2]
    counts, _, _, _, src = tm.merge_model(g, 1, [[0, 0, 2, 2], [0, 0, 2, 1.5]], lm, [0.8, 0.9], 0.5)
    assert counts.tolist() == [1] and src.tolist() == [1]


def test_merge_groups_interior_bits():
    from terran_amd import lib, tiles
    origins = tiles.tile_grid(192, 256, 64, 0)                                            # 3 x 4 tiles
    nt = len(origins)
    counts = np.arange(2 * nt)
    full = np.array([5, 7])
    g = tiles.merge_groups(2, 192, 256, origins, 64, 64, 1.5, counts, full, 0.25)
    assert g.dtype == lib.MERGE_GROUP_DT and len(g) == 2 * (nt + 1)
    assert (np.diff(g['frame']) >= 0).all()                                               # sorted by frame
    per = g.reshape(2, nt + 1)
    by_origin = {tuple(o): k for k, o in enumerate(origins.tolist())}
    corner, side, middle, last = (per[1][by_origin[o]] for o in ((0, 0), (0, 64), (64, 128), (128, 192)))
    assert corner['interior'] == 4 + 8                                                    # right and bottom are inside the frame
    assert side['interior'] == 1 + 4 + 8                                                  # top row: only the top side is on the border
    assert middle['interior'] == 15
    assert last['interior'] == 1 + 2                                                      # bottom right corner
    assert (middle['ox'], middle['oy'], middle['zoom']) == (128.0, 64.0, 1.5)
    assert (middle['x0'], middle['y0'], middle['x1'], middle['y1']) == (128.0, 64.0, 192.0, 128.0)
    # rows: the tiles' candidates frame-major, the whole-frame pass behind all of them
    firsts = np.concatenate([[0], np.cumsum(counts)])
    assert np.array_equal(per[:, :nt]['first'].reshape(-1), firsts[:-1]) and np.array_equal(per[:, :nt]['count'].reshape(-1), counts)
    whole = per[:, nt]
    assert whole['interior'].tolist() == [0, 0] and whole['zoom'].tolist() == [0.25, 0.25]
    assert whole['first'].tolist() == [firsts[-1], firsts[-1] + 5] and whole['count'].tolist() == [5, 7]
    assert (whole['ox'] == 0).all() and (whole['oy'] == 0).all() and whole['x1'].tolist() == [256.0, 256.0] and whole['y1'].tolist() == [192.0, 192.0]
    # without a whole-frame pass: the tiles only
    assert len(tiles.merge_groups(2, 192, 256, origins, 64, 64, 1.0, counts)) == 2 * nt


def test_argument_errors_name_the_argument():
    from terran_amd import TiledDetection, tiles
    with pytest.raises(ValueError, match='overlap'):
        tiles.tile_grid(100, 100, 64, 64)
    with pytest.raises(ValueError, match='overlap'):
        TiledDetection(tile=64, overlap=64)
    with pytest.raises(ValueError, match='overlap'):
        TiledDetection(tile=(64, 32), overlap=40)
    with pytest.raises(ValueError, match='zoom'):
        TiledDetection(zoom=0)
    with pytest.raises(ValueError, match='zoom'):
        tiles.check_args(64, 8, zoom=-1.0)
    with pytest.raises(ValueError, match='metric'):
        TiledDetection(metric='giou')
    with pytest.raises(ValueError, match='edge'):
        TiledDetection(edge=-1)
    with pytest.raises(ValueError, match='tile'):
        TiledDetection(tile=0)
    with pytest.raises(ValueError, match='device.*fan-out'):
        TiledDetection(device=[0, 1])
    assert tiles.check_args(640, 0.2, 1.5, 'ios', 4.0) == 1
