"""CPU tests (no GPU) of tiled pose estimation's host layer: the model of the merge (tests/pose_tiles_model.py) against answers
derived by hand at every boundary of its definition, its extent shortcut against the plain pair test, the pose groups against
records written by hand, and the argument checks."""
import numpy as np
import pytest

from tests import pose_tiles_model as pm

CASES = pm.boundary_cases()


@pytest.mark.parametrize('name', sorted(CASES))
def test_model_boundary_case(name):
    groups, n_frames, kp, sc, params, source = CASES[name]
    stats = {}
    counts, okp, osc, src = pm.merge_model(groups, n_frames, kp, sc, *params, stats=stats)
    assert src.tolist() == source
    assert counts.dtype == np.int32 and okp.dtype == np.int32 and osc.dtype == np.float64 and src.dtype == np.int32
    assert okp.shape == (len(source), 18, 3) and counts.sum() == len(source)
    assert np.array_equal(osc, sc[source])
    assert stats['candidates'] == len(kp) and stats['empty'] == 0
    if name == 'edge_per_side':
        assert stats['cut'] == 4 and counts.tolist() == [2, 2, 2, 2]


def test_model_maps_by_the_origin_and_zeroes_absent_joints():
    kp = np.zeros((2, 18, 3), np.int32)
    kp[0, 3], kp[0, 7], kp[0, 9] = (5, 6, 2), (-4, 9, 1), (77, 88, 0)                  # joint 9 is absent: its numbers do not count
    groups = [pm.group(0, 0, 1, ox=100, oy=-20), pm.group(0, 1, 1)]
    stats = {}
    counts, okp, _, src = pm.merge_model(groups, 1, kp, [0.5, 0.9], stats=stats)
    assert counts.tolist() == [1] and src.tolist() == [0] and stats['empty'] == 1
    want = np.zeros((18, 3), np.int32)
    want[3], want[7] = (105, -14, 2), (96, -11, 1)
    assert np.array_equal(okp[0], want)


def test_extent_shortcut_never_changes_a_pair():
    rng = np.random.default_rng(4)
    kp, _ = pm.clustered_poses(rng, 400, 500)
    g0, g1 = pm.group(0, 0, 200), pm.group(0, 200, 200)
    cands = [pm.Candidate(r, r // 200, (g0, g1)[r // 200], kp[r]) for r in range(400)]
    cands = [c for c in cands if c.np]
    hits = 0
    for radius, agree, ms in ((0.1, 0.5, 3), (0.0, 1.0, 1), (0.3, 0.2, 1), (2.0, 0.5, 3)):
        r2 = radius * radius
        for a in cands[::3]:
            for b in cands:
                d = pm.duplicates(a, b, r2, agree, ms, shortcut=False)
                assert d == pm.duplicates(a, b, r2, agree, ms) == pm.duplicates(b, a, r2, agree, ms)       # and it is symmetric
                hits += d
    assert hits > 100


def test_clustered_poses_give_work():
    rng = np.random.default_rng(9)
    kp, sc = pm.clustered_poses(rng, 300, 600, exact=True)
    groups = pm.split(rng, 0, 0, kp, 600)
    stats = {}
    pm.merge_model(groups, 1, kp, sc, stats=stats)
    assert kp.shape == (300, 18, 3) and kp.dtype == np.int32 and sc.dtype == np.float64
    assert stats['candidates'] == 300 and stats['empty'] > 0 and stats['suppressed'] > 20
    assert len(np.unique(sc)) <= len(pm.SCORES)


# ---- the groups ----------------------------------------------------------------------------------------------------------------------
def test_pose_groups_of_a_2x2_grid():
    from terran_amd import lib, tiles
    origins = tiles.tile_grid(300, 400, (200, 250), (100, 100))
    assert origins.tolist() == [[0, 0], [0, 150], [100, 0], [100, 150]]
    g = tiles.pose_groups(2, 300, 400, origins, 200, 250, [1, 0, 2, 3, 0, 4, 0, 5])
    assert g.dtype == lib.POSE_GROUP_DT and len(g) == 8
    #        frame first count ox   oy   x0   y0   x1   y1  interior
    want = [(0, 0, 1, 0, 0, 0, 0, 250, 200, 4 + 8),
            (0, 1, 0, 150, 0, 150, 0, 400, 200, 1 + 8),
            (0, 1, 2, 0, 100, 0, 100, 250, 300, 2 + 4),
            (0, 3, 3, 150, 100, 150, 100, 400, 300, 1 + 2),
            (1, 6, 0, 0, 0, 0, 0, 250, 200, 4 + 8),
            (1, 6, 4, 150, 0, 150, 0, 400, 200, 1 + 8),
            (1, 10, 0, 0, 100, 0, 100, 250, 300, 2 + 4),
            (1, 10, 5, 150, 100, 150, 100, 400, 300, 1 + 2)]
    assert g.tolist() == want
    g = tiles.pose_groups(2, 300, 400, origins, 200, 250, [1, 0, 2, 3, 0, 4, 0, 5], full_counts=[7, 2])
    assert len(g) == 10 and g[:4].tolist() == want[:4] and g[5:9].tolist() == want[4:]
    assert g[4].tolist() == (0, 15, 7, 0, 0, 0, 0, 400, 300, 0) and g[9].tolist() == (1, 22, 2, 0, 0, 0, 0, 400, 300, 0)
    assert (np.diff(g['frame']) >= 0).all()
    with pytest.raises(ValueError, match='tile counts'):
        tiles.pose_groups(2, 300, 400, origins, 200, 250, [1, 2, 3])
    with pytest.raises(ValueError, match='one count per frame'):
        tiles.pose_groups(2, 300, 400, origins, 200, 250, [0] * 8, full_counts=[1])


def test_a_frame_smaller_than_the_tile_is_one_group_without_interior_sides():
    from terran_amd import tiles
    origins = tiles.tile_grid(100, 120, 368, 0.25)
    th, tw = tiles.tile_shape(100, 120, 368)
    assert tiles.pose_groups(1, 100, 120, origins, th, tw, [3]).tolist() == [(0, 0, 3, 0, 0, 0, 0, 120, 100, 0)]


# ---- arguments -------------------------------------------------------------------------------------------------------------------------
BAD_ARGS = [(dict(tile=0), 'tile'), (dict(tile=(64, 64, 64)), 'tile'), (dict(tile=64, overlap=64), 'overlap'), (dict(overlap=1.5), 'overlap'),
            (dict(zoom=0), 'zoom'), (dict(zoom=float('nan')), 'zoom'), (dict(edge=-1), 'edge'), (dict(edge=2.5), 'edge'),
            (dict(radius=-0.1), 'radius'), (dict(radius=float('inf')), 'radius'), (dict(agree=0), 'agree'), (dict(agree=1.01), 'agree'),
            (dict(min_shared=0), 'min_shared'), (dict(min_shared=19), 'min_shared'), (dict(min_shared=2.0), 'min_shared')]


@pytest.mark.parametrize('kw,name', BAD_ARGS)
def test_argument_errors_name_the_argument(kw, name):
    from terran_amd import TiledEstimation, tiles
    args = dict(tile=368, overlap=0.25)
    args.update(kw)
    with pytest.raises(ValueError, match='`%s`' % name):
        tiles.check_pose_args(**args)
    with pytest.raises(ValueError, match='`%s`' % name):
        TiledEstimation(**kw)


def test_tiled_estimation_arguments():
    from terran_amd import TiledEstimation, tiles
    tiles.check_pose_args(368, 0.25)
    tiles.check_pose_args((192, 256), (32, 0.5), 1.5, 12, 0.0, 1.0, 18, 1)
    with pytest.raises(ValueError, match='`max_tiles`'):
        tiles.check_pose_args(368, 0.25, max_tiles=0)
    with pytest.raises(ValueError, match='`max_tiles`'):
        TiledEstimation(max_tiles=0)
    with pytest.raises(ValueError, match='`device`'):
        TiledEstimation(device=[0, 1])
    with pytest.raises(ValueError, match='`short_side`'):
        TiledEstimation(short_side=0)
    te = TiledEstimation(full_frame=False, short_side=0)                                 # no whole-frame pass: no short side needed
    assert te.model is None and repr(te).startswith('<TiledEstimation(')                  # nothing touches a device before the first call
