"""No GPU: the two statements of the link rule (tests/link_model.py) against each other, head_boxes against values worked out by
hand, and link_faces_poses' host half against a stand-in context whose faces_poses_link is the model."""
import numpy as np
import pytest

from terran_amd import link
from tests import link_model as lm


class ModelContext:
    """What link_faces_poses needs of a context, answered by the model."""

    def __init__(self):
        self.calls = []

    def faces_poses_link(self, face_counts, boxes, pose_counts, keypoints, margin_permille=250, min_inside=1):
        self.calls.append((margin_permille, min_inside))
        return lm.link_rounds_model(face_counts, boxes, pose_counts, keypoints, margin_permille, min_inside)


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_walk_and_rounds_agree_on_random_frames(seed):
    rng = np.random.default_rng(seed)
    counts = [(0, 5), (7, 0), (1, 1), (40, 60), (90, 30)]
    parts = [lm.crowd(rng, a, b, extent=128) for a, b in counts]
    fc, pc = [c[0] for c in counts], [c[1] for c in counts]
    boxes, kp = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    for margin, min_inside in ((250, 1), (0, 2), (4000, 5)):
        walk = lm.link_model(fc, boxes, pc, kp, margin, min_inside)
        rounds = lm.link_rounds_model(fc, boxes, pc, kp, margin, min_inside)
        assert all(np.array_equal(a, b) for a, b in zip(walk, rounds[:3]))
        assert rounds[3] >= 1
        # one to one, and mutual
        f0 = p0 = 0
        for nf, npose in zip(fc, pc):
            pof, fop = walk[0][f0:f0 + nf], walk[1][p0:p0 + npose]
            assert all(fop[p] == f for f, p in enumerate(pof) if p >= 0) and all(pof[f] == p for p, f in enumerate(fop) if f >= 0)
            f0, p0 = f0 + nf, p0 + npose
    assert walk[2].sum() > 0


@pytest.mark.parametrize('length', [1, 2, 5, 64])
def test_chain_takes_as_many_rounds_as_it_has_links(length):
    boxes, kp = lm.chain(length, x_at=-300, y_at=7)
    pof, fop, links, rounds = lm.link_rounds_model([length], boxes, [length], kp, 0, 1)
    assert pof.tolist() == list(range(length)) == fop.tolist() and links.tolist() == [length] and rounds == length + 1
    q = lm.qualifying_per_face([length], boxes, [length], kp, 0, 1)
    assert q.tolist() == [1] + [2] * (length - 1)


def test_pair_by_hand():
    # box 10 .. 17 (w = 7, 250 permille: mx = 1), 0 .. 20 (my = 5); cx = 27, cy = 20
    box = (10, 0, 17, 20)
    assert lm.pair(box, [(9, 0)], 250, 1) == 60 * ((18 - 27) ** 2 + (0 - 20) ** 2)
    assert lm.pair(box, [(8, 0)], 250, 1) is None
    assert lm.pair(box, [(18, 25)], 250, 1) is not None and lm.pair(box, [(18, 26)], 250, 1) is None
    assert lm.pair(box, [(12, 3), (100, 3), (100, 4)], 250, 1) is None          # 1 of 3 inside: no majority
    assert lm.pair(box, [(12, 3), (100, 3)], 250, 1) == 30 * ((24 - 27) ** 2 + (6 - 20) ** 2 + (200 - 27) ** 2 + (6 - 20) ** 2)
    assert lm.pair(box, [(12, 3), (100, 3)], 250, 2) is None
    assert lm.pair((17, 0, 10, 20), [(12, 3)], 250, 1) is None                  # x1 < x0
    assert lm.pair((12, 3, 12, 3), [(12, 3)], 4000, 1) == 0                     # w = h = 0 holds its own point


# ---- head_boxes ------------------------------------------------------------------------------------------------------------
def hb(joints, margin=0.25):
    got = link.head_boxes([{'keypoints': lm.pose_row(joints)}], margin)
    return got[0]['bbox'].tolist() if got else None


def test_head_boxes_by_hand():
    assert hb({0: (50, 60)}) is None                                            # one joint: side 0
    assert hb({1: (50, 60), 5: (3, 4)}) is None                                 # no head joint at all
    # nose + neck only: the extent is a point, q = isqrt(3^2 + 4^2) = 5 = side; m = 5 * 250 // 1000 = 1
    # x0 = (100 - 5) // 2 - 1 = 46, x1 = (100 + 6) // 2 + 1 = 54; y0 = (120 - 5) // 2 - 1 = 56, y1 = (120 + 6) // 2 + 1 = 64
    assert hb({0: (50, 60), 1: (53, 64)}) == [46, 56, 54, 64]
    # isqrt truncates: 4^2 + 4^2 = 32 -> 5
    assert hb({0: (50, 60), 1: (54, 64)}) == [46, 56, 54, 64]
    # eyes 10 and 17 (odd sum 27, side 7), y 20 and 22 (even sum 42); m = 7 * 250 // 1000 = 1
    # x0 = (27 - 7) // 2 - 1 = 9, x1 = (27 + 8) // 2 + 1 = 18; y0 = (42 - 7) // 2 - 1 = 16, y1 = (42 + 8) // 2 + 1 = 26
    assert hb({14: (10, 20), 15: (17, 22)}) == [9, 16, 18, 26]
    # even sum, even side, no margin: 10 and 18 -> x0 = (28 - 8) // 2 = 10, x1 = (28 + 9) // 2 = 18; y 5 and 5 (sum 10, the same
    # side 8): y0 = (10 - 8) // 2 = 1, y1 = (10 + 9) // 2 = 9
    assert hb({14: (10, 5), 15: (18, 5)}, 0.0) == [10, 1, 18, 9]
    # negative coordinates: ears -11 and -4 (sum -15, side 7), y -3 both (sum -6); floor, not truncation
    # x0 = (-15 - 7) // 2 = -11, x1 = (-15 + 8) // 2 = -4 (floor of -3.5); y0 = (-6 - 7) // 2 = -7 (floor of -6.5), y1 = (-6 + 8) // 2 = 1
    assert hb({16: (-11, -3), 17: (-4, -3)}, 0.0) == [-11, -7, -4, 1]
    # the neck decides when it is further than the head is wide: extent 2 x 0, q = isqrt(0 + 30^2) = 30; m = 30 * 500 // 1000 = 15
    # x0 = (10 + 12 - 30) // 2 - 15 = -19, x1 = (22 + 31) // 2 + 15 = 41; y0 = (80 - 30) // 2 - 15 = 10, y1 = (80 + 31) // 2 + 15 = 70
    assert hb({0: (10, 40), 14: (12, 40), 1: (10, 70)}, 0.5) == [-19, 10, 41, 70]
    # an absent joint's coordinates do not count
    row = lm.pose_row({14: (10, 20), 15: (17, 22)})
    row[0] = (900, 900, 0)
    assert link.head_boxes([{'keypoints': row}])[0]['bbox'].tolist() == [9, 16, 18, 26]


def test_head_boxes_forms_and_only_unlinked():
    a, b = {'keypoints': lm.pose_row({14: (10, 20), 15: (17, 22)})}, {'keypoints': lm.pose_row({0: (5, 5)})}
    c = {'keypoints': lm.pose_row({16: (40, 40), 17: (50, 41)}), 'face': 0}
    per_frame = link.head_boxes([[a, b, c], [], [c]])
    assert [[d['pose'] for d in fr] for fr in per_frame] == [[0, 2], [], [0]]
    assert per_frame[0][0]['bbox'].dtype == np.int32 and per_frame[0][0]['bbox'].shape == (4,)
    assert [[d['pose'] for d in fr] for fr in link.head_boxes([[a, b, c], [], [c]], only_unlinked=True)] == [[0], [], []]
    assert [d['pose'] for d in link.head_boxes([a, b, c])] == [0, 2]            # one image's list gives one list


# ---- link_faces_poses --------------------------------------------------------------------------------------------------------
def scene():
    """Two frames.  Frame 0: faces A (10, 10, 30, 30) and B (100, 10, 120, 30); poses: one at B, one far away, one at A.  Frame 1:
    one face, no pose."""
    faces = [[{'bbox': np.array([10, 10, 30, 30], np.float32), 'text': 'ada', 'track': 7},
              {'bbox': np.array([100, 10, 120, 30], np.float32), 'cluster': 3, 'text': 'bob'}],
             [{'bbox': np.array([0, 0, 9, 9], np.float32), 'pose': 5}]]
    poses = [[{'keypoints': lm.pose_row({0: (110, 20), 14: (108, 18)}), 'text': 'mine'},
              {'keypoints': lm.pose_row({0: (200, 200)}), 'face': 1, 'track': 99},
              {'keypoints': lm.pose_row({0: (20, 20), 1: (20, 50)})}],
             []]
    return faces, poses


def test_link_faces_poses_writes_and_removes_keys():
    faces, poses = scene()
    ctx = ModelContext()
    got = link.link_faces_poses(faces, poses, ctx=ctx)
    assert [g.tolist() for g in got] == [[2, 0], [-1]] and all(g.dtype == np.int32 for g in got)
    assert ctx.calls == [(250, 1)]
    assert faces[0][0]['pose'] == 2 and faces[0][1]['pose'] == 0
    assert 'pose' not in faces[1][0]                                            # the stale key is gone
    assert poses[0][2]['face'] == 0 and poses[0][0]['face'] == 1
    assert 'face' not in poses[0][1] and poses[0][1]['track'] == 99             # stale link removed, its own keys stay
    # inheritance: what the face carries and the skeleton lacks
    assert poses[0][2]['text'] == 'ada' and poses[0][2]['track'] == 7 and 'cluster' not in poses[0][2]
    assert poses[0][0]['text'] == 'mine' and poses[0][0]['cluster'] == 3        # an own key is not overwritten
    assert type(faces[0][0]['pose']) is int and type(poses[0][2]['face']) is int


def test_link_faces_poses_inherit_and_parameters():
    faces, poses = scene()
    ctx = ModelContext()
    link.link_faces_poses(faces, poses, margin=0.1234, min_inside=2, inherit=('track',), ctx=ctx)
    assert ctx.calls == [(123, 2)]
    assert poses[0][0]['face'] == 1 and 'cluster' not in poses[0][0]
    assert 'face' not in poses[0][2] and 'text' not in poses[0][2]              # one head joint: min_inside = 2 refuses it


def test_link_faces_poses_single_image_form():
    faces, poses = scene()
    got = link.link_faces_poses(faces[0], poses[0], ctx=ModelContext())
    assert isinstance(got, np.ndarray) and got.tolist() == [2, 0]
    assert faces[0][0]['pose'] == 2 and poses[0][2]['face'] == 0
    assert link.link_faces_poses([], [], ctx=ModelContext()).tolist() == []


def test_link_faces_poses_refuses_mismatched_input():
    faces, poses = scene()
    with pytest.raises(ValueError):
        link.link_faces_poses(faces, poses[:1], ctx=ModelContext())
    with pytest.raises(ValueError):
        link.link_faces_poses(faces, poses[0], ctx=ModelContext())              # nested against flat
    with pytest.raises(ValueError):
        link.link_faces_poses(faces, poses, device=[0, 1])
    assert 'pose' in faces[1][0]                                                # nothing was touched
