"""The crowd inputs of tests/pose_crowd.py are what they claim: conditions on the ORACLE alone (no GPU), read from the
event counters `assemble_humans` records, so a later edit of the generator cannot hollow out what
tests/test_gpu_pose_crowd.py runs on the device.  Every test prints the figures it asserts on (pytest -s).

One requirement cannot be met by any input and is replaced, not dropped: no maps make a connection hit three or more
people (the argument is in tests/pose_crowd.py).  `test_three_or_more_hits_need_a_hand_made_connection_list` pins the
argument (the counter is 0 on every case) and drives that branch of the oracle with a connection list that repeats a
peak inside one limb, which the greedy matching never emits.
"""
import numpy as np
import pytest

from oracle import openpose_post
from tests import pose_crowd

FAST_CASES = ['crowd_fast', 'cap_192', 'cap_193']
OP_MAXP, OP_MAXC, OP_MAXH = 1024, 8192, 192          # the fast path's lists (terran_amd/csrc/openpose_post.hip)


def _figures(name):
    dbg = pose_crowd.case_debug(name)
    ev = dbg['events']
    m = ev['merges']
    fig = dict(ev, merges=len(m),
               second_past_64=sum(b >= 64 for a, b, n in m),
               straddle_64=sum(a < 64 <= b for a, b, n in m),
               both_past_64=sum(a >= 64 for a, b, n in m),
               straddle_128=sum(a < 128 <= b for a, b, n in m),
               tail_64=sum(n - 1 - b >= 64 for a, b, n in m),
               deletes_last=sum(b == n - 1 for a, b, n in m),
               max_peaks=max(len(p[1]) for p in dbg['peaks']),
               max_pairs=max(dbg['accepted_pairs']),
               connections=sum(len(c) for c in dbg['connections'] if c is not None),
               survivors=len(dbg['humans']))
    print('%s: %s' % (name, fig))
    return fig


def _inside_the_fast_lists(fig):
    assert fig['max_peaks'] <= OP_MAXP and fig['max_pairs'] <= OP_MAXC


def test_crowd_fast_reaches_every_branch_of_assembly():
    f = _figures('crowd_fast')
    assert 128 < f['max_humans'] <= OP_MAXH
    _inside_the_fast_lists(f)
    assert f['second_past_64'] >= 10          # `second` found by the second / third ballot chunk
    assert f['straddle_64'] >= 3              # `first` and `second` from different chunks
    assert f['both_past_64'] >= 1 and f['straddle_128'] >= 3
    assert f['tail_64'] >= 3                  # the row-by-row shift crosses a 64-row seam
    assert f['deletes_last'] >= 1             # ... and also has nothing to shift
    assert f['overlap'] >= 1 and f['late'] >= 1
    assert f['created'] >= 128 and f['extended'] >= 128 and f['present'] >= 1
    assert f['cut_count'] >= 5 and f['cut_score'] >= 5
    assert f['survivors'] >= 30
    # survivors and rejects interleave in the list: the packing of `kept` sees both before and after one another
    keep = [not (h[19] < 4 or h[18] / h[19] < 0.4) for h in pose_crowd.case_debug('crowd_fast')['unfiltered']]
    flips = sum(a != b for a, b in zip(keep, keep[1:]))
    print('crowd_fast: %d rows before the filter, %d keep / cut alternations' % (len(keep), flips))
    assert flips >= 10


@pytest.mark.parametrize('name', FAST_CASES + ['crowd_big'])
def test_every_part_is_one_peak_and_every_stroke_one_connection(name):
    """The generator's promise: single peaks (no flat tops, no merged Gaussians) and no connection lost to the greedy
    matching's shared `seen` set, so the events above follow from the drop lists and not from accidents."""
    figs = pose_crowd.crowd_figures(pose_crowd.CASES['crowd_fast' if name == 'crowd_big' else name])
    parts, strokes = np.zeros(18, int), np.zeros(19, int)
    for points, lines, _, _ in figs:
        for p, _ in points:
            parts[p] += 1
        for l in lines:
            strokes[l[0]] += 1
    dbg = pose_crowd.case_debug(name)
    got_parts = [len(p[1]) for p in dbg['peaks']]
    got_conns = [0 if c is None else len(c) for c in dbg['connections']]
    print('%s: peaks per part %s, connections per limb %s' % (name, got_parts, got_conns))
    assert got_parts == parts.tolist() and got_conns == strokes.tolist()


def test_cap_cases_differ_by_one_lone_fragment_and_sit_on_the_cap():
    f192, f193 = _figures('cap_192'), _figures('cap_193')
    assert f192['max_humans'] == OP_MAXH and f193['max_humans'] == OP_MAXH + 1
    _inside_the_fast_lists(f192)
    _inside_the_fast_lists(f193)
    assert f192['merges'] >= 10 and f193['merges'] >= 10       # the list at the cap is merged into, not only grown
    a, b = pose_crowd.crowd_figures(pose_crowd.CASES['cap_192']), pose_crowd.crowd_figures(pose_crowd.CASES['cap_193'])
    assert len(b) == len(a) + 1 and [p for p, _ in b[-1][0]] == [pose_crowd.R_ELB, pose_crowd.R_WRI] and len(b[-1][1]) == 1
    for fa, fb in zip(a, b):
        assert all(pa == pb and np.array_equal(xa, xb) for (pa, xa), (pb, xb) in zip(fa[0], fb[0]))
    # ... and on the maps: the difference is one small patch
    (hm_a, paf_a), (hm_b, paf_b) = pose_crowd.case_maps('cap_192'), pose_crowd.case_maps('cap_193')
    ys, xs = np.nonzero((np.abs(hm_a[:18] - hm_b[:18]) > 1e-3).any(0) | (paf_a != paf_b).any(0))
    print('cap_192 / cap_193 maps differ in rows %d..%d, columns %d..%d' % (ys.min(), ys.max(), xs.min(), xs.max()))
    assert 0 < ys.size and ys.max() - ys.min() < 12 and xs.max() - xs.min() < 8     # a 2.8-cell stroke + 3.3 cells of Gaussian
    # cap_193 has one more person before the filter, the same people after it (a lone fragment has two parts)
    assert f193['created'] == f192['created'] + 1 and f193['cut_count'] == f192['cut_count'] + 1
    assert f193['survivors'] == f192['survivors'] >= 30


def test_crowd_big_is_crowd_fast_moved():
    hm, _ = pose_crowd.case_maps('crowd_big')
    assert hm.shape[1] * hm.shape[2] > 10972 >= pose_crowd.H * pose_crowd.W      # past / inside the LDS staging
    fb, ff = _figures('crowd_big'), _figures('crowd_fast')
    assert fb == ff
    assert pose_crowd.case_debug('crowd_big')['events']['merges'] == pose_crowd.case_debug('crowd_fast')['events']['merges']
    big, fast = pose_crowd.case_people('crowd_big', 1.0), pose_crowd.case_people('crowd_fast', 1.0)
    assert len(big) == len(fast) >= 30
    oy, ox = pose_crowd.BIG_OFFSET
    for a, b in zip(big, fast):
        moved = b['keypoints'] + np.array([8 * ox, 8 * oy, 0], np.int32) * b['keypoints'][:, 2:]
        assert np.array_equal(a['keypoints'], moved) and a['score'] == b['score']


def test_three_or_more_hits_need_a_hand_made_connection_list():
    for name in FAST_CASES + ['crowd_big']:
        assert pose_crowd.case_debug(name)['events']['multi'] == 0, name
    # three peaks per part, all at score 1; the limb-17 list names ear 0 TWICE (no greedy matching does)
    peaks = [(np.array([[8 * k + p, 8 * k] for k in range(3)], np.int64), np.ones(3, np.float32)) for p in range(18)]
    conns = [None] * 19
    conns[0] = [(1, 0, 1.0)]                   # neck 1 -> right shoulder 0: person X, row 0
    conns[2] = [(2, 2, 1.0)]                   # right shoulder 2 -> elbow 2: person Z, row 1
    conns[12] = [(0, 0, 1.0)]                  # neck 0 -> nose 0: person Y, row 2 ...
    conns[13] = [(0, 0, 1.0)]                  # ... nose 0 -> right eye 0
    conns[14] = [(0, 0, 1.0)]                  # ... right eye 0 -> right ear 0
    conns[17] = [(0, 0, 1.0), (2, 0, 1.0)]     # shoulder 0 -> ear 0: X, Y overlap (necks); shoulder 2 -> ear 0: X, Y, Z
    dbg = {}
    openpose_post.assemble_humans(peaks, conns, dbg)
    ev = dbg['events']
    print('hand-made list: %s' % ev)
    assert (ev['created'], ev['extended'], ev['overlap'], ev['multi'], ev['merged'], ev['late']) == (3, 2, 1, 1, 0, 0)
    before = {}
    conns[17] = conns[17][:1]
    openpose_post.assemble_humans(peaks, conns, before)
    assert all(np.array_equal(a, b) for a, b in zip(before['unfiltered'], dbg['unfiltered']))    # the third hit did nothing
