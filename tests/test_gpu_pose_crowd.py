"""-m gpu: pose assembly (assemble_kernel, op_rerun_image in terran_amd/csrc/openpose_post.hip) on crowds.

The inputs are tests/pose_crowd.py's; tests/test_pose_crowd_cpu.py shows from the oracle's event counters what each one
reaches (merges whose two rows come from different 64-lane ballot chunks, row shifts across a 64-row seam, the overlap
and late-limb branches, a list of exactly 192 / 193 people, a filter with keep and cut interleaved).  Here the device
must return the oracle's people EXACTLY -- counts, order, keypoints, float64 scores with `==` -- and its peak and
connection taps must equal the oracle's (`_assert_stage_taps_equal`).  No tolerances.
"""
import hashlib

import numpy as np
import pytest

from terran_amd import synth
from tests import pose_crowd
from tests.test_gpu_pipeline import _assert_stage_taps_equal

pytestmark = pytest.mark.gpu
FAST_ROWS = 1024                 # rows per part of the batch pass's lists (OP_MAXP); a re-run is sized from its own counts


@pytest.fixture(scope='module')
def ctx():
    from terran_amd import runtime
    return runtime.get_context(0)


@pytest.fixture(scope='module', autouse=True)
def oracle_once():
    """The oracle takes seconds per 96 x 112 image and every test here (and `_assert_stage_taps_equal`, which calls it
    itself) asks for the same few images: compute each image's stages once per module.  Keys are digests of the
    network-resolution maps; the stages do not depend on `scale`, only the final keypoint division does, which is
    redone per call."""
    from oracle import openpose_post
    real_up, real_group = openpose_post.bicubic_x8, openpose_post.group_image
    ups, groups, names = {}, {}, {}

    def digest(*arrays):
        d = hashlib.blake2b(digest_size=16)
        for a in arrays:
            d.update(str(a.shape).encode())
            d.update(np.ascontiguousarray(a))
        return d.digest()

    def bicubic_x8(x, impl='numpy'):
        x = np.asarray(x, np.float32)
        if x.ndim not in (3, 4) or impl != 'numpy':
            return real_up(x, impl)
        out = []
        for img in (x if x.ndim == 4 else x[None]):
            k = digest(img)
            if k not in ups:
                ups[k] = real_up(img)
                ups[k].setflags(write=False)
                names[id(ups[k])] = k                       # the x8 maps are kept, so their ids stay theirs
            out.append(ups[k])
        return out if x.ndim == 4 else out[0]              # a batch comes back as a list: the callers index it per image

    def group_image(heatmaps_up, pafs_up, scale, debug=None):
        k = tuple(names[id(a)] if id(a) in names else digest(a) for a in (heatmaps_up, pafs_up))
        if k not in groups:
            dbg = {}
            real_group(heatmaps_up, pafs_up, scale, dbg)
            dbg['peaks_by_id'] = openpose_post.assemble_humans(dbg['peaks'], dbg['connections'])[0]
            groups[k] = dbg
        if debug is not None:
            debug.update(groups[k])
        return openpose_post.keypoints_out(groups[k]['peaks_by_id'], groups[k]['humans'], scale)

    openpose_post.bicubic_x8, openpose_post.group_image = bicubic_x8, group_image
    yield
    openpose_post.bicubic_x8, openpose_post.group_image = real_up, real_group


def _oracle(hm, paf, scale):
    from oracle import openpose_post
    hm_up, paf_up = openpose_post.bicubic_x8(hm), openpose_post.bicubic_x8(paf)
    return [openpose_post.group_image(hm_up[i], paf_up[i], scale) for i in range(len(hm))]


def _assert_people_equal(got, ref, what=''):
    assert [len(g) for g in got] == [len(r) for r in ref], what
    for i, (gp, rp) in enumerate(zip(got, ref)):
        for k, (a, b) in enumerate(zip(gp, rp)):
            assert a['keypoints'].dtype == np.int32 and np.array_equal(a['keypoints'], b['keypoints']), (what, i, k)
            assert isinstance(a['score'], np.float64) and a['score'] == b['score'], (what, i, k)


def _batch(names):
    """Maps of a batch: crowd cases by name, 'ordinary<k>' = a noisy synth.pose_maps image of six people."""
    maps = [synth.pose_maps(40 + int(n[8:]), 6, pose_crowd.H, pose_crowd.W) if n.startswith('ordinary')
            else pose_crowd.case_maps(n) for n in names]
    return np.stack([m[0] for m in maps]), np.stack([m[1] for m in maps])


def test_crowd_alone_equals_the_oracle(ctx):
    """184 people under assembly in LDS, 55 merges, at scale 0.37 (the keypoint division on 38 rows)."""
    from terran_amd import openpose
    hm, paf = _batch(['crowd_fast'])
    got = openpose.group(ctx, paf, hm, 0.37)
    ref = [pose_crowd.case_people('crowd_fast', 0.37)]
    assert len(ref[0]) >= 30
    _assert_people_equal(got, ref, 'crowd_fast')
    assert ctx.pose_debug_capacity(1) == [FAST_ROWS]
    n_peaks, n_conn = _assert_stage_taps_equal(ctx, 1, hm, paf, scale=0.37)
    assert ctx.pose_stats() == (n_peaks, n_conn) and n_conn > 600


def test_crowd_in_the_middle_of_a_batch(ctx):
    from terran_amd import openpose
    hm, paf = _batch(['ordinary0', 'crowd_fast', 'ordinary1'])
    got = openpose.group(ctx, paf, hm, 1.0)
    ref = _oracle(hm, paf, 1.0)
    assert len(ref[0]) > 0 and len(ref[2]) > 0
    _assert_people_equal(got, ref, 'batch of 3')
    _assert_people_equal(got[1:2], [pose_crowd.case_people('crowd_fast', 1.0)], 'crowd_fast as image 1')
    assert ctx.pose_debug_capacity(3) == [FAST_ROWS] * 3
    _assert_stage_taps_equal(ctx, 3, hm, paf)


@pytest.mark.parametrize('name, rerun', [('cap_192', False), ('cap_193', True)])
def test_the_cap_as_an_edge(ctx, name, rerun):
    """192 people under assembly fill the LDS list to its last row and stay on the fast path; one lone fragment more
    sets `over`, the image reports nothing and is re-run alone with lists sized from its own counts (72 peaks of one
    part at the most: assembly alone raised the overflow).  Scale 1.7."""
    from terran_amd import openpose
    hm, paf = _batch([name])
    dbg = pose_crowd.case_debug(name)
    assert dbg['events']['max_humans'] == (193 if rerun else 192)
    got = openpose.group(ctx, paf, hm, 1.7)
    _assert_people_equal(got, [pose_crowd.case_people(name, 1.7)], name)
    most_peaks = max(len(p[1]) for p in dbg['peaks'])
    assert most_peaks < FAST_ROWS and max(dbg['accepted_pairs']) < 8192
    assert ctx.pose_debug_capacity(1) == [most_peaks if rerun else FAST_ROWS]
    n_peaks, n_conn = _assert_stage_taps_equal(ctx, 1, hm, paf, scale=1.7)
    assert ctx.pose_stats() == (n_peaks, n_conn)


def test_reruns_first_and_last_of_a_batch(ctx):
    """[cap_193, ordinary, crowd_fast, cap_193]: the first and the last image are re-run (by assembly's overflow only),
    their rows are spliced in image order around the fast path's, which are untouched; an ordinary call afterwards on
    the same context is still right."""
    from terran_amd import openpose
    names = ['cap_193', 'ordinary0', 'crowd_fast', 'cap_193']
    hm, paf = _batch(names)
    got = openpose.group(ctx, paf, hm, 1.0)
    ref = _oracle(hm, paf, 1.0)
    assert all(len(r) > 0 for r in ref)
    _assert_people_equal(got, ref, 'batch of 4')
    for i in (0, 2, 3):
        _assert_people_equal(got[i:i + 1], [pose_crowd.case_people(names[i], 1.0)], names[i])
    most_peaks = max(len(p[1]) for p in pose_crowd.case_debug('cap_193')['peaks'])
    assert ctx.pose_debug_capacity(4) == [most_peaks, FAST_ROWS, FAST_ROWS, most_peaks]
    n_peaks, n_conn = _assert_stage_taps_equal(ctx, 4, hm, paf)
    assert ctx.pose_stats() == (n_peaks, n_conn)
    hm1, paf1 = _batch(['ordinary1'])
    again = openpose.group(ctx, paf1, hm1, 1.0)
    _assert_people_equal(again, _oracle(hm1, paf1, 1.0), 'ordinary call after the re-runs')
    assert ctx.pose_debug_capacity(1) == [FAST_ROWS] and len(again[0]) > 0


def test_crowd_past_the_lds_staging(ctx):
    """The same crowd in a 100 x 112 canvas: the whole batch takes the global-memory kernels, assemble_kernel<true>
    merges and shifts rows of a list in global memory.  == the oracle, and == the fast path's people moved by the
    embedding offset."""
    from terran_amd import openpose
    hm, paf = _batch(['crowd_big'])
    assert hm.shape[2] * hm.shape[3] > 10972
    got = openpose.group(ctx, paf, hm, 1.0)
    _assert_people_equal(got, [pose_crowd.case_people('crowd_big', 1.0)], 'crowd_big')
    assert ctx.pose_debug_capacity(1) == [FAST_ROWS]          # not re-run: the batch pass itself ran the global-memory kernels
    _assert_stage_taps_equal(ctx, 1, hm, paf)
    hm_f, paf_f = _batch(['crowd_fast'])
    fast = openpose.group(ctx, paf_f, hm_f, 1.0)
    oy, ox = pose_crowd.BIG_OFFSET
    assert len(fast[0]) == len(got[0]) >= 30
    for a, b in zip(got[0], fast[0]):
        moved = b['keypoints'] + np.array([8 * ox, 8 * oy, 0], np.int32) * b['keypoints'][:, 2:]
        assert np.array_equal(a['keypoints'], moved) and a['score'] == b['score']
