"""-m gpu: terran_amd.vis.blur_faces / anonymize_faces / ta_frames_blur against the recorded Pillow golden
(tests/golden/vis_blur.npz) and the numpy restatement of the contract (tests/vis_blur_model.py), bit for bit over whole
frames, so a pixel outside every region is checked too.  Reads no Pillow and no reference."""
import os
import random

import numpy as np
import pytest

from terran_amd import lib, runtime, synth, vis
from tests import vis_blur_model as B
from tests import vis_raster as V

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'vis_blur.npz')

# Region sides on both sides of what csrc/blur.hip switches on: chunks of 8 outputs, at most 256 / lines chunks per line
# (5 in the row stage's 48 lines, 3 in the column stage's 72), strips of 16 rows and of 24 columns, waves of 64, 256 threads.
SIDES = [1, 2, 3, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 33, 40, 41, 47, 48, 49, 63, 64, 65, 71, 73, 127, 129, 140]
WIDE = [255, 256, 257, 300]
RADII = [0.25, 0.3, 1.0, 0.0, 0.1, 2.5, 12.3, 40.0, 300.0, 1024.0]     # float32-sensitive ones, none, r >= n


def _regions(rows):
    q = np.zeros(len(rows), lib.BLUR_DT)
    for i, r in enumerate(rows):
        q[i] = tuple(r)
    return q


def _blur(host, regions, ctx=None):
    ctx = ctx or runtime.get_context(0)
    frames = ctx.upload(host)
    try:
        frames.blur(regions)
        return frames.download()
    finally:
        frames.free()


def _differing(got, want):
    return [int((g != w).any(-1).sum()) for g, w in zip(got, want)]


def fuzz_calls(seed=20261018, calls=6):
    """-> [(host frames (N, H, W, 3), BLUR_DT regions)]: several frames and faces per call, some frames without a face,
    both shapes, sides and radii from the lists above, regions free to overlap."""
    rng = np.random.default_rng(seed)
    out = []
    turn = [0, 0]

    def side(pool, limit, k):                           # every side of the lists gets its turn, in both directions
        while True:
            turn[k] += 1
            s = pool[turn[k] % len(pool)]
            if s <= limit:
                return s
    for c in range(calls):
        n, h, w = int(rng.integers(3, 6)), int(rng.choice([61, 97, 140])), int(rng.choice([83, 257, 300]))
        host = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8) if c % 2 else synth.frames(seed + c, n, h, w)
        rows = []
        for f in range(n):
            for _ in range(0 if f == c % n else int(rng.integers(2, 7))):
                rw, rh = side(WIDE + SIDES, w, 0), side(SIDES[::-1], h, 1)
                x0, y0 = int(rng.integers(0, w - rw + 1)), int(rng.integers(0, h - rh + 1))
                radius = float(rng.choice(RADII)) if rng.random() < 0.8 else max(rw, rh) / 8
                rows.append((f, x0, y0, x0 + rw, y0 + rh, int(rng.integers(0, 2)), radius))
        order = rng.permutation(len(rows))              # regions of different frames interleaved
        out.append((host, _regions([rows[i] for i in order])))
    return out


def test_golden_scenes():
    """anonymize_faces on the host image and blur_faces on a resident batch reproduce every Pillow scene."""
    version, scenes = B.golden_scenes(GOLDEN)
    assert len(scenes) >= 12 and version
    for s in scenes:
        kw = dict(radius=s['radius'], margin=s['margin'], shape=s['shape'])
        base = s['base'].copy()
        got = vis.anonymize_faces(base, s['faces'], **kw)
        assert got is not base and np.array_equal(base, s['base'])
        assert np.array_equal(got, s['expected']), (s['name'], _differing([got], [s['expected']]))
        frames = runtime.get_context(0).upload(np.stack([base, base, base]))
        try:
            assert vis.blur_faces(frames, [[], s['faces']], **kw) is frames
            batch = frames.download()
        finally:
            frames.free()
        assert np.array_equal(batch, np.stack([base, s['expected'], base])), s['name']


def test_fuzz_equals_the_model():
    sides, radii, shapes = set(), set(), set()
    for host, regions in fuzz_calls():
        want = B.blur_regions(host.copy(), regions)
        got = _blur(host, regions)
        assert np.array_equal(got, want), (host.shape, _differing(got, want))
        sides |= set((regions['x1'] - regions['x0']).tolist()) | set((regions['y1'] - regions['y0']).tolist())
        radii |= set(regions['radius'].tolist())
        shapes |= set(regions['shape'].tolist())
    assert shapes == {0, 1} and {np.float32(0.25), np.float32(0.3), 1.0, 1024.0} <= radii
    assert {63, 64, 65, 255, 256, 257} <= sides and {15, 17, 23, 25} <= sides, sorted(sides)


def test_1080p_regions_at_the_lds_limits():
    """One 1080p frame: a 700 x 500 region at radius 40, a full-height 60 x 1080 one (the column stage's largest strip) and
    a full-width 1920 x 40 ellipse (the row stage's longest line)."""
    host = synth.frames(31, 1, 1080, 1920)
    noise = np.random.default_rng(2).integers(0, 256, host.shape, dtype=np.uint8)
    host = np.where(noise < 64, noise, host).astype(np.uint8)       # speckles: rounding shows everywhere
    regions = _regions([(0, 100, 200, 800, 700, lib.BLUR_BOX, 40.0), (0, 1000, 0, 1060, 1080, lib.BLUR_BOX, 7.5),
                        (0, 0, 1030, 1920, 1070, lib.BLUR_ELLIPSE, 3.0), (0, 1100, 100, 1700, 1000, lib.BLUR_ELLIPSE, 112.5)])
    assert lib.blur_plan(regions)[0].tolist() == [0, 0, 1, 0]
    want = B.blur_regions(host.copy(), regions)
    got = _blur(host, regions)
    assert np.array_equal(got, want), _differing(got, want)
    assert (want != host).any(-1).sum() > 700 * 500


def test_overlapping_faces_are_applied_in_list_order():
    rng = np.random.default_rng(17)
    h, w = 120, 160
    host = rng.integers(0, 256, (2, h, w, 3), dtype=np.uint8)
    faces = []
    for _ in range(40):                                 # piled on one frame: a long chain of rounds
        x0, y0 = rng.uniform(-10, w - 20), rng.uniform(-10, h - 20)
        faces.append({'bbox': np.array([x0, y0, x0 + rng.uniform(8, 70), y0 + rng.uniform(8, 70)], np.float32)})
    per_frame = [faces, faces[:2]]
    regions = vis.pack_blur(per_frame, host.shape, shape='ellipse')
    rounds = lib.blur_plan(regions)[0]
    assert len(regions) == 42 and rounds.tolist() == B.rounds(regions) and rounds.max() >= 4
    frames = runtime.get_context(0).upload(host)
    try:
        vis.blur_faces(frames, per_frame, shape='ellipse')
        got = frames.download()
    finally:
        frames.free()
    want = np.stack([B.anonymize(host[0], faces, shape='ellipse'), B.anonymize(host[1], faces[:2], shape='ellipse')])
    assert np.array_equal(got, want), _differing(got, want)
    backwards = B.anonymize(host[0], faces[::-1], shape='ellipse')
    assert not np.array_equal(want[0], backwards)       # the order does matter here


def test_invalid_regions_change_nothing():
    host = synth.frames(4, 2, 50, 70)
    good = (1, 5, 5, 40, 30, lib.BLUR_BOX, 3.0)
    bad = [(2, 0, 0, 9, 9, 0, 1.0), (-1, 0, 0, 9, 9, 0, 1.0),                       # frame index out of range
           (0, 9, 0, 9, 9, 0, 1.0), (0, 0, 12, 9, 12, 0, 1.0), (0, 9, 0, 3, 9, 0, 1.0),   # empty, inverted
           (0, -1, 0, 9, 9, 0, 1.0), (0, 0, 0, 71, 9, 0, 1.0), (0, 0, 0, 9, 51, 0, 1.0), (0, 0, -2, 9, 9, 0, 1.0),
           (0, 0, 0, 9, 9, 2, 1.0), (0, 0, 0, 9, 9, -1, 1.0),                       # unknown shape
           (0, 0, 0, 9, 9, 0, -0.5), (0, 0, 0, 9, 9, 0, np.nan), (0, 0, 0, 9, 9, 0, np.inf), (0, 0, 0, 9, 9, 0, 1024.5)]
    ctx = runtime.get_context(0)
    frames = ctx.upload(host)
    try:
        for b in bad:
            with pytest.raises(lib.TerranAmdError) as e:
                frames.blur(_regions([good, b, good]))
            assert e.value.code == lib.E_INVALID and 'region 1' in str(e.value), b
        assert np.array_equal(frames.download(), host)
        frames.blur(_regions([]))                        # n = 0: TA_OK
        frames.blur(_regions([(0, 0, 0, 70, 50, lib.BLUR_ELLIPSE, 0.0)]))      # radius 0: unchanged
        assert np.array_equal(frames.download(), host)
        with pytest.raises(ValueError):                  # the Python layer refuses before it launches, too
            vis.blur_faces(frames, [[{'bbox': [1, 1, 30, 30]}], [{'bbox': [1, 1, 30, 30]}]], radius=-1)
        with pytest.raises(ValueError):
            vis.blur_faces(frames, [[], [], []])
        assert np.array_equal(frames.download(), host)
        frames.blur(_regions([good]))
        assert np.array_equal(frames.download(), B.blur_regions(host.copy(), _regions([good])))
    finally:
        frames.free()
    img = host[0]
    out = vis.anonymize_faces(img, [])
    assert out is not img and np.array_equal(out, img)
    face = {'bbox': np.array([3.5, 4, 40, 30], np.float32), 'track': 7}           # a single dict, face_tracking's keys
    assert np.array_equal(vis.anonymize_faces(img, face, margin=0.2), B.anonymize(img, [face], margin=0.2))


def test_blur_then_draw_on_one_context_is_ordered(monkeypatch):
    """blur_faces followed by draw_faces on the caller's context: the markers lie over the blurred faces."""
    rng = np.random.default_rng(23)
    n, h, w = 3, 97, 140
    host = synth.frames(8, n, h, w)
    faces = []
    for i in range(n):
        b = []
        for j in range(3):
            x0, y0 = rng.uniform(-10, w - 30), rng.uniform(-10, h - 30)
            b.append({'bbox': np.array([x0, y0, x0 + rng.uniform(15, 80), y0 + rng.uniform(15, 60)], np.float32),
                      'name': 'p%d' % j})
        faces.append(b)
    ctx = runtime.new_context(0)
    frames = runtime.get_context(0).upload(host)
    try:
        monkeypatch.setattr(vis, 'FACE_COLORMAP', vis.build_colormap())
        random.seed(1)
        vis.blur_faces(frames, faces, margin=0.1, ctx=ctx)
        vis.draw_faces(frames, faces, ctx=ctx)
        got = frames.download()
    finally:
        frames.free()
    monkeypatch.setattr(vis, 'FACE_COLORMAP', vis.build_colormap())
    random.seed(1)
    want = np.stack([B.anonymize(img, f, margin=0.1) for img, f in zip(host, faces)])
    blurred = want.copy()
    V.draw_prims(want, vis.pack_faces(faces))
    assert np.array_equal(got, want), _differing(got, want)
    assert not np.array_equal(want, blurred) and not np.array_equal(blurred, host)
