"""-m gpu: ta_frames_transform / ta_frames_transpose and their callers (image.transform_frames, transpose_frames,
rotate_frames, vis.align_faces) against the recorded Pillow golden (tests/golden/transform.npz), bit for bit, and
align_faces against the crops the embedder cuts.  Reads no Pillow and no reference."""
import os

import numpy as np
import pytest

from terran_amd import arcface, image, lib, runtime, vis
from tests import transform_model as M

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'transform.npz')


@pytest.fixture(scope='module')
def golden():
    return M.golden(GOLDEN)


@pytest.fixture(scope='module')
def resident(golden):
    """The golden's sources, uploaded once."""
    ctx = runtime.get_context(0)
    frames = [ctx.upload(s) for s in golden[1]]
    yield frames
    for f in frames:
        f.free()


def _regions(rows):
    q = np.zeros(len(rows), lib.TRANSFORM_DT)
    for i, (frame, method, a) in enumerate(rows):
        q[i]['frame'], q[i]['method'] = frame, method
        q[i]['a'][:len(a)] = a
    return q


def _get(frames):
    try:
        return frames.download()
    finally:
        frames.free()


def test_transform_equals_the_golden(golden, resident):
    """Every matrix of the golden (identity, translations, pure scale, rotation with shear, mirrored, all outside, sample
    points on the borders, two perspectives) for the three filters; sources 1 x 1 .. 300 x 517; outputs 1 x 1, 5 x 3, 64 x 48,
    131 x 67; one call of 8 regions over 3 frames, out of order and repeated."""
    _, S, cases, _, _ = golden
    seen, routes, multi = set(), set(), 0
    for k, c in enumerate(cases):
        got = _get(resident[c['source']].transform(_regions(c['regions']), c['size'][1], c['size'][0], c['filter'], c['fill']))
        assert got.shape == c['expected'].shape, (k, got.shape)
        assert np.array_equal(got, c['expected']), (k, c['source'], c['filter'], c['size'], c['fill'],
                                                    [int((g != e).any(-1).sum()) for g, e in zip(got, c['expected'])])
        for _, m, a in c['regions']:
            seen.add((c['filter'], m, c['fill'] is None))
            if c['filter'] == lib.NEAREST:
                routes.add(M.nearest_route(m, a, *c['size']))
        frames = [r[0] for r in c['regions']]
        if len(frames) == 8:
            assert frames != sorted(frames) and set(frames) == {0, 1, 2}
            multi += 1
    assert seen >= {(f, m, n) for f in lib.TRANSFORM_FILTERS for m in (lib.AFFINE, lib.PERSPECTIVE) for n in (False, True)}
    assert routes == {'scale', 'fixed', 'accumulate', 'generic'} and multi == 3
    assert {c['size'] for c in cases} >= {(1, 1), (5, 3), (64, 48), (131, 67)}


def test_transpose_equals_the_golden(golden, resident):
    _, _, _, transposes, _ = golden
    for c in transposes:
        got = _get(resident[c['source']].transpose(c['op']))
        assert got.shape == c['expected'].shape and np.array_equal(got, c['expected']), (c['source'], c['op'])
    assert {c['op'] for c in transposes} == set(range(7)) and len(transposes) == 21


def test_images_that_do_not_start_on_a_dword_and_tiles_beyond_one():
    """3 regions of 5 x 7 (105 bytes an image: the byte-store path for images 1 and 2 and the ragged tail) and a transpose
    of more than one tile in both directions, against the model."""
    src = M.noise(70, 45, 21)[None]
    rows = [(0, lib.AFFINE, (6.1, 0.4, 1.0, -0.3, 9.7, 2.0)), (0, lib.PERSPECTIVE, (6.0, 0, 0, 0, 9.0, 0, 0.01, 0.002)),
            (0, lib.AFFINE, (1, 0, 20, 0, 1, 30))]
    ctx = runtime.get_context(0)
    frames = ctx.upload(src)
    try:
        for filt in lib.TRANSFORM_FILTERS:
            got = _get(frames.transform(_regions(rows), 7, 5, filt, (200, 100, 50)))
            want = np.stack([M.transform(src[0], (5, 7), m, a, filt, (200, 100, 50)) for _, m, a in rows])
            assert np.array_equal(got, want), filt
        for op in range(7):
            assert np.array_equal(_get(frames.transpose(op)), M.transpose(src, op)), op
    finally:
        frames.free()


def test_the_public_functions_on_a_batch_and_on_a_mixed_list(golden, resident):
    z, S, _, transposes, rotates = golden
    made = []

    def keep(f):
        made.extend(f if isinstance(f, list) else [f])
        return f
    try:
        out = keep(image.transform_frames(resident[2], (40, 30), 'perspective', z['api_one_data'], 'bicubic'))
        assert out.shape == (3, 30, 40, 3) and np.array_equal(out.download(), z['api_one'])
        out = keep(image.transform_frames(resident[2], (40, 30), lib.AFFINE, z['api_per_data'], resample=lib.BILINEAR, fillcolor=(7, 8, 9)))
        assert np.array_equal(out.download(), z['api_per'])
        first = keep(runtime.get_context(0).upload(S[2][:1]))
        mixed = [first, resident[7], resident[1]]
        out = keep(image.transform_frames(mixed, (40, 30), 'affine', z['api_mixed_data'], 'bilinear', (7, 8, 9)))
        assert isinstance(out, lib.Frames) and out.shape == (3, 30, 40, 3) and np.array_equal(out.download(), z['api_mixed'])
        out = keep(image.transform_frames(mixed[::-1], (40, 30), 'affine', np.tile(z['api_mixed_data'], (3, 1)), 'bilinear', (7, 8, 9)))
        assert np.array_equal(out.download(), z['api_mixed'][::-1])

        tp = {(c['source'], c['op']): c['expected'] for c in transposes}
        for op, name in enumerate(('flip_left_right', 'flip_top_bottom', 'rotate_90', 'rotate_180', 'rotate_270', 'transpose', 'transverse')):
            out = keep(image.transpose_frames(resident[5], name))
            assert np.array_equal(out.download(), tp[5, op]), name
            outs = keep(image.transpose_frames([resident[0], resident[6]], op))
            assert isinstance(outs, list) and [np.array_equal(o.download(), tp[s, op]) for o, s in zip(outs, (0, 6))] == [True, True], name

        by = {}
        for c in rotates:
            by[c['source'], c['angle'], c['expand'], c['center'] is not None, c['filter']] = c
        for (src, angle, expand, moved, filt), c in by.items():
            if src != 6:
                continue
            kw = dict(center=c['center'], translate=c['translate']) if moved else {}
            name = {lib.NEAREST: 'nearest', lib.BICUBIC: 'bicubic'}[filt]
            outs = keep(image.rotate_frames([resident[6], resident[7]], angle, name, expand, **kw))
            for o, s in zip(outs, (6, 7)):
                want = by[s, angle, expand, moved, filt]['expected']
                assert o.shape == (1,) + want.shape and np.array_equal(o.download()[0], want), (s, angle, expand, moved, filt)
            _free_now(made)
        out = keep(image.rotate_frames(resident[6], 5.0, 'bilinear', fillcolor=(7, 8, 9)))
        assert np.array_equal(out.download()[0], z['api_tilt'])
        assert np.array_equal(resident[6].download(), S[6])                   # the sources are only read
    finally:
        _free_now(made)


def _free_now(made):
    while made:
        made.pop().free()


def test_align_faces_cuts_the_crops_the_embedder_cuts(states):
    """One 200 x 260 frame, three landmark sets, one of which pushes part of its chip outside the frame: align_faces at
    (112, 112) bilinear equals the crops_out of the embed call (NCHW BGR there), bit for bit; other sizes and filters equal
    the model on the same matrices."""
    from terran_amd import ArcFace
    frame = M.noise(200, 260, 31)
    frame[40:160, 60:200] = M.blocks(120, 140, 2)
    t = arcface._TEMPLATE.astype(np.float64)
    rot = np.array([[np.cos(0.3), -np.sin(0.3)], [np.sin(0.3), np.cos(0.3)]])
    lms = [t * 0.9 + (70, 40), (t - 56) @ rot.T * 1.4 + (150, 110), t * 1.1 + (-30, 120)]          # the last: partly outside on the left
    faces = [[{'bbox': [0, 0, 1, 1], 'landmarks': lm.astype(np.float32)} for lm in lms]]
    arc = ArcFace(device=0, state=states('arcface'))
    frames = arc.ctx.upload(frame[None])
    chips = other = None
    try:
        _, crops = arc.embed_faces(frames, [0, 0, 0], arcface.align_matrices(np.stack(lms)), return_crops=True)
        want = np.ascontiguousarray(crops[:, ::-1].transpose(0, 2, 3, 1))
        chips, index = vis.align_faces(frames, faces, ctx=arc.ctx)
        got = chips.download()
        assert index.tolist() == [[0, 0], [0, 1], [0, 2]] and got.shape == (3, 112, 112, 3)
        assert np.array_equal(got, want), [int((g != w).any(-1).sum()) for g, w in zip(got, want)]
        assert (got[2].reshape(-1, 3) == 0).all(1).mean() > 0.1 and got[0].any() and got[1].any()    # fill inside the third chip
        other, _ = vis.align_faces(frames, faces, size=(64, 64), resample='bicubic', ctx=arc.ctx)
        mats = arcface.align_matrices(np.stack(lms).astype(np.float32), 64)
        assert np.array_equal(other.download(), np.stack([M.transform(frame, (64, 64), M.AFFINE, a, M.BICUBIC) for a in mats]))
        assert vis.align_faces(frames, [[]]) == (None, [])
    finally:
        for f in (chips, other, frames):
            if f is not None:
                f.free()


def test_invalid_arguments_are_rejected_and_a_valid_call_still_works(resident, golden):
    _, S, _, _, _ = golden
    frames = resident[2]
    good = (1, lib.AFFINE, (1, 0, 2, 0, 1, 3))
    assert frames.transform(_regions([]), 5, 5, lib.BICUBIC) is None                  # n = 0
    for bad in [(3, lib.AFFINE, good[2]), (-1, lib.AFFINE, good[2]), (0, 1, good[2]), (0, 3, good[2]), (0, -1, good[2]),
                (0, lib.AFFINE, (1, 0, np.nan, 0, 1, 0)), (0, lib.AFFINE, (np.inf, 0, 0, 0, 1, 0)),
                (0, lib.PERSPECTIVE, (1, 0, 0, 0, 1, 0, 0, -np.inf)), (0, lib.PERSPECTIVE, (1, 0, 0, 0, 1, 0, np.nan, 0))]:
        with pytest.raises(lib.TerranAmdError) as e:
            frames.transform(_regions([good, bad]), 8, 8, lib.BILINEAR)
        assert e.value.code == lib.E_INVALID and 'region 1' in str(e.value), bad
    for filt, oh, ow in [(1, 8, 8), (4, 8, 8), (5, 8, 8), (6, 8, 8), (-1, 8, 8), (2, 0, 8), (2, 8, 0), (2, -3, 8), (2, 16385, 8), (2, 8, 16385)]:
        with pytest.raises(lib.TerranAmdError) as e:
            frames.transform(_regions([good]), oh, ow, filt)
        assert e.value.code == lib.E_INVALID, (filt, oh, ow)
    for op in (-1, 7, 100):
        with pytest.raises(lib.TerranAmdError) as e:
            frames.transpose(op)
        assert e.value.code == lib.E_INVALID, op
    # AFFINE does not read a[6], a[7]
    q = _regions([good])
    q['a'][0, 6:] = np.nan
    want = M.transform(S[2][1], (8, 8), M.AFFINE, good[2], M.BILINEAR, (1, 2, 3))
    assert np.array_equal(_get(frames.transform(q, 8, 8, lib.BILINEAR, (1, 2, 3)))[0], want)
    assert np.array_equal(_get(frames.transpose(lib.ROTATE_90)), M.transpose(S[2], M.ROTATE_90))
    assert np.array_equal(frames.download(), S[2])
