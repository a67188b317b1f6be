"""-m gpu: ta_frames_transform_mesh and its callers (image.mesh_frames, quad_frames, extent_frames, undistort_frames,
vis.quad_chips) against the recorded Pillow golden (tests/golden/mesh.npz), bit for bit.  Reads no Pillow and no reference."""
import os

import numpy as np
import pytest

from terran_amd import image, lib, runtime, vis
from tests import mesh_model as M

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'mesh.npz')


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


def _cells(rows):
    a = np.zeros(len(rows), lib.MESH_CELL_DT)
    for k, r in enumerate(rows):
        a[k] = tuple(int(v) for v in r[:4]) + (tuple(r[4:]),)
    return a


def _images(pairs):
    return np.array(pairs, np.int32).reshape(-1, 2).view(lib.MESH_IMAGE_DT).reshape(-1)


def _get(frames):
    try:
        return frames.download()
    finally:
        frames.free()


def _run(frames, meshes, images, size, filt, fill):
    rows, first = M.pack(meshes)
    return _get(frames.transform_mesh(_cells(rows), first, _images(images), size[1], size[0], filt, fill))


@pytest.mark.parametrize('name', sorted(M.cases()))
def test_a_case_equals_the_golden(golden, resident, name):
    """The cases of tests/mesh_model.py: a 16-pixel lattice over 67 x 35, 1 x 1 cells, one cell over the image (QUAD),
    overlapping cells whose later points leave the source, a gap, a negative origin, cells past and wholly outside the
    output, a mirrored quad, a quad that leaves the source on all sides, outputs of tile - 1, tile, tile + 1 and 3 x 3
    tiles, three 105-byte images, two meshes shared by six images out of order, an empty mesh, sources of 1 x 1 and one row;
    each for the three filters and for fillcolor None and a colour."""
    _, _, C, want = golden
    src, size, meshes, images = C[name]
    for filt in M.FILTERS:
        for nofill in (True, False):
            got = _run(resident[src], meshes, images, size, filt, None if nofill else M.FILL)
            w = want[name, filt, nofill]
            assert got.shape == w.shape, (filt, nofill, got.shape)
            assert np.array_equal(got, w), (filt, nofill, [int((g != e).any(-1).sum()) for g, e in zip(got, w)])


def test_the_cases_cover_what_they_claim(golden):
    _, S, C, want = golden
    tw, th = lib.MESH_TILE_W, lib.MESH_TILE_H
    assert {(tw - 1, th - 1), (tw, th), (tw + 1, th + 1)} <= {c[1] for c in C.values()}
    assert C['bytes'][1][0] * C['bytes'][1][1] * 3 % 4 and len(C['bytes'][3]) == 3
    frames = [f for f, _ in C['two_meshes'][3]]
    assert frames != sorted(frames) and len(set(C['two_meshes'][3])) < len(C['two_meshes'][3]) and {m for _, m in C['two_meshes'][3]} == {0, 1}
    assert S[C['source_1x1'][0]].shape[1:3] == (1, 1) and S[C['source_row'][0]].shape[1] == 1
    assert all(b[2] - b[0] == 1 and b[3] - b[1] == 1 for b, _ in C['ones'][2][0])
    assert any(b[0] < 0 and b[1] < 0 for b, _ in C['negative'][2][0])
    for filt in M.FILTERS:                              # only the fill colour lets the earlier cell show through
        assert (want['overlap', filt, True] != want['overlap', filt, False]).any()


def test_the_public_functions_on_a_batch_and_on_a_mixed_list(golden, resident):
    z, S, _, _ = golden
    ctx = runtime.get_context(0)
    made = []

    def keep(f):
        made.append(f)
        return f
    try:
        fr = resident[3]
        own = M.lattice(53, 37, 10, 53, 37, wobble=0.25, reach=1.1)
        out = keep(image.mesh_frames(fr, own, resample='bilinear'))                       # size: the frames' own
        assert out.shape == (3, 37, 53, 3) and np.array_equal(out.download(), z['api_mesh_batch'])
        per = [M.lattice(40, 30, 9 + k, 53, 37, wobble=0.1 * (k + 1), reach=1.05) for k in range(3)]
        out = keep(image.mesh_frames(fr, per, (40, 30), lib.BICUBIC, M.FILL))             # one mesh per frame
        assert np.array_equal(out.download(), z['api_mesh_per'])
        first = keep(ctx.upload(S[3][:1]))
        mixed = [first, resident[4], resident[0]]
        one = M.lattice(40, 30, 13, 45, 30, reach=1.1)
        out = keep(image.mesh_frames(mixed, one, (40, 30), 'nearest', M.FILL))
        assert isinstance(out, lib.Frames) and out.shape == (3, 30, 40, 3) and np.array_equal(out.download(), z['api_mesh_mixed'])
        out = keep(image.mesh_frames(mixed[::-1], [one] * 3, (40, 30), 'nearest', M.FILL))
        assert np.array_equal(out.download(), z['api_mesh_mixed'][::-1])
        out = keep(image.mesh_frames(fr, M.Deformer(), resample='bilinear'))              # ImageOps.deform
        assert np.array_equal(out.download(), z['api_deform_batch'])
        second = keep(ctx.upload(S[3][1:2]))
        out = keep(image.mesh_frames([resident[4], second], M.Deformer(), (50, 35), 'bilinear'))
        assert out.shape == (2, 35, 50, 3) and np.array_equal(out.download(), z['api_deform_mixed'])

        out = keep(image.quad_frames(fr, (30, 20), M.API_QUADS, 'bilinear'))
        assert np.array_equal(out.download(), z['api_quad_per'])
        out = keep(image.quad_frames(fr, (30, 20), M.API_QUADS[2], 'nearest', M.FILL))
        assert np.array_equal(out.download(), z['api_quad_one'])
        for filt in M.FILTERS:
            out = keep(image.extent_frames(fr, (30, 20), M.API_EXTENTS, filt, M.FILL))
            assert np.array_equal(out.download(), z['api_extent_per_%d' % filt]), filt
        out = keep(image.extent_frames(mixed, (30, 20), M.API_EXTENTS[0], 'bicubic'))
        assert np.array_equal(out.download(), z['api_extent_one'])
        assert np.array_equal(fr.download(), S[3])                                        # the sources are only read
    finally:
        while made:
            made.pop().free()


def test_quad_chips_come_in_index_order(golden, resident):
    z, _, _, _ = golden
    chips, index = vis.quad_chips(resident[3], M.CHIP_QUADS, (16, 12))
    try:
        assert index.tolist() == [[0, 0], [0, 1], [2, 0]] and chips.shape == (3, 12, 16, 3)
        assert np.array_equal(chips.download(), z['api_chips'])
    finally:
        chips.free()
    assert vis.quad_chips(resident[3], [[], [], []], (16, 12)) == (None, [])


def test_undistort_frames_equals_pillow_with_its_own_mesh(golden, resident):
    z, _, _, _ = golden
    for tag, kw in (('new', dict(grid=8, resample='bilinear', new_camera_matrix=M.NEW_CAMERA)), ('own', dict(resample='nearest', fillcolor=M.FILL)),
                    ('cubic', dict(grid=5, resample='bicubic'))):
        out = image.undistort_frames(resident[3], M.CAMERA, M.DIST, **kw)
        assert out.shape == (3, 37, 53, 3) and np.array_equal(_get(out), z['undistort_%s' % tag]), tag


def test_invalid_arguments_are_rejected_and_a_valid_call_still_works(golden, resident):
    _, S, C, want = golden
    frames = resident[3]
    _, size, meshes, _ = C['two_meshes']
    rows, first = M.pack(meshes)
    cells = _cells(rows)
    good = [(0, 0), (2, 1)]

    def call(cells=cells, first=first, images=good, oh=size[1], ow=size[0], filt=lib.BILINEAR):
        return frames.transform_mesh(cells, first, _images(images), oh, ow, filt)
    assert call(images=[]) is None                                                        # n_images = 0
    bad_box = cells.copy()
    bad_box[3]['x1'] = bad_box[3]['x0']
    far = cells.copy()
    far[1]['y0'] = -(1 << 24) - 1
    nan = cells.copy()
    nan[2]['quad'][5] = np.nan
    n = len(cells)
    for kw in [dict(images=[(3, 0)]), dict(images=[(-1, 0)]), dict(images=[(0, 2)]), dict(images=[(0, -1)]), dict(cells=bad_box), dict(cells=far),
               dict(cells=nan), dict(first=[0, n + 1, n + 1]), dict(first=[0, 5, 4]), dict(first=[-1, 2, n]), dict(filt=1), dict(filt=4),
               dict(filt=-1), dict(oh=0), dict(ow=0), dict(oh=16385), dict(ow=-2)]:
        with pytest.raises(lib.TerranAmdError) as e:
            call(**kw)
        assert e.value.code == lib.E_INVALID, kw
    got = _get(call(images=C['two_meshes'][3]))
    assert np.array_equal(got, want['two_meshes', lib.BILINEAR, True])
    assert np.array_equal(frames.download(), S[3])
