"""No GPU: the numpy restatement of ta_frames_transform_mesh (tests/mesh_model.py) against the recorded Pillow golden
(tests/golden/mesh.npz) and, where Pillow is installed, against Pillow itself; the host plan (ta_mesh_plan: coefficients,
clamped boxes, tile lists) against the model; image.undistort_mesh against a restatement of its formula; image.extent_data;
the argument checks of the Python layer."""
import os

import numpy as np
import pytest

from terran_amd import image, lib, vis
from tests import mesh_model as M
from tests import transform_model as T

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'mesh.npz')


@pytest.fixture(scope='module')
def golden():
    return M.golden(GOLDEN)


def _cells(mesh):
    return image.pack_mesh(mesh)


def test_the_model_equals_the_golden(golden):
    z, S, C, want = golden
    assert len(want) == 6 * len(C) and len(C) >= 19
    for (name, filt, nofill), w in want.items():
        got = M.expected(S, C[name], filt, None if nofill else M.FILL)
        assert got.shape == w.shape and np.array_equal(got, w), (name, filt, nofill)
    # the two fill modes part where a later cell's points leave the source over an earlier cell, and only there
    for filt in M.FILTERS:
        assert (want['overlap', filt, True] != want['overlap', filt, False]).any()
        assert np.array_equal(want['quad', filt, True], want['quad', filt, False])
    # the public functions' cases, through the model
    fr = S[3]
    own = M.lattice(53, 37, 10, 53, 37, wobble=0.25, reach=1.1)
    assert np.array_equal(np.stack([M.mesh(f, (53, 37), own, M.BILINEAR) for f in fr]), z['api_mesh_batch'])
    d = M.Deformer()
    assert np.array_equal(np.stack([M.mesh(f, (53, 37), d.getmesh(image._MeshTarget(53, 37)), M.BILINEAR) for f in fr]), z['api_deform_batch'])
    assert np.array_equal(np.stack([M.quad(f, (30, 20), q, M.BILINEAR) for f, q in zip(fr, M.API_QUADS)]), z['api_quad_per'])
    assert np.array_equal(np.stack([M.quad(f, (30, 20), M.API_QUADS[2], M.NEAREST, M.FILL) for f in fr]), z['api_quad_one'])
    for filt in M.FILTERS:                              # EXTENT is the affine map of extent_data and nothing more
        got = np.stack([T.transform(f, (30, 20), T.AFFINE, image.extent_data((30, 20), e), filt, M.FILL) for f, e in zip(fr, M.API_EXTENTS)])
        assert np.array_equal(got, z['api_extent_per_%d' % filt]), filt


def test_the_model_equals_pillow_on_seeded_meshes():
    """300 seeded meshes of 1 .. 6 cells whose boxes overlap, leave gaps, start left of or above the output and reach past
    it, with quads around and beyond the source; the three filters, both fills, sources and outputs from 1 x 1."""
    Image = pytest.importorskip('PIL.Image')
    rng = np.random.default_rng(21)
    for k in range(300):
        h, w = (int(v) for v in rng.integers(1, 40, 2))
        ow, oh = (int(v) for v in rng.integers(1, 48, 2))
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        mesh = []
        for _ in range(int(rng.integers(1, 7))):
            x0, y0 = int(rng.integers(-8, ow)), int(rng.integers(-8, oh))
            box = (x0, y0, x0 + int(rng.integers(1, ow + 8)), y0 + int(rng.integers(1, oh + 8)))
            quad = rng.uniform(-0.3, 1.3, 8) * np.array([w, h] * 4)
            if k % 5 == 0:
                quad = np.round(quad)                   # points on pixel borders
            mesh.append((box, tuple(float(v) for v in quad)))
        filt = M.FILTERS[k % 3]
        fill = None if k % 2 else tuple(int(v) for v in rng.integers(0, 256, 3))
        want = np.asarray(Image.fromarray(img).transform((ow, oh), Image.MESH, mesh, resample=filt, fillcolor=fill))
        assert np.array_equal(M.mesh(img, (ow, oh), mesh, filt, fill), want), (k, (h, w), (ow, oh), filt, fill, mesh)
        if k % 10 == 0:
            q = mesh[0][1]
            want = np.asarray(Image.fromarray(img).transform((ow, oh), Image.QUAD, q, resample=filt, fillcolor=fill))
            assert np.array_equal(M.quad(img, (ow, oh), q, filt, fill), want), (k, 'quad')
            e = tuple(float(v) for v in rng.uniform(-3, 43, 4))
            want = np.asarray(Image.fromarray(img).transform((ow, oh), Image.EXTENT, e, resample=filt, fillcolor=fill))
            assert np.array_equal(T.transform(img, (ow, oh), T.AFFINE, image.extent_data((ow, oh), e), filt, fill), want), (k, 'extent')


def test_mesh_plan_equals_the_model():
    """ta_mesh_plan: the eight coefficients bit for bit, the clamped boxes, and per tile exactly the cells that touch it, in
    list order -- for every mesh of the golden's cases, a 16-pixel lattice over several tiles, and cells in reverse order."""
    meshes = [(m, size) for _, size, ms, _ in M.cases().values() for m in ms]
    big = M.lattice(200, 50, 16, 70, 45, reach=1.2)
    meshes += [(big, (200, 50)), (big[::-1], (200, 50)), (big + big[5:40], (131, 47))]
    touched = 0
    for mesh, (ow, oh) in meshes:
        coefs, boxes, first, entries = lib.mesh_plan(_cells(mesh), oh, ow)
        assert coefs.shape == (len(mesh), 8) and boxes.shape == (len(mesh), 4)
        for k, (box, quad) in enumerate(mesh):
            assert coefs[k].tolist() == list(M.coefficients(box, quad)), (k, box)
            assert boxes[k].tolist() == list(M.clamped(box, ow, oh)), (k, box)
        lists = M.tile_lists(mesh, ow, oh)
        assert len(first) == len(lists) + 1 and first[0] == 0 and first[-1] == len(entries)
        for t, want in enumerate(lists):
            assert entries[first[t]:first[t + 1]].tolist() == want, (t, (ow, oh))
        touched += len(entries)
    assert touched > 2 * len(big)                       # the two big lattices alone: every cell in at least one tile
    # an empty mesh, and a cell over every tile of the largest output
    coefs, boxes, first, entries = lib.mesh_plan(np.zeros(0, lib.MESH_CELL_DT), 16, 64)
    assert len(coefs) == 0 and first.tolist() == [0, 0] and len(entries) == 0
    whole = [((-5, -5, 20000, 20000), (0.0,) * 8)]
    _, boxes, first, entries = lib.mesh_plan(_cells(whole), 16384, 16384)
    assert boxes[0].tolist() == [0, 0, 16384, 16384] and len(entries) == 256 * 1024 and np.array_equal(first, np.arange(256 * 1024 + 1))


def test_mesh_plan_refuses_what_the_call_refuses():
    good = ((0, 0, 8, 8), (0.0, 0.0, 0.0, 8.0, 8.0, 8.0, 8.0, 0.0))

    def cells(*rows):
        a = np.zeros(len(rows), lib.MESH_CELL_DT)
        for k, (box, quad) in enumerate(rows):
            a[k] = tuple(box) + (quad,)
        return a
    lib.mesh_plan(cells(good), 8, 8)
    lim = lib.MESH_COORD_LIMIT
    for bad in [((3, 0, 3, 8), good[1]), ((5, 0, 3, 8), good[1]), ((0, 4, 8, 4), good[1]), ((0, 9, 8, 2), good[1]),
                ((0, 0, lim + 1, 8), good[1]), ((-lim - 1, 0, 8, 8), good[1]), ((0, -lim - 1, 8, 8), good[1]),
                (good[0], (np.nan,) + good[1][1:]), (good[0], good[1][:7] + (np.inf,)), (good[0], good[1][:3] + (-np.inf,) + good[1][4:])]:
        with pytest.raises(lib.TerranAmdError) as e:
            lib.mesh_plan(cells(good, bad), 8, 8)
        assert e.value.code == lib.E_INVALID, bad
    lib.mesh_plan(cells(((-lim, -lim, lim, lim), good[1])), 8, 8)                       # the limit itself is valid
    for oh, ow in [(0, 8), (8, 0), (-1, 8), (16385, 8), (8, 16385)]:
        with pytest.raises(lib.TerranAmdError) as e:
            lib.mesh_plan(cells(good), oh, ow)
        assert e.value.code == lib.E_INVALID, (oh, ow)
    many = np.zeros(lib.MESH_MAX_CELLS + 1, lib.MESH_CELL_DT)
    many['x1'] = many['y1'] = 1
    with pytest.raises(lib.TerranAmdError) as e:
        lib.mesh_plan(many, 8, 8)
    assert e.value.code == lib.E_INVALID
    lib.mesh_plan(many[:-1], 8, 8)
    # 65 cells over all 2^18 tiles of a 16384 x 16384 output: more than 2^24 entries; 64 are exactly the limit
    whole = cells(*[((0, 0, 16384, 16384), good[1])] * 65)
    with pytest.raises(lib.TerranAmdError) as e:
        lib.mesh_plan(whole, 16384, 16384)
    assert e.value.code == lib.E_INVALID
    assert len(lib.mesh_plan(whole[:64], 16384, 16384)[3]) == lib.MESH_MAX_ENTRIES


def test_undistort_mesh_is_the_formula_on_a_lattice():
    for size, grid, new in (((53, 37), 16, None), ((53, 37), 8, M.NEW_CAMERA), ((64, 32), 16, None), ((5, 3), 1, M.NEW_CAMERA), ((7, 9), 100, None)):
        w, h = size
        mesh = image.undistort_mesh(size, M.CAMERA, M.DIST, grid, new)
        xv, yv = list(range(0, w, grid)) + [w], list(range(0, h, grid)) + [h]
        assert len(mesh) == (len(xv) - 1) * (len(yv) - 1)
        k = 0
        for j in range(len(yv) - 1):                    # row by row; the last row and column narrower
            for i in range(len(xv) - 1):
                box, quad = mesh[k]
                k += 1
                assert box == (xv[i], yv[j], xv[i + 1], yv[j + 1]) and all(type(v) is int for v in box)
                corners = [(xv[i], yv[j]), (xv[i], yv[j + 1]), (xv[i + 1], yv[j + 1]), (xv[i + 1], yv[j])]          # nw, sw, se, ne
                want = [float(c) for u, v in corners for c in M.undistort_points(u, v, M.CAMERA, M.DIST, new)]
                assert list(quad) == want and all(type(v) is float for v in quad), (size, grid, box)
        assert image.undistort_mesh(size, M.CAMERA, M.DIST[:4], grid, new) == image.undistort_mesh(size, M.CAMERA, M.DIST[:4] + (0.0,), grid, new)
    # the distortion bends: the corner of a barrel-distorted image comes from inside the source
    mesh = image.undistort_mesh((53, 37), M.CAMERA, M.DIST)
    assert mesh[0][1][0] > 1.0 and mesh[0][1][1] > 1.0
    # without distortion and with equal matrices every vertex maps to itself, up to the rounding of (u - c) / f * f + c in
    # float64: coordinates below 2^7 and five roundings of at most 2^-46 each, far inside 1e-9
    for new in (None, M.CAMERA):
        for box, quad in image.undistort_mesh((53, 37), M.CAMERA, (0, 0, 0, 0), 16, new):
            x0, y0, x1, y1 = box
            assert np.allclose(quad, (x0, y0, x0, y1, x1, y1, x1, y0), rtol=0, atol=1e-9), box
    # skew in both matrices cancels as well
    skew = ((60.0, 1.5, 26.0), (0.0, 58.0, 18.5), (0.0, 0.0, 1.0))
    for box, quad in image.undistort_mesh((53, 37), skew, (0, 0, 0, 0, 0), 16):
        x0, y0, x1, y1 = box
        assert np.allclose(quad, (x0, y0, x0, y1, x1, y1, x1, y0), rtol=0, atol=1e-9), box


def test_pillow_accepts_the_undistort_mesh(golden):
    Image = pytest.importorskip('PIL.Image')
    z, S, _, _ = golden
    mesh = image.undistort_mesh((53, 37), M.CAMERA, M.DIST, grid=8, new_camera_matrix=M.NEW_CAMERA)
    assert np.array_equal(np.array([tuple(b) + tuple(q) for b, q in mesh]), z['undistort_new_mesh'])
    got = np.asarray(Image.fromarray(S[3][0]).transform((53, 37), Image.MESH, mesh, resample=Image.BILINEAR))
    assert np.array_equal(got, z['undistort_new'][0]) and np.array_equal(M.mesh(S[3][0], (53, 37), mesh, M.BILINEAR), got)


def test_the_recorded_undistort_meshes_are_undistort_mesh(golden):
    z = golden[0]
    for tag, kw in (('new', dict(grid=8, new_camera_matrix=M.NEW_CAMERA)), ('own', dict()), ('cubic', dict(grid=5))):
        mesh = image.undistort_mesh((53, 37), M.CAMERA, M.DIST, **kw)
        assert np.array_equal(np.array([tuple(b) + tuple(q) for b, q in mesh]), z['undistort_%s_mesh' % tag]), tag


def test_extent_data_and_what_extent_frames_hands_on(monkeypatch):
    assert image.extent_data((30, 20), (3.5, 2.25, 40.0, 30.0)) == ((40.0 - 3.5) / 30, 0, 3.5, 0, (30.0 - 2.25) / 20, 2.25)
    assert image.extent_data((8, 4), (0, 0, 8, 4)) == (1.0, 0, 0, 0, 1.0, 0)             # the identity
    assert image.extent_data((7, 3), (10, 5, 3, 6)) == (-1.0, 0, 10, 0, 1 / 3, 5)         # mirrored in x
    seen = []
    monkeypatch.setattr(image, 'transform_frames', lambda *a: seen.append(a) or 'out')
    fr = _fake_frames(3)
    assert image.extent_frames(fr, (30, 20), M.API_EXTENTS[0], 'bicubic', (1, 2, 3), 'ctx') == 'out'
    assert seen[-1] == (fr, (30, 20), lib.AFFINE, image.extent_data((30, 20), M.API_EXTENTS[0]), 'bicubic', (1, 2, 3), 'ctx')
    image.extent_frames(fr, (30, 20), M.API_EXTENTS)
    assert seen[-1][3] == [image.extent_data((30, 20), e) for e in M.API_EXTENTS] and seen[-1][4:] == ('nearest', None, None)


def test_pack_mesh_and_pack_quads():
    mesh = M.cases()['negative'][2][0]
    cells = image.pack_mesh(mesh)
    assert cells.dtype == lib.MESH_CELL_DT and lib.MESH_CELL_DT.itemsize == 80 and lib.MESH_IMAGE_DT.itemsize == 8
    assert [(int(c['x0']), int(c['y0']), int(c['x1']), int(c['y1'])) for c in cells] == [b for b, _ in mesh]
    assert [tuple(c['quad']) for c in cells] == [q for _, q in mesh]
    assert len(image.pack_mesh([])) == 0
    assert len(image.pack_mesh([((np.int32(0), 0, 4, 4), np.arange(8))])) == 1
    cells, images, index = vis.pack_quads(M.CHIP_QUADS, (16, 12))
    assert index.tolist() == [[0, 0], [0, 1], [2, 0]] and images['frame'].tolist() == [0, 0, 2] and images['mesh'].tolist() == [0, 1, 2]
    assert [tuple(c['quad']) for c in cells] == [q for qs in M.CHIP_QUADS for q in qs]
    assert {(int(c['x0']), int(c['y0']), int(c['x1']), int(c['y1'])) for c in cells} == {(0, 0, 16, 12)}
    cells, images, index = vis.pack_quads([[], []], (16, 12))
    assert len(cells) == 0 and len(images) == 0 and index.shape == (0, 2)
    assert vis.pack_quads([M.CHIP_QUADS[0][0]], (4, 4))[2].tolist() == [[0, 0]]           # one bare quad for a frame


def _fake_frames(n=2, h=30, w=40):
    """A lib.Frames that owns nothing: the argument checks run before anything touches the device."""
    f = lib.Frames.__new__(lib.Frames)
    f.ctx, f.h, f.shape = None, None, (n, h, w, 3)
    return f


class _NoMesh:
    def getmesh(self, image):
        return [((0, 0, 4), (0,) * 8)]


def test_the_python_layer_checks_its_arguments():
    fr = _fake_frames()
    q = (0, 0, 0, 30, 40, 30, 40, 0)
    cell = ((0, 0, 8, 8), q)
    cam = M.CAMERA
    bad_calls = [
        lambda: image.mesh_frames(None, [cell]),
        lambda: image.mesh_frames([], [cell]),
        lambda: image.mesh_frames(fr, None),
        lambda: image.mesh_frames(fr, 5),
        lambda: image.mesh_frames(fr, [cell], size=(0, 8)),
        lambda: image.mesh_frames(fr, [cell], size=(8, 16385)),
        lambda: image.mesh_frames(fr, [cell], size=8),
        lambda: image.mesh_frames([fr, _fake_frames(1, 20, 20)], [cell]),                  # sizes differ and none is given
        lambda: image.mesh_frames(fr, [cell], resample='lanczos'),
        lambda: image.mesh_frames(fr, [cell], resample=4),
        lambda: image.mesh_frames(fr, [cell], fillcolor=(1, 2)),
        lambda: image.mesh_frames(fr, [cell], fillcolor=(1, 2, 256)),
        lambda: image.mesh_frames(fr, [((0, 0, 8), q)]),                                   # a box of three
        lambda: image.mesh_frames(fr, [((0, 0, 8, 8), q[:7])]),                            # a quad of seven
        lambda: image.mesh_frames(fr, [((0, 0, 8.0, 8), q)]),                              # Pillow takes ints only
        lambda: image.mesh_frames(fr, [((0, 0, True, 8), q)]),
        lambda: image.mesh_frames(fr, [((4, 0, 4, 8), q)]),                                # Pillow would divide by zero
        lambda: image.mesh_frames(fr, [((0, 8, 8, 0), q)]),                                # ... or draw nothing
        lambda: image.mesh_frames(fr, [((0, 0, 2 ** 24 + 1, 8), q)]),
        lambda: image.mesh_frames(fr, [((0, -2 ** 24 - 1, 8, 8), q)]),
        lambda: image.mesh_frames(fr, [((0, 0, 8, 8), q[:7] + (np.nan,))]),
        lambda: image.mesh_frames(fr, [((0, 0, 8, 8), (np.inf,) + q[1:])]),
        lambda: image.mesh_frames(fr, [((0, 0, 8, 8), q[:7] + ('x',))]),
        lambda: image.mesh_frames(fr, [cell, 'cell']),
        lambda: image.mesh_frames(fr, [[cell], [cell], [cell]]),                           # 3 meshes for 2 frames
        lambda: image.mesh_frames(fr, [[cell], [((0, 0, 0, 8), q)]]),                      # the second frame's mesh is bad
        lambda: image.mesh_frames(fr, _NoMesh()),
        lambda: image.mesh_frames(_fake_frames(0), [cell]),                                # no images
        lambda: image.quad_frames(None, (8, 8), q),
        lambda: image.quad_frames(fr, (8, 0), q),
        lambda: image.quad_frames(fr, 8, q),
        lambda: image.quad_frames(fr, (8, 8), q[:6]),
        lambda: image.quad_frames(fr, (8, 8), [q] * 3),                                    # 3 quads for 2 frames
        lambda: image.quad_frames(fr, (8, 8), q[:7] + (np.nan,)),
        lambda: image.quad_frames(fr, (8, 8), 'quad'),
        lambda: image.quad_frames(fr, (8, 8), q, resample='box'),
        lambda: image.quad_frames(fr, (8, 8), q, fillcolor='red'),
        lambda: image.extent_frames(None, (8, 8), (0, 0, 8, 8)),
        lambda: image.extent_frames(fr, (8, 8), (0, 0, 8)),
        lambda: image.extent_frames(fr, (8, 8), [(0, 0, 8, 8)] * 3),
        lambda: image.extent_frames(fr, (8, 8), (0, 0, np.inf, 8)),
        lambda: image.extent_frames(fr, (8, 8), (0, 0, np.nan, 8)),
        lambda: image.extent_frames(fr, (0, 8), (0, 0, 8, 8)),
        lambda: image.extent_frames(fr, (8, 8), (0, 0, 8, 8), resample='hamming'),
        lambda: image.extent_frames(fr, (8, 8), (0, 0, 8, 8), fillcolor=(1, 2)),
        lambda: image.undistort_mesh((0, 8), cam, M.DIST),
        lambda: image.undistort_mesh(8, cam, M.DIST),
        lambda: image.undistort_mesh((8, 8), cam[:2], M.DIST),
        lambda: image.undistort_mesh((8, 8), ((0.0, 0, 4), (0, 8.0, 4), (0, 0, 1)), M.DIST),       # fx = 0
        lambda: image.undistort_mesh((8, 8), ((8.0, 0, np.nan), (0, 8.0, 4), (0, 0, 1)), M.DIST),
        lambda: image.undistort_mesh((8, 8), cam, M.DIST[:3]),
        lambda: image.undistort_mesh((8, 8), cam, M.DIST + (0.0,)),
        lambda: image.undistort_mesh((8, 8), cam, (0, 0, np.inf, 0)),
        lambda: image.undistort_mesh((8, 8), cam, M.DIST, grid=0),
        lambda: image.undistort_mesh((8, 8), cam, M.DIST, grid=2.5),
        lambda: image.undistort_mesh((8, 8), cam, M.DIST, new_camera_matrix=((1, 0, 0), (0, 0, 0), (0, 0, 1))),
        lambda: image.undistort_mesh((4096, 4096), cam, M.DIST, grid=1),                   # more cells than a call takes
        lambda: image.undistort_mesh((8, 8), cam, M.DIST, new_camera_matrix=((1e-300, 0, 0), (0, 1.0, 0), (0, 0, 1))),     # overflows
        lambda: image.undistort_frames(None, cam, M.DIST),
        lambda: image.undistort_frames([fr, _fake_frames(1, 20, 20)], cam, M.DIST),        # one camera, two sizes
        lambda: image.undistort_frames(fr, cam, M.DIST[:2]),
        lambda: image.undistort_frames(fr, cam, M.DIST, grid=-1),
        lambda: image.undistort_frames(fr, cam, M.DIST, resample='box'),
        lambda: image.undistort_frames(fr, cam, M.DIST, fillcolor=(1, 2)),
        lambda: vis.quad_chips(fr, [[q], [], []], (8, 8)),                                 # more lists than frames
        lambda: vis.quad_chips(fr, [[q[:7]]], (8, 8)),
        lambda: vis.quad_chips(fr, [[q[:7] + (np.nan,)]], (8, 8)),
        lambda: vis.quad_chips(fr, [[q]], (0, 8)),
        lambda: vis.quad_chips(fr, [[q]], (8, 8), resample='lanczos'),
        lambda: vis.quad_chips(fr, [['quad']], (8, 8)),
    ]
    for k, call in enumerate(bad_calls):
        with pytest.raises(ValueError):
            call()
            pytest.fail('call %d was accepted' % k)
    assert vis.quad_chips(fr, [[], []], (8, 8)) == (None, [])
    # transform_frames still refuses the methods that have functions of their own
    for method in ('quad', 'mesh', 'extent', 1, 3, 4):
        with pytest.raises(ValueError):
            image.transform_frames(fr, (8, 8), method, q)
