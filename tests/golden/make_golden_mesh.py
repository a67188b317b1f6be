"""Generate tests/golden/mesh.npz with Pillow alone: the contract of ta_frames_transform_mesh and of
terran_amd.image.mesh_frames, quad_frames, extent_frames, undistort_frames and terran_amd.vis.quad_chips.

    <case>_<filter>_<1: fillcolor None, 0: FILL>   Image.fromarray(src[frame]).transform((w, h), Image.MESH, mesh, filter,
                     fillcolor=fill) for every (frame, mesh) of the case; sources, meshes and cases are the formulas of
                     tests/mesh_model.py (not stored)
    api_*            whole-batch and mixed-size-list calls of the public functions: MESH, ImageOps.deform, QUAD, EXTENT
    undistort_*      Image.MESH with the mesh terran_amd.image.undistort_mesh returns (host only, numpy), the mesh beside it

The maker asserts that every source point is finite and below 2^31 (the conversion to int is undefined in Pillow's C
otherwise).  Reads no reference.

    python tests/golden/make_golden_mesh.py
"""
import os
import sys

import numpy as np
import PIL
from PIL import Image, ImageOps

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import mesh_model as M           # noqa: E402  (the shared sources and cases)
from terran_amd import image                # noqa: E402  (undistort_mesh: host only)


def check_defined(mesh, ow, oh):
    for box, quad in mesh:
        cx0, cy0, cx1, cy1 = M.clamped(box, ow, oh)
        if cx1 > cx0 and cy1 > cy0:
            xs, ys = M.points(box, quad, ow, oh)
            assert np.isfinite(xs).all() and np.isfinite(ys).all() and max(np.abs(xs).max(), np.abs(ys).max()) < 2.0 ** 31 - 1


def warp(img, size, mesh, filt, fill):
    check_defined(mesh, *size)
    return np.asarray(Image.fromarray(img).transform(size, Image.MESH, mesh, resample=filt, fillcolor=fill))


def main():
    S = M.sources()
    out = {'pillow_version': np.array(PIL.__version__)}
    for name, (src, size, meshes, images) in M.cases().items():
        for filt in M.FILTERS:
            for nofill in (True, False):
                fill = None if nofill else M.FILL
                out['%s_%d_%d' % (name, filt, int(nofill))] = np.stack([warp(S[src][f], size, meshes[m], filt, fill) for f, m in images])

    frames = S[3]
    own = M.lattice(53, 37, 10, 53, 37, wobble=0.25, reach=1.1)
    out['api_mesh_batch'] = np.stack([warp(f, (53, 37), own, M.BILINEAR, None) for f in frames])
    per = [M.lattice(40, 30, 9 + k, 53, 37, wobble=0.1 * (k + 1), reach=1.05) for k in range(3)]
    out['api_mesh_per'] = np.stack([warp(f, (40, 30), m, M.BICUBIC, M.FILL) for f, m in zip(frames, per)])
    mixed = [S[3][0], S[4][0], S[0][0]]
    one = M.lattice(40, 30, 13, 45, 30, reach=1.1)
    out['api_mesh_mixed'] = np.stack([warp(f, (40, 30), one, M.NEAREST, M.FILL) for f in mixed])
    d = M.Deformer()
    out['api_deform_batch'] = np.stack([np.asarray(ImageOps.deform(Image.fromarray(f), d, M.BILINEAR)) for f in frames])
    out['api_deform_mixed'] = np.stack([warp(f, (50, 35), d.getmesh(Image.fromarray(f)), M.BILINEAR, None) for f in (S[4][0], S[3][1])])
    out['api_quad_per'] = np.stack([np.asarray(Image.fromarray(f).transform((30, 20), Image.QUAD, q, M.BILINEAR))
                                    for f, q in zip(frames, M.API_QUADS)])
    out['api_quad_one'] = np.stack([np.asarray(Image.fromarray(f).transform((30, 20), Image.QUAD, M.API_QUADS[2], M.NEAREST, fillcolor=M.FILL))
                                    for f in frames])
    for filt in M.FILTERS:
        out['api_extent_per_%d' % filt] = np.stack([np.asarray(Image.fromarray(f).transform((30, 20), Image.EXTENT, e, filt, fillcolor=M.FILL))
                                                    for f, e in zip(frames, M.API_EXTENTS)])
    out['api_extent_one'] = np.stack([np.asarray(Image.fromarray(f).transform((30, 20), Image.EXTENT, M.API_EXTENTS[0], M.BICUBIC)) for f in mixed])
    out['api_chips'] = np.stack([np.asarray(Image.fromarray(frames[f]).transform((16, 12), Image.QUAD, q, M.BILINEAR))
                                 for f, qs in enumerate(M.CHIP_QUADS) for q in qs])

    for tag, kw, filt, fill in (('new', dict(grid=8, new_camera_matrix=M.NEW_CAMERA), M.BILINEAR, None), ('own', dict(), M.NEAREST, M.FILL),
                                ('cubic', dict(grid=5), M.BICUBIC, None)):
        mesh = image.undistort_mesh((53, 37), M.CAMERA, M.DIST, **kw)
        out['undistort_%s_mesh' % tag] = np.array([tuple(b) + tuple(q) for b, q in mesh], np.float64)
        out['undistort_%s' % tag] = np.stack([warp(f, (53, 37), mesh, filt, fill) for f in frames])
    path = os.path.join(HERE, 'mesh.npz')
    np.savez_compressed(path, **out)
    print('%s: %d arrays, %d bytes, Pillow %s' % (path, len(out), os.path.getsize(path), PIL.__version__))


if __name__ == '__main__':
    main()
