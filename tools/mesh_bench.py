"""Tools: time image.undistort_frames (ta_frames_transform_mesh) on a resident 32 x 1080 x 1920 batch with a 16-pixel lattice
(8 160 cells), for each of the three filters, against two yardsticks measured in the same run:

    affine   image.transform_frames with an affine map of the same filter on the same batch: the same taps and the same
             packed stores with ONE map in place of the lattice's cells (a small rotation, so that NEAREST takes a per-pixel
             route and not the table look-up of a pure scale)
    pillow   download the batch, Image.transform(size, MESH, the same mesh, the same filter) on 16 threads, upload the result

Per filter: device time (HIP events around the library call) and wall time of the public call for both GPU legs, their
ratio mesh / affine, and under "pillow" the wall time of each host leg and their sum (null when Pillow is not installed).
One JSON line.

    python tools/mesh_bench.py [--frames 32] [--reps 30] [--grid 16]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from terran_amd import image, lib, runtime, synth      # noqa: E402
from tools.transform_bench import pillow_leg, timed    # noqa: E402

FILTERS = (('nearest', lib.NEAREST), ('bilinear', lib.BILINEAR), ('bicubic', lib.BICUBIC))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=32)
    ap.add_argument('--height', type=int, default=1080)
    ap.add_argument('--width', type=int, default=1920)
    ap.add_argument('--grid', type=int, default=16)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--pillow-reps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=3)
    a = ap.parse_args()
    ctx = runtime.get_context(0)
    host = np.zeros((a.frames, a.height, a.width, 3), np.uint8)
    host[:] = synth.frames(1, 1, a.height, a.width)[0]
    frames = ctx.upload(host)
    del host
    size = (a.width, a.height)
    # a wide-angle lens: strong barrel distortion, the principal point a little off the centre
    f = 0.6 * a.width
    camera = ((f, 0.0, a.width / 2 + 7.3), (0.0, f, a.height / 2 - 4.1), (0.0, 0.0, 1.0))
    dist = (-0.30, 0.10, 0.001, -0.0015, -0.015)
    mesh = image.undistort_mesh(size, camera, dist, a.grid)
    cells = image.pack_mesh(mesh)
    first = np.array([0, len(cells)], np.int32)
    images = np.zeros(a.frames, lib.MESH_IMAGE_DT)
    images['frame'] = np.arange(a.frames)
    _, matrix, _ = image.rotate_plan(a.width, a.height, 2.0)
    affine = np.zeros(a.frames, lib.TRANSFORM_DT)
    affine['frame'], affine['a'][:, :6] = np.arange(a.frames), matrix
    out = {'metric': 'mesh: undistort_frames per batch against an affine transform_frames and against Pillow MESH', 'frames': a.frames,
           'height': a.height, 'width': a.width, 'grid': a.grid, 'cells': len(cells), 'reps': a.reps}
    try:
        from PIL import Image
    except ImportError:
        Image = None
    for name, code in FILTERS:
        leg = {'mesh': timed(ctx, a, lambda: frames.transform_mesh(cells, first, images, a.height, a.width, code),
                             lambda: image.undistort_frames(frames, camera, dist, a.grid, name)),
               'affine': timed(ctx, a, lambda: frames.transform(affine, a.height, a.width, code),
                               lambda: image.transform_frames(frames, size, 'affine', matrix, name))}
        leg['device_ratio'] = round(leg['mesh']['device_ms'] / leg['affine']['device_ms'], 3)
        leg['pillow'] = pillow_leg(ctx, frames, a, lambda img, k: np.asarray(Image.fromarray(img).transform(size, Image.MESH, mesh, resample=code)),
                                   True)
        out[name] = leg
    frames.free()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
