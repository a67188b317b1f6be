"""Tools: time the three uses of ta_frames_transform / ta_frames_transpose on a resident 32 x 1080 x 1920 batch, each against
the way it has to be done without them (download the batch, Pillow on 16 threads, and for the whole-frame legs upload the
result again):

    rotate_90  image.transpose_frames(frames, 'rotate_90') of every frame
    tilt       image.rotate_frames(frames, 5.0, 'bicubic') of every frame
    chips      vis.align_faces: two faces of about 200 x 200 per frame -> 112 x 112 bilinear landmark-aligned chips

Per leg: device time (HIP events around the library call), wall time of the public call, and under "pillow" the wall
time of each host leg and their sum (null when Pillow is not installed).  One JSON line.

    python tools/transform_bench.py [--frames 32] [--reps 30] [--side 200]
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from terran_amd import arcface, image, lib, runtime, synth, vis      # noqa: E402


def med(x):
    return round(float(np.median(x)), 4)


def timed(ctx, a, device_call, public_call):
    dev, wall = [], []
    for rep in range(a.warmup + a.reps):
        ctx.timer_start()
        r = device_call()
        d = ctx.timer_stop()
        if r is not None:
            r.free()
        t0 = time.perf_counter()
        r = public_call()
        t1 = time.perf_counter()
        if isinstance(r, lib.Frames):
            r.free()
        if rep >= a.warmup:
            dev.append(d)
            wall.append((t1 - t0) * 1e3)
    return {'device_ms': med(dev), 'device_ms_min': round(min(dev), 4), 'wall_ms': med(wall), 'wall_ms_min': round(min(wall), 4)}


def pillow_leg(ctx, frames, a, per_frame, upload):
    """download + per_frame(host frame, index) on 16 threads (+ upload of what it returned)."""
    try:
        import PIL
    except ImportError:
        return None
    down, work, up = [], [], []
    with ThreadPoolExecutor(16) as pool:
        for rep in range(a.warmup + a.pillow_reps):
            t0 = time.perf_counter()
            host = frames.download()
            t1 = time.perf_counter()
            made = list(pool.map(lambda f: per_frame(host[f], f), range(a.frames)))
            t2 = time.perf_counter()
            if upload:
                again = ctx.upload(np.stack(made))
                ctx.sync()
                again.free()
            t3 = time.perf_counter()
            if rep >= a.warmup:
                down.append((t1 - t0) * 1e3)
                work.append((t2 - t1) * 1e3)
                up.append((t3 - t2) * 1e3)
    total = [d + w + u for d, w, u in zip(down, work, up)]
    return {'version': PIL.__version__, 'threads': 16, 'download_ms': med(down), 'pillow_ms': med(work),
            'upload_ms': med(up) if upload else None, 'total_ms': med(total), 'total_ms_min': round(min(total), 4),
            'reps': a.pillow_reps}


def landmark_scene(seed, frames, height, width, side, per_frame=2):
    """`per_frame` faces of about side x side per frame: the embedder's template scaled, turned a little and placed inside."""
    rng = np.random.default_rng(seed)
    t = arcface._TEMPLATE.astype(np.float64) - 56.0
    out = []
    for _ in range(frames):
        faces = []
        for _ in range(per_frame):
            s, phi = side / 112.0 * rng.uniform(0.9, 1.1), rng.uniform(-0.3, 0.3)
            rot = np.array([[np.cos(phi), -np.sin(phi)], [np.sin(phi), np.cos(phi)]])
            centre = (rng.uniform(side, width - side), rng.uniform(side, height - side))
            faces.append({'landmarks': ((t @ rot.T) * s + centre).astype(np.float32)})
        out.append(faces)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=32)
    ap.add_argument('--height', type=int, default=1080)
    ap.add_argument('--width', type=int, default=1920)
    ap.add_argument('--side', type=float, default=200.0)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--pillow-reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=3)
    a = ap.parse_args()
    ctx = runtime.get_context(0)
    host = np.zeros((a.frames, a.height, a.width, 3), np.uint8)
    host[:] = synth.frames(1, 1, a.height, a.width)[0]
    frames = ctx.upload(host)
    out = {'metric': 'transform: rotate_90, tilt, aligned chips per batch', 'frames': a.frames, 'height': a.height, 'width': a.width,
           'reps': a.reps}
    try:
        from PIL import Image
    except ImportError:
        Image = None

    out['rotate_90'] = timed(ctx, a, lambda: frames.transpose(lib.ROTATE_90), lambda: image.transpose_frames(frames, 'rotate_90'))
    out['rotate_90']['pillow'] = pillow_leg(ctx, frames, a, lambda img, f: np.asarray(Image.fromarray(img).transpose(Image.ROTATE_90)), True)

    _, matrix, (w, h) = image.rotate_plan(a.width, a.height, 5.0)
    tilt = np.zeros(a.frames, lib.TRANSFORM_DT)
    tilt['frame'], tilt['a'][:, :6] = np.arange(a.frames), matrix
    out['tilt'] = timed(ctx, a, lambda: frames.transform(tilt, h, w, lib.BICUBIC), lambda: image.rotate_frames(frames, 5.0, 'bicubic'))
    out['tilt']['pillow'] = pillow_leg(ctx, frames, a, lambda img, f: np.asarray(Image.fromarray(img).rotate(5.0, Image.BICUBIC)), True)

    faces = landmark_scene(7, a.frames, a.height, a.width, a.side)
    regions, _ = vis.pack_align(faces)
    of_frame = [regions[regions['frame'] == f] for f in range(a.frames)]
    out['chips'] = timed(ctx, a, lambda: frames.transform(regions, 112, 112, lib.BILINEAR), lambda: vis.align_faces(frames, faces)[0])
    out['chips']['regions'] = len(regions)
    out['chips']['pillow'] = pillow_leg(ctx, frames, a, lambda img, f: [
        Image.fromarray(img).transform((112, 112), Image.AFFINE, tuple(q['a'][:6]), resample=Image.BILINEAR) for q in of_frame[f]], False)
    frames.free()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
