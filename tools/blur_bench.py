"""Tools: time terran_amd.vis.blur_faces on a resident 32 x 1080 x 1920 batch with 2 faces of about 200 x 200 per frame at
the default radius, for both shapes.  Per batch: host packing time (dicts -> regions), device time (HIP events around
ta_frames_blur: staging copy + both kernels) and wall time of the public call.  The same work the way it has to be done
without it, under "pillow": download the batch, crop / GaussianBlur / paste every face with Pillow on 16 threads, upload
it again (wall time of each leg and their sum; null when Pillow is not installed).  One JSON line.

    python tools/blur_bench.py [--frames 32] [--reps 30] [--side 200]
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from terran_amd import runtime, synth, vis      # noqa: E402


def scene(seed, n, h, w, side):
    rng = np.random.default_rng(seed)
    faces = []
    for i in range(n):
        b = []
        for j in range(2):
            s = rng.uniform(0.9 * side, 1.1 * side)
            x0, y0 = rng.uniform(0, w / 2 - 1.2 * s) + j * w / 2, rng.uniform(0, h - 1.2 * s)   # one per half: disjoint
            b.append({'bbox': np.array([x0, y0, x0 + s, y0 + 1.1 * s], np.float32), 'track': j + 1})
        faces.append(b)
    return faces


def pillow_frame(img, regions, ellipse):
    """The crop / filter / paste loop on one host frame, in place."""
    from PIL import Image, ImageDraw, ImageFilter
    im = Image.fromarray(img)
    for q in regions:
        box = (int(q['x0']), int(q['y0']), int(q['x1']), int(q['y1']))
        region = im.crop(box).filter(ImageFilter.GaussianBlur(float(q['radius'])))
        if ellipse:
            mask = Image.new('L', region.size)
            ImageDraw.Draw(mask).ellipse([0, 0, region.size[0] - 1, region.size[1] - 1], fill=255)
            im.paste(region, box, mask)
        else:
            im.paste(region, box)
    img[...] = np.asarray(im)


def pillow_leg(ctx, frames, regions, ellipse, a, med):
    try:
        import PIL
    except ImportError:
        return None
    per_frame = [regions[regions['frame'] == f] for f in range(a.frames)]
    down, blur, up = [], [], []
    with ThreadPoolExecutor(16) as pool:
        for rep in range(a.warmup + a.pillow_reps):
            t0 = time.perf_counter()
            host = frames.download()
            t1 = time.perf_counter()
            list(pool.map(lambda f: pillow_frame(host[f], per_frame[f], ellipse), range(a.frames)))
            t2 = time.perf_counter()
            again = ctx.upload(host)
            ctx.sync()
            t3 = time.perf_counter()
            again.free()
            if rep >= a.warmup:
                down.append((t1 - t0) * 1e3)
                blur.append((t2 - t1) * 1e3)
                up.append((t3 - t2) * 1e3)
    total = [d + b + u for d, b, u in zip(down, blur, up)]
    return {'version': PIL.__version__, 'threads': 16, 'download_ms': med(down), 'blur_ms': med(blur), 'upload_ms': med(up),
            'total_ms': med(total), 'total_ms_min': round(min(total), 4), 'reps': a.pillow_reps}


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
    faces = scene(7, a.frames, a.height, a.width, a.side)
    med = lambda x: round(float(np.median(x)), 4)      # noqa: E731
    out = {'metric': 'vis blur_faces per batch', 'frames': a.frames, 'height': a.height, 'width': a.width, 'reps': a.reps}
    for shape in ('box', 'ellipse'):
        regions = vis.pack_blur(faces, frames.shape, shape=shape)
        pack_ms, dev_ms, wall_ms = [], [], []
        for rep in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            q = vis.pack_blur(faces, frames.shape, shape=shape)
            t1 = time.perf_counter()
            ctx.timer_start()
            frames.blur(q)
            d = ctx.timer_stop()
            w0 = time.perf_counter()
            vis.blur_faces(frames, faces, shape=shape)   # the public call, packing included
            w1 = time.perf_counter()
            if rep >= a.warmup:
                pack_ms.append((t1 - t0) * 1e3)
                dev_ms.append(d)
                wall_ms.append((w1 - w0) * 1e3)
        out[shape] = {'regions': len(regions), 'region_pixels': int(((regions['x1'] - regions['x0']) * (regions['y1'] - regions['y0'])).sum()),
                      'mean_radius': round(float(regions['radius'].mean()), 3), 'host_pack_ms': med(pack_ms),
                      'device_ms': med(dev_ms), 'device_ms_min': round(min(dev_ms), 4), 'wall_ms': med(wall_ms),
                      'wall_ms_min': round(min(wall_ms), 4), 'pillow': pillow_leg(ctx, frames, regions, shape == 'ellipse', a, med)}
    frames.free()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
