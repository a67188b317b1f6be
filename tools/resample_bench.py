"""Tools: time the three uses of ta_frames_resample / ta_frames_pixelate on a resident 32 x 1080 x 1920 batch, each against
the way it has to be done without them (download the batch, Pillow on 16 threads, and for pixelate upload it again):

    chips     vis.crop_faces: two faces of about 200 x 200 per frame -> 112 x 112 bicubic chips
    resize    image.resize_frames: every frame -> 1280 x 720 lanczos
    pixelate  vis.blur_faces(method='pixelate') of the same faces, both shapes

Per leg: device time (HIP events around the library call), wall time of the public call, and under "pillow" the wall
time of each host leg and their sum (null when Pillow is not installed).  One JSON line.

    python tools/resample_bench.py [--frames 32] [--reps 30] [--side 200]
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from terran_amd import image, lib, runtime, synth, vis      # noqa: E402
from tools.blur_bench import scene                          # noqa: E402


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
    """download + per_frame(host frame, index) on 16 threads (+ upload)."""
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
            list(pool.map(lambda f: per_frame(host[f], f), range(a.frames)))
            t2 = time.perf_counter()
            if upload:
                again = ctx.upload(host)
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
    out = {'metric': 'resample: chips, resize, pixelate per batch', 'frames': a.frames, 'height': a.height, 'width': a.width,
           'reps': a.reps}
    try:
        from PIL import Image, ImageDraw
    except ImportError:
        Image = None

    crops, _ = vis.pack_crops(faces, frames.shape)
    of_frame = [crops[crops['frame'] == f] for f in range(a.frames)]
    out['chips'] = timed(ctx, a, lambda: frames.resample(crops, 112, 112, lib.BICUBIC), lambda: vis.crop_faces(frames, faces)[0])
    out['chips']['regions'] = len(crops)
    out['chips']['pillow'] = pillow_leg(ctx, frames, a, lambda img, f: [
        Image.fromarray(img).resize((112, 112), Image.BICUBIC, box=tuple(float(q[k]) for k in ('x0', 'y0', 'x1', 'y1')))
        for q in of_frame[f]], False)

    whole = np.zeros(a.frames, lib.RESAMPLE_DT)
    whole['frame'], whole['x1'], whole['y1'] = np.arange(a.frames), a.width, a.height
    out['resize'] = timed(ctx, a, lambda: frames.resample(whole, 720, 1280, lib.LANCZOS),
                          lambda: image.resize_frames(frames, (1280, 720), 'lanczos'))
    out['resize']['pillow'] = pillow_leg(ctx, frames, a, lambda img, f: Image.fromarray(img).resize((1280, 720), Image.LANCZOS), False)

    def pillow_pixelate(img, regions, ellipse):
        im = Image.fromarray(img)
        for q in regions:
            box = tuple(int(q[k]) for k in ('x0', 'y0', 'x1', 'y1'))
            w, h, b = box[2] - box[0], box[3] - box[1], int(q['block'])
            region = im.crop(box).resize((max(1, w // b), max(1, h // b)), Image.BOX).resize((w, h), Image.NEAREST)
            if ellipse:
                mask = Image.new('L', region.size)
                ImageDraw.Draw(mask).ellipse([0, 0, w - 1, h - 1], fill=255)
                im.paste(region, box, mask)
            else:
                im.paste(region, box)
        img[...] = np.asarray(im)
    for shape in ('box', 'ellipse'):
        regions = vis.pack_pixelate(faces, frames.shape, shape=shape)
        per = [regions[regions['frame'] == f] for f in range(a.frames)]
        leg = timed(ctx, a, lambda: frames.pixelate(regions), lambda: vis.blur_faces(frames, faces, shape=shape, method='pixelate') and None)   # in place: nothing to free
        leg['regions'], leg['mean_block'] = len(regions), round(float(regions['block'].mean()), 2)
        leg['pillow'] = pillow_leg(ctx, frames, a, lambda img, f: pillow_pixelate(img, per[f], shape == 'ellipse'), True)
        out['pixelate_' + shape] = leg
    frames.free()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
