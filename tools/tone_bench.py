"""Tools: time the pixel-value operations on a resident 32 x 1080 x 1920 batch.  Per case: device time (HIP events around
the library call: staging copy, kernels, for the histogram the copy of the counts back) and wall time of the public call;
for the two kernels that stream whole frames the achieved GB/s against the bytes they must move (histogram: the frames
once; point: the frames read and written).  The same work the way it has to be done without them, under "pillow":
download the batch, the Pillow call per frame on 16 threads and, for the in-place cases, upload it again (wall time of
each leg and their sum; null when Pillow is not installed).  One JSON line.

    python tools/tone_bench.py [--frames 32] [--reps 20]
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from terran_amd import image, lib, runtime, synth      # noqa: E402


def timed(ctx, a, device_call, public_call):
    dev, wall = [], []
    for rep in range(a.warmup + a.reps):
        ctx.timer_start()
        device_call()
        d = ctx.timer_stop()
        t0 = time.perf_counter()
        public_call()
        t1 = time.perf_counter()
        if rep >= a.warmup:
            dev.append(d)
            wall.append((t1 - t0) * 1e3)
    med = lambda x: round(float(np.median(x)), 4)      # noqa: E731
    return {'device_ms': med(dev), 'device_ms_min': round(min(dev), 4), 'wall_ms': med(wall), 'wall_ms_min': round(min(wall), 4)}


def pillow_leg(ctx, frames, a, per_frame, upload):
    """per_frame(host frame) does the Pillow work (in place where it changes pixels)."""
    try:
        import PIL
    except ImportError:
        return None
    down, work, up = [], [], []
    with ThreadPoolExecutor(16) as pool:
        for rep in range(1 + a.pillow_reps):
            t0 = time.perf_counter()
            host = frames.download()
            t1 = time.perf_counter()
            list(pool.map(lambda f: per_frame(f, host[f]), range(len(host))))
            t2 = time.perf_counter()
            if upload:
                again = ctx.upload(host)
                ctx.sync()
                again.free()
            t3 = time.perf_counter()
            if rep:
                down.append((t1 - t0) * 1e3)
                work.append((t2 - t1) * 1e3)
                up.append((t3 - t2) * 1e3)
    med = lambda x: round(float(np.median(x)), 4)      # noqa: E731
    total = [d + w + u for d, w, u in zip(down, work, up)]
    return {'version': PIL.__version__, 'threads': 16, 'download_ms': med(down), 'pillow_ms': med(work),
            'upload_ms': med(up) if upload else None, 'total_ms': med(total), 'total_ms_min': round(min(total), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=32)
    ap.add_argument('--height', type=int, default=1080)
    ap.add_argument('--width', type=int, default=1920)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--pillow-reps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=3)
    a = ap.parse_args()
    ctx = runtime.get_context(0)
    n, h, w = a.frames, a.height, a.width
    rng = np.random.default_rng(5)
    scene = np.zeros((n, h, w, 3), np.uint8)
    scene[:] = (40 + synth.frames(1, 1, h, w)[0].astype(np.int32) * 120 // 255).astype(np.uint8)     # under-exposed video
    sources = {'noise': rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8), 'flat': np.full((n, h, w, 3), 117, np.uint8)}
    batch_bytes = n * h * w * 3
    out = {'metric': 'pixel-value operations per batch', 'frames': n, 'height': h, 'width': w, 'reps': a.reps}

    def pil():
        from PIL import Image, ImageEnhance, ImageOps
        return Image, ImageEnhance, ImageOps

    whole = np.zeros(n, lib.HIST_DT)
    whole['frame'], whole['x1'], whole['y1'] = np.arange(n), w, h
    for name, host in sources.items():
        frames = ctx.upload(host)
        r = timed(ctx, a, lambda: frames.histogram(whole), lambda: image.histogram_frames(frames))
        r['kernel_GBps'] = round(batch_bytes / (r['device_ms_min'] * 1e-3) / 1e9, 1)
        r['pillow'] = pillow_leg(ctx, frames, a, lambda f, img: pil()[0].fromarray(img).histogram(), upload=False)
        out['histogram_rgb_' + name] = r
        frames.free()
    out['histogram_flat_over_noise'] = round(out['histogram_rgb_flat']['device_ms'] / out['histogram_rgb_noise']['device_ms'], 2)

    frames = ctx.upload(scene)
    boxes = np.zeros(64, lib.HIST_DT)
    boxes['frame'] = np.arange(64) % n
    boxes['x0'], boxes['y0'] = rng.integers(0, w - 200, 64), rng.integers(0, h - 200, 64)
    boxes['x1'], boxes['y1'] = boxes['x0'] + 200, boxes['y0'] + 200
    r = timed(ctx, a, lambda: frames.histogram(boxes), lambda: frames.histogram(boxes, lib.HIST_L))
    per = [boxes[boxes['frame'] == f] for f in range(n)]

    def face_hists(f, img):
        im = pil()[0].fromarray(img)
        return [im.crop((int(q['x0']), int(q['y0']), int(q['x1']), int(q['y1']))).histogram() for q in per[f]]
    r['pillow'] = pillow_leg(ctx, frames, a, face_hists, upload=False)
    out['histogram_64_boxes_200'] = r

    ident = np.zeros(n, lib.POINT_DT)
    ident['frame'], ident['x1'], ident['y1'] = np.arange(n), w, h
    table = np.tile(image.brightness_lut(1.1), 3)[None]
    r = timed(ctx, a, lambda: frames.point(ident, table), lambda: image.brightness_frames(frames, 1.0))
    r['kernel_GBps'] = round(2 * batch_bytes / (r['device_ms_min'] * 1e-3) / 1e9, 1)
    out['point_whole_frames'] = r

    def in_place(fn):
        def per_frame(f, img):
            img[...] = np.asarray(fn(pil()[0].fromarray(img)))
        return per_frame
    cases = [('equalize_frames', lambda: image.equalize_frames(frames), lambda im: pil()[2].equalize(im)),
             ('contrast_frames_1.3', lambda: image.contrast_frames(frames, 1.3), lambda im: pil()[1].Contrast(im).enhance(1.3)),
             ('color_frames_0.0', lambda: image.color_frames(frames, 0.0), lambda im: pil()[1].Color(im).enhance(0.0))]
    for name, call, fn in cases:
        frames.free()
        frames = ctx.upload(scene)
        r = timed(ctx, a, call, call)                    # end to end: histogram, host tables, point
        r['pillow'] = pillow_leg(ctx, frames, a, in_place(fn), upload=True)
        out[name] = r
    frames.free()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
