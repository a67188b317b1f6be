"""Tools: time the neighbourhood filters on a resident 32 x 1080 x 1920 batch.  Per case: device time (HIP events around
the library call: staging copy and kernels) and wall time of the public call; for the whole-frame cases the ratio of the
device time to the traffic floor, one read and one write of the batch at the 1.87 TB/s the histogram kernel reaches.  The
same work the way it has to be done without them, under "pillow": download the batch, the Pillow call per frame on 16
threads, upload it again (wall time of each leg and their sum; null when Pillow is not installed).  One JSON line.

    python tools/filter_bench.py [--frames 32] [--reps 20]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from terran_amd import image, lib, runtime, synth      # noqa: E402
from tone_bench import pillow_leg, timed               # noqa: E402

FLOOR_GBPS = 1870.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=32)
    ap.add_argument('--height', type=int, default=1080)
    ap.add_argument('--width', type=int, default=1920)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--pillow-reps', type=int, default=2)
    ap.add_argument('--warmup', type=int, default=2)
    a = ap.parse_args()
    ctx = runtime.get_context(0)
    n, h, w = a.frames, a.height, a.width
    rng = np.random.default_rng(5)
    scene = np.zeros((n, h, w, 3), np.uint8)
    scene[:] = synth.frames(1, 1, h, w)[0]
    scene ^= rng.integers(0, 16, scene.shape, dtype=np.uint8)              # grain
    floor_ms = 2 * scene.nbytes / (FLOOR_GBPS * 1e9) * 1e3
    out = {'metric': 'neighbourhood filters per batch', 'frames': n, 'height': h, 'width': w, 'reps': a.reps,
           'traffic_floor_ms': round(floor_ms, 4)}

    def pil():
        from PIL import Image, ImageEnhance, ImageFilter
        return Image, ImageEnhance, ImageFilter

    def in_place(fn):
        def per_frame(f, img):
            img[...] = np.asarray(fn(pil()[0].fromarray(img)))
        return per_frame

    whole = np.zeros(n, lib.FILTER_REGION_DT)
    whole['frame'], whole['x1'], whole['y1'] = np.arange(n), w, h
    size, scale, offset, kernel = image.FILTER_BUILTINS['smooth']
    cases = [('sharpen', image.filter_spec('sharpen'), lambda f: image.filter_frames(f, 'sharpen'), lambda im: im.filter(pil()[2].SHARPEN)),
             ('median_3', image.rank_spec(3, 4), lambda f: image.median_frames(f, 3), lambda im: im.filter(pil()[2].MedianFilter(3))),
             ('median_5', image.rank_spec(5, 12), lambda f: image.median_frames(f, 5), lambda im: im.filter(pil()[2].MedianFilter(5))),
             ('unsharp_2_150_3', image.unsharp_spec(2, 150, 3), lambda f: image.unsharp_frames(f), lambda im: im.filter(pil()[2].UnsharpMask(2, 150, 3))),
             ('sharpness_2.0', image.kernel_spec(size, kernel, scale, offset, factor=2.0), lambda f: image.sharpness_frames(f, 2.0),
              lambda im: pil()[1].Sharpness(im).enhance(2.0))]
    frames = ctx.upload(scene)
    for name, spec, call, fn in cases:
        r = timed(ctx, a, lambda: frames.filter(whole, spec), lambda: call(frames))
        r['device_over_floor'] = round(r['device_ms_min'] / floor_ms, 2)
        r['pillow'] = pillow_leg(ctx, frames, a, in_place(fn), upload=True)
        out[name] = r
        frames.free()
        frames = ctx.upload(scene)

    boxes = np.zeros(64, lib.FILTER_REGION_DT)
    boxes['frame'] = np.arange(64) % n
    boxes['x0'], boxes['y0'] = rng.integers(0, w - 200, 64), rng.integers(0, h - 200, 64)
    boxes['x1'], boxes['y1'] = boxes['x0'] + 200, boxes['y0'] + 200
    spec = image.filter_spec('sharpen')
    r = timed(ctx, a, lambda: frames.filter(boxes, spec), lambda: frames.filter(boxes, spec))
    per = [boxes[boxes['frame'] == f] for f in range(n)]

    def face_sharpen(f, img):
        im = pil()[0].fromarray(img)
        for q in per[f]:
            box = (int(q['x0']), int(q['y0']), int(q['x1']), int(q['y1']))
            im.paste(im.crop(box).filter(pil()[2].SHARPEN), box)
        img[...] = np.asarray(im)
    r['pillow'] = pillow_leg(ctx, frames, a, face_sharpen, upload=True)
    out['sharpen_64_boxes_200'] = r
    frames.free()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
