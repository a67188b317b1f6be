"""Tools: time the colour operations on a resident 32 x 1080 x 1920 batch.  Per case: device time (HIP events around the
library call: staging copy and kernels) and wall time of the public call, the achieved GB/s against the bytes a whole-batch
case must move (the frames read and written) and its ratio to the yardstick, `point_frames` on the same batch: one read
and one write of the batch through a 768-byte table.  Every timed call starts from the same pixels (the batch is restored
from a resident copy outside the timers: a conversion applied to its own output over and over would soon be timing flat
frames, whose table reads all hit one node).  The same work the way it has to be done without them, under
"pillow": download the batch, the Pillow call per frame on 16 threads, upload it again (wall time of each leg and their
sum; null when Pillow is not installed).  One JSON line.

    python tools/color_bench.py [--frames 32] [--reps 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from terran_amd import image, lib, runtime, synth, vis      # noqa: E402
from tone_bench import pillow_leg                           # noqa: E402

SEPIA = (0.393, 0.769, 0.189, 0.0, 0.349, 0.686, 0.168, 0.0, 0.272, 0.534, 0.131, 0.0)


def grade(size):
    """A mild grade as a size^3 table: lifted shadows, a warm tint, values a little outside 0 .. 1."""
    b, g, r = np.meshgrid(*(np.arange(size) / (size - 1.0),) * 3, indexing='ij')
    return np.stack([1.08 * r + 0.02 - 0.04 * b, 0.03 + 0.95 * g + 0.02 * r * b, 0.9 * b * b + 0.08 * g - 0.01], -1).astype(np.float32).reshape(-1)


def timed(ctx, a, frames, pristine, device_call, public_call):
    dev, wall = [], []
    for rep in range(a.warmup + a.reps):
        image.paste_frames(frames, pristine)
        ctx.timer_start()
        device_call()
        d = ctx.timer_stop()
        image.paste_frames(frames, pristine)
        ctx.sync()
        t0 = time.perf_counter()
        public_call()
        t1 = time.perf_counter()
        if rep >= a.warmup:
            dev.append(d)
            wall.append((t1 - t0) * 1e3)
    med = lambda x: round(float(np.median(x)), 4)      # noqa: E731
    return {'device_ms': med(dev), 'device_ms_min': round(min(dev), 4), 'wall_ms': med(wall), 'wall_ms_min': round(min(wall), 4)}


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
    scene[:] = synth.frames(1, 1, h, w)[0]
    scene ^= rng.integers(0, 8, scene.shape, dtype=np.uint8)             # sensor noise: neighbours read different nodes
    batch_bytes = n * h * w * 3
    out = {'metric': 'colour operations per batch', 'frames': n, 'height': h, 'width': w, 'reps': a.reps}

    def pil():
        from PIL import Image, ImageFilter
        return Image, ImageFilter

    def in_place(fn):
        def per_frame(f, img):
            img[...] = np.asarray(fn(pil()[0].fromarray(img)))
        return per_frame

    whole = np.zeros(n, lib.COLOR_REGION_DT)
    whole['frame'], whole['x1'], whole['y1'] = np.arange(n), w, h
    frames, pristine = ctx.upload(scene), ctx.upload(scene)
    ident = np.zeros(n, lib.POINT_DT)
    ident['frame'], ident['x1'], ident['y1'] = np.arange(n), w, h
    table = np.tile(image.brightness_lut(1.1), 3)[None]
    r = timed(ctx, a, frames, pristine, lambda: frames.point(ident, table), lambda: image.point_frames(frames, table[0]))
    r['kernel_GBps'] = round(2 * batch_bytes / (r['device_ms_min'] * 1e-3) / 1e9, 1)
    out['point_whole_frames'] = yard = r

    luts = {s: grade(s) for s in (17, 33)}
    as_rgb = lambda im: pil()[0].frombytes('RGB', im.size, im.tobytes())      # noqa: E731
    cases = [('matrix_frames', SEPIA, lambda: image.matrix_frames(frames, SEPIA), lambda im: im.convert('RGB', SEPIA)),
             ('convert_frames_YCbCr', 'ycbcr', lambda: image.convert_frames(frames, 'YCbCr'), lambda im: as_rgb(im.convert('YCbCr'))),
             ('convert_frames_HSV', 'hsv', lambda: image.convert_frames(frames, 'HSV'), lambda im: as_rgb(im.convert('HSV')))]
    for s in (17, 33):
        flt = []

        def with_lut(im, s=s, flt=flt):
            if not flt:
                flt.append(pil()[1].Color3DLUT(s, luts[s].tolist()))
            return im.filter(flt[0])
        cases.append(('color_lut_frames_%d' % s, (s, luts[s]), lambda s=s: image.color_lut_frames(frames, (s, luts[s])), with_lut))
    for name, op, call, fn in cases:
        rec, tab = image.color_spec(op)
        r = timed(ctx, a, frames, pristine, lambda: frames.color(whole, rec, tab), call)
        r['kernel_GBps'] = round(2 * batch_bytes / (r['device_ms_min'] * 1e-3) / 1e9, 1)
        r['device_over_point'] = round(r['device_ms'] / yard['device_ms'], 2)
        image.paste_frames(frames, pristine)
        r['pillow'] = pillow_leg(ctx, frames, a, in_place(fn), upload=True)
        out[name] = r

    image.paste_frames(frames, pristine)
    which = np.arange(64) % n
    x0, y0 = rng.integers(0, w - 200, 64), rng.integers(0, h - 200, 64)
    faces = [[{'bbox': (x0[k], y0[k], x0[k] + 200, y0[k] + 200)} for k in range(64) if which[k] == f] for f in range(n)]
    regions = vis.pack_color(faces, frames.shape)
    rec, tab = image.color_spec(SEPIA)
    r = timed(ctx, a, frames, pristine, lambda: frames.color(regions, rec, tab), lambda: vis.color_faces(frames, faces, SEPIA))

    def face_matrix(f, img):
        im = pil()[0].fromarray(img)
        for face in faces[f]:
            box = tuple(int(v) for v in face['bbox'])
            im.paste(im.crop(box).convert('RGB', SEPIA), box)
        img[...] = np.asarray(im)
    r['pillow'] = pillow_leg(ctx, frames, a, face_matrix, upload=True)
    out['color_faces_64_boxes_200'] = r
    frames.free()
    pristine.free()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
