"""Tools: time the silhouette calls on a resident batch.  One JSON line, one leg per crowd:

  few    `--frames` (32) frames of 1080 x 1920 with 4 people of about 300 px each
  many   the same frames with 64 people of about 80 px

Per leg, medians over `--reps` after warm-ups: the device time (HIP events round the library call: staging copy and kernels) of
ta_poses_paint as `paint_poses` calls it (alpha 128, clear = 0) and as `pose_masks` calls it (clear = 1, into a batch allocated
once outside the timing); device and wall time of the whole `blur_poses` call (copy, blur of the boxes, matte, composite); and IN
THE SAME RUN `point_frames` on the same batch, the project's yardstick for one read and one write of it: every figure also as a
multiple of that.  The share of the batch's 64 x 16 tiles a person's box touches is reported beside them.  The host's way to the
same pixels -- tests/silhouette_model.paint per frame on 16 threads, download and upload included -- on `--model-frames` frames,
scaled to all frames and labelled so.

    python tools/silhouette_bench.py [--frames 32] [--reps 10] [--model-frames 4]
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

os.environ.setdefault('OMP_NUM_THREADS', '16')

import numpy as np      # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from terran_amd import image, lib, runtime, vis      # noqa: E402


def med(x):
    return round(float(np.median(x)), 4)


def timed(ctx, a, call):
    dev, wall = [], []
    for rep in range(a.warmup + a.reps):
        ctx.timer_start()
        call()
        d = ctx.timer_stop()
        t0 = time.perf_counter()
        call()
        ctx.sync()
        t1 = time.perf_counter()
        if rep >= a.warmup:
            dev.append(d)
            wall.append((t1 - t0) * 1e3)
    return {'device_ms': med(dev), 'device_ms_min': round(min(dev), 4), 'wall_ms': med(wall)}


def crowd(rng, n_frames, per_frame, size, h, w):
    from tests import silhouette_model as sm
    return [[dict(keypoints=sm.person(rng, rng.integers(size // 2, w - size // 2), rng.integers(size // 2, h - size // 2),
                                      int(size * rng.uniform(0.85, 1.15))).astype(np.float64), pose_track=k)
             for k in range(per_frame)] for _ in range(n_frames)]


def leg(ctx, a, frames, host, per_frame, size):
    from tests import silhouette_model as sm
    n, h, w = host.shape[:3]
    rng = np.random.default_rng(per_frame)
    poses = crowd(rng, n, per_frame, size, h, w)
    counts, kp, rgba = vis.pack_silhouettes(poses, 'track', 128)
    white = np.full_like(rgba, 255)
    permille = (90, 90, 50)
    touched = np.zeros((n, (h + 15) // 16, (w + 63) // 64), bool)
    for f, _, x0, y0, x1, y1 in vis.pose_boxes(poses, host.shape):
        touched[f, y0 // 16:(y1 + 15) // 16, x0 // 64:(x1 + 63) // 64] = True
    matte = lib.Frames.zeros(ctx, n, h, w)
    ident = np.arange(256, dtype=np.uint8)
    r = {'people_per_frame': per_frame, 'size_px': size, 'tiles_touched_share': round(float(touched.mean()), 3)}
    r['point_frames'] = timed(ctx, a, lambda: image.point_frames(frames, ident, ctx=ctx))
    r['paint_poses'] = timed(ctx, a, lambda: ctx.poses_paint(frames, counts, kp, rgba, permille, 2))
    r['pose_masks'] = timed(ctx, a, lambda: ctx.poses_paint(matte, counts, kp, white, permille, 2, clear=True))
    r['blur_poses'] = timed(ctx, a, lambda: vis.blur_poses(frames, poses, ctx=ctx))
    yard = r['point_frames']['device_ms']
    for k in ('paint_poses', 'pose_masks', 'blur_poses'):
        r[k]['over_point_frames'] = round(r[k]['device_ms'] / yard, 2)
    # the same matte as the model makes it, on the frames the model is run on
    mf = min(a.model_frames, n)
    got = matte.download()[:mf]
    matte.free()
    sub = int(counts[:mf].sum())
    t0 = time.perf_counter()
    down = frames.download()[:mf]
    with ThreadPoolExecutor(16) as pool:
        starts = np.concatenate([[0], np.cumsum(counts[:mf])])
        done = list(pool.map(lambda f: sm.paint(down[f:f + 1], counts[f:f + 1], kp[starts[f]:starts[f + 1]], rgba[starts[f]:starts[f + 1]],
                                                 permille, 2), range(mf)))
    again = ctx.upload(np.concatenate(done))
    ctx.sync()
    again.free()
    model_ms = (time.perf_counter() - t0) * 1e3
    r['model'] = {'frames': mf, 'threads': 16, 'wall_ms_scaled_to_all_frames': round(model_ms * n / mf, 1)}
    r['same_as_model'] = bool(np.array_equal(got, sm.masks((mf, h, w), counts[:mf], kp[:sub], permille, 2)))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=32)
    ap.add_argument('--height', type=int, default=1080)
    ap.add_argument('--width', type=int, default=1920)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--model-frames', type=int, default=4)
    a = ap.parse_args()
    ctx = runtime.get_context(0)
    n, h, w = a.frames, a.height, a.width
    host = np.random.default_rng(5).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    frames = ctx.upload(host)
    out = {'metric': 'silhouettes from skeletons', 'frames': n, 'height': h, 'width': w, 'reps': a.reps, 'batch_MB': round(host.nbytes / 1e6, 1)}
    out['few'] = leg(ctx, a, frames, host, 4, 300)
    out['many'] = leg(ctx, a, frames, host, 64, 80)
    frames.free()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
