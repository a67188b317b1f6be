"""Tools: time track filling's device code.  One JSON line, one leg per size:

  fill   ta_tracks_fill on `--frames` (32) frames of 64, 512 and 4 096 tracks of 18 joints, seeded: people moving a few pixels a
         frame, 10 % of the rows and 10 % of the joints dropped, max_gap 5: HIP-event time per kernel and of all kernels, device
         and wall time of the whole call (staging copy, kernels, read-back); the model on the host for the same answer on the
         first `--model-frames` frames, scaled to all frames and labelled so; and the yardstick: one read of the input rows plus
         one write of the output rows (12 bytes a point) at the rate `point_frames` reaches IN THE SAME RUN on a resident 32 x
         1080 x 1920 batch (bytes read + written over device time).  Every kernel figure also as a multiple of that; reported, not
         asserted.

    python tools/fill_bench.py [--frames 32] [--reps 5] [--model-frames 3] [--sizes 64,512,4096] [--max-gap 5]
"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault('OMP_NUM_THREADS', '16')

import numpy as np      # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from terran_amd import image, runtime      # noqa: E402
from pose_tiles_bench import med, timed      # noqa: E402

KERNELS = ('tf_link_kernel', 'tf_rank_kernel', 'tf_points_kernel')


def point_frames_rate(ctx, reps):
    """Bytes a second of point_frames over 32 x 1080 x 1920 (bytes read + written over device time)."""
    host = np.random.default_rng(5).integers(0, 256, (32, 1080, 1920, 3), dtype=np.uint8)
    frames = ctx.upload(host)
    ident = np.arange(256, dtype=np.uint8)
    ms = []
    for rep in range(2 + reps):
        ctx.timer_start()
        image.point_frames(frames, ident, ctx=ctx)
        d = ctx.timer_stop()
        if rep >= 2:
            ms.append(d)
    frames.free()
    return 2 * host.nbytes / (med(ms) * 1e-3), med(ms)


def clip(per_frame, n_frames, row_drop=0.1, point_drop=0.1):
    """-> (counts, points (rows, 18, 3) int32, prev): `per_frame` tracks, each row there with probability 1 - row_drop and linked to
    its track's last row, each joint present with probability 1 - point_drop; the rows of a frame are shuffled."""
    rng = np.random.default_rng(per_frame)
    extent = int(60 * np.sqrt(per_frame)) + 80
    pos = rng.integers(0, extent, (per_frame, 1, 2)) + rng.integers(-20, 21, (per_frame, 18, 2))
    last, at = np.full(per_frame, -1, np.int64), 0
    counts, points, prev = [], [], []
    for _ in range(n_frames):
        pos = pos + rng.integers(-3, 4, (per_frame, 1, 2)) + rng.integers(-1, 2, (per_frame, 18, 2))
        here = rng.permutation(per_frame)[rng.random(per_frame) >= row_drop]
        rows = np.zeros((len(here), 18, 3), np.int32)
        rows[:, :, :2] = pos[here]
        rows[:, :, 2] = rng.random((len(here), 18)) >= point_drop
        prev.append(last[here].copy())
        last[here] = at + np.arange(len(here))
        counts.append(len(here))
        points.append(rows)
        at += len(here)
    return np.array(counts, np.int32), np.concatenate(points), np.concatenate(prev).astype(np.int32)


def fill_leg(ctx, n_frames, per_frame, max_gap, reps, model_frames, rate):
    from tests import fill_model as fm
    counts, points, prev = clip(per_frame, n_frames)
    got, per, kern, dev, wall = timed(ctx, lambda: ctx.tracks_fill(counts, points, prev, max_gap, 2), KERNELS, 3, reps)
    mf = min(model_frames, n_frames)
    sub = int(counts[:mf].sum())
    t0 = time.perf_counter()
    want = fm.fill_model(counts[:mf], points[:sub], prev[:sub], max_gap, 2)
    model_ms = (time.perf_counter() - t0) * 1e3
    part = ctx.tracks_fill(counts[:mf], points[:sub], prev[:sub], max_gap, 2)       # the model's frames as a call of their own
    moved = points.nbytes + got[1].nbytes
    yard_ms = moved / rate * 1e3
    r = {'frames': n_frames, 'tracks_per_frame': per_frame, 'max_gap': max_gap, 'rows_in': int(len(points)), 'rows_out': int(len(got[1])),
         'points_filled': int((got[1][:, :, 2] == 2).sum()), 'bytes_moved': moved, 'yardstick_ms': round(yard_ms, 4),
         'kernels_ms': kern, 'device_ms': dev, 'wall_ms': wall, 'kernels_over_yardstick': round(kern / yard_ms, 2),
         'device_over_yardstick': round(dev / yard_ms, 2), 'model_frames': mf,
         'model_wall_ms_scaled_to_all_frames': round(model_ms * n_frames / mf, 1),
         'same_as_model': bool(all(np.array_equal(g, w) for g, w in zip(part, want)))}
    r.update(per)
    for k in KERNELS:
        r[k + '_over_yardstick'] = round(per[k + '_ms'] / yard_ms, 2)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=32)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--model-frames', type=int, default=3)
    ap.add_argument('--sizes', default='64,512,4096')
    ap.add_argument('--max-gap', type=int, default=5)
    a = ap.parse_args()
    ctx = runtime.get_context(0)
    rate, pf_ms = point_frames_rate(ctx, a.reps)
    out = {'metric': 'track filling', 'frames': a.frames, 'reps': a.reps, 'point_frames_ms_32x1080p': pf_ms,
           'point_frames_GBps': round(rate / 1e9, 1)}
    for per_frame in (int(s) for s in a.sizes.split(',')):
        out['fill_%d' % per_frame] = fill_leg(ctx, a.frames, per_frame, a.max_gap, a.reps, a.model_frames, rate)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
