"""Tools: time tiled detection's device code on a resident 32 x 2160 x 3840 batch cut into 640-pixel tiles with 128 pixels of
overlap (4 x 8 tiles a frame, 1 024 in all).  One JSON line with three legs:

  cut     ta_frames_tiles, HIP-event time of its kernel (the library's profiling class of the frame kernels) and of the whole
          call, against one read and one write of the tile bytes at the rate `point_frames` reaches on the same batch
  merge   ta_detections_merge on 32 frames of 512 and of 4 096 synthetic candidates (clusters of 1 to 4 near-duplicates, as
          overlaps produce): HIP-event time per kernel and of all kernels, device and wall time of the whole call, and the numpy
          model (tests/tiles_model.py) on the host for the same answer
  detect  RetinaFace.detect_tiles on the seeded detector, wall time of the whole call against the sum of its detect_arrays
          calls on the same tile chunks (cut beforehand): the difference is what cutting and merging add

    python tools/tiles_bench.py [--frames 32] [--reps 5] [--skip-detect]
"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault('OMP_NUM_THREADS', '16')

import numpy as np      # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from terran_amd import image, lib, runtime, tiles      # noqa: E402

H, W, TILE, OVERLAP = 2160, 3840, 640, 128


def med(x):
    return round(float(np.median(x)), 4)


def stream_rate(ctx, frames, reps):
    """GB/s of point_frames over the whole batch (bytes read + written over device time)."""
    n = frames.shape[0]
    ident = np.zeros(n, lib.POINT_DT)
    ident['frame'], ident['x1'], ident['y1'] = np.arange(n), W, H
    table = np.tile(image.brightness_lut(1.1), 3)[None]
    ms = []
    for rep in range(2 + reps):
        ctx.timer_start()
        frames.point(ident, table)
        d = ctx.timer_stop()
        if rep >= 2:
            ms.append(d)
    return 2 * n * H * W * 3 / (min(ms) * 1e-3) / 1e9


def cut_leg(ctx, frames, recs, reps, rate):
    kern, dev = [], []
    for rep in range(2 + reps):
        ctx.profile(True)
        ctx.profile_reset()
        out = ctx.frames_tiles(frames, recs, TILE, TILE)
        ctx.profile(False)
        kms = ctx.profile_read(2)[0]
        out.free()
        ctx.timer_start()
        out = ctx.frames_tiles(frames, recs, TILE, TILE)
        d = ctx.timer_stop()
        out.free()
        if rep >= 2:
            kern.append(kms)
            dev.append(d)
    nbytes = len(recs) * TILE * TILE * 3
    yard = 2 * nbytes / (rate * 1e9) * 1e3
    return {'tiles': len(recs), 'tile_MB': round(nbytes / 1e6, 1), 'kernel_ms': med(kern), 'kernel_ms_min': round(min(kern), 4),
            'call_device_ms': med(dev), 'read_plus_write_at_stream_rate_ms': round(yard, 4), 'kernel_over_yardstick': round(med(kern) / yard, 2),
            'kernel_GBps': round(2 * nbytes / (med(kern) * 1e-3) / 1e9, 1)}


def merge_leg(ctx, n_frames, per_frame, reps):
    from tests import tiles_model as tm
    rng = np.random.default_rng(per_frame)
    parts = [tm.clustered_candidates(rng, per_frame, extent=3000.0) for _ in range(n_frames)]
    boxes, lm, scores = (np.concatenate([p[k] for p in parts]) for k in range(3))
    groups = np.zeros(n_frames, lib.MERGE_GROUP_DT)
    groups['frame'], groups['first'], groups['count'], groups['zoom'] = np.arange(n_frames), np.arange(n_frames) * per_frame, per_frame, 1.0
    names = ('dm_map_kernel', 'dm_rank_kernel', 'dm_matrix_kernel', 'dm_scan_kernel')
    per, kern, dev, wall = {k: [] for k in names}, [], [], []
    for rep in range(2 + reps):
        ctx.kernel_work(reset=True)
        ctx.profile(True)
        ctx.profile_reset()
        got = ctx.detections_merge(groups, n_frames, boxes, lm, scores, 0.4)
        ctx.profile(False)
        kms = ctx.profile_read(3)[0]
        work = ctx.kernel_work(reset=True)
        ctx.timer_start()
        ctx.detections_merge(groups, n_frames, boxes, lm, scores, 0.4)
        d = ctx.timer_stop()
        t0 = time.perf_counter()
        ctx.detections_merge(groups, n_frames, boxes, lm, scores, 0.4)
        t1 = time.perf_counter()
        if rep >= 2:
            for k in names:
                per[k].append(work[k][2])
            kern.append(kms)
            dev.append(d)
            wall.append((t1 - t0) * 1e3)
    t0 = time.perf_counter()
    want = tm.merge_model(groups, n_frames, boxes, lm, scores, 0.4)
    model_ms = (time.perf_counter() - t0) * 1e3
    r = {'frames': n_frames, 'candidates_per_frame': per_frame, 'kept': int(got[0].sum()), 'kernels_ms': med(kern), 'device_ms': med(dev),
         'wall_ms': med(wall), 'numpy_model_wall_ms': round(model_ms, 1), 'same_as_model': bool(all(np.array_equal(a, b) for a, b in zip(got, want)))}
    r.update({k + '_ms': med(v) for k, v in per.items()})
    return r


def detect_leg(ctx, frames, recs, reps, max_tiles=256):
    from terran_amd import weights
    from terran_amd.retinaface import RetinaFace
    det = RetinaFace(device=0, state=weights.make_retinaface_state(), ctx=ctx)
    chunks = [ctx.frames_tiles(frames, recs[lo:lo + max_tiles], TILE, TILE) for lo in range(0, len(recs), max_tiles)]
    # pure noise makes the seeded network fire everywhere: the threshold at which a frame's tiles bring a crowd's worth of candidates
    per_frame = len(recs) // frames.shape[0]
    for threshold in (0.5, 0.7, 0.9, 0.97, 0.99, 0.999):
        if det.detect_arrays(chunks[0], threshold)[0].sum() / (chunks[0].shape[0] / per_frame) <= 4096:
            break
    parts, whole = [], []
    for rep in range(1 + reps):
        t0 = time.perf_counter()
        counts = [det.detect_arrays(c, threshold)[0] for c in chunks]
        t1 = time.perf_counter()
        if rep >= 1:
            parts.append((t1 - t0) * 1e3)
    for c in chunks:
        c.free()
    for rep in range(1 + reps):
        t0 = time.perf_counter()
        out = det.detect_tiles(frames, TILE, OVERLAP, threshold=threshold, max_tiles=max_tiles)
        t1 = time.perf_counter()
        if rep >= 1:
            whole.append((t1 - t0) * 1e3)
    return {'tiles': len(recs), 'chunks': len(chunks), 'threshold': threshold, 'candidates': int(np.concatenate(counts).sum()), 'detections': int(out[0].sum()),
            'detect_arrays_sum_wall_ms': med(parts), 'detect_tiles_wall_ms': med(whole), 'cut_and_merge_add_ms': round(med(whole) - med(parts), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=32)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--skip-detect', action='store_true')
    a = ap.parse_args()
    ctx = runtime.get_context(0)
    one = np.random.default_rng(0).integers(0, 256, (1, H, W, 3), dtype=np.uint8)
    frames = ctx.upload(np.ascontiguousarray(np.broadcast_to(one, (a.frames, H, W, 3))))
    recs = tiles.tile_records(a.frames, tiles.tile_grid(H, W, TILE, OVERLAP))
    out = {'metric': 'tiled detection', 'frames': a.frames, 'reps': a.reps}
    rate = stream_rate(ctx, frames, a.reps)
    out['stream_GBps'] = round(rate, 1)
    out['cut'] = cut_leg(ctx, frames, recs, a.reps, rate)
    for per_frame in (512, 4096):
        out['merge_%d' % per_frame] = merge_leg(ctx, 32, per_frame, a.reps)
    try:
        out['detect'] = 'not measured (--skip-detect)' if a.skip_detect else detect_leg(ctx, frames, recs, max(1, a.reps // 2))
    except lib.TerranAmdError as e:
        out['detect'] = 'not measured: %s' % e
    frames.free()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
