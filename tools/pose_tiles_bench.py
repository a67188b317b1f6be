"""Tools: time tiled pose estimation's device code.  One JSON line with two legs:

  merge     ta_poses_merge on `--frames` (32) frames of 512 and of 4 096 synthetic skeletons (clusters of 1 to 4 near-duplicates
            dealt out to three groups a frame, tests/pose_tiles_model.py): HIP-event time per kernel and of all kernels, device and
            wall time of the whole call; the model on the host for the same answer (all frames at 512; the first `--model-frames`
            at 4 096, where its explicit loops take seconds a frame, scaled to all frames and labelled so); and, in the same run,
            ta_detections_merge on as many boxes (tools/tiles_bench.py's candidates): the yardstick, reported as a ratio and not
            asserted
  estimate  OpenPose.estimate_tiles on a resident `--frames` x 2160 x 3840 batch of coded frames (synth.pose_code_frames on the
            decoder weights, so that people assemble) cut into 368-pixel tiles with 96 pixels of overlap (8 x 14 a frame), wall time of the
            whole call against the sum of its own ta_openpose_run calls on the same tile chunks (cut beforehand): the difference is
            what cutting and merging add

    python tools/pose_tiles_bench.py [--frames 32] [--reps 5] [--model-frames 2] [--skip-estimate]

`--frames` sizes both legs: the frames of each merge and the 2160p batch of the estimate leg.
"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault('OMP_NUM_THREADS', '16')

import numpy as np      # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from terran_amd import lib, runtime, tiles      # noqa: E402

H, W, TILE, OVERLAP = 2160, 3840, 368, 96


def med(x):
    return round(float(np.median(x)), 4)


def timed(ctx, call, names, klass, reps):
    """-> (the call's answer, {kernel: ms}, all kernels ms, device ms, wall ms), medians over `reps` after two warm-ups."""
    per, kern, dev, wall = {k: [] for k in names}, [], [], []
    for rep in range(2 + reps):
        ctx.kernel_work(reset=True)
        ctx.profile(True)
        ctx.profile_reset()
        got = call()
        ctx.profile(False)
        kms = ctx.profile_read(klass)[0]
        work = ctx.kernel_work(reset=True)
        ctx.timer_start()
        call()
        d = ctx.timer_stop()
        t0 = time.perf_counter()
        call()
        t1 = time.perf_counter()
        if rep >= 2:
            for k in names:
                per[k].append(work[k][2])
            kern.append(kms)
            dev.append(d)
            wall.append((t1 - t0) * 1e3)
    return got, {k + '_ms': med(v) for k, v in per.items()}, med(kern), med(dev), med(wall)


def merge_leg(ctx, n_frames, per_frame, reps, model_frames):
    from tests import pose_tiles_model as pm
    from tests import tiles_model as tm
    rng = np.random.default_rng(per_frame)
    groups, parts = [], []
    for f in range(n_frames):
        kp, sc = pm.clustered_poses(rng, per_frame, 3000)
        groups += pm.split(rng, f, f * per_frame, kp, 3000)
        parts.append((kp, sc))
    kp, sc = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    recs = pm.records(groups)
    names = ('pm_map_kernel', 'pm_rank_kernel', 'pm_matrix_kernel', 'pm_scan_kernel')
    got, per, kern, dev, wall = timed(ctx, lambda: ctx.poses_merge(recs, n_frames, kp, sc), names, 3, reps)
    mf = n_frames if per_frame <= 512 else min(model_frames, n_frames)
    sub = [g for g in groups if g['frame'] < mf]
    t0 = time.perf_counter()
    want = pm.merge_model(sub, mf, kp, sc)
    model_ms = (time.perf_counter() - t0) * 1e3
    head = int(got[0][:mf].sum())
    r = {'frames': n_frames, 'candidates_per_frame': per_frame, 'kept': int(got[0].sum()), 'kernels_ms': kern, 'device_ms': dev, 'wall_ms': wall,
         'model_frames': mf, 'model_wall_ms_scaled_to_all_frames': round(model_ms * n_frames / mf, 1),
         'same_as_model': bool(np.array_equal(got[0][:mf], want[0]) and all(np.array_equal(a[:head], b) for a, b in zip(got[1:], want[1:])))}
    r.update(per)
    # the yardstick: the box merge of the parent commit on as many candidates, in the same run
    rng = np.random.default_rng(per_frame)
    bparts = [tm.clustered_candidates(rng, per_frame, extent=3000.0) for _ in range(n_frames)]
    boxes, lm, scores = (np.concatenate([p[k] for p in bparts]) for k in range(3))
    bg = np.zeros(n_frames, lib.MERGE_GROUP_DT)
    bg['frame'], bg['first'], bg['count'], bg['zoom'] = np.arange(n_frames), np.arange(n_frames) * per_frame, per_frame, 1.0
    bnames = ('dm_map_kernel', 'dm_rank_kernel', 'dm_matrix_kernel', 'dm_scan_kernel')
    bgot, bper, bkern, bdev, bwall = timed(ctx, lambda: ctx.detections_merge(bg, n_frames, boxes, lm, scores, 0.4), bnames, 3, reps)
    r['boxes'] = dict(kept=int(bgot[0].sum()), kernels_ms=bkern, device_ms=bdev, wall_ms=bwall, **bper)
    r['kernels_over_boxes'] = round(kern / bkern, 2)
    r['matrix_over_boxes'] = round(per['pm_matrix_kernel_ms'] / bper['dm_matrix_kernel_ms'], 2)
    r['wall_over_boxes'] = round(wall / bwall, 2)
    return r


def estimate_leg(ctx, n_frames, reps, max_tiles=32):
    from terran_amd import synth, weights
    from terran_amd.openpose import OpenPose
    one = synth.pose_code_frames(3, 1, H, W, 60)
    frames = ctx.upload(np.ascontiguousarray(np.broadcast_to(one, (n_frames, H, W, 3))))
    pose = OpenPose(device=0, state=weights.make_openpose_decoder_state(), ctx=ctx)
    recs = tiles.tile_records(n_frames, tiles.tile_grid(H, W, TILE, OVERLAP))
    parts, whole = [], []
    try:
        for rep in range(1 + reps):
            total = 0.0
            for lo in range(0, len(recs), max_tiles):                # the chunks one at a time: all of them would not fit beside the arena
                chunk = ctx.frames_tiles(frames, recs[lo:lo + max_tiles], TILE, TILE)
                t0 = time.perf_counter()
                counts = pose._estimate_arrays(chunk, 1.0)[0]
                total += time.perf_counter() - t0
                chunk.free()
            if rep >= 1:
                parts.append(total * 1e3)
        for rep in range(1 + reps):
            t0 = time.perf_counter()
            out = pose.estimate_tiles(frames, TILE, OVERLAP, max_tiles=max_tiles)
            t1 = time.perf_counter()
            if rep >= 1:
                whole.append((t1 - t0) * 1e3)
    finally:
        frames.free()
    return {'tiles': len(recs), 'chunks': (len(recs) + max_tiles - 1) // max_tiles, 'max_tiles': max_tiles, 'poses_last_chunk': int(counts.sum()),
            'poses': int(out[0].sum()), 'openpose_run_sum_wall_ms': med(parts), 'estimate_tiles_wall_ms': med(whole),
            'cut_and_merge_add_ms': round(med(whole) - med(parts), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=32)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--model-frames', type=int, default=2)
    ap.add_argument('--skip-estimate', action='store_true')
    a = ap.parse_args()
    ctx = runtime.get_context(0)
    out = {'metric': 'tiled pose estimation', 'frames': a.frames, 'reps': a.reps}
    for per_frame in (512, 4096):
        out['merge_%d' % per_frame] = merge_leg(ctx, a.frames, per_frame, a.reps, a.model_frames)
    try:
        out['estimate'] = 'not measured (--skip-estimate)' if a.skip_estimate else estimate_leg(ctx, a.frames, max(1, a.reps // 2))
    except lib.TerranAmdError as e:
        out['estimate'] = 'not measured: %s' % e
    print(json.dumps(out))


if __name__ == '__main__':
    main()
