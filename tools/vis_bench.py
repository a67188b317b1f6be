"""Tools: time terran_amd.vis.draw_faces + draw_poses on a resident 32 x 1080 x 1920 batch with the bench's scene
(4 synth.people stick figures and 2 boxes per frame).  Per batch: host packing time (dicts -> primitives, both calls),
device time (HIP events around each ta_frames_draw: staging copy + kernel) and wall time of the two calls.  A second leg
draws the same scene with labels=True (every face carries a track id, so every face gets its '#<track>' tab): host packing
with the label cache emptied before every repetition (cold: every distinct label is rasterised) and left alone (warm),
device time and wall time, under "labels".  One JSON line.

    python tools/vis_bench.py [--frames 32] [--reps 30] [--scale 1.0]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from terran_amd import runtime, synth, vis      # noqa: E402


def scene(seed, n, h, w):
    rng = np.random.default_rng(seed)
    faces, poses = [], []
    for i in range(n):
        kps, v = synth.people(seed + i, 4, h, w)
        k = np.concatenate([kps, v[..., None]], -1).astype(np.int32)
        poses.append([{'keypoints': x, 'score': 1.0} for x in k])
        b = []
        for j in range(2):
            x0, y0 = rng.uniform(0, w - 300), rng.uniform(0, h - 300)
            s = rng.uniform(60, 250)
            b.append({'bbox': np.array([x0, y0, x0 + s, y0 + 1.2 * s], np.float32), 'track': int(rng.integers(1, 9))})
        faces.append(b)
    return faces, poses


def labels_leg(ctx, frames, faces, poses, a, med):
    """draw_faces(labels=True) + draw_poses on the same batch and scene."""
    cold_ms, warm_ms, dev_ms, wall_ms, wall_cold_ms = [], [], [], [], []
    pf, atlas = vis.pack_faces(faces, a.scale, labels=True)
    n_prims, n_masks = len(pf) + len(vis.pack_poses(poses, a.scale)), int((pf['kind'] == 3).sum())
    for rep in range(a.warmup + a.reps):
        vis._masks.clear()
        t0 = time.perf_counter()
        vis.pack_faces(faces, a.scale, labels=True)
        vis.pack_poses(poses, a.scale)
        t1 = time.perf_counter()
        pf, atlas = vis.pack_faces(faces, a.scale, labels=True)
        pp = vis.pack_poses(poses, a.scale)
        t2 = time.perf_counter()
        ctx.timer_start()
        frames.draw(pf, atlas)
        d0 = ctx.timer_stop()
        ctx.timer_start()
        frames.draw(pp)
        d1 = ctx.timer_stop()
        w0 = time.perf_counter()
        vis.draw_faces(frames, faces, a.scale, labels=True)  # the public calls, packing included, cache warm
        vis.draw_poses(frames, poses, a.scale)
        w1 = time.perf_counter()
        vis._masks.clear()
        vis.draw_faces(frames, faces, a.scale, labels=True)  # the same with every label to rasterise
        vis.draw_poses(frames, poses, a.scale)
        w2 = time.perf_counter()
        if rep >= a.warmup:
            cold_ms.append((t1 - t0) * 1e3)
            warm_ms.append((t2 - t1) * 1e3)
            dev_ms.append(d0 + d1)
            wall_ms.append((w1 - w0) * 1e3)
            wall_cold_ms.append((w2 - w1) * 1e3)
    return {'primitives': n_prims, 'masks': n_masks, 'distinct_masks': len(vis._masks), 'mask_bytes': int(len(atlas)),
            'host_pack_cold_ms': med(cold_ms), 'host_pack_warm_ms': med(warm_ms), 'device_ms': med(dev_ms),
            'wall_ms': med(wall_ms), 'wall_cold_ms': med(wall_cold_ms), 'wall_ms_min': round(min(wall_ms), 4),
            'device_ms_min': round(min(dev_ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=32)
    ap.add_argument('--height', type=int, default=1080)
    ap.add_argument('--width', type=int, default=1920)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--scale', type=float, default=1.0)
    a = ap.parse_args()
    ctx = runtime.get_context(0)
    host = np.zeros((a.frames, a.height, a.width, 3), np.uint8)
    host[:] = synth.frames(1, 1, a.height, a.width)[0]
    frames = ctx.upload(host)
    faces, poses = scene(7, a.frames, a.height, a.width)
    pack_ms, dev_ms, wall_ms = [], [], []
    n_prims = len(vis.pack_faces(faces, a.scale)) + len(vis.pack_poses(poses, a.scale))
    for rep in range(a.warmup + a.reps):
        t0 = time.perf_counter()
        pf = vis.pack_faces(faces, a.scale)
        pp = vis.pack_poses(poses, a.scale)
        t1 = time.perf_counter()
        ctx.timer_start()
        frames.draw(pf)
        d0 = ctx.timer_stop()
        ctx.timer_start()
        frames.draw(pp)
        d1 = ctx.timer_stop()
        t2 = time.perf_counter()
        w0 = time.perf_counter()
        vis.draw_faces(frames, faces, a.scale)           # the public calls, packing included
        vis.draw_poses(frames, poses, a.scale)
        w1 = time.perf_counter()
        if rep >= a.warmup:
            pack_ms.append((t1 - t0) * 1e3)
            dev_ms.append(d0 + d1)
            wall_ms.append((w1 - w0) * 1e3)
    drawn = int((frames.download() != host).any(-1).sum())
    med = lambda x: round(float(np.median(x)), 4)      # noqa: E731
    labels = labels_leg(ctx, frames, faces, poses, a, med)
    frames.free()
    print(json.dumps({'metric': 'vis draw_faces + draw_poses per batch', 'frames': a.frames, 'height': a.height,
                      'width': a.width, 'scale': a.scale, 'primitives': n_prims, 'pixels_changed': drawn,
                      'host_pack_ms': med(pack_ms), 'device_ms': med(dev_ms), 'wall_ms': med(wall_ms),
                      'wall_ms_min': round(min(wall_ms), 4), 'device_ms_min': round(min(dev_ms), 4), 'reps': a.reps,
                      'target_ms': 1.0, 'labels': labels}))


if __name__ == '__main__':
    main()
