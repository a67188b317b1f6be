"""Tools: time the face-to-skeleton link's device code.  One JSON line, one leg per size:

  link   ta_faces_poses_link on `--frames` (32) frames of 64, 512 and 4 096 faces and as many skeletons: people stand in groups
         of three whose heads lie within one face box of each other, so a face qualifies with about three skeletons (the realised
         average is reported); HIP-event time per kernel and of all kernels, device and wall time of the whole call, the rounds
         the call ran; the model on the host for the same answer (all frames at 64 and 512; the first `--model-frames` at 4 096,
         where its loop over faces takes seconds a frame, scaled to all frames and labelled so); the pair scan against its
         yardstick: F * P * 5 point tests per frame, four integer compares each, at the vector unit's 78.6 T lane-operations a second
         (256 CUs x 128 lanes a cycle x 2.4 GHz; the guide's 157.3 TFLOP/s f32 vector peak counts an FMA as two), the scan running
         once a call whatever the rounds; and, in the same process, ta_poses_merge on as many skeletons per frame
         (tools/pose_tiles_bench.py's candidates): the neighbour to compare with, reported as a ratio and not asserted

    python tools/link_bench.py [--frames 32] [--reps 5] [--model-frames 2] [--sizes 64,512,4096]
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
from terran_amd import runtime      # noqa: E402
from pose_tiles_bench import med, timed      # noqa: E402

LANE_OPS_PER_S = 256 * 128 * 2.4e9
KERNELS = ('fl_pack_kernel', 'fl_matrix_kernel', 'fl_best_kernel', 'fl_commit_kernel')


def people(rng, n, size=48):
    """n faces and n skeletons of one frame: groups of three people whose heads are about a third of a face apart, the groups
    spread so that they seldom meet.  -> (boxes (n, 4), keypoints (n, 18, 3)) int32, both in random order."""
    from tests import link_model as lm
    groups = (n + 2) // 3
    extent = int(size * 6 * np.sqrt(groups)) + size
    centre = rng.integers(size, extent, (groups, 1, 2)) + rng.integers(-size // 3, size // 3 + 1, (groups, 3, 2))
    head = centre.reshape(-1, 2)[:n]
    boxes = np.concatenate([head - size // 2, head + size // 2], 1).astype(np.int32)
    kp = np.zeros((n, 18, 3), np.int32)
    kp[:, :, :2] = head[:, None, :] + rng.integers(-size // 6, size // 6 + 1, (n, 18, 2))
    kp[:, :, 2] = rng.random((n, 18)) < 0.8
    kp[:, 1:14, 1] += size
    return boxes[rng.permutation(n)], kp[rng.permutation(n)]


def link_leg(ctx, n_frames, per_frame, reps, model_frames):
    from tests import link_model as lm
    rng = np.random.default_rng(per_frame)
    parts = [people(rng, per_frame) for _ in range(n_frames)]
    boxes, kp = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    counts = np.full(n_frames, per_frame, np.int32)
    got, per, kern, dev, wall = timed(ctx, lambda: ctx.faces_poses_link(counts, boxes, counts, kp), KERNELS, 3, reps)
    mf = n_frames if per_frame <= 512 else min(model_frames, n_frames)
    sub = (counts[:mf], boxes[:mf * per_frame], counts[:mf], kp[:mf * per_frame])
    t0 = time.perf_counter()
    want = lm.link_model(*sub)
    model_ms = (time.perf_counter() - t0) * 1e3
    q = lm.qualifying_per_face(*sub)
    points = float(n_frames) * per_frame * per_frame * 5
    yard_ms = points * 4 / LANE_OPS_PER_S * 1e3
    r = {'frames': n_frames, 'faces_per_frame': per_frame, 'poses_per_frame': per_frame, 'qualifying_per_face': round(float(q.mean()), 2),
         'links': int(got[2].sum()), 'rounds': got[3], 'kernels_ms': kern, 'device_ms': dev, 'wall_ms': wall, 'model_frames': mf,
         'model_wall_ms_scaled_to_all_frames': round(model_ms * n_frames / mf, 1),
         'same_as_model': bool(np.array_equal(got[0][:mf * per_frame], want[0]) and np.array_equal(got[1][:mf * per_frame], want[1])),
         'scan_yardstick_ms': round(yard_ms, 4), 'scan_over_yardstick': round(per['fl_matrix_kernel_ms'] / yard_ms, 2)}
    r.update(per)
    # the neighbour: the skeleton merge on as many candidates a frame, in the same process
    from tests import pose_tiles_model as pm
    rng = np.random.default_rng(per_frame)
    groups, pparts = [], []
    for f in range(n_frames):
        pk, sc = pm.clustered_poses(rng, per_frame, 3000)
        groups += pm.split(rng, f, f * per_frame, pk, 3000)
        pparts.append((pk, sc))
    pk, sc = np.concatenate([p[0] for p in pparts]), np.concatenate([p[1] for p in pparts])
    recs = pm.records(groups)
    names = ('pm_map_kernel', 'pm_rank_kernel', 'pm_matrix_kernel', 'pm_scan_kernel')
    mgot, mper, mkern, mdev, mwall = timed(ctx, lambda: ctx.poses_merge(recs, n_frames, pk, sc), names, 3, reps)
    r['poses_merge'] = dict(kept=int(mgot[0].sum()), kernels_ms=mkern, device_ms=mdev, wall_ms=mwall, **mper)
    r['kernels_over_poses_merge'] = round(kern / mkern, 2)
    r['scan_over_poses_merge_matrix'] = round(per['fl_matrix_kernel_ms'] / mper['pm_matrix_kernel_ms'], 2)
    r['wall_over_poses_merge'] = round(wall / mwall, 2)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=32)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--model-frames', type=int, default=2)
    ap.add_argument('--sizes', default='64,512,4096')
    a = ap.parse_args()
    ctx = runtime.get_context(0)
    out = {'metric': 'face-to-skeleton link', 'frames': a.frames, 'reps': a.reps, 'lane_ops_per_s': LANE_OPS_PER_S}
    for per_frame in (int(s) for s in a.sizes.split(',')):
        out['link_%d' % per_frame] = link_leg(ctx, a.frames, per_frame, a.reps, a.model_frames)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
