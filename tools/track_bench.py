"""Tools: time skeleton tracking's device code.  One JSON line, one leg per size and max_gap:

  track  ta_poses_track on one sequence of `--frames` (32) frames of 64, 512 and 4 096 skeletons, people moving a few pixels a
         frame on a canvas that grows with the crowd, max_gap 0 and 5: HIP-event time per kernel (the pair scan and the
         resolution separately) and of all kernels, device and wall time of the whole call; the model on the host for the same
         answer (all frames at 64 and 512; the first `--model-frames` at 4 096, scaled to all frames and labelled so); the pair
         scan against its yardsticks at the vector unit's 78.6 T lane-operations a second (256 CUs x 128 lanes a cycle x 2.4 GHz):
         the s-tests alone -- and, popcount, compare: 3 operations a pair -- and the 18-joint sums if every pair ran one -- two
         subtractions, two multiply-adds, a select and a 64-bit add (2): 8 operations a joint; and, in the same process, the
         kernels of ta_faces_poses_link on as many faces and skeletons a frame (tools/link_bench.py's people): the neighbour to
         compare with, per pair and as a ratio, reported and not asserted

    python tools/track_bench.py [--frames 32] [--reps 5] [--model-frames 3] [--sizes 64,512,4096] [--gaps 0,5]
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
from pose_tiles_bench import timed      # noqa: E402
from link_bench import people, KERNELS as LINK_KERNELS      # noqa: E402

LANE_OPS_PER_S = 256 * 128 * 2.4e9
KERNELS = ('pt_pack_kernel', 'pt_scan_kernel', 'pt_resolve_kernel', 'pt_root_kernel')


def track_leg(ctx, n_frames, per_frame, max_gap, reps, model_frames, link):
    from tests import track_model as tm
    rng = np.random.default_rng(per_frame)
    frames, _ = tm.walkers(rng, per_frame, n_frames, step=3, extent=int(60 * np.sqrt(per_frame)) + 80)
    counts, kp = tm.call_of(frames)
    args = (150, 3, max_gap)
    got, per, kern, dev, wall = timed(ctx, lambda: ctx.poses_track([n_frames], [0], counts, kp, None, *args), KERNELS, 3, reps)
    mf = n_frames if per_frame <= 512 else min(model_frames, n_frames)
    t0 = time.perf_counter()
    want = tm.track_model([mf], [0], counts[:mf], kp[:mf * per_frame], None, *args)
    model_ms = (time.perf_counter() - t0) * 1e3
    pairs = float(sum(min(t, max_gap + 1) for t in range(n_frames))) * per_frame * per_frame
    s_ms, sum_ms = pairs * 3 / LANE_OPS_PER_S * 1e3, pairs * 18 * 8 / LANE_OPS_PER_S * 1e3
    r = {'frames': n_frames, 'poses_per_frame': per_frame, 'max_gap': max_gap, 'links': int(got[2].sum()), 'tracks': int((got[0] < 0).sum()),
         'pairs': pairs, 'kernels_ms': kern, 'device_ms': dev, 'wall_ms': wall, 'model_frames': mf,
         'model_wall_ms_scaled_to_all_frames': round(model_ms * n_frames / mf, 1),
         'same_as_model': bool(np.array_equal(got[0][:mf * per_frame], want[0]) and np.array_equal(got[1][:mf * per_frame], want[1])),
         's_test_yardstick_ms': round(s_ms, 4), 'joint_sum_yardstick_ms': round(sum_ms, 4),
         'scan_over_s_test_yardstick': round(per['pt_scan_kernel_ms'] / s_ms, 2),
         'scan_over_joint_sum_yardstick': round(per['pt_scan_kernel_ms'] / sum_ms, 2),
         'scan_ns_per_1000_pairs': round(per['pt_scan_kernel_ms'] * 1e9 / pairs, 3)}
    r.update(per)
    r['link'] = link
    r['kernels_over_link'] = round(kern / link['kernels_ms'], 2)
    r['scan_per_pair_over_link_scan_per_pair'] = round(r['scan_ns_per_1000_pairs'] / link['scan_ns_per_1000_pairs'], 2)
    r['wall_over_link'] = round(wall / link['wall_ms'], 2)
    return r


def link_leg(ctx, n_frames, per_frame, reps):
    """The neighbour: ta_faces_poses_link on as many faces and skeletons a frame."""
    rng = np.random.default_rng(per_frame)
    parts = [people(rng, per_frame) for _ in range(n_frames)]
    boxes, kp = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    counts = np.full(n_frames, per_frame, np.int32)
    got, per, kern, dev, wall = timed(ctx, lambda: ctx.faces_poses_link(counts, boxes, counts, kp), LINK_KERNELS, 3, reps)
    pairs = float(n_frames) * per_frame * per_frame
    return dict(links=int(got[2].sum()), rounds=got[3], pairs=pairs, kernels_ms=kern, device_ms=dev, wall_ms=wall,
                scan_ns_per_1000_pairs=round(per['fl_matrix_kernel_ms'] * 1e9 / pairs, 3), **per)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=32)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--model-frames', type=int, default=3)
    ap.add_argument('--sizes', default='64,512,4096')
    ap.add_argument('--gaps', default='0,5')
    a = ap.parse_args()
    ctx = runtime.get_context(0)
    out = {'metric': 'skeleton tracking', 'frames': a.frames, 'reps': a.reps, 'lane_ops_per_s': LANE_OPS_PER_S}
    for per_frame in (int(s) for s in a.sizes.split(',')):
        link = link_leg(ctx, a.frames, per_frame, a.reps)
        for gap in (int(s) for s in a.gaps.split(',')):
            out['track_%d_gap%d' % (per_frame, gap)] = track_leg(ctx, a.frames, per_frame, gap, a.reps, a.model_frames, link)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
