"""Tools: time FaceGallery's search (lib.Gallery.search) on a resident gallery of 512-float embeddings.  Per case -- q queries,
k results, n rows -- the device time of the two search kernels (HIP events: the library's profiling class of the
post-processing kernels), the device time of the whole call (events around it: query upload, kernels, results back) and
its wall time.  Yardsticks of the same run: one read of the gallery's bytes at the rate `point_frames` reaches on a
32 x 1080p batch (frames read and written), `ctx.cosine_distance` + a host argpartition for 64 queries over 10^5 rows (the only
way to the same answer without the gallery), and numpy on 16 threads (float32 matrix product + argpartition).  One JSON line.

    python tools/gallery_bench.py [--rows 100000 1000000] [--reps 10]
    python tools/gallery_bench.py --cluster [--reps 5]      # lib.Gallery.cluster at 8 192 and 65 536 rows: see cluster_leg
"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault('OMP_NUM_THREADS', '16')

import numpy as np      # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from terran_amd import image, lib, runtime      # noqa: E402


def med(x):
    return round(float(np.median(x)), 4)


def stream_rate(ctx, reps):
    """GB/s of point_frames on 32 x 1080 x 1920 (bytes read + written over device time)."""
    frames = lib.Frames.zeros(ctx, 32, 1080, 1920)
    ident = np.zeros(32, lib.POINT_DT)
    ident['frame'], ident['x1'], ident['y1'] = np.arange(32), 1920, 1080
    table = np.tile(image.brightness_lut(1.1), 3)[None]
    ms = []
    for rep in range(3 + reps):
        ctx.timer_start()
        frames.point(ident, table)
        d = ctx.timer_stop()
        if rep >= 3:
            ms.append(d)
    frames.free()
    return 2 * 32 * 1080 * 1920 * 3 / (min(ms) * 1e-3) / 1e9


def time_search(ctx, g, q, k, reps, warmup=2):
    kern, dev, wall = [], [], []
    for rep in range(warmup + reps):
        ctx.profile(True)
        ctx.profile_reset()
        g.search(q, k)
        ctx.profile(False)
        kms = ctx.profile_read(3)[0]
        ctx.timer_start()
        g.search(q, k)
        d = ctx.timer_stop()
        t0 = time.perf_counter()
        g.search(q, k)
        t1 = time.perf_counter()
        if rep >= warmup:
            kern.append(kms)
            dev.append(d)
            wall.append((t1 - t0) * 1e3)
    return {'kernel_ms': med(kern), 'kernel_ms_min': round(min(kern), 4), 'device_ms': med(dev), 'wall_ms': med(wall)}


F32_MFMA_PEAK = 157e12          # FLOP/s of the exact-f32 MFMA (DESIGN: the yardstick of the exact-f32 conv kernels)


def cluster_leg(ctx, dim, sizes, reps):
    """lib.Gallery.cluster (ta_gallery_cluster) on n rows: n / 16 identities of 16 noisy embeddings each (cosine distance
    about 0.27 inside an identity, about 1 between two), threshold 0.5, min_samples 4.  Per n: HIP-event time of the
    adjacency kernel, of the propagation rounds and of all the call's kernels, device and wall time of the whole call, the
    rounds, and the adjacency kernel's multiple of the time its n (n + 128) dim FLOP (every unordered pair of 128-row
    tiles once, 2 FLOP per multiply-add) take at the exact-f32 MFMA peak.  At n <= 8192 the same answer through sklearn's
    DBSCAN(metric='cosine') on the downloaded rows, 16 threads."""
    out = {}
    rng = np.random.default_rng(2)
    for n in sizes:
        centers = rng.standard_normal((n // 16, dim), dtype=np.float32)
        centers /= np.linalg.norm(centers, axis=1, keepdims=True)
        rows = np.repeat(centers, 16, axis=0) + 0.6 / np.sqrt(dim) * rng.standard_normal((n // 16 * 16, dim), dtype=np.float32)
        rows = rows[rng.permutation(len(rows))]
        g = lib.Gallery(ctx, dim, reserve=len(rows))
        g.add(rows, np.zeros(len(rows), np.int32))
        adj, prop, kern, dev, wall = [], [], [], [], []
        for rep in range(1 + reps):
            ctx.kernel_work(reset=True)
            ctx.profile(True)
            ctx.profile_reset()
            labels, degree, count, rounds = g.cluster(0.5, 4)
            ctx.profile(False)
            kms = ctx.profile_read(3)[0]
            work = ctx.kernel_work(reset=True)
            ctx.timer_start()
            g.cluster(0.5, 4)
            d = ctx.timer_stop()
            t0 = time.perf_counter()
            g.cluster(0.5, 4)
            t1 = time.perf_counter()
            if rep >= 1:
                adj.append(work['gallery_adj_kernel'][2])
                prop.append(work['gallery_propagate_kernel'][2])
                kern.append(kms)
                dev.append(d)
                wall.append((t1 - t0) * 1e3)
        ideal_ms = len(rows) * (len(rows) + 128) * dim / F32_MFMA_PEAK * 1e3
        r = {'rows': len(rows), 'clusters': count, 'noise': int((labels < 0).sum()), 'mean_degree': round(float(degree.mean()), 2), 'rounds': rounds,
             'adjacency_kernel_ms': med(adj), 'adjacency_kernel_ms_min': round(min(adj), 4), 'adjacency_at_peak_ms': round(ideal_ms, 4),
             'adjacency_over_peak': round(med(adj) / ideal_ms, 2), 'propagation_ms': med(prop), 'kernels_ms': med(kern), 'device_ms': med(dev),
             'wall_ms': med(wall)}
        if len(rows) <= 8192:
            try:
                from sklearn.cluster import DBSCAN
                stored, _ = g.download()
                ts = []
                for rep in range(2):
                    t0 = time.perf_counter()
                    want = DBSCAN(eps=0.5, min_samples=4, metric='cosine', n_jobs=16).fit(stored).labels_
                    ts.append((time.perf_counter() - t0) * 1e3)
                r['sklearn_dbscan_16_threads_wall_ms'] = round(min(ts), 1)
                r['sklearn_same_labels'] = bool(np.array_equal(want, labels))
            except ImportError:
                r['sklearn_dbscan_16_threads_wall_ms'] = 'not measured (no sklearn)'
        out['rows_%d' % n] = r
        g.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cluster', action='store_true', help='time ta_gallery_cluster instead of the search (8 192 and 65 536 rows)')
    ap.add_argument('--rows', type=int, nargs='+', default=[100000, 1000000])
    ap.add_argument('--queries', type=int, nargs='+', default=[1, 32, 64, 256])
    ap.add_argument('--k', type=int, nargs='+', default=[1, 8])
    ap.add_argument('--dim', type=int, default=512)
    ap.add_argument('--reps', type=int, default=10)
    a = ap.parse_args()
    ctx = runtime.get_context(0)
    if a.cluster:
        out = {'metric': 'gallery cluster', 'dim': a.dim, 'reps': a.reps}
        out.update(cluster_leg(ctx, a.dim, [8192, 65536], a.reps))
        print(json.dumps(out))
        return
    rng = np.random.default_rng(1)
    out = {'metric': 'gallery search', 'dim': a.dim, 'reps': a.reps}
    rate = stream_rate(ctx, a.reps)
    out['stream_GBps'] = round(rate, 1)
    for n in a.rows:
        rows = rng.standard_normal((n, a.dim), dtype=np.float32)
        g = lib.Gallery(ctx, a.dim, reserve=n)
        t0 = time.perf_counter()
        g.add(rows, np.arange(n, dtype=np.int32))
        add_ms = (time.perf_counter() - t0) * 1e3
        one_read_ms = n * a.dim * 4 / (rate * 1e9) * 1e3
        block = {'add_wall_ms': round(add_ms, 1), 'one_read_ms': round(one_read_ms, 4), 'cases': {}}
        for nq in a.queries:
            q = rng.standard_normal((nq, a.dim), dtype=np.float32)
            for k in a.k:
                r = time_search(ctx, g, q, k, a.reps)
                r['over_one_read'] = round(r['kernel_ms'] / one_read_ms, 2)
                r['gallery_GBps'] = round(n * a.dim * 4 / (r['kernel_ms'] * 1e-3) / 1e9, 1)
                block['cases']['q%d_k%d' % (nq, k)] = r
        if n <= 100000:                                   # the ways to the same answer without the gallery, 64 queries, k = 8
            q = rng.standard_normal((64, a.dim), dtype=np.float32)
            wall = []
            for rep in range(3):
                t0 = time.perf_counter()
                d = ctx.cosine_distance(q, rows)
                idx = np.argpartition(d, 8, axis=1)[:, :8]
                wall.append((time.perf_counter() - t0) * 1e3)
            block['cosine_distance_argpartition_q64_k8_wall_ms'] = med(wall[1:])
            rn = rows / np.linalg.norm(rows, axis=1, keepdims=True)
            wall = []
            for rep in range(3):
                t0 = time.perf_counter()
                d = 1.0 - (q / np.linalg.norm(q, axis=1, keepdims=True)) @ rn.T
                idx = np.argpartition(d, 8, axis=1)[:, :8]      # noqa: F841
                wall.append((time.perf_counter() - t0) * 1e3)
            block['numpy_16_threads_q64_k8_wall_ms'] = med(wall[1:])
        out['rows_%d' % n] = block
        g.free()
        del rows
    print(json.dumps(out))


if __name__ == '__main__':
    main()
