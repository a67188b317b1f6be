"""JPEG ingest: Pillow decode + ta_frames_upload versus ta_jpeg_decode (Huffman on 1 / 16 host threads, pixels on the GPU).

Two sets: 32 x 1080p 4:2:0 q90 (an MJPEG-like batch) and 8 x 12 MP (4000 x 3000) 4:2:0 q90 photos.  The images are
synth.frames at a quarter of the size, bicubic-upscaled and encoded by Pillow (smooth, photo-like content), cached in
--cache.  Encoding needs Pillow; so does the Pillow leg (skipped, and said so, without it).  Reported per set and leg:
images/s (wall), host CPU-seconds per image (process CPU time over the timed loop, every thread), and for the device
path the HIP-event times of the two kernels and the host-to-device copy (ta_jpeg_last_stats with profiling on).

    python tools/jpeg_bench.py [--reps 5] [--cache out/jpeg_bench] [--json out.json]
"""
import argparse
import io
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from terran_amd import runtime, synth   # noqa: E402

SETS = {'1080p_x32': (32, 1080, 1920), '12mp_x8': (8, 3000, 4000)}


def make_set(cache, name, n, h, w):
    d = os.path.join(cache, name)
    files = [os.path.join(d, '%03d.jpg' % i) for i in range(n)]
    if not all(os.path.exists(f) for f in files):
        from PIL import Image
        os.makedirs(d, exist_ok=True)
        small = synth.frames(7 + n, n, h // 4, w // 4)
        for i, f in enumerate(files):
            Image.fromarray(small[i]).resize((w, h), Image.BICUBIC).save(f, 'JPEG', quality=90, subsampling=2)
    out = []
    for f in files:
        with open(f, 'rb') as fh:
            out.append(fh.read())
    return out


def timed(fn, reps):
    fn()                                                     # warm-up (allocations, first launches)
    w0, c0 = time.perf_counter(), time.process_time()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - w0) / reps, (time.process_time() - c0) / reps


def pillow_leg(ctx, datas, threads, reps):
    from PIL import Image

    def one(d):
        return np.asarray(Image.open(io.BytesIO(d)).convert('RGB'))

    pool = ThreadPoolExecutor(threads) if threads > 1 else None

    def run():
        imgs = list(pool.map(one, datas)) if pool else [one(d) for d in datas]
        f = ctx.upload(np.stack(imgs))                          # one batch: ta_frames_upload
        f.free()
    try:
        return timed(run, reps)
    finally:
        if pool:
            pool.shutdown()


def device_leg(ctx, datas, threads, reps):
    def run():
        outs, _ = ctx.jpeg_decode(datas, threads)
        for o in outs:
            o.free()
    wall, cpu = timed(run, reps)
    ctx.profile(True)
    run()
    ms, counts = ctx.jpeg_stats()
    ctx.profile(False)
    return wall, cpu, ms, counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--cache', default=os.path.join(REPO, 'out', 'jpeg_bench'))
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    ctx = runtime.get_context(0)
    try:
        import PIL                                              # noqa: F401
        have_pil = True
    except ImportError:
        have_pil = False
    report = {}
    for name, (n, h, w) in SETS.items():
        datas = make_set(a.cache, name, n, h, w)
        row = {'images': n, 'size': [h, w], 'mb_jpeg': sum(map(len, datas)) / 1e6}
        for threads in (1, 16):
            if have_pil:
                wall, cpu = pillow_leg(ctx, datas, threads, a.reps)
                row['pillow_t%d' % threads] = {'img_per_s': n / wall, 'cpu_s_per_img': cpu / n}
            else:
                row['pillow_t%d' % threads] = 'not measured: Pillow absent'
            wall, cpu, ms, counts = device_leg(ctx, datas, threads, a.reps)
            row['device_t%d' % threads] = {'img_per_s': n / wall, 'cpu_s_per_img': cpu / n, 'host_ms': ms['host'],
                                           'h2d_ms': ms['h2d'], 'idct_ms': ms['idct'], 'color_ms': ms['color'],
                                           'blocks': counts['blocks'], 'upload_mb': counts['bytes'] / 1e6}
        report[name] = row
        print(json.dumps({name: row}), flush=True)
    if a.json:
        with open(a.json, 'w') as fh:
            json.dump(report, fh, indent=1)


if __name__ == '__main__':
    main()
