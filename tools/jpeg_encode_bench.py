"""JPEG output: resident frames -> JPEG files with ta_jpeg_encode (every stage on the GPU, only the files copied back)
versus download() + Pillow on 1 and 16 host threads.

Frames: 32 x 1080p resident frames, the smooth photo-like content tools/jpeg_bench.py encodes (synth.frames at a
quarter of the size, bicubic-upscaled) and a uniform-noise batch; each at q75 and q90, 4:2:0 (Pillow's default).
Reported per set, quality and leg: images/s (wall), host CPU-seconds per image (process CPU time over the timed loop,
every thread) and bytes copied device to host; for the device path also the HIP-event time of each pass
(ta_jpeg_encode_last_stats with profiling on).  The Pillow legs need Pillow (skipped, and said so, without it).
--optimize adds, per set and quality, the same device leg with optimize=True (per-image Huffman tables): its images/s,
host CPU, bytes to host, pass times (with `statistics`, the symbol-count pass, and `tables`, the host's table building)
and the size of its files over the standard ones; --no-pillow leaves the Pillow legs out.

    python tools/jpeg_encode_bench.py [--reps 5] [--optimize] [--no-pillow] [--json out.json]
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

N, H, W = 32, 1080, 1920


def make_frames(kind):
    if kind == 'noise':
        return np.random.default_rng(5).integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    from PIL import Image
    small = synth.frames(7 + N, N, H // 4, W // 4)
    return np.stack([np.asarray(Image.fromarray(s).resize((W, H), Image.BICUBIC)) for s in small])


def make_frames_no_pillow(kind):
    if kind == 'noise':
        return make_frames(kind)
    small = synth.frames(7 + N, N, H // 4, W // 4)
    return np.repeat(np.repeat(small, 4, 1), 4, 2)          # nearest upscale when Pillow is absent (said so in the report)


def timed(fn, reps):
    fn()                                                     # warm-up (allocations, first launches)
    w0, c0 = time.perf_counter(), time.process_time()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - w0) / reps, (time.process_time() - c0) / reps


def pillow_leg(frames, quality, threads, reps):
    from PIL import Image

    def one(px):
        f = io.BytesIO()
        Image.fromarray(px).save(f, 'JPEG', quality=quality, subsampling=2)
        return f.getvalue()

    pool = ThreadPoolExecutor(threads) if threads > 1 else None

    def run():
        host = frames.download()                             # the whole batch over PCIe
        return list(pool.map(one, host)) if pool else [one(px) for px in host]
    try:
        return timed(run, reps)
    finally:
        if pool:
            pool.shutdown()


def device_leg(ctx, frames, quality, reps, optimize=False):
    def run():
        return frames.encode_jpeg(quality, 2, ctx=ctx, optimize=optimize)
    wall, cpu = timed(run, reps)
    ctx.profile(True)
    files = run()
    ms, counts = ctx.jpeg_encode_stats()
    ctx.profile(False)
    return wall, cpu, ms, counts, files


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--json', default=None)
    ap.add_argument('--optimize', action='store_true', help='also measure optimize=True')
    ap.add_argument('--no-pillow', action='store_true', help='skip the download + Pillow legs')
    a = ap.parse_args()
    ctx = runtime.get_context(0)
    try:
        import PIL                                              # noqa: F401
        have_pil = True
    except ImportError:
        have_pil = False
    report = {}
    for kind in ('synthetic', 'noise'):
        host = make_frames(kind) if have_pil or kind == 'noise' else make_frames_no_pillow(kind)
        frames = ctx.upload(host)
        for quality in (75, 90):
            row = {'images': N, 'size': [H, W], 'quality': quality, 'subsampling': '4:2:0',
                   'rgb_mb': host.nbytes / 1e6}
            wall, cpu, ms, counts, files = device_leg(ctx, frames, quality, a.reps)
            row['device'] = {'img_per_s': N / wall, 'cpu_ms_per_img': 1e3 * cpu / N, 'd2h_mb': counts['bytes'] / 1e6,
                             'pass_ms': {k: round(v, 4) for k, v in ms.items()}, 'blocks': counts['blocks']}
            if a.optimize:
                standard_bytes = sum(len(f) for f in files)
                wall, cpu, ms, counts, files = device_leg(ctx, frames, quality, a.reps, optimize=True)
                row['device_optimize'] = {'img_per_s': N / wall, 'cpu_ms_per_img': 1e3 * cpu / N,
                                          'd2h_mb': counts['bytes'] / 1e6,
                                          'pass_ms': {k: round(v, 4) for k, v in ms.items()},
                                          'size_ratio': sum(len(f) for f in files) / standard_bytes,
                                          'speed_vs_standard': N / wall / row['device']['img_per_s']}
            for threads in (() if a.no_pillow else (1, 16)):
                if have_pil:
                    wall, cpu = pillow_leg(frames, quality, threads, max(1, a.reps // (2 if threads == 1 else 1)))
                    row['pillow_t%d' % threads] = {'img_per_s': N / wall, 'cpu_ms_per_img': 1e3 * cpu / N,
                                                   'd2h_mb': host.nbytes / 1e6}
                else:
                    row['pillow_t%d' % threads] = 'not measured: Pillow absent'
            if have_pil and not a.no_pillow:
                row['speedup_vs_pillow_t16'] = row['device']['img_per_s'] / row['pillow_t16']['img_per_s']
            name = '%s_q%d' % (kind, quality)
            report[name] = row
            print(json.dumps({name: row}), flush=True)
        frames.free()
    if a.json:
        with open(a.json, 'w') as fh:
            json.dump(report, fh, indent=1)


if __name__ == '__main__':
    main()
