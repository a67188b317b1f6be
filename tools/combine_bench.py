"""Tools: time the two-image operations on a resident 32 x 1080 x 1920 batch.  Per case: device time (HIP events around
the library call: staging copy and kernels) and wall time of the public call; for the cases that stream whole frames the
bytes they must move (both batches read, one written; under a resident matte a third one read), the time that traffic
takes at the 1.87 TB/s the histogram kernel streams at, and the ratio of the measured device time to it.  The same work
the way it has to be done without them, under "pillow": download the batch, the Pillow call per frame on 16 threads,
upload it again (null when Pillow is not installed).  Every case runs in a child process of its own under a time limit;
the first one that fails ends the run.  One JSON line.

    python tools/combine_bench.py [--frames 32] [--reps 20] [--case NAME]
"""
import argparse
import json
import os
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = ['difference_frames', 'blend_frames_0.5', 'composite_frames_matte', 'composite_faces_64x200', 'inset_chips_64x112']
STREAM_GBPS = 1870.0                       # the histogram kernel's measured rate


def timed(ctx, a, call):
    dev, wall = [], []
    for rep in range(a.warmup + a.reps):
        ctx.timer_start()
        call()
        d = ctx.timer_stop()
        t0 = time.perf_counter()
        call()
        t1 = time.perf_counter()
        if rep >= a.warmup:
            dev.append(d)
            wall.append((t1 - t0) * 1e3)
    med = lambda x: round(float(np.median(x)), 4)      # noqa: E731
    return {'device_ms': med(dev), 'device_ms_min': round(min(dev), 4), 'wall_ms': med(wall), 'wall_ms_min': round(min(wall), 4)}


def pillow_leg(ctx, frames, a, per_frame):
    """per_frame(index, host frame) does the Pillow work in place."""
    try:
        import PIL
    except ImportError:
        return None
    down, work, up = [], [], []
    with ThreadPoolExecutor(16) as pool:
        for rep in range(1 + a.pillow_reps):
            t0 = time.perf_counter()
            host = frames.download()
            t1 = time.perf_counter()
            list(pool.map(lambda f: per_frame(f, host[f]), range(len(host))))
            t2 = time.perf_counter()
            again = ctx.upload(host)
            ctx.sync()
            again.free()
            t3 = time.perf_counter()
            if rep:
                down.append((t1 - t0) * 1e3)
                work.append((t2 - t1) * 1e3)
                up.append((t3 - t2) * 1e3)
    med = lambda x: round(float(np.median(x)), 4)      # noqa: E731
    total = [d + w + u for d, w, u in zip(down, work, up)]
    return {'version': PIL.__version__, 'threads': 16, 'download_ms': med(down), 'pillow_ms': med(work), 'upload_ms': med(up),
            'total_ms': med(total), 'total_ms_min': round(min(total), 4)}


def run_case(a):
    from terran_amd import image, runtime, synth, vis
    ctx = runtime.get_context(0)
    n, h, w = a.frames, a.height, a.width
    rng = np.random.default_rng(5)
    scene = np.zeros((n, h, w, 3), np.uint8)
    scene[:] = synth.frames(1, 1, h, w)[0]
    other_host = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    frames, other = ctx.upload(scene), ctx.upload(other_host)
    batch_bytes = n * h * w * 3

    def pil():
        from PIL import Image, ImageChops
        return Image, ImageChops

    def in_place(fn):
        def per_frame(f, img):
            img[...] = np.asarray(fn(f, pil()[0].fromarray(img)))
        return per_frame
    passes = 0
    if a.case == 'difference_frames':
        call, passes = (lambda: image.difference_frames(frames, other)), 3
        fn = lambda f, im: pil()[1].difference(im, pil()[0].fromarray(other_host[f]))      # noqa: E731
    elif a.case == 'blend_frames_0.5':
        call, passes = (lambda: image.blend_frames(frames, other, 0.5)), 3
        fn = lambda f, im: pil()[0].blend(im, pil()[0].fromarray(other_host[f]), 0.5)      # noqa: E731
    elif a.case == 'composite_frames_matte':
        y, x = np.mgrid[:h, :w]
        matte_host = np.repeat(np.clip((x + y) % 512 - 128, 0, 255).astype(np.uint8)[..., None], 3, -1)[None]
        matte_host = np.ascontiguousarray(np.broadcast_to(matte_host, (n, h, w, 3)))
        matte = ctx.upload(matte_host)
        call, passes = (lambda: image.composite_frames(frames, other, matte)), 4
        fn = lambda f, im: pil()[0].composite(pil()[0].fromarray(other_host[f]), im, pil()[0].fromarray(matte_host[f, :, :, 0]))      # noqa: E731
    elif a.case == 'composite_faces_64x200':
        x0, y0 = rng.integers(0, w - 200, 64), rng.integers(0, h - 200, 64)
        faces = [[{'bbox': (x0[k], y0[k], x0[k] + 200, y0[k] + 200)} for k in range(64) if k % n == f] for f in range(n)]
        call = lambda: vis.composite_faces(frames, other, faces)      # noqa: E731

        def fn(f, im):
            for face in faces[f]:
                box = tuple(int(v) for v in face['bbox'])
                im.paste(pil()[0].fromarray(other_host[f]).crop(box), box)
            return im
    elif a.case == 'inset_chips_64x112':
        chips_host = rng.integers(0, 256, (64, 112, 112, 3), dtype=np.uint8)
        chips = ctx.upload(chips_host)
        index = np.array([(k % n, k // n) for k in range(64)], np.int32)
        index = index[np.argsort(index[:, 0], kind='stable')]
        call = lambda: vis.inset_chips(frames, chips, index)      # noqa: E731
        places = vis.pack_insets(index, chips.shape, frames.shape)

        def fn(f, im):
            for q in places[places['frame'] == f]:
                im.paste(pil()[0].fromarray(chips_host[q['src_frame']]), (int(q['x0']), int(q['y0'])))
            return im
    else:
        raise SystemExit('unknown case %r' % a.case)
    r = timed(ctx, a, call)
    if passes:
        r['traffic_MB'] = round(passes * batch_bytes / 1e6, 1)
        r['traffic_ms_at_1.87TBps'] = round(passes * batch_bytes / (STREAM_GBPS * 1e9) * 1e3, 4)
        r['device_over_traffic'] = round(r['device_ms_min'] / r['traffic_ms_at_1.87TBps'], 2)
        r['kernel_GBps'] = round(passes * batch_bytes / (r['device_ms_min'] * 1e-3) / 1e9, 1)
    r['pillow'] = pillow_leg(ctx, frames, a, in_place(fn))
    print(json.dumps(r))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=32)
    ap.add_argument('--height', type=int, default=1080)
    ap.add_argument('--width', type=int, default=1920)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--pillow-reps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--case', default=None, help='run this case alone, in this process')
    ap.add_argument('--case-timeout', type=int, default=240, help='seconds a case may take')
    a = ap.parse_args()
    if a.case:
        return run_case(a)
    out = {'metric': 'two-image operations per batch', 'frames': a.frames, 'height': a.height, 'width': a.width, 'reps': a.reps}
    passed = ['--frames', a.frames, '--height', a.height, '--width', a.width, '--reps', a.reps, '--pillow-reps', a.pillow_reps,
              '--warmup', a.warmup]
    for case in CASES:
        cmd = ['timeout', '-k', '10', str(a.case_timeout), sys.executable, os.path.abspath(__file__), '--case', case] + [str(v) for v in passed]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        if p.returncode != 0:
            out[case] = {'failed': p.returncode, 'stderr': p.stderr.decode(errors='replace')[-400:]}
            print(json.dumps(out))
            return 1
        out[case] = json.loads(p.stdout.decode().strip().splitlines()[-1])
    print(json.dumps(out))
    return 0


if __name__ == '__main__':
    sys.exit(main())
