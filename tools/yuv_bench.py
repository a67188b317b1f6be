"""Tools: time the raw YUV conversions on a 32 x 1080 x 1920 batch.  One JSON line.

  * `from_yuv` / `to_yuv` for yuv420p and nv12 with chroma 'nearest' and 'bilinear': time of the library call between HIP
    events (the staging copy over the bus and the kernel), the same copy alone (an upload / download of as many bytes), and
    the kernel ALONE, from the library's own event pair around its launch (ta_profile_*), as a multiple of the yardstick,
    `point_frames` on the same batch in the same run: one read and one write of the RGB batch.  from_yuv moves 4.5 bytes
    per pixel against point_frames' 6.
  * `RawVideoReader` frames per second from an in-memory stream as yuv420p against rgb24: upload plus conversion against
    upload alone.
  * `frames_to_yuv` against downloading the batch.
  * the CPU leg: the yuv420p -> RGB conversion restated in numpy (16-bit fixed point, nearest chroma), per frame on 16 threads.

    python tools/yuv_bench.py [--frames 32] [--reps 20]
"""
import argparse
import io
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from terran_amd import image, lib, runtime, synth, video      # noqa: E402


def med(x):
    return round(float(np.median(x)), 4)


def device_ms(ctx, a, call):
    t = []
    for rep in range(a.warmup + a.reps):
        ctx.timer_start()
        call()
        d = ctx.timer_stop()
        if rep >= a.warmup:
            t.append(d)
    return med(t), round(min(t), 4)


def kernel_ms(ctx, a, klass, call):
    """The event time of the one launch of profiling class `klass` inside call(): median and minimum."""
    t = []
    ctx.profile(True)
    try:
        for rep in range(a.warmup + a.reps):
            ctx.profile_reset()
            call()
            ms, launches, _ = ctx.profile_read(klass)
            assert launches == 1, launches
            if rep >= a.warmup:
                t.append(ms)
    finally:
        ctx.profile(False)
    return med(t), round(min(t), 4)


def wall_ms(a, call):
    t = []
    for rep in range(a.warmup + a.reps):
        t0 = time.perf_counter()
        call()
        t1 = time.perf_counter()
        if rep >= a.warmup:
            t.append((t1 - t0) * 1e3)
    return med(t)


def numpy_yuv420p_to_rgb(frame, h, w, out):
    """BT.709 tv range, nearest chroma, 16-bit fixed point: what a host without swscale would run."""
    ch, cw = (h + 1) >> 1, (w + 1) >> 1
    y = frame[:h * w].reshape(h, w).astype(np.int32) - 16
    u = frame[h * w:h * w + ch * cw].reshape(ch, cw).astype(np.int32) - 128
    v = frame[h * w + ch * cw:].reshape(ch, cw).astype(np.int32) - 128
    u, v = (np.repeat(np.repeat(c, 2, 0), 2, 1)[:h, :w] for c in (u, v))
    y = 76309 * y + 32768
    out[..., 0] = np.clip((y + 117489 * v) >> 16, 0, 255)
    out[..., 1] = np.clip((y - 13975 * u - 34925 * v) >> 16, 0, 255)
    out[..., 2] = np.clip((y + 138438 * u) >> 16, 0, 255)


def reader_fps(a, data, w, h, n, pix_fmt):
    rates = []
    for rep in range(a.reader_reps + 1):
        stream = io.BytesIO(data)
        t0 = time.perf_counter()
        frames = 0
        with video.RawVideoReader(stream, w, h, batch_size=n, pix_fmt=pix_fmt) as reader:
            for batch in reader:
                frames += len(batch)
                batch.free()
        t1 = time.perf_counter()
        if rep:                                                          # the first pass creates the context and its buffers
            rates.append(frames / (t1 - t0))
    return round(float(np.median(rates)), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=32)
    ap.add_argument('--height', type=int, default=1080)
    ap.add_argument('--width', type=int, default=1920)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reader-reps', type=int, default=3)
    ap.add_argument('--reader-batches', type=int, default=4)
    ap.add_argument('--cpu-reps', type=int, default=2)
    a = ap.parse_args()
    ctx = runtime.get_context(0)
    n, h, w = a.frames, a.height, a.width
    scene = np.zeros((n, h, w, 3), np.uint8)
    scene[:] = synth.frames(1, 1, h, w)[0]
    scene ^= np.random.default_rng(5).integers(0, 8, scene.shape, dtype=np.uint8)
    out = {'metric': 'raw YUV conversions per batch', 'frames': n, 'height': h, 'width': w, 'reps': a.reps}

    frames = ctx.upload(scene)
    ident = np.zeros(n, lib.POINT_DT)
    ident['frame'], ident['x1'], ident['y1'] = np.arange(n), w, h
    table = np.tile(image.brightness_lut(1.0), 3)[None]
    yard, yard_min = device_ms(ctx, a, lambda: frames.point(ident, table))
    out['point_whole_frames'] = {'device_ms': yard, 'device_ms_min': yard_min}

    per = image.yuv_frame_bytes('yuv420p', (w, h))
    pinned, pinned_ptr = ctx.pinned_array((n, per))
    same_bytes, same_ptr = ctx.pinned_array((n, per // (3 * w), w, 3)) if per % (3 * w) == 0 else (None, None)
    if same_bytes is not None:
        def copy_in():
            ctx.upload(same_bytes).free()
        out['h2d_of_a_yuv420p_batch'] = {'device_ms': device_ms(ctx, a, copy_in)[0]}
        part = ctx.upload(same_bytes)

        def copy_out():
            ctx.check(ctx.lib.ta_frames_download(part.h, lib.ptr(same_bytes)))
        out['d2h_of_a_yuv420p_batch'] = {'device_ms': device_ms(ctx, a, copy_out)[0]}
    for fmt in ('yuv420p', 'nv12'):
        pinned[...] = image.frames_to_yuv(frames, fmt)
        for chroma in ('nearest', 'bilinear'):
            spec = image.yuv_spec(fmt, chroma=chroma)

            def call():
                ctx.frames_from_yuv(pinned, n, h, w, spec).free()
            d, dmin = device_ms(ctx, a, call)
            r = {'device_ms': d, 'device_ms_min': dmin}
            r['kernel_ms'], r['kernel_ms_min'] = kernel_ms(ctx, a, 2, call)
            r['kernel_over_point'] = round(r['kernel_ms'] / yard, 2)
            r['kernel_GBps'] = round((n * per + n * h * w * 3) / (r['kernel_ms_min'] * 1e-3) / 1e9, 1)
            out['from_yuv_%s_%s' % (fmt, chroma)] = r
        spec = image.yuv_spec(fmt)
        d, dmin = device_ms(ctx, a, lambda: frames.to_yuv(spec, out=pinned))
        r = {'device_ms': d, 'device_ms_min': dmin}
        r['kernel_ms'], r['kernel_ms_min'] = kernel_ms(ctx, a, 3, lambda: frames.to_yuv(spec, out=pinned))
        r['kernel_over_point'] = round(r['kernel_ms'] / yard, 2)
        r['kernel_GBps'] = round((n * per + n * h * w * 3) / (r['kernel_ms_min'] * 1e-3) / 1e9, 1)
        out['to_yuv_%s' % fmt] = r

    # the way out: the batch as yuv420p against the batch as it is
    host = np.empty(scene.shape, np.uint8)
    out['frames_to_yuv_wall_ms'] = wall_ms(a, lambda: image.frames_to_yuv(frames, 'yuv420p'))
    out['download_wall_ms'] = wall_ms(a, lambda: ctx.check(ctx.lib.ta_frames_download(frames.h, lib.ptr(host))))

    # the way in: the reader over an in-memory stream
    yuv = image.frames_to_yuv(frames, 'yuv420p')
    out['reader_fps_yuv420p'] = reader_fps(a, yuv.tobytes() * a.reader_batches, w, h, n, 'yuv420p')
    out['reader_fps_rgb24'] = reader_fps(a, scene.tobytes() * a.reader_batches, w, h, n, 'rgb24')

    # the CPU leg
    rgb = np.empty(scene.shape, np.uint8)
    with ThreadPoolExecutor(16) as pool:
        t = []
        for rep in range(a.cpu_reps):
            t0 = time.perf_counter()
            list(pool.map(lambda f: numpy_yuv420p_to_rgb(yuv[f], h, w, rgb[f]), range(n)))
            t.append((time.perf_counter() - t0) * 1e3)
    out['numpy_16_threads_from_yuv420p_wall_ms'] = med(t)

    ctx.free_pinned(pinned_ptr)
    if same_ptr is not None:
        ctx.free_pinned(same_ptr)
    frames.free()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
