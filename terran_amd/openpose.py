"""`OpenPose` -- drop-in for terran/pose/openpose/wrapper.py:166-485 on MI355X."""
import ctypes as C

import numpy as np

from . import lib, pack, runtime


class PoseOverflow(RuntimeError):
    """Kept for callers that catch it: the library no longer caps the grouping lists (an image that outgrows the LDS
    fast path is recomputed with lists in global memory, include/terran_amd.h: ta_openpose_run), so a per-image count
    of -1 -- what this exception reported, `results` holding `None` at the positions in `images` -- cannot come back."""

    def __init__(self, message, results, images):
        super().__init__(message)
        self.results = results
        self.images = images


def _unpack(counts, kp, sc):
    out, o = [], 0
    for c in counts:
        if c < 0:                                   # over a cap: no rows for this image
            out.append(None)
            continue
        out.append([{'keypoints': kp[i].copy(), 'score': np.float64(sc[i])} for i in range(o, o + int(c))])
        o += int(c)
    return out


def _run_arrays(ctx, fn, n):
    """-> (counts (n,) int32, keypoints (T, 18, 3) int32, scores (T,) float64), the capacity grown until the call fits."""
    counts = np.zeros(max(n, 1), np.int32)
    cap = max(64, 16 * n)
    while True:
        kp = np.empty((cap, 18, 3), np.int32)
        sc = np.empty(cap, np.float64)
        req = C.c_int32(0)
        rc = fn(cap, lib.ptr(counts), lib.ptr(kp), lib.ptr(sc), C.byref(req))
        if rc == lib.E_CAPACITY:
            cap = int(req.value)
            continue
        ctx.check(rc)
        return counts[:n], kp, sc


def _run(ctx, fn, n):
    counts, kp, sc = _run_arrays(ctx, fn, n)
    out = _unpack(counts, kp, sc)
    over = [i for i, r in enumerate(out) if r is None]
    if over:
        raise PoseOverflow(ctx.last_error() + '; images %s' % over, out, over)
    return out


class OpenPose(runtime.RangeFallback):

    def __init__(self, device=None, short_side=184, state=None, ctx=None, precision=None):
        self.device = device
        self.precision = runtime.resolve_precision(precision)
        self.short_side = short_side
        self.ctx = ctx if ctx is not None else runtime.get_context(device)     # ctx: an extra stream on the same GPU
        self.model = lib.Model(self.ctx, runtime.packed_program('openpose', state, self.precision))
        self._init_fallback('openpose', state)

    def call_frames(self, frames):
        """frames: lib.Frames at ORIGINAL resolution; resized on the device to `short_side`."""
        n, H, W = frames.shape[:3]
        if n == 0:
            return []
        scale = self.short_side / min(H, W)
        nw, nh = int(W * scale), int(H * scale)                  # openpose/wrapper.py:95-99
        resized = frames if (nh, nw) == (H, W) else frames.resize(nh, nw, ctx=self.ctx)
        try:
            return self._with_fallback(lambda model: _run(self.ctx, lambda cap, *a: self.ctx.lib.ta_openpose_run(
                model.h, resized.h, float(scale), cap, *a), n))
        finally:
            if resized is not frames:
                resized.free()

    def _estimate_arrays(self, frames, scale):
        """One `ta_openpose_run` on resident frames at network resolution -> (counts, keypoints, scores) trimmed to the poses
        found; TA_E_RANGE falls back as in `call_frames`."""
        n = frames.shape[0]
        counts, kp, sc = self._with_fallback(lambda model: _run_arrays(self.ctx, lambda cap, *a: self.ctx.lib.ta_openpose_run(
            model.h, frames.h, float(scale), cap, *a), n))
        if (counts < 0).any():
            raise PoseOverflow(self.ctx.last_error(), None, np.nonzero(counts < 0)[0].tolist())
        t = int(counts.sum())
        return counts.copy(), kp[:t], sc[:t]

    def estimate_tiles(self, frames, tile, overlap, zoom=1.0, full_frame_short_side=None, edge=0, radius=0.1, agree=0.5, min_shared=3,
                       max_tiles=32):
        """Sliced inference on resident `frames` (lib.Frames, one size): every frame is cut into overlapping tiles
        (`tiles.tile_grid`), at most `max_tiles` at a time; each chunk is resized to (int(th * zoom), int(tw * zoom)) when that
        differs from the tile and goes through `ta_openpose_run` with scale = zoom, which answers in the un-zoomed tile's
        pixels; optionally one pass over the whole frames is made exactly as `call_frames` makes it, at
        `full_frame_short_side`; one `ta_poses_merge` then maps every pose into its frame, drops the bodies a tile cut
        (`edge`) and suppresses the duplicates across tiles (`radius`, `agree`, `min_shared`: include/terran_amd.h).
        -> (counts (N,) int32, keypoints (T, 18, 3) int32, scores (T,) float64) in frame coordinates, frames concatenated.
        `max_tiles` = 32 is a guess at what the activation arena takes comfortably; it is not measured."""
        from . import tiles as tl
        tl.check_pose_args(tile, overlap, zoom, edge, radius, agree, min_shared, max_tiles)
        ctx = self.ctx
        n, H, W = frames.shape[:3]
        if n == 0:
            return np.zeros(0, np.int32), np.empty((0, 18, 3), np.int32), np.empty(0, np.float64)
        th, tw = tl.tile_shape(H, W, tile)
        origins = tl.tile_grid(H, W, tile, overlap)
        recs = tl.tile_records(n, origins)
        zh, zw = int(th * zoom), int(tw * zoom)
        if zh < 1 or zw < 1:
            raise ValueError('`zoom` %r leaves nothing of a %d x %d tile' % (zoom, tw, th))
        parts = []
        for lo in range(0, len(recs), int(max_tiles)):
            cut = ctx.frames_tiles(frames, recs[lo:lo + int(max_tiles)], th, tw)
            big = None
            try:
                if (zh, zw) != (th, tw):
                    big = cut.resize(zh, zw, ctx=ctx)
                parts.append(self._estimate_arrays(big if big is not None else cut, zoom))
            finally:
                cut.free()
                if big is not None:
                    big.free()
        tile_counts = np.concatenate([p[0] for p in parts])
        full_counts = None
        if full_frame_short_side is not None:
            scale = full_frame_short_side / min(H, W)
            nw, nh = int(W * scale), int(H * scale)
            whole = frames if (nh, nw) == (H, W) else frames.resize(nh, nw, ctx=ctx)
            try:
                parts.append(self._estimate_arrays(whole, scale))
            finally:
                if whole is not frames:
                    whole.free()
            full_counts = parts[-1][0]
        groups = tl.pose_groups(n, H, W, origins, th, tw, tile_counts, full_counts)
        kp, sc = np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts])
        return ctx.poses_merge(groups, n, kp, sc, radius, agree, min_shared, edge)[:3]

    def call(self, images):
        """images: (N,H,W,3) uint8 RGB -> list[N] of list[{'keypoints': int32 (18,3), 'score': float64}],
        keypoints (x, y, present) in the coordinates of `images`."""
        frames = self.ctx.upload(np.asarray(images))
        try:
            return self.call_frames(frames)
        finally:
            frames.free()


def group(ctx, pafs, heatmaps, scale=1.0):
    """Debug/parity entry: grouping only, on network-resolution maps (N,38,h,w), (N,19,h,w)."""
    pafs = np.ascontiguousarray(pafs, dtype=np.float32)
    heatmaps = np.ascontiguousarray(heatmaps, dtype=np.float32)
    n, _, h, w = pafs.shape
    return _run(ctx, lambda cap, *a: ctx.lib.ta_openpose_group(ctx.h, lib.ptr(pafs), lib.ptr(heatmaps), n, h, w,
                                                               float(scale), cap, *a), n)
