"""Host layer of tiled (sliced) detection: where the tiles of a frame lie, and the `ta_merge_group` records that tell
`ta_detections_merge` how each tile's detections map back into its frame.

A frame is cut into overlapping tiles at its own resolution (or zoomed in), the detector runs on every tile, and the
detections are mapped back and suppressed across tiles.  The cutting (`ta_frames_tiles`) and the merge run on the device;
`RetinaFace.detect_tiles` and `facade.TiledDetection` tie them together.  Nothing here touches the device.
"""
import math

import numpy as np

from . import lib


def _pair(v, what):
    if isinstance(v, (tuple, list, np.ndarray)):
        if len(v) != 2:
            raise ValueError('`%s` must be one number or a pair (for the height, for the width)' % what)
        return v[0], v[1]
    return v, v


def tile_shape(height, width, tile):
    """(th, tw): `tile` (an int or (th, tw)) clamped to the frame."""
    th, tw = _pair(tile, 'tile')
    if int(th) != th or int(tw) != tw or th < 1 or tw < 1:
        raise ValueError('`tile` must be a positive int or a pair of them, not %r' % (tile,))
    if height < 1 or width < 1:
        raise ValueError('a frame of %d x %d has no tiles' % (width, height))
    return min(int(th), int(height)), min(int(tw), int(width))


def overlap_pixels(tile, overlap):
    """(oy, ox) in pixels: an int `overlap` is pixels, a float below 1 a fraction of the (unclamped) tile side.  It must be
    below the tile side."""
    out = []
    for side, ov in zip(_pair(tile, 'tile'), _pair(overlap, 'overlap')):
        if isinstance(ov, (float, np.floating)) and not float(ov).is_integer():
            if not 0 <= ov < 1:
                raise ValueError('`overlap` as a fraction must lie in [0, 1), not %r' % (ov,))
            px = int(round(float(ov) * int(side)))
        else:
            px = int(ov)
        if px < 0 or px >= int(side):
            raise ValueError('`overlap` (%d pixels) must be at least 0 and below the tile side (%d)' % (px, int(side)))
        out.append(px)
    return out[0], out[1]


def _axis(length, t, overlap):
    """Origins along one axis: 0, s, 2s, ... while origin + t < length, then length - t (moved inward, never padded)."""
    step = t - overlap
    out = []
    o = 0
    while o + t < length:
        out.append(o)
        o += step
    if not out or out[-1] != length - t:
        out.append(length - t)
    return out


def tile_grid(height, width, tile, overlap):
    """(n, 2) int32 (y, x) origins of the tiles of a height x width frame, row-major."""
    oy, ox = overlap_pixels(tile, overlap)
    th, tw = tile_shape(height, width, tile)
    ys, xs = _axis(int(height), th, min(oy, th - 1)), _axis(int(width), tw, min(ox, tw - 1))
    return np.array([(y, x) for y in ys for x in xs], np.int32).reshape(-1, 2)


def check_args(tile, overlap, zoom=1.0, metric='iou', edge=0.0, max_tiles=256):
    """The checks `detect_tiles` and `TiledDetection` share: ValueError naming the argument.  -> lib.MERGE_* of `metric`."""
    th, tw = _pair(tile, 'tile')
    if int(th) != th or int(tw) != tw or th < 1 or tw < 1:
        raise ValueError('`tile` must be a positive int or a pair of them, not %r' % (tile,))
    overlap_pixels(tile, overlap)
    if not (isinstance(zoom, (int, float, np.integer, np.floating)) and math.isfinite(zoom) and zoom > 0):
        raise ValueError('`zoom` must be a positive number, not %r' % (zoom,))
    if metric not in lib.MERGE_METRICS:
        raise ValueError('`metric` must be one of %s, not %r' % (sorted(lib.MERGE_METRICS), metric))
    if not (math.isfinite(edge) and edge >= 0):
        raise ValueError('`edge` must be at least 0, not %r' % (edge,))
    if int(max_tiles) < 1:
        raise ValueError('`max_tiles` must be at least 1, not %r' % (max_tiles,))
    return lib.MERGE_METRICS[metric]


def tile_records(n_frames, origins):
    """The TILE_DT array of every frame's tiles, frame-major: the order `merge_groups` expects the tile counts in."""
    origins = np.asarray(origins, np.int32).reshape(-1, 2)
    t = np.zeros(n_frames * len(origins), lib.TILE_DT)
    t['frame'] = np.repeat(np.arange(n_frames, dtype=np.int32), len(origins))
    t['y'] = np.tile(origins[:, 0], n_frames)
    t['x'] = np.tile(origins[:, 1], n_frames)
    return t


def merge_groups(n_frames, height, width, origins, th, tw, zoom, tile_counts, full_counts=None, full_scale=None):
    """The MERGE_GROUP_DT records of a batch of `n_frames` frames of height x width.

    The candidate arrays hold the detections of every tile, frame-major (frame 0's tiles in `origins` order, frame 1's,
    ...: `tile_counts` per tile), each detected on the tile resized by `zoom`; then, if `full_counts` is given, those of a
    whole-frame pass (`full_counts` per frame) detected on the frame resized by `full_scale`.  A tile's rectangle is its
    own, and a side of it is interior when it does not lie on the frame's border; a whole-frame pass is one more group per
    frame with no interior side, origin 0 and its scale as the zoom.  The records come sorted by frame."""
    origins = np.asarray(origins, np.int32).reshape(-1, 2)
    nt = len(origins)
    tile_counts = np.asarray(tile_counts, np.int64).reshape(-1)
    if len(tile_counts) != n_frames * nt:
        raise ValueError('merge_groups: %d tile counts for %d frames of %d tiles' % (len(tile_counts), n_frames, nt))
    per = nt + (full_counts is not None)
    g = np.zeros((n_frames, per), lib.MERGE_GROUP_DT)
    g['frame'] = np.arange(n_frames, dtype=np.int32)[:, None]
    first = np.concatenate([[0], np.cumsum(tile_counts)])
    t = g[:, :nt]
    t['first'] = first[:-1].reshape(n_frames, nt)
    t['count'] = tile_counts.reshape(n_frames, nt)
    y, x = origins[:, 0][None], origins[:, 1][None]
    t['ox'], t['oy'], t['zoom'] = x, y, zoom
    t['x0'], t['y0'], t['x1'], t['y1'] = x, y, x + tw, y + th
    t['interior'] = (x > 0) * 1 + (y > 0) * 2 + (x + tw < width) * 4 + (y + th < height) * 8
    if full_counts is not None:
        full_counts = np.asarray(full_counts, np.int64).reshape(-1)
        if len(full_counts) != n_frames or full_scale is None:
            raise ValueError('merge_groups: the whole-frame pass needs one count per frame and its scale')
        w = g[:, nt]
        w['first'] = first[-1] + np.concatenate([[0], np.cumsum(full_counts)])[:-1]
        w['count'] = full_counts
        w['zoom'] = full_scale
        w['x1'], w['y1'] = width, height
    return g.reshape(-1)


def check_pose_args(tile, overlap, zoom=1.0, edge=0, radius=0.1, agree=0.5, min_shared=3, max_tiles=32):
    """The checks `estimate_tiles` and `TiledEstimation` share: ValueError naming the argument."""
    th, tw = _pair(tile, 'tile')
    if int(th) != th or int(tw) != tw or th < 1 or tw < 1:
        raise ValueError('`tile` must be a positive int or a pair of them, not %r' % (tile,))
    overlap_pixels(tile, overlap)
    if not (isinstance(zoom, (int, float, np.integer, np.floating)) and math.isfinite(zoom) and zoom > 0):
        raise ValueError('`zoom` must be a positive number, not %r' % (zoom,))
    if not (isinstance(edge, (int, np.integer)) and not isinstance(edge, bool) and edge >= 0):
        raise ValueError('`edge` must be an int of at least 0 (pixels), not %r' % (edge,))
    if not (isinstance(radius, (int, float, np.integer, np.floating)) and math.isfinite(radius) and radius >= 0):
        raise ValueError('`radius` must be a finite number of at least 0, not %r' % (radius,))
    if not (isinstance(agree, (int, float, np.integer, np.floating)) and 0 < agree <= 1):
        raise ValueError('`agree` must lie in (0, 1], not %r' % (agree,))
    if not (isinstance(min_shared, (int, np.integer)) and not isinstance(min_shared, bool) and 1 <= min_shared <= 18):
        raise ValueError('`min_shared` must be an int in 1 .. 18, not %r' % (min_shared,))
    if int(max_tiles) < 1:
        raise ValueError('`max_tiles` must be at least 1, not %r' % (max_tiles,))


def pose_groups(n_frames, height, width, origins, th, tw, tile_counts, full_counts=None):
    """The POSE_GROUP_DT records of a batch of `n_frames` frames of height x width: `merge_groups` in integers.

    The candidate arrays hold the poses of every tile, frame-major (frame 0's tiles in `origins` order, frame 1's, ...:
    `tile_counts` per tile), in the coordinates of the un-zoomed tile (`ta_openpose_run` divides by its scale); then, if
    `full_counts` is given, those of a whole-frame pass (`full_counts` per frame), already in frame coordinates.  A tile's
    rectangle is its own, and a side of it is interior when it does not lie on the frame's border; a whole-frame pass is
    one more group per frame with origin 0, the rectangle (0, 0, width, height) and no interior side.  The records come
    sorted by frame."""
    origins = np.asarray(origins, np.int32).reshape(-1, 2)
    nt = len(origins)
    tile_counts = np.asarray(tile_counts, np.int64).reshape(-1)
    if len(tile_counts) != n_frames * nt:
        raise ValueError('pose_groups: %d tile counts for %d frames of %d tiles' % (len(tile_counts), n_frames, nt))
    per = nt + (full_counts is not None)
    g = np.zeros((n_frames, per), lib.POSE_GROUP_DT)
    g['frame'] = np.arange(n_frames, dtype=np.int32)[:, None]
    first = np.concatenate([[0], np.cumsum(tile_counts)])
    t = g[:, :nt]
    t['first'] = first[:-1].reshape(n_frames, nt)
    t['count'] = tile_counts.reshape(n_frames, nt)
    y, x = origins[:, 0][None], origins[:, 1][None]
    t['ox'], t['oy'] = x, y
    t['x0'], t['y0'], t['x1'], t['y1'] = x, y, x + tw, y + th
    t['interior'] = (x > 0) * 1 + (y > 0) * 2 + (x + tw < width) * 4 + (y + th < height) * 8
    if full_counts is not None:
        full_counts = np.asarray(full_counts, np.int64).reshape(-1)
        if len(full_counts) != n_frames:
            raise ValueError('pose_groups: the whole-frame pass needs one count per frame')
        w = g[:, nt]
        w['first'] = first[-1] + np.concatenate([[0], np.cumsum(full_counts)])[:-1]
        w['count'] = full_counts
        w['x1'], w['y1'] = width, height
    return g.reshape(-1)
