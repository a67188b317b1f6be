"""Image files in: the reference's `terran.io.open_image`, and JPEG decoding into resident frames on the GPU.

`open_image(uri)` keeps the reference's signature and return value (terran/io/image.py:17-52): a host uint8 (H, W, 3)
RGB array, Pillow's `Image.open(f).convert('RGB')`, for a path or `pathlib.Path` (URLs are not fetched).

`open_images(items)` / `decode_jpeg(buffers)` return RESIDENT frames for the facades (`Detection`, `Recognition`,
`Estimation` take a `lib.Frames` batch or a list of single-frame ones): one (n, H, W, 3) `lib.Frames` when every image has
the same size (an MJPEG or burst batch), else a list of (1, H_i, W_i, 3) `lib.Frames`, in input order.  Baseline JPEGs
are decoded by `ta_jpeg_decode` -- Huffman on up to 16 host threads, dequantisation, IDCT, upsampling and colour on the
device -- with the pixels of `open_image` bit for bit.  Every other JPEG (progressive, CMYK, ...) and every other format
(PNG, ...) is decoded by Pillow and uploaded, so these calls accept what `open_image` accepts.  Each returned batch
carries `decode_paths`: per image lib.JPEG_DEVICE (0) or the reason it took Pillow (a TA_JPEG_FALLBACK_* code;
lib.JPEG_INVALID (-1) for a JPEG the library's strict decoder refused -- libjpeg accepts some such files with a warning,
and Pillow then decodes it or raises as `open_image` would; NOT_JPEG (-2) for another format).  Pillow is imported only
when such an image comes along.  No EXIF orientation is applied (the reference applies none).

Out: `encode_jpeg(images, quality, subsampling)` encodes resident batches (or host arrays, uploaded first) on the GPU
(`ta_jpeg_encode`) into JPEG files that are byte for byte what Pillow's `Image.fromarray(frame).save(f, 'JPEG',
quality=quality, subsampling=subsampling)` writes; only the compressed bytes leave the device.  `save_images` writes
them to files.  Pillow's argument semantics: quality 1..100 (default 75), subsampling -1 (default: 4:2:0), 0 / '4:4:4',
1 / '4:2:2', 2 / '4:2:0'; optimize=True codes every image with Huffman tables built from its own statistics
(`ta_jpeg_encode_opt`: smaller files, the same pixels), again Pillow's bytes.  Other options (progressive, qtables, dpi,
exif, ...) are not offered.

`resize_frames(frames, size, resample, box)` resizes resident batches on the GPU (`ta_frames_resample`) with the pixels of
Pillow's `Image.resize(size, resample, box=box)` bit for bit, for every Pillow filter, and always returns ONE batch, so a
mixed-size list from `open_images` becomes a batch of a common size (for `encode_jpeg`, a video writer, a network).

`transform_frames`, `transpose_frames` and `rotate_frames` are Pillow's `Image.transform` (AFFINE, PERSPECTIVE),
`Image.transpose` and `Image.rotate` on resident batches (`ta_frames_transform`, `ta_frames_transpose`), bit for bit:
sideways video turned upright, a tilted camera de-rotated, a screen or a sign perspective-corrected, without a download.
`mesh_frames`, `quad_frames` and `extent_frames` are the other three methods of `Image.transform` -- MESH (which is
`ImageOps.deform`), QUAD and EXTENT -- the first two on `ta_frames_transform_mesh`, bit for bit; `undistort_cells` /
`undistort_mesh` build the mesh that removes a lens's Brown-Conrady distortion and `undistort_frames` warps resident frames
through it.

Pixel values: `histogram_frames` / `frame_stats` are Pillow's `Image.histogram` and `ImageStat.Stat` of resident frames
(`ta_frames_histogram`; only the counts leave the device), and `point_frames`, `equalize_frames`, `autocontrast_frames`,
`brightness_frames`, `contrast_frames`, `color_frames`, `grayscale_frames`, `invert_frames`, `posterize_frames` and
`solarize_frames` change resident frames in place with the pixels of `Image.point`, `ImageOps` and `ImageEnhance`, bit
for bit (`ta_frames_point`, `ta_frames_saturate`): at most one histogram call, tables built on the host by the `*_lut`
functions (usable without a device), and one in-place call per batch.

Two batches: `paste_frames`, `composite_frames`, `blend_frames`, `chop_frames` / `difference_frames` and `copy_frames` are
Pillow's `Image.paste`, `Image.composite`, `Image.blend` and the two-image `ImageChops` functions between resident frames
(`ta_frames_combine`), in place and bit for bit; `pack_combine` builds their records without a device.

Colour: `convert_frames` ('YCbCr', 'HSV' and back, or 'RGB' with a matrix), `matrix_frames`, `color_lut_frames`
(`ImageFilter.Color3DLUT`) and `hue_frames` are Pillow's `Image.convert` and 3-D table filter on resident frames
(`ta_frames_color`), in place and bit for bit; `color_spec` builds their op records without a device.  A batch has no
mode: after a conversion its three bytes per pixel are Y, Cb, Cr or H, S, V, and the caller keeps track of that.

Raw video: `frames_from_yuv` / `frames_to_yuv` convert between raw `yuv420p`, `nv12` or `yuv444p` frames (ffmpeg's
`-f rawvideo` layout) and resident RGB batches on the GPU (`ta_frames_from_yuv`, `ta_frames_to_yuv`).  The conversion is
the standards' affine map (BT.601 or BT.709, tv or pc range) with exact rational coefficients, rounded once, half up;
it is NOT bit for bit what ffmpeg's swscale computes, and no such parity is claimed.  `yuv_spec` and `yuv_frame_bytes`
work without a device.
"""
import os
from pathlib import Path
from urllib.parse import urlparse

import numpy as np

from . import lib, runtime

NOT_JPEG = -2                    # decode_paths of a file that is not a JPEG (lib.JPEG_INVALID = -1: a JPEG the library
                                 # refused as malformed, decoded by Pillow)


def _pillow_rgb(source):
    """The reference's decode: Pillow, convert('RGB'), grayscale stacked to 3 channels.  `source`: path or file object."""
    from PIL import Image                     # optional dependency: only the fallback needs it
    image = np.asarray(Image.open(source).convert('RGB'))
    if len(image.shape) == 2:
        image = np.stack([image] * 3, axis=-1)
    return image


def _path(uri):
    if isinstance(uri, Path):
        return uri
    if urlparse(str(uri)).scheme and not os.path.exists(str(uri)):
        raise ValueError('terran_amd.image does not fetch URLs: %r' % (uri,))
    return Path(uri).expanduser()


def open_image(uri):
    """terran.io.open_image: the image at `uri` (str or pathlib.Path) as an (H, W, 3) uint8 RGB ndarray."""
    return _pillow_rgb(_path(uri))


def _read(item):
    if isinstance(item, (bytes, bytearray, memoryview)):
        return bytes(item)
    with open(_path(item), 'rb') as fh:
        return fh.read()


def _is_jpeg(data):
    return len(data) >= 2 and data[0] == 0xFF and data[1] == 0xD8


def decode_jpeg(buffers, ctx=None, threads=0):
    """JPEG byte strings -> resident frames (see the module doc); `threads`: host threads for the Huffman decode
    (0 = min(n, 16))."""
    return open_images(list(buffers), ctx=ctx, threads=threads)


def open_images(uris_or_bytes, device=None, ctx=None, threads=0):
    """Paths, `pathlib.Path`s or encoded bytes -> one resident `lib.Frames` (all images of one size) or a list of
    single-image `lib.Frames` (mixed sizes), in input order."""
    ctx = ctx if ctx is not None else runtime.get_context(device)
    datas = [_read(x) for x in uris_or_bytes]
    n = len(datas)
    if n == 0:
        raise ValueError('open_images: no images')
    paths = np.full(n, NOT_JPEG, np.int32)
    jpeg_idx = [i for i, d in enumerate(datas) if _is_jpeg(d)]
    host = {i: _pillow_rgb(_BytesIO(d)) for i, d in enumerate(datas) if not _is_jpeg(d)}   # other formats: Pillow
    outs, jp, jpeg_idx = _decode_jpegs(ctx, datas, jpeg_idx, threads, paths)
    for i in np.nonzero(paths == lib.JPEG_INVALID)[0]:
        # refused by the library's strict decoder (libjpeg only warns about e.g. a missing restart marker): Pillow
        # decodes it or raises, exactly as open_image would
        try:
            host[int(i)] = _pillow_rgb(_BytesIO(datas[i]))
        except Exception:
            _free(outs)
            raise
    if not host:
        # the common case: every image went to the library -- it shaped the output; fallback images are filled in place
        try:
            for k in np.nonzero(jp != lib.JPEG_DEVICE)[0]:
                dst, slot = (outs[0], int(k)) if len(outs) == 1 else (outs[int(k)], 0)
                _paste_host(ctx, _pillow_rgb(_BytesIO(datas[jpeg_idx[k]])), dst, slot)
        except Exception:
            _free(outs)
            raise
        return _tag(outs, paths)
    # some images came from Pillow: lay every image out anew
    dev = {i: ((outs[0], k) if len(outs) == 1 else (outs[k], 0)) for k, i in enumerate(jpeg_idx)}
    result = []
    try:
        shapes = [host[i].shape[:2] if i in host else dev[i][0].shape[1:3] for i in range(n)]
        same = all(s == shapes[0] for s in shapes)
        if same:
            result.append(lib.Frames.zeros(ctx, n, *shapes[0]))
        else:
            for s in shapes:
                result.append(lib.Frames.zeros(ctx, 1, *s))
        for i in range(n):
            dst, k = (result[0], i) if same else (result[i], 0)
            if i in host:
                _paste_host(ctx, host[i], dst, k)
            elif paths[i] != lib.JPEG_DEVICE:
                _paste_host(ctx, _pillow_rgb(_BytesIO(datas[i])), dst, k)
            else:
                dst.paste(dev[i][0], dev[i][1], k, 0, 0)
    except Exception:
        _free(result)
        raise
    finally:
        _free(outs)
    return _tag(result, paths)


def _decode_jpegs(ctx, datas, idx, threads, paths):
    """ta_jpeg_decode over datas[idx] -> (frames, per-image paths, the indices decoded).  Images the library refuses as
    malformed are marked JPEG_INVALID in `paths` and the others decoded again without them."""
    if not idx:
        return [], np.zeros(0, np.int32), []
    try:
        outs, jp = ctx.jpeg_decode([datas[i] for i in idx], threads)
    except lib.TerranAmdError as e:
        bad = getattr(e, 'paths', None)
        if e.code != lib.E_INVALID or bad is None or not (bad == lib.JPEG_INVALID).any():
            raise
        for k in np.nonzero(bad == lib.JPEG_INVALID)[0]:
            paths[idx[k]] = lib.JPEG_INVALID
        idx = [i for k, i in enumerate(idx) if bad[k] != lib.JPEG_INVALID]
        if not idx:
            return [], np.zeros(0, np.int32), []
        outs, jp = ctx.jpeg_decode([datas[i] for i in idx], threads)
    paths[idx] = jp
    return outs, jp, idx


def _free(frames):
    for f in frames:
        f.free()


def _BytesIO(data):
    import io
    return io.BytesIO(data)


def _paste_host(ctx, pixels, dst, index):
    src = ctx.upload(pixels[None])
    try:
        dst.paste(src, 0, index, 0, 0)
    finally:
        src.free()


def _tag(frames, paths):
    if len(frames) == 1 and frames[0].shape[0] == len(paths):
        frames[0].decode_paths = paths
        return frames[0]
    for f, p in zip(frames, paths):
        f.decode_paths = np.array([p], np.int32)
    return frames


def resize_frames(frames, size, resample='bicubic', box=None, ctx=None):
    """Resident frames resized -> one NEW resident `lib.Frames` (sum(n), height, width, 3), images in input order, each
    Pillow's `Image.fromarray(frame).resize(size, resample, box=box)`.  `frames`: a `lib.Frames` batch or a list of them
    (as `open_images` returns for mixed sizes); `size`: (width, height), as in Pillow; `resample`: 'nearest', 'box',
    'bilinear', 'hamming', 'bicubic', 'lanczos' or Pillow's integer code; `box`: Pillow's (x0, y0, x1, y1) source
    rectangle, fractional, applied to every frame (None: the whole frame).  `ctx`: the context the work runs on and the
    result belongs to (default: the first batch's own).  Every argument is checked before anything is launched."""
    who = 'resize_frames'
    batches, _ = _batches(frames, who)
    code = lib.resample_filter(resample)
    width, height = _size(size, who)
    if box is not None:
        box = tuple(float(np.float32(v)) for v in box)          # Pillow reads the box as float32
        if len(box) != 4:
            raise ValueError('resize_frames: box must be (x0, y0, x1, y1), got %r' % (box,))
    total = sum(b.shape[0] for b in batches)
    if total == 0:
        raise ValueError('resize_frames: no images')
    for b in batches:
        h, w = b.shape[1:3]
        x0, y0, x1, y1 = box if box is not None else (0.0, 0.0, float(w), float(h))
        if not (0 <= x0 < x1 <= w and 0 <= y0 < y1 <= h):
            raise ValueError('resize_frames: box %r must satisfy 0 <= x0 < x1 <= %d and 0 <= y0 < y1 <= %d' % (box, w, h))
    ctx = ctx if ctx is not None else batches[0].ctx
    parts = []
    for b in batches:
        n, h, w = b.shape[:3]
        if not n:
            continue
        regions = np.zeros(n, lib.RESAMPLE_DT)
        regions['frame'] = np.arange(n)
        regions['x0'], regions['y0'], regions['x1'], regions['y1'] = box if box is not None else (0, 0, w, h)
        parts.append(b.resample(regions, height, width, code, ctx=ctx))
    return _one_batch(ctx, parts, height, width)


def _one_batch(ctx, parts, height, width):
    """Batches of one size -> one batch with their images in order (the parts are freed); a single part is returned as it is."""
    if len(parts) == 1:
        return parts[0]
    try:
        out = lib.Frames.zeros(ctx, sum(p.shape[0] for p in parts), height, width)
        at = 0
        for p in parts:
            for k in range(p.shape[0]):
                out.paste(p, k, at, 0, 0)
                at += 1
        ctx.sync()
    finally:
        _free(parts)
    return out


def _batches(frames, who):
    if isinstance(frames, lib.Frames):
        return [frames], False
    if isinstance(frames, (list, tuple)) and frames and all(isinstance(b, lib.Frames) for b in frames):
        return list(frames), True
    raise ValueError('%s: a lib.Frames batch or a non-empty list of them' % who)


def _size(size, who):
    try:
        width, height = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError('%s: size must be (width, height), got %r' % (who, size)) from None
    if not (1 <= width <= lib.RESAMPLE_SIDE_LIMIT and 1 <= height <= lib.RESAMPLE_SIDE_LIMIT):
        raise ValueError('%s: size must be within 1 .. %d a side, got %r' % (who, lib.RESAMPLE_SIDE_LIMIT, size))
    return width, height


def _transform_filter(resample, who):
    code = lib.resample_filter(resample)
    if code not in lib.TRANSFORM_FILTERS:
        raise ValueError("%s: resample must be 'nearest', 'bilinear' or 'bicubic' (Pillow offers no other here), got %r" % (who, resample))
    return code


def _fillcolor(fillcolor, who):
    if fillcolor is None:
        return None
    try:
        rgb = [int(v) for v in fillcolor]
    except (TypeError, ValueError):
        rgb = []
    if len(rgb) != 3 or not all(0 <= v <= 255 for v in rgb):
        raise ValueError('%s: fillcolor must be None or three values 0 .. 255, got %r' % (who, fillcolor))
    return tuple(rgb)


def transform_frames(frames, size, method, data, resample='nearest', fillcolor=None, ctx=None):
    """Resident frames warped -> one NEW resident `lib.Frames` (sum(n), height, width, 3), images in input order, each
    Pillow's `Image.fromarray(frame).transform(size, method, data, resample=resample, fillcolor=fillcolor)` bit for bit
    (`ta_frames_transform`).  `frames`: a `lib.Frames` batch or a list of them (as `open_images` returns for mixed sizes);
    `size`: (width, height); `method`: 'affine' / 'perspective' or Pillow's Image.AFFINE / Image.PERSPECTIVE; `data`:
    Pillow's 6 (affine) or 8 (perspective) coefficients, OUTPUT to INPUT coordinates, one tuple for all frames or one per
    frame; `resample`: 'nearest', 'bilinear', 'bicubic' or Pillow's code; `fillcolor`: None (zeros) or (r, g, b).  `ctx`: the
    context the work runs on and the result belongs to (default: the first batch's own).  Every argument is checked before
    anything is launched."""
    who = 'transform_frames'
    batches, _ = _batches(frames, who)
    width, height = _size(size, who)
    code = _transform_filter(resample, who)
    fill = _fillcolor(fillcolor, who)
    if isinstance(method, str) and method.lower() in lib.TRANSFORM_METHODS:
        method = lib.TRANSFORM_METHODS[method.lower()]
    if isinstance(method, bool) or not isinstance(method, (int, np.integer)) or int(method) not in (lib.AFFINE, lib.PERSPECTIVE):
        raise ValueError("%s: method must be 'affine' (0) or 'perspective' (2), got %r" % (who, method))
    method = int(method)
    count = 6 if method == lib.AFFINE else 8
    total = sum(b.shape[0] for b in batches)
    if total == 0:
        raise ValueError('%s: no images' % who)
    try:
        coef = np.asarray(data, np.float64)
    except (TypeError, ValueError):
        coef = np.zeros(0)
    if coef.ndim == 1 and coef.shape[0] == count:
        coef = np.broadcast_to(coef, (total, count))
    elif coef.shape != (total, count):
        raise ValueError('%s: data must be %d coefficients, or %d of them for each of the %d frames' % (who, count, count, total))
    if not np.isfinite(coef).all():
        raise ValueError('%s: data must be finite' % who)
    ctx = ctx if ctx is not None else batches[0].ctx
    parts, at = [], 0
    for b in batches:
        n = b.shape[0]
        if not n:
            continue
        regions = np.zeros(n, lib.TRANSFORM_DT)
        regions['frame'], regions['method'] = np.arange(n), method
        regions['a'][:, :count] = coef[at:at + n]
        at += n
        parts.append(b.transform(regions, height, width, code, fill, ctx=ctx))
    return _one_batch(ctx, parts, height, width)


def transpose_frames(frames, op, ctx=None):
    """Pillow's `Image.transpose(op)` of every resident frame (`ta_frames_transpose`): a NEW batch for a batch, a list of new
    batches, one per input batch, for a list (the sizes of a mixed list stay mixed).  `op`: Pillow's code 0 .. 6 or
    'flip_left_right', 'flip_top_bottom', 'rotate_90' (counter-clockwise, as in Pillow), 'rotate_180', 'rotate_270',
    'transpose', 'transverse'."""
    batches, listed = _batches(frames, 'transpose_frames')
    code = lib.transpose_op(op)
    outs = [b.transpose(code, ctx=ctx if ctx is not None else batches[0].ctx) for b in batches]
    return outs if listed else outs[0]


def rotate_plan(width, height, angle, expand=False, center=None, translate=None):
    """What Pillow's `Image.rotate(angle, resample, expand, center, translate)` does to a width x height image, host only:
    ('copy', None, size), ('transpose', op, size) for its fast paths (a multiple of 360; 180; 90 and 270 when `expand` is
    set or the image is square; all only without `center` and `translate`), else ('transform', the six AFFINE
    coefficients, size) built as Pillow builds them: the rotation rounded to 15 decimals, the expanded canvas from the
    transformed corners."""
    import math
    angle = angle % 360.0
    if not (center or translate):
        if angle == 0:
            return 'copy', None, (width, height)
        if angle == 180:
            return 'transpose', lib.ROTATE_180, (width, height)
        if angle in (90, 270) and (expand or width == height):
            return 'transpose', lib.ROTATE_90 if angle == 90 else lib.ROTATE_270, (height, width)
    w, h = width, height
    post_trans = (0, 0) if translate is None else translate
    if center is None:
        center = (w / 2, h / 2)
    angle = -math.radians(angle)
    matrix = [round(math.cos(angle), 15), round(math.sin(angle), 15), 0.0,
              round(-math.sin(angle), 15), round(math.cos(angle), 15), 0.0]

    def transform(x, y, matrix):
        a, b, c, d, e, f = matrix
        return a * x + b * y + c, d * x + e * y + f
    matrix[2], matrix[5] = transform(-center[0] - post_trans[0], -center[1] - post_trans[1], matrix)
    matrix[2] += center[0]
    matrix[5] += center[1]
    if expand:
        xx, yy = zip(*[transform(x, y, matrix) for x, y in ((0, 0), (w, 0), (w, h), (0, h))])
        nw = math.ceil(max(xx)) - math.floor(min(xx))
        nh = math.ceil(max(yy)) - math.floor(min(yy))
        matrix[2], matrix[5] = transform(-(nw - w) / 2.0, -(nh - h) / 2.0, matrix)
        w, h = nw, nh
    return 'transform', matrix, (w, h)


def rotate_frames(frames, angle, resample='nearest', expand=False, center=None, translate=None, fillcolor=None, ctx=None):
    """Pillow's `Image.rotate(angle, resample, expand, center, translate, fillcolor)` of every resident frame, bit for bit:
    a NEW batch for a batch, a list of new batches for a list.  It takes the paths Pillow takes (`rotate_plan`): a copy, a
    `ta_frames_transpose`, or one `ta_frames_transform` call per batch with Pillow's matrix.  `angle`: degrees
    counter-clockwise; `center`, `translate`: (x, y) or None."""
    who = 'rotate_frames'
    batches, listed = _batches(frames, who)
    code = _transform_filter(resample, who)
    fill = _fillcolor(fillcolor, who)
    try:
        angle = float(angle)
        center = None if center is None else tuple(float(v) for v in center)
        translate = None if translate is None else tuple(float(v) for v in translate)
    except (TypeError, ValueError):
        raise ValueError('%s: angle must be a number, center and translate None or (x, y)' % who) from None
    if not np.isfinite(angle) or any(t is not None and (len(t) != 2 or not np.isfinite(t).all()) for t in (center, translate)):
        raise ValueError('%s: angle must be finite, center and translate None or two finite values' % who)
    if any(b.shape[0] == 0 for b in batches):
        raise ValueError('%s: a batch without images' % who)
    plans = [rotate_plan(b.shape[2], b.shape[1], angle, expand, center, translate) for b in batches]
    for kind, _, size in plans:
        _size(size, who)
    outs = []
    for b, (kind, arg, (width, height)) in zip(batches, plans):
        on = ctx if ctx is not None else batches[0].ctx
        n = b.shape[0]
        if kind == 'transpose':
            outs.append(b.transpose(arg, ctx=on))
            continue
        regions = np.zeros(n, lib.TRANSFORM_DT)
        regions['frame'], regions['method'] = np.arange(n), lib.AFFINE
        regions['a'][:, :6] = (1, 0, 0, 0, 1, 0) if kind == 'copy' else arg
        out = b.transform(regions, height, width, lib.NEAREST if kind == 'copy' else code, fill, ctx=on)
        outs.append(out)
    return outs if listed else outs[0]


# ---- Image.transform's other methods: MESH (ImageOps.deform), QUAD, EXTENT -------------------------------------------------
class _MeshTarget:
    """What a deformer's `getmesh(image)` is called with in place of a Pillow image: `.size`, `.width`, `.height`."""

    def __init__(self, width, height):
        self.size, self.width, self.height = (width, height), width, height


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def _quad(quad, who):
    """8 finite numbers nw.x, nw.y, sw.x, sw.y, se.x, se.y, ne.x, ne.y -> a tuple of floats."""
    try:
        q = tuple(float(v) for v in quad)
    except (TypeError, ValueError):
        q = ()
    if len(q) != 8 or not np.isfinite(q).all():
        raise ValueError('%s: a quad must be 8 finite numbers (nw, sw, se, ne; x, y each), got %r' % (who, quad))
    return q


def _looks_like_cell(item):
    try:
        return len(item) == 2 and len(item[0]) == 4 and len(item[1]) == 8
    except TypeError:
        return False


def pack_mesh(mesh, who='pack_mesh'):
    """Pillow's mesh [(box, quad), ...] -> a lib.MESH_CELL_DT array, cells in order.  `box`: four ints (x0, y0, x1, y1) of the
    OUTPUT, half-open, x0 < x1 and y0 < y1 (Pillow divides by zero or draws nothing otherwise), within +-2^24, inside the
    output or not; `quad`: 8 finite numbers, the corners nw, sw, se, ne of the INPUT quadrilateral.  Host only."""
    if isinstance(mesh, np.ndarray) and mesh.dtype == lib.MESH_CELL_DT:       # packed before: only the values are checked
        boxes = np.stack([mesh[k].reshape(-1) for k in ('x0', 'y0', 'x1', 'y1')], 1).astype(np.int64)
        quads = mesh['quad'].reshape(-1, 8)
    else:
        try:
            rows = list(mesh)
        except TypeError:
            raise ValueError('%s: a mesh must be a list of (box, quad), got %r' % (who, mesh)) from None
        for k, item in enumerate(rows):
            if not _looks_like_cell(item):
                raise ValueError('%s: cell %d must be ((x0, y0, x1, y1), 8 numbers), got %r' % (who, k, item))
            if not all(_is_int(v) and abs(int(v)) <= lib.MESH_COORD_LIMIT for v in item[0]):
                raise ValueError('%s: cell %d: the box must be four ints within +-2^24, got %r' % (who, k, tuple(item[0])))
        boxes = np.array([tuple(r[0]) for r in rows], np.int64).reshape(-1, 4)
        try:
            quads = np.array([tuple(r[1]) for r in rows], np.float64).reshape(-1, 8)
        except (TypeError, ValueError):
            quads = np.full((len(rows), 8), np.nan)
            for k, r in enumerate(rows):
                quads[k] = _quad(r[1], '%s: cell %d' % (who, k))
    bad = (np.abs(boxes) > lib.MESH_COORD_LIMIT).any(1)
    if bad.any():
        raise ValueError('%s: cell %d: the box must lie within +-2^24, got %r' % (who, bad.argmax(), tuple(boxes[bad.argmax()])))
    bad = (boxes[:, 2] <= boxes[:, 0]) | (boxes[:, 3] <= boxes[:, 1])
    if bad.any():
        raise ValueError('%s: cell %d: the box %r must have x0 < x1 and y0 < y1' % (who, bad.argmax(), tuple(boxes[bad.argmax()])))
    bad = ~np.isfinite(quads).all(1)
    if bad.any():
        _quad(quads[bad.argmax()], '%s: cell %d' % (who, bad.argmax()))
    cells = np.zeros(len(boxes), lib.MESH_CELL_DT)
    cells['x0'], cells['y0'], cells['x1'], cells['y1'] = boxes.T
    cells['quad'] = quads
    return cells


def _run_mesh(who, batches, per_batch, size, code, fill, ctx):
    """per_batch[i]: (cells, mesh_first, mesh of every frame) of batch i -> the one new batch."""
    width, height = size
    if max(len(c) for c, _, _ in per_batch) > lib.MESH_MAX_CELLS:
        raise ValueError('%s: more than %d cells for one batch' % (who, lib.MESH_MAX_CELLS))
    ctx = ctx if ctx is not None else batches[0].ctx
    parts = []
    try:
        for b, (cells, first, of_frame) in zip(batches, per_batch):
            n = b.shape[0]
            if not n:
                continue
            images = np.zeros(n, lib.MESH_IMAGE_DT)
            images['frame'], images['mesh'] = np.arange(n), of_frame
            parts.append(b.transform_mesh(cells, first, images, height, width, code, fill, ctx=ctx))
    except Exception:
        _free(parts)
        raise
    return _one_batch(ctx, parts, height, width)


def _mesh_size(batches, size, who):
    if size is not None:
        return _size(size, who)
    sizes = {(b.shape[2], b.shape[1]) for b in batches}
    if len(sizes) != 1:
        raise ValueError('%s: size is needed when the frames differ in size' % who)
    return _size(sizes.pop(), who)


def mesh_frames(frames, mesh, size=None, resample='nearest', fillcolor=None, ctx=None):
    """Resident frames warped through a mesh -> one NEW resident `lib.Frames` (sum(n), height, width, 3), images in input
    order, each Pillow's `Image.fromarray(frame).transform(size, Image.MESH, mesh, resample=resample, fillcolor=fillcolor)`
    bit for bit (`ta_frames_transform_mesh`), which is also `ImageOps.deform`.  `frames`: a `lib.Frames` batch or a list of
    them (as `open_images` returns for mixed sizes); `mesh`: Pillow's list of (box, quad) -- `pack_mesh` has the rules --,
    one list for all frames (or what `pack_mesh` made of it: a caller that warps batch after batch through one mesh packs
    it once) or a list of such lists, one per frame, or a deformer: an object whose `getmesh(image)` returns
    the list, called once per batch with a stand-in that has `.size`, `.width` and `.height` of the batch's frames; `size`:
    (width, height) of the output, default the frames' own (they must then agree); `resample`: 'nearest', 'bilinear',
    'bicubic' or Pillow's code; `fillcolor`: None (zeros, and a cell's pixels whose point leaves the source become 0) or
    (r, g, b) (such pixels keep what lay there).  A shared mesh is built and sent once per batch however many frames it
    warps.  Every argument is checked before anything is launched."""
    who = 'mesh_frames'
    batches, _ = _batches(frames, who)
    width, height = _mesh_size(batches, size, who)
    code = _transform_filter(resample, who)
    fill = _fillcolor(fillcolor, who)
    total = sum(b.shape[0] for b in batches)
    if total == 0:
        raise ValueError('%s: no images' % who)
    per_batch = []
    if hasattr(mesh, 'getmesh'):
        for b in batches:
            cells = pack_mesh(mesh.getmesh(_MeshTarget(b.shape[2], b.shape[1])), who)
            per_batch.append((cells, [0, len(cells)], 0))
    else:
        packed = isinstance(mesh, np.ndarray) and mesh.dtype == lib.MESH_CELL_DT
        try:
            rows = mesh if packed else list(mesh)
        except TypeError:
            raise ValueError('%s: mesh must be a list of (box, quad), one such list per frame, or have getmesh()' % who) from None
        if packed or all(_looks_like_cell(r) for r in rows):    # one mesh (an empty one: all fill)
            cells = pack_mesh(rows, who)
            per_batch = [(cells, [0, len(cells)], 0)] * len(batches)
        elif len(rows) == total:
            packed = [pack_mesh(r, '%s: frame %d' % (who, k)) for k, r in enumerate(rows)]
            at = 0
            for b in batches:
                mine = packed[at:at + b.shape[0]]
                at += b.shape[0]
                first = np.concatenate([[0], np.cumsum([len(c) for c in mine])]).astype(np.int32)
                cells = np.concatenate(mine) if mine else np.zeros(0, lib.MESH_CELL_DT)
                per_batch.append((cells, first, np.arange(b.shape[0])))
        else:
            raise ValueError('%s: mesh must be a list of (box, quad) or one such list for each of the %d frames' % (who, total))
    return _run_mesh(who, batches, per_batch, (width, height), code, fill, ctx)


def quad_frames(frames, size, quad, resample='nearest', fillcolor=None, ctx=None):
    """Pillow's `Image.transform(size, Image.QUAD, quad, resample, fillcolor=)` of every resident frame, bit for bit: the
    quadrilateral `quad` of the frame -- 8 numbers, the corners nw, sw, se, ne as (x, y) -- stretched over a size[0] x
    size[1] image (a screen, a whiteboard, a plate cut out by its corners).  One quad for all frames or one per frame.
    It is `mesh_frames` with the one cell ((0, 0) + size, quad); the other arguments and the result are as there."""
    who = 'quad_frames'
    batches, _ = _batches(frames, who)
    width, height = _size(size, who)
    code = _transform_filter(resample, who)
    fill = _fillcolor(fillcolor, who)
    total = sum(b.shape[0] for b in batches)
    if total == 0:
        raise ValueError('%s: no images' % who)
    try:
        q = np.asarray(quad, np.float64)
    except (TypeError, ValueError):
        q = np.zeros(0)
    shared = q.shape == (8,)
    if not shared and q.shape != (total, 8):
        raise ValueError('%s: quad must be 8 numbers, or 8 for each of the %d frames' % (who, total))
    if not np.isfinite(q).all():
        raise ValueError('%s: quad must be finite' % who)
    per_batch, at = [], 0
    for b in batches:
        n = 1 if shared else b.shape[0]
        cells = np.zeros(n, lib.MESH_CELL_DT)
        cells['x1'], cells['y1'] = width, height
        cells['quad'] = q if shared else q[at:at + n]
        per_batch.append((cells, np.arange(n + 1), 0 if shared else np.arange(n)))
        at += b.shape[0]
    return _run_mesh(who, batches, per_batch, (width, height), code, fill, ctx)


def extent_data(size, extent):
    """Pillow's AFFINE coefficients for `Image.transform(size, Image.EXTENT, extent)`: the rectangle (x0, y0, x1, y1) of the
    source stretched over the output, ((x1 - x0) / width, 0, x0, 0, (y1 - y0) / height, y0).  Host only."""
    width, height = size
    x0, y0, x1, y1 = extent
    return ((x1 - x0) / width, 0, x0, 0, (y1 - y0) / height, y0)


def extent_frames(frames, size, extent, resample='nearest', fillcolor=None, ctx=None):
    """Pillow's `Image.transform(size, Image.EXTENT, extent, resample, fillcolor=)` of every resident frame, bit for bit:
    the source rectangle `extent` = (x0, y0, x1, y1), fractional, inside the frame or not, stretched over the output.  One
    extent for all frames or one per frame.  Pillow turns it into the affine map of `extent_data` and nothing more, and so
    does this: the work is `transform_frames`'s, whose arguments and result these are."""
    who = 'extent_frames'
    batches, _ = _batches(frames, who)
    width, height = _size(size, who)
    total = sum(b.shape[0] for b in batches)
    try:
        e = np.asarray(extent, np.float64)
    except (TypeError, ValueError):
        e = np.zeros(0)
    if e.shape != (4,) and (total == 0 or e.shape != (total, 4)):
        raise ValueError('%s: extent must be (x0, y0, x1, y1), or one for each of the %d frames' % (who, total))
    if not np.isfinite(e).all():
        raise ValueError('%s: extent must be finite' % who)
    data = [extent_data((width, height), [float(v) for v in row]) for row in e.reshape(-1, 4)]
    return transform_frames(frames, (width, height), lib.AFFINE, data[0] if e.ndim == 1 else data, resample, fillcolor, ctx)


def _camera(matrix, what, who):
    try:
        k = np.asarray(matrix, np.float64)
    except (TypeError, ValueError):
        k = np.zeros(0)
    if k.shape != (3, 3) or not np.isfinite(k).all() or k[0, 0] == 0 or k[1, 1] == 0:
        raise ValueError('%s: %s must be a finite 3 x 3 matrix with non-zero focal lengths, got %r' % (who, what, matrix))
    return k


def undistort_cells(size, camera_matrix, dist_coeffs, grid=16, new_camera_matrix=None):
    """The mesh that removes a lens's distortion from a size[0] x size[1] image, host only, numpy float64: a lattice
    of `grid`-pixel cells over the OUTPUT (the last column and row narrower where the size is no multiple), each vertex
    mapped to the source point the Brown-Conrady model gives it.  A vertex (u, v) -- a pixel CORNER in Pillow's
    coordinates, (u - 0.5, v - 0.5) in the matrices', which put whole numbers at pixel centres -- is normalised with the
    new matrix, y = (v - 0.5 - cy') / fy', x = (u - 0.5 - cx' - s' y) / fx'; distorted, with r2 = x x + y y and
    radial = 1 + k1 r2 + k2 r2^2 + k3 r2^3,
        xd = x radial + 2 p1 x y + p2 (r2 + 2 x x),  yd = y radial + p1 (r2 + 2 y y) + 2 p2 x y;
    and projected with the camera matrix, (fx xd + s yd + cx + 0.5, fy yd + cy + 0.5).  `camera_matrix`: 3 x 3, rows
    (fx, s, cx), (0, fy, cy), (0, 0, 1); `dist_coeffs`: (k1, k2, p1, p2) or (k1, k2, p1, p2, k3);
    `new_camera_matrix`: the view wanted, default the camera's own.  Returns a lib.MESH_CELL_DT array, cells row by row,
    as `pack_mesh` makes and `mesh_frames` takes; `undistort_mesh` is the same as Pillow's list."""
    who = 'undistort_mesh'
    width, height = _size(size, who)
    k = _camera(camera_matrix, 'camera_matrix', who)
    kn = k if new_camera_matrix is None else _camera(new_camera_matrix, 'new_camera_matrix', who)
    try:
        d = np.asarray(dist_coeffs, np.float64).reshape(-1)
    except (TypeError, ValueError):
        d = np.zeros(0)
    if d.shape[0] not in (4, 5) or not np.isfinite(d).all():
        raise ValueError('%s: dist_coeffs must be (k1, k2, p1, p2) or (k1, k2, p1, p2, k3), finite, got %r' % (who, dist_coeffs))
    if not _is_int(grid) or not 1 <= grid <= lib.RESAMPLE_SIDE_LIMIT:
        raise ValueError('%s: grid must be an int within 1 .. %d, got %r' % (who, lib.RESAMPLE_SIDE_LIMIT, grid))
    grid = int(grid)
    k1, k2, p1, p2 = d[:4]
    k3 = d[4] if d.shape[0] == 5 else 0.0
    xv = np.array(list(range(0, width, grid)) + [width], np.float64)
    yv = np.array(list(range(0, height, grid)) + [height], np.float64)
    if (len(xv) - 1) * (len(yv) - 1) > lib.MESH_MAX_CELLS:
        raise ValueError('%s: a %d-pixel lattice over %d x %d has more than %d cells' % (who, grid, width, height, lib.MESH_MAX_CELLS))
    with np.errstate(all='ignore'):                     # what overflows is refused below
        y = ((yv - 0.5 - kn[1, 2]) / kn[1, 1])[:, None] + np.zeros((1, len(xv)))
        x = (xv[None, :] - 0.5 - kn[0, 2] - kn[0, 1] * y) / kn[0, 0]
        r2 = x * x + y * y
        radial = 1 + k1 * r2 + k2 * r2 * r2 + k3 * r2 * r2 * r2
        xd = x * radial + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        yd = y * radial + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        us = k[0, 0] * xd + k[0, 1] * yd + k[0, 2] + 0.5
        vs = k[1, 1] * yd + k[1, 2] + 0.5
    if not (np.isfinite(us).all() and np.isfinite(vs).all()):
        raise ValueError('%s: the model leaves the finite numbers over this image' % who)
    cells = np.zeros((len(yv) - 1, len(xv) - 1), lib.MESH_CELL_DT)
    cells['x0'], cells['x1'] = xv[None, :-1], xv[None, 1:]
    cells['y0'], cells['y1'] = yv[:-1, None], yv[1:, None]
    cells['quad'] = np.stack([us[:-1, :-1], vs[:-1, :-1], us[1:, :-1], vs[1:, :-1], us[1:, 1:], vs[1:, 1:], us[:-1, 1:], vs[:-1, 1:]], -1)
    return cells.reshape(-1)


def undistort_mesh(size, camera_matrix, dist_coeffs, grid=16, new_camera_matrix=None):
    """`undistort_cells` as the plain list Pillow takes: [((x0, y0, x1, y1), (8 floats: nw, sw, se, ne)), ...], cells row by
    row, for `Image.transform(size, Image.MESH, ...)`, `ImageOps.deform` and `mesh_frames`.  Host only."""
    cells = undistort_cells(size, camera_matrix, dist_coeffs, grid, new_camera_matrix)
    return [((int(c['x0']), int(c['y0']), int(c['x1']), int(c['y1'])), tuple(float(v) for v in c['quad'])) for c in cells]


def undistort_frames(frames, camera_matrix, dist_coeffs, grid=16, resample='bilinear', new_camera_matrix=None, fillcolor=None,
                     ctx=None):
    """Resident frames of a wide-angle or otherwise distorting camera made rectilinear -> one NEW batch of the same size:
    `mesh_frames` with `undistort_mesh(frame size, camera_matrix, dist_coeffs, grid, new_camera_matrix)`, so all frames must
    have one size.  The result is Pillow's MESH of that lattice, bit for bit: exact at the lattice's vertices and bilinear
    in the source position within a cell.  It is NOT a per-pixel remap, and no parity with OpenCV's undistort is claimed; a
    finer `grid` follows the model more closely at the cost of more cells."""
    who = 'undistort_frames'
    batches, _ = _batches(frames, who)
    size = _mesh_size(batches, None, who)
    cells = undistort_cells(size, camera_matrix, dist_coeffs, grid, new_camera_matrix)
    return mesh_frames(frames, cells, size, resample, fillcolor, ctx)


# ---- pixel values: histograms, statistics, look-up tables ---------------------------------------------------------------
def _frame_boxes(batches, boxes, who):
    """-> per batch an int (n, 4) array of half-open boxes (x0, y0, x1, y1), one per frame: `boxes` (one per frame of the
    whole input, in order) or the whole frames; checked against the frames here, before anything is launched."""
    total = sum(b.shape[0] for b in batches)
    if total == 0:
        raise ValueError('%s: no images' % who)
    if boxes is not None:
        try:
            boxes = np.asarray(boxes)
            ok = boxes.shape == (total, 4) and np.array_equal(boxes, boxes.astype(np.int64))
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError('%s: boxes must be one integer (x0, y0, x1, y1) for each of the %d frames' % (who, total))
        boxes = boxes.astype(np.int64)
    out, at = [], 0
    for b in batches:
        n, h, w = b.shape[:3]
        q = boxes[at:at + n] if boxes is not None else np.tile(np.array([0, 0, w, h], np.int64), (n, 1))
        at += n
        if len(q) and not ((0 <= q[:, 0]) & (q[:, 0] < q[:, 2]) & (q[:, 2] <= w) & (0 <= q[:, 1]) & (q[:, 1] < q[:, 3]) & (q[:, 3] <= h)).all():
            raise ValueError('%s: every box must satisfy 0 <= x0 < x1 <= %d and 0 <= y0 < y1 <= %d' % (who, w, h))
        out.append(q)
    return out


def _regions(dt, boxes, shape=lib.BLUR_BOX):
    q = np.zeros(len(boxes), dt)
    q['frame'] = np.arange(len(boxes))
    q['x0'], q['y0'], q['x1'], q['y1'] = boxes[:, 0], boxes[:, 1], boxes[:, 2], boxes[:, 3]
    q['shape'] = shape
    return q


def _hist_mode(mode, who):
    if mode not in lib.HIST_MODES:
        raise ValueError("%s: mode must be 'RGB' or 'L', got %r" % (who, mode))
    return lib.HIST_MODES[mode]


def histogram_frames(frames, mode='RGB', boxes=None, ctx=None):
    """Pillow's `Image.histogram()` of every resident frame -> uint32 (N, 3, 256) (mode 'RGB': the R, G and B counts), or
    (N, 256) for mode 'L': the histogram of `convert('L')`.  `frames`: a `lib.Frames` batch or a list of them (N frames in
    all, in order); `boxes`: None, or one half-open integer (x0, y0, x1, y1) per frame: the histogram of `crop(box)`.  One
    `ta_frames_histogram` call per batch; only the counts leave the device."""
    who = 'histogram_frames'
    batches, _ = _batches(frames, who)
    code = _hist_mode(mode, who)
    per_batch = _frame_boxes(batches, boxes, who)
    parts = [b.histogram(_regions(lib.HIST_DT, q), code, ctx=ctx) for b, q in zip(batches, per_batch) if len(q)]
    return np.concatenate(parts)


def histogram_stats(hist):
    """`ImageStat.Stat(histogram)` for a stack of histograms, host only: `hist` integer (..., 256), one row of counts per
    band -> dict of arrays shaped like hist[..., 0]: `count` (int64), `sum`, `sum2`, `mean`, `rms`, `var`, `stddev`
    (float64), `median` (int64), and `extrema` (int64, one more axis: min, max).  Every value is what Stat computes, in its
    order of float64 operations: the sums are integers below 2^53, so they are exact in any order; the quotients, the
    `** 2.0` and the roots are Python's.  A band without pixels gives Stat's values: mean, rms and var 0, median 255,
    extrema (255, 0)."""
    import math
    h = np.asarray(hist)
    if h.ndim < 1 or h.shape[-1] != 256 or h.dtype.kind not in 'iu':
        raise ValueError('histogram_stats: integer counts (..., 256), got %s %s' % (h.dtype, h.shape))
    shape = h.shape[:-1]
    h = h.reshape(-1, 256).astype(np.int64)
    j = np.arange(256, dtype=np.int64)
    count, total, total2 = h.sum(1), (h * j).sum(1), (h * (j * j)).sum(1)
    m = len(h)
    out = {k: np.zeros(m, np.float64) for k in ('sum', 'sum2', 'mean', 'rms', 'var', 'stddev')}
    median, extrema = np.full(m, 255, np.int64), np.tile(np.array([255, 0], np.int64), (m, 1))
    for i in range(m):
        n, s, s2 = int(count[i]), float(int(total[i])), float(int(total2[i]))
        out['sum'][i], out['sum2'][i] = s, s2
        if n:
            out['mean'][i] = s / n
            out['rms'][i] = math.sqrt(s2 / n)
            out['var'][i] = (s2 - (s ** 2.0) / n) / n
            used = np.nonzero(h[i])[0]
            extrema[i] = used[0], used[-1]
            median[i] = min(int(np.searchsorted(np.cumsum(h[i]), n // 2, side='right')), 255)
        out['stddev'][i] = math.sqrt(out['var'][i])
    out = {k: v.reshape(shape) for k, v in out.items()}
    out.update(count=count.reshape(shape), median=median.reshape(shape), extrema=extrema.reshape(shape + (2,)))
    return out


def frame_stats(frames, mode='RGB', boxes=None, ctx=None):
    """`ImageStat.Stat` of every resident frame (or of `crop(box)` of each: `boxes` as in `histogram_frames`) -> dict of
    arrays (N, 3) for mode 'RGB', (N, 1) for mode 'L' (Stat of `convert('L')`): `histogram_stats` of one
    `histogram_frames` call, equal to Stat's values exactly."""
    hist = histogram_frames(frames, mode, boxes, ctx=ctx)
    return histogram_stats(hist if hist.ndim == 3 else hist[:, None])


def _bands(hist, who):
    h = np.asarray(hist)
    if h.size == 0 or h.size % 256 or h.dtype.kind not in 'iu':
        raise ValueError('%s: integer counts, 256 per band, got %s %s' % (who, h.dtype, h.shape))
    return [[int(v) for v in row] for row in h.reshape(-1, 256)]


def equalize_lut(hist):
    """The table `ImageOps.equalize` applies to an image with this histogram, host only: `hist` 256 counts per band ((256,),
    (3, 256) or (768,)) -> uint8 (256 x bands,).  Pillow's integer steps: the non-zero counts without the last one, summed
    and floor-divided by 255, give the step (a band with one used bin, or a step of 0: the identity); entry i is
    (step // 2 + counts below i) // step, clipped to 255 as point() clips it."""
    lut = []
    for h in _bands(hist, 'equalize_lut'):
        histo = [v for v in h if v]
        step = (sum(histo) - histo[-1]) // 255 if len(histo) > 1 else 0
        if not step:
            lut.extend(range(256))
            continue
        n = step // 2
        for i in range(256):
            lut.append(min(n // step, 255))             # point() clips its table's entries; the quotient can pass 255
            n += h[i]
    return np.array(lut, np.uint8)


def autocontrast_lut(hist, cutoff=0, ignore=None):
    """The table `ImageOps.autocontrast(cutoff=, ignore=)` applies to an image with this histogram, host only; `hist` and
    the result as in `equalize_lut`.  `cutoff`: percent cut from both ends, or (low, high); `ignore`: a bin or bins whose
    counts are dropped first.  Pillow's steps: int(n * cutoff // 100) counts removed from each end, the lowest and highest
    bin left, the identity when hi <= lo, else int(i * (255.0 / (hi - lo)) - lo * scale) clipped to 0 .. 255."""
    if cutoff and not isinstance(cutoff, tuple):
        cutoff = (cutoff, cutoff)
    ignore = [] if ignore is None else ([int(ignore)] if isinstance(ignore, (int, np.integer)) else [int(v) for v in ignore])
    lut = []
    for h in _bands(hist, 'autocontrast_lut'):
        for ix in ignore:
            h[ix] = 0
        if cutoff:
            n = sum(h)
            for c, order in ((cutoff[0], range(256)), (cutoff[1], range(255, -1, -1))):
                cut = int(n * c // 100)
                for i in order:
                    if cut > h[i]:
                        cut -= h[i]
                        h[i] = 0
                    else:
                        h[i] -= cut
                        cut = 0
                    if cut <= 0:
                        break
        used = [i for i in range(256) if h[i]]
        lo, hi = (used[0], used[-1]) if used else (255, 0)
        if hi <= lo:
            lut.extend(range(256))
            continue
        scale = 255.0 / (hi - lo)
        offset = -lo * scale
        lut.extend(min(max(int(ix * scale + offset), 0), 255) for ix in range(256))
    return np.array(lut, np.uint8)


def _factor(factor, who):
    try:
        f = np.float32(factor)                          # Image.blend takes its alpha as a C float
    except (TypeError, ValueError):
        f = np.float32(np.nan)
    if not np.isfinite(f):
        raise ValueError('%s: factor must be a finite number, got %r' % (who, factor))
    return f


def blend_lut(in1, factor):
    """`Image.blend(Image.new('L', size, in1), im, factor)` as a table over im's values, host only -> uint8 (256,):
    libImaging's float32 in1 + factor * (v - in1), a multiply and an add; truncated when 0 <= factor <= 1, clipped to
    0 .. 255 first otherwise; factor 0 copies in1, factor 1 the image."""
    f = _factor(factor, 'blend_lut')
    in1 = int(in1)
    if not 0 <= in1 <= 255:
        raise ValueError('blend_lut: in1 must be within 0 .. 255, got %r' % (in1,))
    v = np.arange(256, dtype=np.int32)
    if f == 0:
        return np.full(256, in1, np.uint8)
    if f == 1:
        return v.astype(np.uint8)
    t = np.float32(in1) + f * (v - in1).astype(np.float32)
    assert t.dtype == np.float32
    if 0 <= f <= 1:
        return t.astype(np.int32).astype(np.uint8)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, np.clip(t, 0, 255).astype(np.int32))).astype(np.uint8)


def brightness_lut(factor):
    """The table of `ImageEnhance.Brightness(im).enhance(factor)`: a blend with black."""
    return blend_lut(0, _factor(factor, 'brightness_lut'))


def contrast_lut(factor, mean):
    """The table of `ImageEnhance.Contrast(im).enhance(factor)` for an image whose `convert('L')` has the mean `mean`
    (`ImageStat`'s float, as `frame_stats(frames, 'L')['mean']` returns it): a blend with the grey int(mean + 0.5)."""
    return blend_lut(int(float(mean) + 0.5), _factor(factor, 'contrast_lut'))


def invert_lut():
    """The table of `ImageOps.invert`."""
    return np.arange(255, -1, -1).astype(np.uint8)


def posterize_lut(bits):
    """The table of `ImageOps.posterize(im, bits)`: the top `bits` bits (1 .. 8) of every value."""
    if isinstance(bits, bool) or not isinstance(bits, (int, np.integer)) or not 1 <= bits <= 8:
        raise ValueError('posterize_lut: bits must be an int within 1 .. 8, got %r' % (bits,))
    return (np.arange(256) & ~(2 ** (8 - int(bits)) - 1)).astype(np.uint8)


def solarize_lut(threshold=128):
    """The table of `ImageOps.solarize(im, threshold)`: values from `threshold` on are inverted."""
    i = np.arange(256)
    return np.where(i < threshold, i, 255 - i).astype(np.uint8)


def _tables(lut, total, who):
    """-> uint8 (1, 768) or (total, 768): a table of 256 entries (all bands), 768 (R, G, B), or one of 768 per frame."""
    try:
        a = np.asarray(lut)
        ok = a.dtype.kind in 'iu' and a.size and int(a.min()) >= 0 and int(a.max()) <= 255
    except (TypeError, ValueError):
        ok = False
    if ok and a.shape == (256,):
        return np.tile(a.astype(np.uint8), 3)[None]
    if ok and a.shape == (768,):
        return a.astype(np.uint8)[None]
    if ok and a.shape == (total, 768):
        return np.ascontiguousarray(a.astype(np.uint8))
    raise ValueError('%s: a table of 256 or 768 integers within 0 .. 255, or one of 768 for each of the %d frames' % (who, total))


def point_frames(frames, lut, ctx=None):
    """Pillow's `Image.point(lut)` of every resident frame, in place (`ta_frames_point`, one call per batch); returns
    `frames`.  `frames`: a `lib.Frames` batch or a list of them; `lut`: 256 entries (applied to the three bands), 768 (R, G
    and B table), or (N, 768): a table per frame."""
    who = 'point_frames'
    batches, _ = _batches(frames, who)
    per_batch = _frame_boxes(batches, None, who)
    tables = _tables(lut, sum(len(q) for q in per_batch), who)
    at = 0
    for b, q in zip(batches, per_batch):
        regions = _regions(lib.POINT_DT, q)
        if len(tables) > 1:
            regions['lut'] = np.arange(len(q))
        if len(q):
            b.point(regions, tables[at:at + len(q)] if len(tables) > 1 else tables, ctx=ctx)
        at += len(q)
    return frames


def equalize_frames(frames, ctx=None):
    """`ImageOps.equalize` of every resident frame, in place: one histogram call, a table per frame, one point call."""
    hist = histogram_frames(frames, 'RGB', ctx=ctx)
    return point_frames(frames, np.stack([equalize_lut(h) for h in hist]), ctx=ctx)


def autocontrast_frames(frames, cutoff=0, ignore=None, preserve_tone=False, ctx=None):
    """`ImageOps.autocontrast(im, cutoff, ignore, preserve_tone=)` of every resident frame, in place.  `preserve_tone`: one
    table from the histogram of `convert('L')` for the three bands, instead of a table per band."""
    hist = histogram_frames(frames, 'L' if preserve_tone else 'RGB', ctx=ctx)
    luts = [autocontrast_lut(h, cutoff, ignore) for h in hist]
    return point_frames(frames, np.stack([np.tile(t, 3) if preserve_tone else t for t in luts]), ctx=ctx)


def brightness_frames(frames, factor, ctx=None):
    """`ImageEnhance.Brightness(im).enhance(factor)` of every resident frame, in place."""
    return point_frames(frames, brightness_lut(factor), ctx=ctx)


def contrast_frames(frames, factor, ctx=None):
    """`ImageEnhance.Contrast(im).enhance(factor)` of every resident frame, in place: each frame blended with the grey of
    its own mean luma, which comes from one 'L' histogram call."""
    f = _factor(factor, 'contrast_frames')
    mean = frame_stats(frames, 'L', ctx=ctx)['mean'][:, 0]
    return point_frames(frames, np.stack([np.tile(contrast_lut(f, m), 3) for m in mean]), ctx=ctx)


def color_frames(frames, factor, ctx=None):
    """`ImageEnhance.Color(im).enhance(factor)` of every resident frame, in place (`ta_frames_saturate`): every pixel blended
    with its own luma; 0 greys the frame, values above 1 saturate it."""
    who = 'color_frames'
    f = _factor(factor, who)
    batches, _ = _batches(frames, who)
    for b, q in zip(batches, _frame_boxes(batches, None, who)):
        regions = _regions(lib.SATURATE_DT, q)
        regions['factor'] = f
        if len(q):
            b.saturate(regions, ctx=ctx)
    return frames


def grayscale_frames(frames, ctx=None):
    """`im.convert('L').convert('RGB')` of every resident frame, in place."""
    return color_frames(frames, 0.0, ctx=ctx)


def invert_frames(frames, ctx=None):
    """`ImageOps.invert` of every resident frame, in place."""
    return point_frames(frames, invert_lut(), ctx=ctx)


def posterize_frames(frames, bits, ctx=None):
    """`ImageOps.posterize(im, bits)` of every resident frame, in place."""
    return point_frames(frames, posterize_lut(bits), ctx=ctx)


def solarize_frames(frames, threshold=128, ctx=None):
    """`ImageOps.solarize(im, threshold)` of every resident frame, in place."""
    return point_frames(frames, solarize_lut(threshold), ctx=ctx)


# ---- two images: paste, composite, blend, ImageChops --------------------------------------------------------------------
def _int_rows(value, n, widths, what, who):
    """`value` as an int64 (n, k) array, k in `widths`: one row for all frames, or one per frame."""
    try:
        a = np.asarray(value)
        ok = a.dtype.kind in 'iuf' and a.ndim in (1, 2) and a.shape[-1] in widths and np.array_equal(a, a.astype(np.int64))
    except (TypeError, ValueError):
        ok = False
    if ok and a.ndim == 2 and len(a) != n:
        ok = False
    if not ok:
        raise ValueError('%s: %s must be %s integers, one such row for all frames or one for each of the %d frames'
                         % (who, what, ' or '.join(str(k) for k in widths), n))
    return np.broadcast_to(a.astype(np.int64), (n, a.shape[-1]))


def pack_combine(frames_shape, other_shape, op='paste', box=None, source=(0, 0), mask=None, mask_band=0, alpha=0.0, offset=0,
                 shape='box'):
    """Host only: the records of one `Frames.combine` call -> (lib.COMBINE_DT array, uint8 buffer of packed bitmaps or None).
    `frames_shape`, `other_shape`: the (N, H, W, 3) of the batch written and of the batch read, which has N frames or one
    (then every frame reads it).  `op`: a name of lib.COMBINE_OPS or its code.  `box`: None (the corner (0, 0)), Pillow's
    (x, y), where the piece of `other` right and below `source` goes, or (x0, y0, x1, y1), whose size the piece takes; one
    for all frames or one per frame, and `source` = (x, y) in `other` likewise.  The box is clipped against the frame with
    the source shifted accordingly, as Image.paste clips; a frame whose box is empty then gets no record.  `mask` ('paste'
    only): None, an int 0 .. 255, a uint8 (h, w) array of the unclipped box's size (packed once per distinct clipping), or
    the (M, h, w, 3) shape of a resident mask batch of M = N or one frames at least as large as the box, read in band
    `mask_band` from its corner.  `alpha`: Image.blend's, or the scale of 'add' / 'subtract'; `offset`: theirs."""
    who = 'pack_combine'
    n, H, W = (int(v) for v in frames_shape[:3])
    m, oh, ow = (int(v) for v in other_shape[:3])
    if m not in (1, n):
        raise ValueError('%s: other must have one frame or %d, got %d' % (who, n, m))
    code = lib.COMBINE_OPS.get(op.lower()) if isinstance(op, str) else op if op in lib.COMBINE_OPS.values() else None
    if code is None:
        raise ValueError('%s: op must be one of %s, got %r' % (who, sorted(lib.COMBINE_OPS), op))
    if shape not in _SHAPES:
        raise ValueError("%s: shape must be 'box' or 'ellipse', got %r" % (who, shape))
    a = _factor(alpha, who)
    if code in (lib.COMBINE_ADD, lib.COMBINE_SUBTRACT) and a == 0:
        raise ValueError('%s: scale must not be 0' % who)
    if isinstance(offset, bool) or not isinstance(offset, (int, np.integer)) or abs(int(offset)) >= 2 ** 31:
        raise ValueError('%s: offset must be an int, got %r' % (who, offset))
    boxes = _int_rows((0, 0) if box is None else box, n, (2, 4), 'box', who)
    sources = _int_rows(source, n, (2,), 'source', who)
    kind, value, bitmap, mask_frames = lib.MASK_NONE, 0, None, 1
    if mask is not None:
        if code != lib.COMBINE_PASTE:
            raise ValueError("%s: only 'paste' takes a mask" % who)
        if isinstance(mask, (int, np.integer)) and not isinstance(mask, bool):
            if not 0 <= int(mask) <= 255:
                raise ValueError('%s: a constant mask must be within 0 .. 255, got %r' % (who, mask))
            kind, value = lib.MASK_CONSTANT, int(mask)
        elif isinstance(mask, np.ndarray) and mask.ndim == 2 and mask.dtype == np.uint8:
            kind, bitmap = lib.MASK_BITMAP, mask
        elif isinstance(mask, (tuple, list)) and len(mask) == 4:
            kind, mask_frames = lib.MASK_FRAMES, int(mask[0])
            if mask_frames not in (1, n) or mask_band not in (0, 1, 2):
                raise ValueError('%s: a mask batch must have one frame or %d, and its band be 0, 1 or 2' % (who, n))
        else:
            raise ValueError('%s: mask must be None, an int, a uint8 (h, w) array or the shape of a resident batch' % who)
    rows, packed, at = [], {}, 0
    for i in range(n):
        sx, sy = (int(v) for v in sources[i])
        x0, y0 = int(boxes[i][0]), int(boxes[i][1])
        pw, ph = (int(boxes[i][2]) - x0, int(boxes[i][3]) - y0) if boxes.shape[1] == 4 else (ow - sx, oh - sy)
        if pw <= 0 or ph <= 0 or sx < 0 or sy < 0 or sx + pw > ow or sy + ph > oh:
            raise ValueError('%s: the %d x %d piece at (%d, %d) is empty or not inside the %d x %d other' % (who, pw, ph, sx, sy, ow, oh))
        if bitmap is not None and bitmap.shape != (ph, pw):
            raise ValueError('%s: the mask is %s, the pasted piece (%d, %d)' % (who, bitmap.shape, ph, pw))
        if kind == lib.MASK_FRAMES and (int(mask[1]) < ph or int(mask[2]) < pw):
            raise ValueError('%s: the mask batch is smaller than the pasted piece' % who)
        cx0, cy0, cx1, cy1 = max(x0, 0), max(y0, 0), min(x0 + pw, W), min(y0 + ph, H)
        if cx1 <= cx0 or cy1 <= cy0:
            continue
        dx, dy = cx0 - x0, cy0 - y0
        if bitmap is not None:
            key = (dx, dy, cx1 - cx0, cy1 - cy0)
            if key not in packed:
                packed[key] = (at, np.ascontiguousarray(bitmap[dy:dy + cy1 - cy0, dx:dx + cx1 - cx0]).reshape(-1))
                at += packed[key][1].size
            value = packed[key][0]
        rows.append((i, cx0, cy0, cx1, cy1, _SHAPES[shape], i if m > 1 else 0, sx + dx, sy + dy, code, a, int(offset), kind, value,
                     i if mask_frames > 1 else 0, dx, dy, int(mask_band) if kind == lib.MASK_FRAMES else 0))
    masks = np.concatenate([v[1] for v in packed.values()]) if packed else None
    return np.array(rows, lib.COMBINE_DT), masks


def _partners(batches, other, what, who):
    """-> per batch the batch it is combined with: `other` is one batch (of one frame when `frames` is a list: every frame
    reads it) or a list with a batch of one frame or as many for every batch of `frames`."""
    if isinstance(other, lib.Frames):
        if len(batches) > 1 and other.shape[0] != 1:
            raise ValueError('%s: %s must be a one-frame batch, or a list like frames' % (who, what))
        others = [other] * len(batches)
    elif isinstance(other, (list, tuple)) and len(other) == len(batches) and all(isinstance(o, lib.Frames) for o in other):
        others = list(other)
    else:
        raise ValueError('%s: %s must be a lib.Frames batch or a list of %d of them' % (who, what, len(batches)))
    for b, o in zip(batches, others):
        if o.shape[0] not in (1, b.shape[0]):
            raise ValueError('%s: %s has %d frames for a batch of %d' % (who, what, o.shape[0], b.shape[0]))
    return others


def _combine(who, frames, other, op, box=None, source=(0, 0), mask=None, mask_band=0, alpha=0.0, offset=0, shape='box',
             same_size=False, ctx=None):
    """Every batch of `frames` with its partner: everything is packed and checked before anything is launched."""
    batches, _ = _batches(frames, who)
    others = _partners(batches, other, 'other', who)
    resident = isinstance(mask, lib.Frames) or (isinstance(mask, (list, tuple)) and mask and isinstance(mask[0], lib.Frames))
    mattes = _partners(batches, mask, 'mask', who) if resident else [None] * len(batches)
    total = sum(b.shape[0] for b in batches)
    per_frame = [np.ndim(v) == 2 for v in (box, source)]
    for v, each, what in ((box, per_frame[0], 'box'), (source, per_frame[1], 'source')):
        if each and len(v) != total:
            raise ValueError('%s: one %s for each of the %d frames' % (who, what, total))
    plans, at = [], 0
    for b, o, mt in zip(batches, others, mattes):
        n = b.shape[0]
        if same_size and (o.shape[1:3] != b.shape[1:3] or (mt is not None and mt.shape[1:3] != b.shape[1:3])):
            raise ValueError('%s: frames of %s need an other and a mask of that size' % (who, b.shape[1:3]))
        bx = np.asarray(box)[at:at + n] if per_frame[0] else box
        so = np.asarray(source)[at:at + n] if per_frame[1] else source
        at += n
        if n:
            plans.append((b, o, mt) + pack_combine(b.shape, o.shape, op, bx, so, mt.shape if mt is not None else mask, mask_band,
                                                   alpha, offset, shape))
    for b, o, mt, regions, masks in plans:
        if len(regions):
            b.combine(o, regions, masks, mask_frames=mt, ctx=ctx)
    return frames


def copy_frames(frames, ctx=None):
    """A NEW resident batch (or list of them) with the pixels of `frames`: allocated, then pasted into on the device."""
    batches, listed = _batches(frames, 'copy_frames')
    outs = []
    for b in batches:
        c = ctx if ctx is not None else b.ctx
        n, h, w = b.shape[:3]
        out = lib.Frames.zeros(c, n, h, w)
        if n:
            out.combine(b, pack_combine(b.shape, b.shape)[0], ctx=c)
        outs.append(out)
    return outs if listed else outs[0]


def paste_frames(frames, other, box=None, mask=None, source=(0, 0), mask_band=0, ctx=None):
    """Pillow's `frame.paste(other_frame, box, mask)` for every resident frame, in place (`ta_frames_combine`, one call per
    batch); returns `frames`.  `frames`: a `lib.Frames` batch or a list of them; `other`: a batch with one frame (pasted
    into every frame) or as many as `frames`, or a list of such batches, one per batch of `frames`.  `box`: None, (x, y) or
    (x0, y0, x1, y1), one for all frames or one per frame; it may leave the frame and is clipped as Image.paste clips.
    `source`: the corner in `other` of the piece that is pasted (default: all of it).  `mask`: None, an int 0 .. 255 (a
    constant 'L' mask), a host uint8 (h, w) array of the piece's size, or a resident batch (a list of them for a list of
    frames) whose band `mask_band` is the mask."""
    return _combine('paste_frames', frames, other, 'paste', box, source, mask, mask_band, ctx=ctx)


def composite_frames(frames, other, mask, mask_band=0, ctx=None):
    """`Image.composite(other, frame, mask)` written into every resident frame, in place: `other` where the mask is 255,
    the frame where it is 0, blended between.  `other` and `mask` (paste_frames' kinds) have the frames' size."""
    return _combine('composite_frames', frames, other, 'paste', None, (0, 0), mask, mask_band, same_size=True, ctx=ctx)


def blend_frames(frames, other, alpha, ctx=None):
    """`Image.blend(frame, other, alpha)` of every resident frame, in place: a cross-fade; alpha outside 0 .. 1 extrapolates
    and clips."""
    return _combine('blend_frames', frames, other, 'blend', alpha=alpha, same_size=True, ctx=ctx)


def chop_frames(frames, other, op, scale=1.0, offset=0, boxes=None, shape='box', ctx=None):
    """`ImageChops.<op>(frame, other)` of every resident frame, in place: `op` one of 'lighter', 'darker', 'difference',
    'multiply', 'screen', 'add', 'subtract' (with `scale` and `offset`), 'add_modulo', 'subtract_modulo', 'soft_light',
    'hard_light', 'overlay'.  `boxes`: None, or one half-open (x0, y0, x1, y1) per frame: only that box changes, from the
    same box of `other`, under `shape` 'ellipse' only the ellipse Pillow draws into it."""
    who = 'chop_frames'
    if not isinstance(op, str) or op.lower() not in lib.COMBINE_OPS or op.lower() in ('paste', 'blend'):
        raise ValueError('%s: op must be one of %s, got %r' % (who, sorted(set(lib.COMBINE_OPS) - {'paste', 'blend'}), op))
    if boxes is None:
        return _combine(who, frames, other, op, alpha=scale, offset=offset, shape=shape, same_size=True, ctx=ctx)
    batches, _ = _batches(frames, who)
    q = np.concatenate(_frame_boxes(batches, boxes, who))
    return _combine(who, frames, other, op, q, q[:, :2], alpha=scale, offset=offset, shape=shape, same_size=True, ctx=ctx)


def difference_frames(frames, other, ctx=None):
    """`ImageChops.difference(frame, other)` of every resident frame, in place: |frame - other|, the motion between two
    clips when `other` holds the frames before."""
    return chop_frames(frames, other, 'difference', ctx=ctx)


# ---- neighbourhood filters: Image.filter --------------------------------------------------------------------------------
# Pillow's ten built-in filters (ImageFilter.BLUR ... SMOOTH_MORE): name -> (size, scale, offset, kernel), kept here so
# that the names work without Pillow
FILTER_BUILTINS = {
    'blur': (5, 16, 0, (1, 1, 1, 1, 1, 1, 0, 0, 0, 1, 1, 0, 0, 0, 1, 1, 0, 0, 0, 1, 1, 1, 1, 1, 1)),
    'contour': (3, 1, 255, (-1, -1, -1, -1, 8, -1, -1, -1, -1)),
    'detail': (3, 6, 0, (0, -1, 0, -1, 10, -1, 0, -1, 0)),
    'edge_enhance': (3, 2, 0, (-1, -1, -1, -1, 10, -1, -1, -1, -1)),
    'edge_enhance_more': (3, 1, 0, (-1, -1, -1, -1, 9, -1, -1, -1, -1)),
    'emboss': (3, 1, 128, (-1, 0, 0, 0, 1, 0, 0, 0, 0)),
    'find_edges': (3, 1, 0, (-1, -1, -1, -1, 8, -1, -1, -1, -1)),
    'sharpen': (3, 16, 0, (-2, -2, -2, -2, 32, -2, -2, -2, -2)),
    'smooth': (3, 13, 0, (1, 1, 1, 1, 5, 1, 1, 1, 1)),
    'smooth_more': (5, 100, 0, (1, 1, 1, 1, 1, 1, 5, 5, 5, 1, 1, 5, 44, 5, 1, 1, 5, 5, 5, 1, 1, 1, 1, 1, 1)),
}
FILTER_GAUSSIAN = 3                     # a spec kind of this module only: filter_frames routes it to ta_frames_blur
FILTER_RANK_LIMIT = 7                   # the largest window of ta_frames_filter's rank filter
_SHAPES = {'box': lib.BLUR_BOX, 'ellipse': lib.BLUR_ELLIPSE}


def _finite32(values, what, who):
    try:
        a = np.asarray(values, np.float64).astype(np.float32)
    except (TypeError, ValueError):
        a = np.float32(np.nan)
    if not np.isfinite(a).all():
        raise ValueError('%s: %s must be finite, got %r' % (who, what, values))
    return a


def kernel_spec(size, kernel, scale=None, offset=0, factor=None):
    """`ImageFilter.Kernel((size, size), kernel, scale, offset)` as a lib.FILTER_SPEC_DT record: size 3 or 5, scale None:
    the sum of the kernel.  `factor`: blend the filtered image with the original as `ImageEnhance.Sharpness` does
    (`Image.blend(filtered, original, factor)`)."""
    who = 'kernel_spec'
    if isinstance(size, (tuple, list)):
        if len(size) != 2 or size[0] != size[1]:
            raise ValueError('%s: a square kernel of size 3 or 5, got %r' % (who, size))
        size = size[0]
    if size not in (3, 5) or len(kernel) != size * size:
        raise ValueError('%s: a kernel of 3 x 3 or 5 x 5 entries, got size %r and %d entries' % (who, size, len(kernel)))
    if scale is None:
        scale = sum(kernel)
    spec = np.zeros((), lib.FILTER_SPEC_DT)
    spec['kind'], spec['size'] = lib.FILTER_KERNEL, size
    spec['kernel'][:size * size] = _finite32(kernel, 'the kernel', who)
    spec['scale'], spec['offset'] = _finite32(scale, 'scale', who), _finite32(offset, 'offset', who)
    if spec['scale'] == 0:
        raise ValueError('%s: scale (the sum of the kernel, if none is given) must not be 0' % who)
    if factor is not None:
        spec['has_factor'], spec['factor'] = 1, _factor(factor, who)
    return spec


def rank_spec(size, rank):
    """`ImageFilter.RankFilter(size, rank)` as a lib.FILTER_SPEC_DT record: odd size 1 .. 7, 0 <= rank < size * size."""
    ints = all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in (size, rank))
    if not ints or size % 2 == 0 or not 1 <= size <= FILTER_RANK_LIMIT or not 0 <= rank < size * size:
        raise ValueError('RankFilter(%r, %r): an odd size within 1 .. %d and 0 <= rank < size * size' % (size, rank, FILTER_RANK_LIMIT))
    spec = np.zeros((), lib.FILTER_SPEC_DT)
    spec['kind'], spec['size'], spec['rank'] = lib.FILTER_RANK, size, rank
    return spec


def unsharp_spec(radius=2, percent=150, threshold=3):
    """`ImageFilter.UnsharpMask(radius, percent, threshold)` as a lib.FILTER_SPEC_DT record: a scalar radius 0 .. 1024,
    integers percent >= 0 and threshold >= 0."""
    who = 'UnsharpMask(%r, %r, %r)' % (radius, percent, threshold)
    if isinstance(radius, (tuple, list)):
        raise ValueError('%s: a radius per axis is not offered' % who)
    ints = all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) and 0 <= v < 2 ** 31 for v in (percent, threshold))
    if not ints or not 0 <= _finite32(radius, 'radius', who) <= 1024:
        raise ValueError('%s: a radius within 0 .. 1024 and integers percent >= 0, threshold >= 0' % who)
    spec = np.zeros((), lib.FILTER_SPEC_DT)
    spec['kind'], spec['radius'], spec['percent'], spec['threshold'] = lib.FILTER_UNSHARP, radius, percent, threshold
    return spec


def filter_spec(flt):
    """What `Image.filter(flt)` takes -> a lib.FILTER_SPEC_DT record for `Frames.filter` / `filter_frames`.  `flt`: a Pillow
    `ImageFilter` instance or built-in class -- `Kernel`, the ten built-ins (`BLUR`, `CONTOUR`, `DETAIL`, `EDGE_ENHANCE`,
    `EDGE_ENHANCE_MORE`, `EMBOSS`, `FIND_EDGES`, `SHARPEN`, `SMOOTH`, `SMOOTH_MORE`), `RankFilter` / `MinFilter` /
    `MedianFilter` / `MaxFilter` up to size 7, `UnsharpMask`, and `GaussianBlur` with a scalar radius (kind
    FILTER_GAUSSIAN, which `filter_frames` routes to `ta_frames_blur`) -- or a built-in's lower-case name, which needs no
    Pillow.  A record passes through.  ValueError, naming the filter, for what is not offered: `ModeFilter`, `BoxBlur`, a
    radius per axis, `MultibandFilter`s such as `Color3DLUT` (that one is `color_lut_frames`' and `color_spec`'s, through
    `ta_frames_color`), rank sizes above 7."""
    if isinstance(flt, np.ndarray) and flt.dtype == lib.FILTER_SPEC_DT and flt.shape == ():
        return flt
    if isinstance(flt, str):
        if flt not in FILTER_BUILTINS:
            raise ValueError('filter_spec: %r is not one of %s' % (flt, sorted(FILTER_BUILTINS)))
        size, scale, offset, kernel = FILTER_BUILTINS[flt]
        return kernel_spec(size, kernel, scale, offset)
    if isinstance(flt, type):
        try:
            flt = flt()                                  # Image.filter does the same with a class
        except TypeError:
            raise ValueError('filter_spec: %s needs arguments: pass an instance' % flt.__name__) from None
    names = [c.__name__ for c in type(flt).__mro__]
    name = names[0]
    if 'RankFilter' in names:
        if flt.size > FILTER_RANK_LIMIT:
            raise ValueError('filter_spec: %s of size %r: rank filters are offered up to size %d' % (name, flt.size, FILTER_RANK_LIMIT))
        return rank_spec(flt.size, flt.rank)
    if 'UnsharpMask' in names:
        return unsharp_spec(flt.radius, flt.percent, flt.threshold)
    if 'GaussianBlur' in names:
        if isinstance(flt.radius, (tuple, list)):
            raise ValueError('filter_spec: GaussianBlur(%r): a radius per axis is not offered' % (flt.radius,))
        spec = np.zeros((), lib.FILTER_SPEC_DT)
        spec['kind'], spec['radius'] = FILTER_GAUSSIAN, _finite32(flt.radius, 'radius', 'GaussianBlur')
        if not 0 <= spec['radius'] <= 1024:
            raise ValueError('filter_spec: GaussianBlur(%r): a radius within 0 .. 1024' % (flt.radius,))
        return spec
    if 'BuiltinFilter' in names and hasattr(flt, 'filterargs'):
        size, scale, offset, kernel = flt.filterargs
        return kernel_spec(size, kernel, scale, offset)
    raise ValueError('filter_spec: %s is not offered (kernels of 3 x 3 and 5 x 5, rank filters up to size 7, UnsharpMask and '
                     'GaussianBlur with one radius are)' % name)


def filter_frames(frames, flt, boxes=None, shape='box', ctx=None):
    """Pillow's `Image.filter(flt)` of every resident frame, in place (`ta_frames_filter`, one call per batch; a
    `GaussianBlur`: `ta_frames_blur`); returns `frames`.  `frames`: a `lib.Frames` batch or a list of them; `flt`: what
    `filter_spec` takes; `boxes`: None, or one half-open integer (x0, y0, x1, y1) per frame, as `histogram_frames` takes
    them: `im.paste(im.crop(box).filter(flt), box)`, the filter seeing the box's own pixels only; `shape`: 'box', or
    'ellipse' (only the ellipse Pillow draws into the box is replaced)."""
    who = 'filter_frames'
    if shape not in _SHAPES:
        raise ValueError("%s: shape must be 'box' or 'ellipse', got %r" % (who, shape))
    spec = filter_spec(flt)
    batches, _ = _batches(frames, who)
    for b, q in zip(batches, _frame_boxes(batches, boxes, who)):
        if not len(q):
            continue
        if spec['kind'] == FILTER_GAUSSIAN:
            regions = _regions(lib.BLUR_DT, q, _SHAPES[shape])
            regions['radius'] = spec['radius']
            b.blur(regions, ctx=ctx)
        else:
            b.filter(_regions(lib.FILTER_REGION_DT, q, _SHAPES[shape]), spec, ctx=ctx)
    return frames


def sharpness_frames(frames, factor, ctx=None):
    """`ImageEnhance.Sharpness(im).enhance(factor)` of every resident frame, in place: each frame blended with its own
    `SMOOTH`; 0 smooths, 1 leaves the frame as it is, 2 sharpens."""
    size, scale, offset, kernel = FILTER_BUILTINS['smooth']
    return filter_frames(frames, kernel_spec(size, kernel, scale, offset, factor=_factor(factor, 'sharpness_frames')), ctx=ctx)


def unsharp_frames(frames, radius=2, percent=150, threshold=3, ctx=None):
    """`im.filter(ImageFilter.UnsharpMask(radius, percent, threshold))` of every resident frame, in place."""
    return filter_frames(frames, unsharp_spec(radius, percent, threshold), ctx=ctx)


def median_frames(frames, size=3, ctx=None):
    """`im.filter(ImageFilter.MedianFilter(size))` of every resident frame, in place: odd size up to 7."""
    if isinstance(size, (int, np.integer)) and size > FILTER_RANK_LIMIT:
        raise ValueError('median_frames: MedianFilter of size %r: rank filters are offered up to size %d' % (size, FILTER_RANK_LIMIT))
    return filter_frames(frames, rank_spec(size, size * size // 2 if isinstance(size, (int, np.integer)) else size), ctx=ctx)


# ---- colour: matrices, YCbCr / HSV, 3-D look-up tables --------------------------------------------------------------------
COLOR_CONVERSIONS = {'ycbcr': lib.COLOR_RGB2YCBCR, 'rgb_from_ycbcr': lib.COLOR_YCBCR2RGB, 'hsv': lib.COLOR_RGB2HSV,
                     'rgb_from_hsv': lib.COLOR_HSV2RGB}
COLOR_LUT_AXIS = (2, 65)                # Color3DLUT's own limits of an axis


def color_spec(op):
    """What a colour call takes -> (a lib.COLOR_OP_DT record whose `table` is 0, its float32 table) for `Frames.color`:

        a 12-tuple                          `convert('RGB', matrix)`
        'ycbcr', 'rgb_from_ycbcr'           `convert('YCbCr')`, `convert('RGB')` of a 'YCbCr' image
        'hsv', 'rgb_from_hsv'               `convert('HSV')`, `convert('RGB')` of an 'HSV' image
        an `ImageFilter.Color3DLUT`, or (size, table): size an int or (s0, s1, s2), table 3 * s0 * s1 * s2 numbers as
                                            Pillow stores them (R fastest, the three channels of a node together)

    A (record, table) pair passes through.  ValueError for what is not offered: 4-tuples (an 'L' output), 1- and 4-channel
    tables, an axis outside 2 .. 65, a table of another length, numbers that are not finite."""
    who = 'color_spec'
    rec = np.zeros((), lib.COLOR_OP_DT)
    if isinstance(op, tuple) and len(op) == 2 and isinstance(op[0], np.ndarray) and op[0].dtype == lib.COLOR_OP_DT:
        return op[0].reshape(()), np.ascontiguousarray(op[1], np.float32).reshape(-1)
    if isinstance(op, str):
        if op not in COLOR_CONVERSIONS:
            raise ValueError('%s: %r is not one of %s' % (who, op, sorted(COLOR_CONVERSIONS)))
        rec['kind'] = COLOR_CONVERSIONS[op]
        return rec, np.zeros(0, np.float32)
    if hasattr(op, 'table') and hasattr(op, 'channels'):            # ImageFilter.Color3DLUT
        if op.channels != 3 or getattr(op, 'mode', None) not in (None, 'RGB'):
            raise ValueError('%s: a Color3DLUT of %r channels and target mode %r: three channels in and out are offered'
                             % (who, op.channels, getattr(op, 'mode', None)))
        op = (tuple(op.size), op.table)
    if isinstance(op, (tuple, list)) and len(op) == 2 and not np.isscalar(op[1]):
        size, table = op
        size = (size,) * 3 if isinstance(size, (int, np.integer)) and not isinstance(size, bool) else tuple(size)
        if len(size) != 3 or not all(isinstance(v, (int, np.integer)) and COLOR_LUT_AXIS[0] <= v <= COLOR_LUT_AXIS[1] for v in size):
            raise ValueError('%s: a 3-D table size of three integers within %d .. %d, got %r' % ((who,) + COLOR_LUT_AXIS + (size,)))
        table = _finite32(table, 'the table', who).reshape(-1)
        nodes = size[0] * size[1] * size[2]
        if len(table) != 3 * nodes:
            raise ValueError('%s: a table of 3 x %d x %d x %d = %d entries, got %d (1- and 4-channel tables are not offered)'
                             % ((who,) + size + (3 * nodes, len(table))))
        rec['kind'], rec['size'] = lib.COLOR_LUT3D, size
        return rec, np.ascontiguousarray(table)
    if isinstance(op, (tuple, list, np.ndarray)) and len(op) == 12:
        rec['kind'] = lib.COLOR_MATRIX
        return rec, np.ascontiguousarray(_finite32(op, 'the matrix', who).reshape(-1))
    if isinstance(op, (tuple, list, np.ndarray)) and len(op) == 4:
        raise ValueError("%s: a 4-tuple converts to 'L': only 12-tuples ('RGB' output) are offered" % who)
    raise ValueError('%s: %r is not a 12-tuple, one of %s, a Color3DLUT or (size, table)' % (who, op, sorted(COLOR_CONVERSIONS)))


def _color(who, frames, op, boxes=None, shape='box', ctx=None):
    if shape not in _SHAPES:
        raise ValueError("%s: shape must be 'box' or 'ellipse', got %r" % (who, shape))
    rec, table = color_spec(op)
    batches, _ = _batches(frames, who)
    for b, q in zip(batches, _frame_boxes(batches, boxes, who)):
        if len(q):
            b.color(_regions(lib.COLOR_REGION_DT, q, _SHAPES[shape]), rec, table, ctx=ctx)
    return frames


def convert_frames(frames, mode, matrix=None, source='RGB', boxes=None, shape='box', ctx=None):
    """Pillow's `Image.convert(mode[, matrix])` of every resident frame, in place (`ta_frames_color`, one call per batch);
    returns `frames`.  `source` is the mode the frames' bytes are in now: a batch carries three bytes per pixel and no
    mode, so the caller says it.  Offered: source 'RGB' to 'YCbCr', 'HSV', or 'RGB' with a 12-tuple `matrix`; source
    'YCbCr' or 'HSV' to 'RGB'.  `boxes`, `shape`: as `filter_frames` takes them."""
    who = 'convert_frames'
    if matrix is not None:
        if (source, mode) != ('RGB', 'RGB'):
            raise ValueError("%s: a matrix converts 'RGB' to 'RGB' here, got %r to %r" % (who, source, mode))
        op = matrix
    else:
        op = {('RGB', 'YCbCr'): 'ycbcr', ('YCbCr', 'RGB'): 'rgb_from_ycbcr', ('RGB', 'HSV'): 'hsv', ('HSV', 'RGB'): 'rgb_from_hsv'}.get((source, mode))
        if op is None:
            raise ValueError("%s: %r to %r is not offered ('RGB' to 'YCbCr' or 'HSV' and back are)" % (who, source, mode))
    return _color(who, frames, op, boxes, shape, ctx)


def matrix_frames(frames, matrix, boxes=None, shape='box', ctx=None):
    """`im.convert('RGB', matrix)` of every resident frame, in place: a 12-tuple, row by row (white balance, channel
    mixing, sepia, a camera's colour matrix)."""
    if not isinstance(matrix, (tuple, list, np.ndarray)) or len(matrix) != 12:
        raise ValueError("matrix_frames: a 12-tuple ('RGB' output), got %r" % (matrix,))
    return _color('matrix_frames', frames, matrix, boxes, shape, ctx)


def color_lut_frames(frames, lut, boxes=None, shape='box', ctx=None):
    """`im.filter(ImageFilter.Color3DLUT(size, table))` of every resident frame, in place: `lut` is the Pillow object or
    (size, table), three channels in and out, every axis 2 .. 65."""
    rec, table = color_spec(lut)
    if rec['kind'] != lib.COLOR_LUT3D:
        raise ValueError('color_lut_frames: a Color3DLUT or (size, table), got %r' % (lut,))
    return _color('color_lut_frames', frames, (rec, table), boxes, shape, ctx)


def hue_lut(shift):
    """`point()`'s table of `hue_frames`: (h + shift) mod 256 on the first band, the other two as they are."""
    if not isinstance(shift, (int, np.integer)) or isinstance(shift, bool):
        raise ValueError('hue_frames: shift must be an integer (256 is a full turn), got %r' % (shift,))
    i = np.arange(256)
    return np.concatenate([(i + int(shift)) % 256, i, i]).astype(np.uint8)


def hue_frames(frames, shift, ctx=None):
    """Turn the hue of every resident frame by `shift` / 256 of a full turn, in place: `convert('HSV')`, `point()` with
    (h + shift) mod 256 on H, `convert('RGB')`, equal to the same three Pillow steps."""
    table = hue_lut(shift)
    convert_frames(frames, 'HSV', ctx=ctx)
    point_frames(frames, table, ctx=ctx)
    return convert_frames(frames, 'RGB', source='HSV', ctx=ctx)


_SUBSAMPLING = {-1: 2, 0: 0, 1: 1, 2: 2, '4:4:4': 0, '4:2:2': 1, '4:2:0': 2}


def jpeg_options(quality=75, subsampling=-1, optimize=False):
    """Pillow's save() arguments -> (quality, subsampling code for ta_jpeg_encode); ValueError for anything else
    (`optimize` must be True or False)."""
    lib.check_jpeg_optimize(optimize)
    key = subsampling if isinstance(subsampling, str) else (
        int(subsampling) if isinstance(subsampling, (int, np.integer)) and not isinstance(subsampling, bool) else None)
    if key not in _SUBSAMPLING:
        raise ValueError('subsampling must be -1, 0, 1, 2, \'4:4:4\', \'4:2:2\' or \'4:2:0\', got %r' % (subsampling,))
    return lib.check_jpeg_options(quality, _SUBSAMPLING[key])


def encode_jpeg(images, quality=75, subsampling=-1, ctx=None, device=None, optimize=False):
    """Resident frames -> JPEG files (list of bytes, one per frame, in order).  `images`: a `lib.Frames` batch, a list of
    them (as `open_images` returns for mixed sizes), or a host uint8 (H, W, 3) / (N, H, W, 3) array (uploaded first).
    `optimize`: Pillow's optimize=True.  Every option is checked before anything is launched."""
    quality, code = jpeg_options(quality, subsampling, optimize)
    if isinstance(images, lib.Frames):
        batches = [images]
    elif isinstance(images, (list, tuple)):
        batches = list(images)
        if not batches or not all(isinstance(b, lib.Frames) for b in batches):
            raise ValueError('encode_jpeg: a list must hold lib.Frames batches')
    else:
        arr = np.asarray(images)
        if arr.dtype != np.uint8 or arr.ndim not in (3, 4) or arr.shape[-1] != 3 or 0 in arr.shape:
            raise ValueError('encode_jpeg: host images must be uint8 (H, W, 3) or (N, H, W, 3) RGB, got %s %s'
                             % (arr.dtype, arr.shape))
        if max(arr.shape[-3:-1]) > 65535:
            raise ValueError('encode_jpeg: JPEG sides are at most 65535 pixels')
        ctx = ctx if ctx is not None else runtime.get_context(device)
        up = ctx.upload(arr[None] if arr.ndim == 3 else arr)
        try:
            return ctx.jpeg_encode(up, quality, code, optimize)
        finally:
            up.free()
    for b in batches:
        if max(b.shape[1:3]) > 65535:
            raise ValueError('encode_jpeg: JPEG sides are at most 65535 pixels')
    files = []
    for b in batches:
        files.extend(b.encode_jpeg(quality, code, ctx=ctx, optimize=optimize))
    return files


def save_images(images, paths, quality=75, subsampling=-1, ctx=None, device=None, optimize=False):
    """encode_jpeg(images, ...) written to `paths` (one per frame, in order)."""
    paths = list(paths)
    jpeg_options(quality, subsampling, optimize)
    if isinstance(images, lib.Frames):
        n = images.shape[0]
    elif isinstance(images, (list, tuple)):
        n = sum(b.shape[0] for b in images if isinstance(b, lib.Frames))
    else:
        shape = np.shape(images)
        n = 1 if len(shape) == 3 else (shape[0] if shape else 0)
    if n != len(paths):
        raise ValueError('save_images: %d frames, %d paths' % (n, len(paths)))
    files = encode_jpeg(images, quality, subsampling, ctx=ctx, device=device, optimize=optimize)
    for data, path in zip(files, paths):
        with open(_path(path), 'wb') as fh:
            fh.write(data)


# ---- raw YUV video frames --------------------------------------------------------------------------------------------
def _yuv_choice(value, table, what):
    if not isinstance(value, str) or value not in table:
        raise ValueError('yuv_spec: %s must be one of %s, got %r' % (what, ', '.join(repr(k) for k in table), value))
    return table[value]


def yuv_spec(pix_fmt, matrix='bt709', range='tv', chroma='bilinear', siting='left'):
    """The lib.YUV_SPEC_DT record of a raw YUV conversion; ValueError names the argument that is wrong.
    pix_fmt: 'yuv420p', 'nv12' or 'yuv444p'.  matrix: 'bt601' or 'bt709'.  range: 'tv' (16 .. 235 / 240) or 'pc' (0 .. 255).
    chroma: how a 4:2:0 format's chroma is brought to every pixel on the way IN, 'nearest' or 'bilinear'; siting: where its
    samples sit horizontally, 'left' (MPEG-2, H.264) or 'center' (JPEG, MPEG-1).  On the way OUT (frames_to_yuv) a chroma
    sample is the conversion of its block's mean, and `chroma` and `siting` are checked but not used; yuv444p uses neither."""
    return np.array((_yuv_choice(pix_fmt, lib.YUV_FORMATS, 'pix_fmt'), _yuv_choice(matrix, lib.YUV_MATRICES, 'matrix'),
                     _yuv_choice(range, lib.YUV_RANGES, 'range'), _yuv_choice(chroma, lib.YUV_CHROMAS, 'chroma'),
                     _yuv_choice(siting, lib.YUV_SITINGS, 'siting')), dtype=lib.YUV_SPEC_DT)


def _yuv_size(size, who):
    try:
        width, height = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError('%s: size must be (width, height), got %r' % (who, size)) from None
    if not (1 <= width <= 65535 and 1 <= height <= 65535):
        raise ValueError('%s: size must be within 1 .. 65535 a side, got %r' % (who, size))
    return width, height


def yuv_frame_bytes(pix_fmt, size):
    """The bytes of one raw frame of `size` = (width, height): w h + 2 ((w + 1) >> 1) ((h + 1) >> 1) for 'yuv420p' and
    'nv12', 3 w h for 'yuv444p'.  Host only."""
    code = _yuv_choice(pix_fmt, lib.YUV_FORMATS, 'pix_fmt')
    width, height = _yuv_size(size, 'yuv_frame_bytes')
    return lib.yuv_frame_bytes(code, height, width)


def frames_from_yuv(data, size, pix_fmt='yuv420p', matrix='bt709', range='tv', chroma='bilinear', siting='left', ctx=None,
                    device=None):
    """Raw YUV frames -> ONE resident RGB batch (ta_frames_from_yuv).  `data`: bytes or a uint8 array of whole frames of
    `size` = (width, height), back to back as `ffmpeg -f rawvideo -pix_fmt <pix_fmt>` writes them.  The other arguments
    are yuv_spec's."""
    spec = yuv_spec(pix_fmt, matrix, range, chroma, siting)
    width, height = _yuv_size(size, 'frames_from_yuv')
    per = lib.yuv_frame_bytes(spec['format'], height, width)
    if isinstance(data, (bytes, bytearray, memoryview)):
        arr = np.frombuffer(data, np.uint8)
    else:
        arr = np.asarray(data)
        if arr.dtype != np.uint8:
            raise ValueError('frames_from_yuv: data must be bytes or a uint8 array, got %s' % arr.dtype)
        arr = np.ascontiguousarray(arr).reshape(-1)
    if arr.size == 0 or arr.size % per:
        raise ValueError('frames_from_yuv: %d bytes are not whole %s frames of %d x %d (%d bytes each)'
                         % (arr.size, pix_fmt, width, height, per))
    ctx = ctx if ctx is not None else runtime.get_context(device)
    return ctx.frames_from_yuv(arr, arr.size // per, height, width, spec)


def frames_to_yuv(frames, pix_fmt='yuv420p', matrix='bt709', range='tv', chroma='bilinear', siting='left', ctx=None, device=None):
    """Resident frames -> raw YUV frames, a uint8 (n, frame_bytes) array in frame order (ta_frames_to_yuv): written to a
    file or a pipe as it is, it is what `ffmpeg -f rawvideo -pix_fmt <pix_fmt> -s WxH -i pipe:` reads.  `frames`: what
    encode_jpeg accepts -- a `lib.Frames` batch, a list of them (all of one size), or a host uint8 (H, W, 3) / (N, H, W, 3)
    array (uploaded first).  A 4:2:0 chroma sample is the conversion of the mean of its block; `chroma` and `siting` are
    checked but not used in this direction.  The conversion runs on `ctx`, by default the CALLING thread's context of the
    batch's device (runtime.get_context) and never the batch's own: a batch from a video reader belongs to the reader
    thread's context, which that thread is using."""
    spec = yuv_spec(pix_fmt, matrix, range, chroma, siting)
    if isinstance(frames, lib.Frames):
        batches = [frames]
    elif isinstance(frames, (list, tuple)):
        batches = list(frames)
        if not batches or not all(isinstance(b, lib.Frames) for b in batches):
            raise ValueError('frames_to_yuv: a list must hold lib.Frames batches')
        if len({b.shape[1:3] for b in batches}) != 1:
            raise ValueError('frames_to_yuv: the batches of a list must have one frame size')
    else:
        arr = np.asarray(frames)
        if arr.dtype != np.uint8 or arr.ndim not in (3, 4) or arr.shape[-1] != 3 or 0 in arr.shape:
            raise ValueError('frames_to_yuv: host images must be uint8 (H, W, 3) or (N, H, W, 3) RGB, got %s %s'
                             % (arr.dtype, arr.shape))
        _yuv_size(arr.shape[-2:-4:-1], 'frames_to_yuv')
        ctx = ctx if ctx is not None else runtime.get_context(device)
        up = ctx.upload(arr[None] if arr.ndim == 3 else arr)
        try:
            return up.to_yuv(spec, ctx=ctx)
        finally:
            up.free()
    for b in batches:
        _yuv_size(b.shape[2:0:-1], 'frames_to_yuv')
    if ctx is None:
        ctx = runtime.get_context(device if device is not None else batches[0].ctx.device_id)
    if len(batches) == 1:
        return batches[0].to_yuv(spec, ctx=ctx)
    per = lib.yuv_frame_bytes(spec['format'], batches[0].shape[1], batches[0].shape[2])
    out = np.empty((sum(b.shape[0] for b in batches), per), np.uint8)
    at = 0
    for b in batches:
        b.to_yuv(spec, out=out[at:at + b.shape[0]], ctx=ctx)
        at += b.shape[0]
    return out
