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
    if isinstance(frames, lib.Frames):
        batches = [frames]
    elif isinstance(frames, (list, tuple)) and frames and all(isinstance(b, lib.Frames) for b in frames):
        batches = list(frames)
    else:
        raise ValueError('resize_frames: a lib.Frames batch or a non-empty list of them')
    code = lib.resample_filter(resample)
    try:
        width, height = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError('resize_frames: size must be (width, height), got %r' % (size,)) from None
    if not (1 <= width <= lib.RESAMPLE_SIDE_LIMIT and 1 <= height <= lib.RESAMPLE_SIDE_LIMIT):
        raise ValueError('resize_frames: size must be within 1 .. %d a side, got %r' % (lib.RESAMPLE_SIDE_LIMIT, size))
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
