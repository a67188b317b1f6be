"""ctypes binding of `libterran_amd.so` (the C ABI in include/terran_amd.h).

There is no fallback: if the library is missing or no gfx950 device is usable, the
product path raises `TerranAmdError`.  Nothing here imports `oracle/`.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, 'libterran_amd.so')

OK, E_INVALID, E_DEVICE, E_CAPACITY, E_OVERFLOW, E_RANGE = 0, -1, -2, -3, -4, -5
_CODES = {E_INVALID: 'TA_E_INVALID', E_DEVICE: 'TA_E_DEVICE', E_CAPACITY: 'TA_E_CAPACITY', E_OVERFLOW: 'TA_E_OVERFLOW',
          E_RANGE: 'TA_E_RANGE'}


class TerranAmdError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__('%s: %s' % (_CODES.get(code, code), msg))
        self.code = code


c_int, c_float, c_double, c_void_p, c_size_t = C.c_int, C.c_float, C.c_double, C.c_void_p, C.c_size_t
P = C.POINTER
u8p, i32p, f32p, f64p = P(C.c_uint8), P(C.c_int32), P(C.c_float), P(C.c_double)

# name -> (restype, argtypes); mirrors include/terran_amd.h one to one
SIGNATURES = {
    'ta_version': (C.c_char_p, []),
    'ta_device_count': (c_int, []),
    'ta_device_pci_bus_id': (c_int, [c_int, C.c_char_p, c_int]),
    'ta_ctx_create': (c_int, [c_int, P(c_void_p)]),
    'ta_ctx_destroy': (None, [c_void_p]),
    'ta_last_error': (C.c_char_p, [c_void_p]),
    'ta_ctx_sync': (c_int, [c_void_p]),
    'ta_profile_enable': (c_int, [c_void_p, c_int]),
    'ta_profile_reset': (c_int, [c_void_p]),
    'ta_profile_read': (c_int, [c_void_p, c_int, f64p, P(C.c_int64), f64p]),
    'ta_timer_start': (c_int, [c_void_p]),
    'ta_timer_stop': (c_int, [c_void_p, f64p]),
    'ta_host_alloc': (c_int, [c_void_p, c_size_t, P(c_void_p)]),
    'ta_host_free': (None, [c_void_p, c_void_p]),
    'ta_frames_upload': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, P(c_void_p)]),
    'ta_frames_alloc': (c_int, [c_void_p, c_int, c_int, c_int, P(c_void_p)]),
    'ta_frames_shape': (c_int, [c_void_p, P(c_int), P(c_int), P(c_int)]),
    'ta_frames_download': (c_int, [c_void_p, c_void_p]),
    'ta_frames_free': (None, [c_void_p]),
    'ta_frames_resize': (c_int, [c_void_p, c_void_p, c_int, c_int, P(c_void_p)]),
    'ta_frames_resize_bicubic': (c_int, [c_void_p, c_void_p, c_int, c_int, P(c_void_p)]),
    'ta_frames_paste': (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int]),
    'ta_frames_draw': (c_int, [c_void_p, c_void_p, c_void_p, c_int]),
    'ta_frames_draw_masks': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_size_t]),
    'ta_frames_blur': (c_int, [c_void_p, c_void_p, c_void_p, c_int]),
    'ta_blur_plan': (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    'ta_frames_resample': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, P(c_void_p)]),
    'ta_resample_plan': (c_int, [c_int, c_double, c_double, c_int, c_int, c_void_p, c_void_p, c_int, P(c_int)]),
    'ta_frames_pixelate': (c_int, [c_void_p, c_void_p, c_void_p, c_int]),
    'ta_frames_transform': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, P(c_void_p)]),
    'ta_frames_transform_mesh': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int,
                                         c_void_p, P(c_void_p)]),
    'ta_mesh_plan': (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, P(c_int)]),
    'ta_frames_transpose': (c_int, [c_void_p, c_void_p, c_int, P(c_void_p)]),
    'ta_frames_histogram': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p]),
    'ta_frames_point': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int]),
    'ta_frames_saturate': (c_int, [c_void_p, c_void_p, c_void_p, c_int]),
    'ta_frames_filter': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int]),
    'ta_filter_plan': (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    'ta_frames_color': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_size_t]),
    'ta_color_plan': (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_size_t, c_void_p, c_void_p]),
    'ta_yuv_frame_bytes': (c_size_t, [c_int, c_int, c_int]),
    'ta_frames_from_yuv': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, P(c_void_p)]),
    'ta_frames_to_yuv': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    'ta_yuv_convert_samples': (c_int, [c_void_p, c_int, c_void_p, c_size_t, c_void_p]),
    'ta_frames_combine': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_size_t]),
    'ta_frames_tiles': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, P(c_void_p)]),
    'ta_jpeg_coefficients': (c_int, [c_void_p, c_size_t, c_void_p, c_void_p, C.c_int64, C.c_char_p, c_int]),
    'ta_jpeg_decode': (c_int, [c_void_p, P(c_void_p), P(c_size_t), c_int, c_int, c_int, P(c_void_p), P(C.c_int32),
                               P(C.c_int32)]),
    'ta_jpeg_last_stats': (c_int, [c_void_p, c_void_p, c_void_p]),
    'ta_jpeg_encode_header': (c_int, [c_int, c_int, c_int, c_int, c_void_p, c_size_t, P(c_size_t)]),
    'ta_jpeg_encode': (c_int, [c_void_p, c_void_p, c_int, c_int, P(c_void_p), P(c_size_t)]),
    'ta_jpeg_encode_last_stats': (c_int, [c_void_p, c_void_p, c_void_p]),
    'ta_jpeg_encode_opt': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, P(c_void_p), P(c_size_t)]),
    'ta_jpeg_optimal_table': (c_int, [c_void_p, c_void_p, c_void_p, P(c_int)]),
    'ta_jpeg_encode_last_opt_stats': (c_int, [c_void_p, c_void_p]),
    'ta_program_check': (c_int, [c_int, c_void_p, c_size_t, C.c_char_p, c_size_t]),
    'ta_model_load': (c_int, [c_void_p, c_int, c_void_p, c_size_t, P(c_void_p)]),
    'ta_model_free': (None, [c_void_p]),
    'ta_model_kind': (c_int, [c_void_p]),
    'ta_model_forward_frames': (c_int, [c_void_p, c_void_p]),
    'ta_model_forward_crops': (c_int, [c_void_p, c_void_p, c_int]),
    'ta_model_tensor_shape': (c_int, [c_void_p, c_int, P(c_int), P(c_int), P(c_int), P(c_int)]),
    'ta_model_tensor_unscale': (c_int, [c_void_p, c_int, c_void_p, c_int]),
    'ta_model_debug_amax': (c_int, [c_void_p, c_int, c_void_p, c_int]),
    'ta_model_graph_probe': (c_int, [c_void_p, c_int, c_void_p]),
    'ta_model_read_tensor': (c_int, [c_void_p, c_int, c_int, c_int, c_void_p]),
    'ta_retinaface_run': (c_int, [c_void_p, c_void_p, c_float, c_float, c_int, c_void_p, c_void_p, c_void_p,
                                  c_void_p, P(C.c_int32)]),
    'ta_retinaface_postprocess': (c_int, [c_void_p, P(c_void_p), c_int, c_int, c_int, c_float, c_float, c_int,
                                          c_void_p, c_void_p, c_void_p, c_void_p, P(C.c_int32)]),
    'ta_detections_merge': (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_float, c_int, c_float,
                                    c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, P(C.c_int32)]),
    'ta_poses_merge': (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_int, c_double, c_double, c_int, c_int, c_int,
                               c_void_p, c_void_p, c_void_p, c_void_p, P(C.c_int32)]),
    'ta_faces_poses_link': (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p,
                                    c_void_p, P(C.c_int32)]),
    'ta_poses_track': (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p,
                               c_void_p, c_void_p]),
    'ta_poses_paint': (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int]),
    'ta_tracks_fill': (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int,
                               P(C.c_int32)]),
    'ta_arcface_embed_crops': (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p]),
    'ta_arcface_embed_faces': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    'ta_arcface_embed_faces_multi': (c_int, [c_void_p, P(c_void_p), c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p,
                                             c_void_p]),
    'ta_cosine_distance': (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_void_p]),
    'ta_gallery_create': (c_int, [c_void_p, c_int, C.c_int64, P(c_void_p)]),
    'ta_gallery_free': (None, [c_void_p]),
    'ta_gallery_add': (c_int, [c_void_p, c_void_p, c_void_p, C.c_int64, c_int]),
    'ta_gallery_remove': (c_int, [c_void_p, c_void_p, c_int, P(C.c_int64)]),
    'ta_gallery_clear': (c_int, [c_void_p]),
    'ta_gallery_size': (c_int, [c_void_p, P(C.c_int64), P(C.c_int64)]),
    'ta_gallery_download': (c_int, [c_void_p, c_void_p, c_void_p]),
    'ta_gallery_search': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    'ta_gallery_cluster': (c_int, [c_void_p, C.c_float, c_int, c_void_p, c_void_p, P(C.c_int32), P(C.c_int32)]),
    'ta_openpose_run': (c_int, [c_void_p, c_void_p, c_double, c_int, c_void_p, c_void_p, c_void_p, P(C.c_int32)]),
    'ta_openpose_group': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_double, c_int, c_void_p,
                                  c_void_p, c_void_p, P(C.c_int32)]),
    'ta_bicubic_x8': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    'ta_openpose_last_stats': (c_int, [c_void_p, c_void_p, c_void_p]),
    'ta_openpose_debug_read': (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                       c_void_p]),
    'ta_openpose_debug_capacity': (c_int, [c_void_p, c_int, c_void_p]),
    'ta_debug_conv_variant': (c_int, [c_void_p, c_int]),
    'ta_debug_range_check': (c_int, [c_void_p]),
    'ta_debug_conv_counts': (c_int, [c_void_p, c_void_p, c_int]),
    'ta_debug_kernel_work': (c_int, [c_void_p, C.c_char_p, c_size_t, c_int]),
}

# gallery.hip: rows per workgroup tile, queries per MFMA group, the largest k of ta_gallery_search
GALLERY_ROW_TILE, GALLERY_QUERY_GROUP, GALLERY_MAX_K = 128, 32, 16
# gallery_cluster.hip: ta_gallery_cluster pairs tiles of GALLERY_ROW_TILE rows; the most rows it takes (a bit matrix of 8 GiB)
GALLERY_CLUSTER_MAX_ROWS = 1 << 18

# ta_draw_prim (include/terran_amd.h) and its kinds TA_DRAW_*
DRAW_BAR, DRAW_LINE, DRAW_DISC, DRAW_MASK = 0, 1, 2, 3
PRIM_DT = np.dtype([('frame', '<i4'), ('kind', '<i4'), ('x0', '<i4'), ('y0', '<i4'), ('x1', '<i4'), ('y1', '<i4'),
                    ('width', '<i4'), ('rgba', 'u1', (4,))])
assert PRIM_DT.itemsize == 32

# ta_blur_region (include/terran_amd.h) and its shapes TA_BLUR_*; the box is half-open
BLUR_BOX, BLUR_ELLIPSE = 0, 1
BLUR_DT = np.dtype([('frame', '<i4'), ('x0', '<i4'), ('y0', '<i4'), ('x1', '<i4'), ('y1', '<i4'), ('shape', '<i4'),
                    ('radius', '<f4')])
assert BLUR_DT.itemsize == 28


def blur_plan(regions):
    """Host only (no context, no device): ta_blur_plan -> (round of every region, float32 box radius, uint32 (n, 2)
    weights ww, fw): what ta_frames_blur derives from a BLUR_DT array before it launches anything."""
    lib = load()
    regions, p, n = _records(regions, BLUR_DT)
    rounds, fr, w = np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros((n, 2), np.uint32)
    rc = lib.ta_blur_plan(p, n, ptr(rounds), ptr(fr), ptr(w))
    if rc != OK:
        raise TerranAmdError(rc, 'blur_plan: an empty or inverted box, an unknown shape or a bad radius')
    return rounds, fr, w


# ta_resample_region, ta_pixelate_region (include/terran_amd.h) and the filters TA_RESAMPLE_*: Pillow's codes
NEAREST, LANCZOS, BILINEAR, BICUBIC, BOX, HAMMING = 0, 1, 2, 3, 4, 5
RESAMPLE_FILTERS = {'nearest': NEAREST, 'lanczos': LANCZOS, 'bilinear': BILINEAR, 'bicubic': BICUBIC, 'box': BOX,
                    'hamming': HAMMING}
RESAMPLE_DT = np.dtype([('frame', '<i4'), ('x0', '<f4'), ('y0', '<f4'), ('x1', '<f4'), ('y1', '<f4')])
assert RESAMPLE_DT.itemsize == 20
PIXELATE_DT = np.dtype([('frame', '<i4'), ('x0', '<i4'), ('y0', '<i4'), ('x1', '<i4'), ('y1', '<i4'), ('shape', '<i4'),
                        ('block', '<i4')])
assert PIXELATE_DT.itemsize == 28
RESAMPLE_SIDE_LIMIT = 16384                             # an output side, a pixelate block

# ta_hist_region, ta_point_region, ta_saturate_region (include/terran_amd.h) and the modes TA_HIST_*; shapes: BLUR_*
HIST_RGB, HIST_L = 0, 1
HIST_MODES = {'RGB': HIST_RGB, 'L': HIST_L}
HIST_DT = np.dtype([('frame', '<i4'), ('x0', '<i4'), ('y0', '<i4'), ('x1', '<i4'), ('y1', '<i4'), ('shape', '<i4')])
assert HIST_DT.itemsize == 24
POINT_DT = np.dtype([('frame', '<i4'), ('x0', '<i4'), ('y0', '<i4'), ('x1', '<i4'), ('y1', '<i4'), ('shape', '<i4'),
                     ('lut', '<i4')])
assert POINT_DT.itemsize == 28
SATURATE_DT = np.dtype([('frame', '<i4'), ('x0', '<i4'), ('y0', '<i4'), ('x1', '<i4'), ('y1', '<i4'), ('shape', '<i4'),
                        ('factor', '<f4')])
assert SATURATE_DT.itemsize == 28

# ta_filter_region, ta_filter_spec (include/terran_amd.h) and the kinds TA_FILTER_*; shapes: BLUR_*
FILTER_KERNEL, FILTER_RANK, FILTER_UNSHARP = 0, 1, 2
FILTER_REGION_DT = np.dtype([('frame', '<i4'), ('x0', '<i4'), ('y0', '<i4'), ('x1', '<i4'), ('y1', '<i4'), ('shape', '<i4'),
                             ('spec', '<i4')])
assert FILTER_REGION_DT.itemsize == 28
FILTER_SPEC_DT = np.dtype([('kind', '<i4'), ('size', '<i4'), ('rank', '<i4'), ('has_factor', '<i4'), ('kernel', '<f4', (25,)),
                           ('scale', '<f4'), ('offset', '<f4'), ('factor', '<f4'), ('radius', '<f4'), ('percent', '<i4'),
                           ('threshold', '<i4')])
assert FILTER_SPEC_DT.itemsize == 140

# ta_combine_region (include/terran_amd.h), the ops TA_COMBINE_* and the mask kinds TA_MASK_*; shapes: BLUR_*
(COMBINE_PASTE, COMBINE_BLEND, COMBINE_LIGHTER, COMBINE_DARKER, COMBINE_DIFFERENCE, COMBINE_MULTIPLY, COMBINE_SCREEN, COMBINE_ADD,
 COMBINE_SUBTRACT, COMBINE_ADD_MODULO, COMBINE_SUBTRACT_MODULO, COMBINE_SOFT_LIGHT, COMBINE_HARD_LIGHT, COMBINE_OVERLAY) = range(14)
COMBINE_OPS = {'paste': COMBINE_PASTE, 'blend': COMBINE_BLEND, 'lighter': COMBINE_LIGHTER, 'darker': COMBINE_DARKER,
               'difference': COMBINE_DIFFERENCE, 'multiply': COMBINE_MULTIPLY, 'screen': COMBINE_SCREEN, 'add': COMBINE_ADD,
               'subtract': COMBINE_SUBTRACT, 'add_modulo': COMBINE_ADD_MODULO, 'subtract_modulo': COMBINE_SUBTRACT_MODULO,
               'soft_light': COMBINE_SOFT_LIGHT, 'hard_light': COMBINE_HARD_LIGHT, 'overlay': COMBINE_OVERLAY}
MASK_NONE, MASK_CONSTANT, MASK_BITMAP, MASK_FRAMES = 0, 1, 2, 3
COMBINE_DT = np.dtype([('frame', '<i4'), ('x0', '<i4'), ('y0', '<i4'), ('x1', '<i4'), ('y1', '<i4'), ('shape', '<i4'),
                       ('src_frame', '<i4'), ('src_x', '<i4'), ('src_y', '<i4'), ('op', '<i4'), ('alpha', '<f4'), ('offset', '<i4'),
                       ('mask_kind', '<i4'), ('mask_value', '<i4'), ('mask_frame', '<i4'), ('mask_x', '<i4'), ('mask_y', '<i4'),
                       ('mask_band', '<i4')])
assert COMBINE_DT.itemsize == 72

# ta_tile, ta_merge_group (include/terran_amd.h); MERGE_MAX_PER_FRAME: the candidates ta_detections_merge takes per frame
TILE_DT = np.dtype([('frame', '<i4'), ('y', '<i4'), ('x', '<i4')])
assert TILE_DT.itemsize == 12
MERGE_GROUP_DT = np.dtype([('frame', '<i4'), ('first', '<i4'), ('count', '<i4'), ('ox', '<f4'), ('oy', '<f4'), ('zoom', '<f4'),
                           ('x0', '<f4'), ('y0', '<f4'), ('x1', '<f4'), ('y1', '<f4'), ('interior', '<i4')])
assert MERGE_GROUP_DT.itemsize == 44
MERGE_IOU, MERGE_IOS = 0, 1
MERGE_METRICS = {'iou': MERGE_IOU, 'ios': MERGE_IOS}
MERGE_MAX_PER_FRAME = 16384
# ta_pose_group: the integer analogue for ta_poses_merge, with the same limit per frame
POSE_GROUP_DT = np.dtype([('frame', '<i4'), ('first', '<i4'), ('count', '<i4'), ('ox', '<i4'), ('oy', '<i4'), ('x0', '<i4'), ('y0', '<i4'),
                          ('x1', '<i4'), ('y1', '<i4'), ('interior', '<i4')])
assert POSE_GROUP_DT.itemsize == 40
# ta_faces_poses_link: the faces, and the poses, it takes per frame
LINK_MAX_PER_FRAME = 16384
# ta_poses_track: the skeletons it takes per frame
TRACK_MAX_PER_FRAME = 4096
# ta_tracks_fill: the rows it takes, and gives, per frame
FILL_MAX_PER_FRAME = 16384

# ta_color_region, ta_color_op (include/terran_amd.h) and the kinds TA_COLOR_*; shapes: BLUR_*
COLOR_MATRIX, COLOR_RGB2YCBCR, COLOR_YCBCR2RGB, COLOR_RGB2HSV, COLOR_HSV2RGB, COLOR_LUT3D = range(6)
COLOR_REGION_DT = np.dtype([('frame', '<i4'), ('x0', '<i4'), ('y0', '<i4'), ('x1', '<i4'), ('y1', '<i4'), ('shape', '<i4'),
                            ('op', '<i4')])
assert COLOR_REGION_DT.itemsize == 28
COLOR_OP_DT = np.dtype([('kind', '<i4'), ('size', '<i4', (3,)), ('table', '<i4')])
assert COLOR_OP_DT.itemsize == 20


def _color_args(ops, tables):
    ops = np.ascontiguousarray(ops, dtype=COLOR_OP_DT).reshape(-1)
    tables = np.ascontiguousarray(tables if tables is not None else [], dtype=np.float32).reshape(-1)
    return ops, tables


def color_plan(regions, ops, tables=None):
    """Host only (no context, no device): ta_color_plan -> (round of every region, a list with one entry per op: the int16
    (s2, s1, s0, 4) nodes the device reads for a COLOR_LUT3D op -- R, G, B entry and 0 --, None for another kind): what
    ta_frames_color derives from a COLOR_REGION_DT array, a COLOR_OP_DT array and their float32 tables before it launches
    anything."""
    lib = load()
    regions, p, n = _records(regions, COLOR_REGION_DT)
    ops, tables = _color_args(ops, tables)
    counts = [int(np.prod(o['size'], dtype=np.int64)) if o['kind'] == COLOR_LUT3D and o['size'].min() >= 2 and o['size'].max() <= 65 else 0 for o in ops]
    rounds, nodes = np.zeros(n, np.int32), np.zeros(4 * sum(counts) + 4, np.int16)
    rc = lib.ta_color_plan(p, n, ptr(ops) if len(ops) else None, len(ops), ptr(tables) if len(tables) else None, len(tables),
                           ptr(rounds), ptr(nodes))
    if rc != OK:
        raise TerranAmdError(rc, 'color_plan: a bad box, shape or op index, or an op ta_frames_color refuses')
    out, at = [], 0
    for o, c in zip(ops, counts):
        out.append(nodes[at:at + 4 * c].reshape(int(o['size'][2]), int(o['size'][1]), int(o['size'][0]), 4) if c else None)
        at += 4 * c
    return rounds, out


# ta_yuv_spec (include/terran_amd.h) and the values of its fields, TA_YUV_*
YUV_420P, YUV_NV12, YUV_444P = 0, 1, 2
YUV_BT601, YUV_BT709 = 0, 1
YUV_TV, YUV_PC = 0, 1
YUV_NEAREST, YUV_BILINEAR = 0, 1
YUV_LEFT, YUV_CENTER = 0, 1
YUV_FORMATS = {'yuv420p': YUV_420P, 'nv12': YUV_NV12, 'yuv444p': YUV_444P}
YUV_MATRICES = {'bt601': YUV_BT601, 'bt709': YUV_BT709}
YUV_RANGES = {'tv': YUV_TV, 'pc': YUV_PC}
YUV_CHROMAS = {'nearest': YUV_NEAREST, 'bilinear': YUV_BILINEAR}
YUV_SITINGS = {'left': YUV_LEFT, 'center': YUV_CENTER}
YUV_SPEC_DT = np.dtype([('format', '<i4'), ('matrix', '<i4'), ('range', '<i4'), ('chroma', '<i4'), ('siting', '<i4')])
assert YUV_SPEC_DT.itemsize == 20


def _yuv_spec(spec):
    """One ta_yuv_spec record: a YUV_SPEC_DT record or five integers (format, matrix, range, chroma, siting)."""
    if isinstance(spec, np.ndarray) and spec.dtype == YUV_SPEC_DT:
        return np.ascontiguousarray(spec).reshape(1)
    return np.array([tuple(int(v) for v in spec)], dtype=YUV_SPEC_DT)


def yuv_frame_bytes(format, h, w):
    """Host only: ta_yuv_frame_bytes, the bytes of one h x w frame; 0 for an unknown format or a side outside 1 .. 65535."""
    return int(load().ta_yuv_frame_bytes(int(format), int(h), int(w)))


def yuv_convert_samples(spec, to_yuv, triples):
    """Host only (no context, no device): ta_yuv_convert_samples, (n, 3) uint8 triples through the arithmetic the kernels
    run -- (Y, Cb, Cr) -> (R, G, B), or with to_yuv (R, G, B) -> (Y, Cb, Cr) of a single pixel."""
    src = np.ascontiguousarray(triples, dtype=np.uint8)
    if src.ndim != 2 or src.shape[1] != 3:
        raise ValueError('yuv_convert_samples: triples must be (n, 3) uint8, got %s' % (src.shape,))
    s = _yuv_spec(spec)
    out = np.empty_like(src)
    rc = load().ta_yuv_convert_samples(ptr(s), int(bool(to_yuv)), ptr(src), len(src), ptr(out))
    if rc != OK:
        raise TerranAmdError(rc, 'yuv_convert_samples: invalid spec')
    return out


def filter_plan(regions, specs):
    """Host only (no context, no device): ta_filter_plan -> (round of every region, float32 (n_specs, 25) normalised
    kernels kernel / scale, float32 (n_specs,) offsets offset + 0.5): what ta_frames_filter derives from a FILTER_REGION_DT
    and a FILTER_SPEC_DT array before it launches anything; zeros for the specs that are no kernels."""
    lib = load()
    regions, p, n = _records(regions, FILTER_REGION_DT)
    specs = np.ascontiguousarray(specs, dtype=FILTER_SPEC_DT).reshape(-1)
    m = len(specs)
    rounds, kernels, offsets = np.zeros(n, np.int32), np.zeros((m, 25), np.float32), np.zeros(m, np.float32)
    rc = lib.ta_filter_plan(p, n, ptr(specs) if m else None, m, ptr(rounds), ptr(kernels), ptr(offsets))
    if rc != OK:
        raise TerranAmdError(rc, 'filter_plan: a bad box, shape or spec index, or a spec ta_frames_filter refuses')
    return rounds, kernels, offsets


def resample_filter(resample):
    """A filter's name ('nearest', 'lanczos', 'bilinear', 'bicubic', 'box', 'hamming') or Pillow's integer code -> the
    code, or ValueError."""
    if isinstance(resample, str) and resample.lower() in RESAMPLE_FILTERS:
        return RESAMPLE_FILTERS[resample.lower()]
    if isinstance(resample, (int, np.integer)) and not isinstance(resample, bool) and int(resample) in RESAMPLE_FILTERS.values():
        return int(resample)
    raise ValueError('resample must be one of %s or Pillow\'s code 0 .. 5, got %r' % (sorted(RESAMPLE_FILTERS), resample))


def resample_plan(in_size, b0, b1, out_size, filter):
    """Host only (no context, no device): ta_resample_plan -> (int32 (out_size, 2) bounds: first source sample and tap
    count, int32 (out_size, ksize) coefficients, 2^22 = 1): one axis' tables as ta_frames_resample derives them."""
    lib = load()
    k = c_int()
    rc = lib.ta_resample_plan(int(in_size), float(b0), float(b1), int(out_size), int(filter), None, None, 0, C.byref(k))
    if rc != E_CAPACITY:
        raise TerranAmdError(rc, 'resample_plan(%r, %r, %r, %r, %r)' % (in_size, b0, b1, out_size, filter))
    bounds, coefs = np.zeros((out_size, 2), np.int32), np.zeros((out_size, k.value), np.int32)
    rc = lib.ta_resample_plan(int(in_size), float(b0), float(b1), int(out_size), int(filter), ptr(bounds), ptr(coefs),
                              coefs.size, C.byref(k))
    if rc != OK:
        raise TerranAmdError(rc, 'resample_plan(%r, %r, %r, %r, %r)' % (in_size, b0, b1, out_size, filter))
    return bounds, coefs


# ta_transform_region (include/terran_amd.h), the methods TA_TRANSFORM_* and the ops of ta_frames_transpose: Pillow's codes
AFFINE, PERSPECTIVE = 0, 2
TRANSFORM_METHODS = {'affine': AFFINE, 'perspective': PERSPECTIVE}
TRANSFORM_FILTERS = (NEAREST, BILINEAR, BICUBIC)
TRANSFORM_DT = np.dtype([('frame', '<i4'), ('method', '<i4'), ('a', '<f8', (8,))])
assert TRANSFORM_DT.itemsize == 72
FLIP_LEFT_RIGHT, FLIP_TOP_BOTTOM, ROTATE_90, ROTATE_180, ROTATE_270, TRANSPOSE, TRANSVERSE = range(7)
TRANSPOSE_OPS = {'flip_left_right': FLIP_LEFT_RIGHT, 'flip_top_bottom': FLIP_TOP_BOTTOM, 'rotate_90': ROTATE_90,
                 'rotate_180': ROTATE_180, 'rotate_270': ROTATE_270, 'transpose': TRANSPOSE, 'transverse': TRANSVERSE}


# ta_mesh_cell, ta_mesh_image (include/terran_amd.h): a cell's half-open box of the OUTPUT and its quadrilateral of the INPUT
# in Pillow's corner order nw, sw, se, ne; an output image's source frame and mesh.  TA_MESH_*: the tile and the limits
MESH_CELL_DT = np.dtype([('x0', '<i4'), ('y0', '<i4'), ('x1', '<i4'), ('y1', '<i4'), ('quad', '<f8', (8,))])
assert MESH_CELL_DT.itemsize == 80
MESH_IMAGE_DT = np.dtype([('frame', '<i4'), ('mesh', '<i4')])
assert MESH_IMAGE_DT.itemsize == 8
MESH_TILE_W, MESH_TILE_H = 64, 16
MESH_MAX_CELLS, MESH_MAX_ENTRIES = 1 << 20, 1 << 24
MESH_COORD_LIMIT = 1 << 24


def mesh_plan(cells, out_h, out_w):
    """Host only (no context, no device): ta_mesh_plan -> (float64 (n, 8) coefficients a0 .. a7, int32 (n, 4) clamped boxes
    cx0, cy0, cx1, cy1, int32 (tiles + 1,) tile_first, int32 tile_cells): what ta_frames_transform_mesh derives from ONE
    mesh (a MESH_CELL_DT array) and an output size before it launches anything.  Tile t (row-major over the
    MESH_TILE_W x MESH_TILE_H tiles of the output) holds the cells tile_cells[tile_first[t]:tile_first[t + 1]]."""
    lib = load()
    cells, p, n = _records(cells, MESH_CELL_DT)
    out_h, out_w = int(out_h), int(out_w)
    k = c_int()
    rc = lib.ta_mesh_plan(p, n, out_h, out_w, None, None, None, None, -1, C.byref(k))
    if rc != E_CAPACITY:
        raise TerranAmdError(rc, 'mesh_plan: a bad output size, box or corner, or more cells or tile entries than the limits')
    tiles = -(-out_w // MESH_TILE_W) * -(-out_h // MESH_TILE_H)
    coefs, boxes = np.zeros((n, 8), np.float64), np.zeros((n, 4), np.int32)
    first, entries = np.zeros(tiles + 1, np.int32), np.zeros(k.value, np.int32)
    rc = lib.ta_mesh_plan(p, n, out_h, out_w, ptr(coefs), ptr(boxes), ptr(first), ptr(entries), k.value, C.byref(k))
    if rc != OK:
        raise TerranAmdError(rc, 'mesh_plan')
    return coefs, boxes, first, entries


def transpose_op(op):
    """An op's name ('flip_left_right', ..., 'transverse') or Pillow's integer code -> the code, or ValueError."""
    if isinstance(op, str) and op.lower() in TRANSPOSE_OPS:
        return TRANSPOSE_OPS[op.lower()]
    if isinstance(op, (int, np.integer)) and not isinstance(op, bool) and 0 <= int(op) <= 6:
        return int(op)
    raise ValueError('op must be one of %s or Pillow\'s code 0 .. 6, got %r' % (sorted(TRANSPOSE_OPS), op))


# ta_jpeg_header and the decode paths TA_JPEG_* (include/terran_amd.h)
JPEG_DEVICE = 0
JPEG_INVALID = -1
JPEG_PATHS = {-1: 'invalid', 0: 'device', 1: 'progressive/lossless/hierarchical', 2: 'arithmetic', 3: 'precision',
              4: 'components', 5: 'rgb', 6: 'scans', 7: 'sampling'}
JPEG_HEADER_DT = np.dtype([('width', '<i4'), ('height', '<i4'), ('components', '<i4'), ('path', '<i4'),
                           ('h_samp', '<i4', (3,)), ('v_samp', '<i4', (3,)), ('quant_index', '<i4', (3,)),
                           ('blocks_w', '<i4', (3,)), ('blocks_h', '<i4', (3,)), ('restart_interval', '<i4'),
                           ('reserved', '<i4', (2,)), ('block_offset', '<i8', (3,)), ('blocks_total', '<i8'),
                           ('quant', '<u2', (4, 64))])
assert JPEG_HEADER_DT.itemsize == 632


def jpeg_coefficients(data, header_only=False):
    """Host only (no context, no device): ta_jpeg_coefficients -> (header record of JPEG_HEADER_DT, int16
    (blocks_total, 64) quantised coefficients in natural order, or None for a fallback image / header_only).
    Raises TerranAmdError(TA_E_INVALID) on malformed data."""
    lib = load()
    buf = np.frombuffer(bytes(data), np.uint8)
    hdr = np.zeros(1, JPEG_HEADER_DT)
    err = C.create_string_buffer(256)
    rc = lib.ta_jpeg_coefficients(ptr(buf), buf.size, ptr(hdr), None, 0, err, len(err))
    if rc != OK:
        raise TerranAmdError(rc, err.value.decode(errors='replace'))
    if header_only or hdr['path'][0] != JPEG_DEVICE:
        return hdr[0], None
    coefs = np.empty((int(hdr['blocks_total'][0]), 64), np.int16)
    rc = lib.ta_jpeg_coefficients(ptr(buf), buf.size, ptr(hdr), ptr(coefs), coefs.shape[0], err, len(err))
    if rc != OK:
        raise TerranAmdError(rc, err.value.decode(errors='replace'))
    return hdr[0], coefs


def jpeg_encode_header(h, w, quality=75, subsampling=2):
    """Host only (no context, no device): ta_jpeg_encode_header -> the bytes SOI .. SOS Pillow writes for an h x w RGB
    image."""
    lib = load()
    size = c_size_t()
    buf = np.zeros(1024, np.uint8)
    rc = lib.ta_jpeg_encode_header(int(h), int(w), int(quality), int(subsampling), ptr(buf), buf.size, C.byref(size))
    if rc != OK:
        raise TerranAmdError(rc, 'jpeg_encode_header(%r, %r, %r, %r)' % (h, w, quality, subsampling))
    return buf[:size.value].tobytes()


def jpeg_optimal_table(freq):
    """Host only (no context, no device): ta_jpeg_optimal_table -> (counts of codes of length 1..16, symbols in code
    order) of libjpeg's optimal Huffman table for the symbol frequencies freq[0..255] (a 257th entry is ignored)."""
    lib = load()
    f = np.zeros(257, np.int64)
    freq = np.asarray(freq, np.int64).reshape(-1)
    f[:min(256, freq.size)] = freq[:256]
    bits, vals, n = np.zeros(17, np.uint8), np.zeros(256, np.uint8), c_int()
    rc = lib.ta_jpeg_optimal_table(ptr(f), ptr(bits), ptr(vals), C.byref(n))
    if rc != OK:
        raise TerranAmdError(rc, 'jpeg_optimal_table: frequencies must be 0 .. 10^9 - 1 and not all zero')
    return bits[1:].tolist(), vals[:n.value].tolist()


def check_program(program_or_blob, kind=None):
    """Host only (no context, no device): ta_program_check on a pack.Program or on the bytes of a blob (then `kind` is
    needed) -- what ta_model_load refuses before it touches the device.  Raises TerranAmdError(TA_E_INVALID) with the defect."""
    lib = load()
    if isinstance(program_or_blob, (bytes, bytearray, memoryview)):
        blob = bytes(program_or_blob)
        if kind is None:
            raise ValueError('check_program: the bytes of a blob need `kind` (a pack.MODEL_* constant)')
    else:
        blob, kind = program_or_blob.blob(), program_or_blob.kind if kind is None else kind
    err = C.create_string_buffer(256)
    rc = lib.ta_program_check(int(kind), blob, len(blob), err, len(err))
    if rc != OK:
        raise TerranAmdError(rc, err.value.decode(errors='replace'))


def check_jpeg_options(quality, subsampling):
    """The encoder's options as ints, or ValueError (before anything is launched): quality 1..100, subsampling 0 / 1 / 2."""
    if isinstance(quality, bool) or not isinstance(quality, (int, np.integer)) or not 1 <= quality <= 100:
        raise ValueError('JPEG quality must be an int in 1..100, got %r' % (quality,))
    if isinstance(subsampling, bool) or not isinstance(subsampling, (int, np.integer)) or subsampling not in (0, 1, 2):
        raise ValueError('JPEG subsampling must be 0 (4:4:4), 1 (4:2:2) or 2 (4:2:0), got %r' % (subsampling,))
    return int(quality), int(subsampling)


def check_jpeg_optimize(optimize):
    """Pillow's `optimize` as a bool, or ValueError (before anything is launched)."""
    if not isinstance(optimize, (bool, np.bool_)):
        raise ValueError('JPEG optimize must be True or False, got %r' % (optimize,))
    return bool(optimize)


# conv kernel variants (include/terran_amd.h TA_CONV_*)
CONV_VARIANTS = {'auto': 0, 'generic': 1, 'pipe64': 2, 'pipe128': 3, 'split_2x2': 4, 'split_2x2_p8': 5, 'split_2x4': 6,
                 'split_1x4': 7, 'win_2x2': 8, 'win_2x4': 9, 'win_1x4': 10, 'split_1x4_w2': 11, 'split_2x2_w2': 12}

_lib = None


def load():
    """Load the shared library (once).  Raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise TerranAmdError(E_DEVICE, 'libterran_amd.so not built (run `python -m terran_amd.build`); '
                                           'there is no CPU fallback')
        # the .so travels prebuilt to the GPU box: it must be the build of the sources that travel beside it
        from . import build as _build
        try:
            with open(_build.STAMP) as fh:
                stamp = fh.read().strip()
        except OSError:
            stamp = None
        try:
            current = _build.source_hash()
        except OSError:                             # relocated package without its sources: nothing to compare with
            current = stamp
        if (stamp is None or stamp != current) and not os.environ.get('TA_ALLOW_STALE_LIB'):
            raise TerranAmdError(E_DEVICE, 'libterran_amd.so was not built from the sources in terran_amd/csrc '
                                           '(run `python -m terran_amd.build`)')
        # A lane of the StreamPipeline is four HIP streams and a GPU runs several lanes; ROCm maps all streams of a process
        # onto GPU_MAX_HW_QUEUES hardware queues (default 4), and kernels of different streams that share a queue wait for
        # each other.  12 queues measured +3 % on the 1080p pipeline (16 streams).  Only a default: the user's setting wins,
        # and it has no effect when the HIP runtime was initialised before this library was loaded.
        os.environ.setdefault('GPU_MAX_HW_QUEUES', '12')
        # kernel-argument blocks in device memory instead of host-coherent memory: a conv workgroup's first instruction is the
        # fetch of its 400-byte launch record (~2 000 cycles from host memory; ArcFace at 64 crops 4.84 -> 4.67 ms)
        os.environ.setdefault('HIP_FORCE_DEV_KERNARG', '1')
        lib = C.CDLL(LIB_PATH)
        missing = []
        for name, (res, args) in SIGNATURES.items():
            try:
                fn = getattr(lib, name)
            except AttributeError:
                missing.append(name)
                continue
            fn.restype = res
            fn.argtypes = args
        if missing and not os.environ.get('TA_BRINGUP_ALLOW_MISSING'):
            raise TerranAmdError(E_INVALID, 'libterran_amd.so lacks ABI symbols: %s' % ', '.join(missing))
        _lib = lib
    return _lib


def ptr(a):
    return a.ctypes.data_as(c_void_p) if a is not None else None


def _records(a, dtype):
    """A record list as an ABI call takes it: (the contiguous array, its pointer or None when empty, its length)."""
    a = np.ascontiguousarray(a, dtype=dtype)
    return a, (ptr(a) if len(a) else None), len(a)


class Context:
    """One per GPU (and per host thread)."""

    def __init__(self, device_id=0):
        self.lib = load()
        h = c_void_p()
        rc = self.lib.ta_ctx_create(int(device_id), C.byref(h))
        if rc != OK:
            raise TerranAmdError(rc, 'ta_ctx_create(%d) failed: no usable gfx950 device '
                                     '(ta_device_count=%d)' % (device_id, self.lib.ta_device_count()))
        self.h = h
        self.device_id = device_id

    def check(self, rc):
        if rc != OK:
            raise TerranAmdError(rc, self.lib.ta_last_error(self.h).decode(errors='replace'))

    def last_error(self):
        return self.lib.ta_last_error(self.h).decode(errors='replace')

    def sync(self):
        self.check(self.lib.ta_ctx_sync(self.h))

    def close(self):
        if getattr(self, 'h', None):
            self.lib.ta_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # profiling / timing
    def profile(self, on):
        self.check(self.lib.ta_profile_enable(self.h, int(on)))

    def profile_reset(self):
        self.check(self.lib.ta_profile_reset(self.h))

    def profile_read(self, klass):
        ms, n, w = c_double(), C.c_int64(), c_double()
        self.check(self.lib.ta_profile_read(self.h, klass, C.byref(ms), C.byref(n), C.byref(w)))
        return ms.value, n.value, w.value

    def timer_start(self):
        self.check(self.lib.ta_timer_start(self.h))

    def timer_stop(self):
        ms = c_double()
        self.check(self.lib.ta_timer_stop(self.h, C.byref(ms)))
        return ms.value

    # frames
    def upload(self, images):
        images = np.ascontiguousarray(images, dtype=np.uint8)
        assert images.ndim == 4 and images.shape[3] == 3
        return Frames(self, images)

    def frames_from_yuv(self, data, n, h, w, spec):
        """ta_frames_from_yuv: `data`, a contiguous uint8 array of exactly n raw YUV frames of h x w (pinned or not), ->
        a NEW resident Frames batch.  `spec`: a YUV_SPEC_DT record (image.yuv_spec)."""
        s = _yuv_spec(spec)
        if not (isinstance(data, np.ndarray) and data.dtype == np.uint8 and data.flags['C_CONTIGUOUS']):
            data = np.ascontiguousarray(np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else data,
                                        dtype=np.uint8)
        n, h, w = int(n), int(h), int(w)
        per = yuv_frame_bytes(s['format'][0], h, w)
        if per and n > 0 and data.size != n * per:
            raise ValueError('frames_from_yuv: %d bytes are not %d frames of %d bytes' % (data.size, n, per))
        hd = c_void_p()
        self.check(self.lib.ta_frames_from_yuv(self.h, ptr(data), n, h, w, ptr(s), C.byref(hd)))
        return Frames(self, handle=hd)

    def pinned_array(self, shape):
        """uint8 numpy array backed by page-locked host memory (freed with `free_pinned`)."""
        n = int(np.prod(shape))
        p = c_void_p()
        self.check(self.lib.ta_host_alloc(self.h, n, C.byref(p)))
        arr = np.ctypeslib.as_array((C.c_uint8 * n).from_address(p.value)).reshape(shape)
        arr_ptr = p.value
        return arr, arr_ptr

    def free_pinned(self, ptr):
        if getattr(self, 'h', None):
            self.lib.ta_host_free(self.h, c_void_p(ptr))

    def frames_tiles(self, src, tiles, th, tw):
        """ta_frames_tiles: `tiles`, a TILE_DT array (frame, y, x), cut out of the resident batch `src` in one launch -> a NEW
        resident Frames batch (n, th, tw, 3), or None for no tiles."""
        tiles, p, n = _records(tiles, TILE_DT)
        hd = c_void_p()
        self.check(self.lib.ta_frames_tiles(self.h, src.h, p, n, int(th), int(tw), C.byref(hd)))
        return Frames(self, handle=hd) if hd.value else None

    def detections_merge(self, groups, n_frames, boxes, landmarks, scores, nms_thr, metric=MERGE_IOU, edge=0.0, capacity=None):
        """ta_detections_merge: candidates of tiles (`groups`, a MERGE_GROUP_DT array sorted by frame) -> (counts (n_frames,)
        int32, boxes (T, 4), landmarks (T, 5, 2), scores (T,) float32, source (T,) int32 candidate rows): mapped to frame
        coordinates, cut faces dropped, ordered and suppressed across tiles, frames concatenated.  `capacity`: the first
        size of the output arrays (tests); a short one is retried with what the call asks for."""
        groups, gp, ng = _records(groups, MERGE_GROUP_DT)
        boxes = np.ascontiguousarray(boxes, dtype=np.float32).reshape(-1, 4)
        landmarks = np.ascontiguousarray(landmarks, dtype=np.float32).reshape(-1, 5, 2)
        scores = np.ascontiguousarray(scores, dtype=np.float32).reshape(-1)
        c = len(scores)
        if len(boxes) != c or len(landmarks) != c:
            raise ValueError('detections_merge: %d boxes, %d landmarks, %d scores' % (len(boxes), len(landmarks), c))
        n_frames = int(n_frames)
        counts = np.zeros(max(n_frames, 1), np.int32)
        cap = c if capacity is None else int(capacity)
        while True:
            ob, ol = np.empty((max(cap, 1), 4), np.float32), np.empty((max(cap, 1), 5, 2), np.float32)
            osc, src = np.empty(max(cap, 1), np.float32), np.empty(max(cap, 1), np.int32)
            req = C.c_int32(0)
            rc = self.lib.ta_detections_merge(self.h, gp, ng, n_frames, ptr(boxes), ptr(landmarks), ptr(scores), c, float(nms_thr),
                                              int(metric), float(edge), cap, ptr(counts), ptr(ob), ptr(ol), ptr(osc), ptr(src),
                                              C.byref(req))
            if rc == E_CAPACITY and req.value > cap:
                cap = int(req.value)
                continue
            self.check(rc)
            break
        t = int(counts[:n_frames].sum())
        return counts[:n_frames], ob[:t], ol[:t], osc[:t], src[:t]

    def poses_merge(self, groups, n_frames, keypoints, scores, radius=0.1, agree=0.5, min_shared=3, edge=0, capacity=None):
        """ta_poses_merge: poses of tiles (`groups`, a POSE_GROUP_DT array sorted by frame; keypoints (C, 18, 3) int32, scores (C,)
        float64) -> (counts (n_frames,) int32, keypoints (T, 18, 3) int32, scores (T,) float64, source (T,) int32 candidate
        rows): mapped to frame coordinates, cut bodies dropped, ordered and the duplicates across tiles suppressed, frames
        concatenated.  `capacity`: the first size of the output arrays (tests); a short one is retried with what the call asks
        for."""
        groups, gp, ng = _records(groups, POSE_GROUP_DT)
        keypoints = np.ascontiguousarray(keypoints, dtype=np.int32).reshape(-1, 18, 3)
        scores = np.ascontiguousarray(scores, dtype=np.float64).reshape(-1)
        c = len(scores)
        if len(keypoints) != c:
            raise ValueError('poses_merge: %d keypoint rows, %d scores' % (len(keypoints), c))
        n_frames = int(n_frames)
        counts = np.zeros(max(n_frames, 1), np.int32)
        cap = c if capacity is None else int(capacity)
        while True:
            okp = np.empty((max(cap, 1), 18, 3), np.int32)
            osc, src = np.empty(max(cap, 1), np.float64), np.empty(max(cap, 1), np.int32)
            req = C.c_int32(0)
            rc = self.lib.ta_poses_merge(self.h, gp, ng, n_frames, ptr(keypoints), ptr(scores), c, float(radius), float(agree),
                                         int(min_shared), int(edge), cap, ptr(counts), ptr(okp), ptr(osc), ptr(src), C.byref(req))
            if rc == E_CAPACITY and req.value > cap:
                cap = int(req.value)
                continue
            self.check(rc)
            break
        t = int(counts[:n_frames].sum())
        return counts[:n_frames], okp[:t], osc[:t], src[:t]

    def faces_poses_link(self, face_counts, boxes, pose_counts, keypoints, margin_permille=250, min_inside=1):
        """ta_faces_poses_link: per frame (face_counts, pose_counts (n_frames,); boxes (F, 4) int32; keypoints (P, 18, 3) int32, frames
        concatenated) the greedy one-to-one link of faces and skeletons by head joints inside the widened box -> (pose_of_face (F,)
        int32, face_of_pose (P,) int32, frame-local indices or -1; links (n_frames,) int32; the rounds the call ran)."""
        fc = np.ascontiguousarray(face_counts, dtype=np.int32).reshape(-1)
        pc = np.ascontiguousarray(pose_counts, dtype=np.int32).reshape(-1)
        if len(fc) != len(pc):
            raise ValueError('faces_poses_link: %d face counts, %d pose counts' % (len(fc), len(pc)))
        boxes = np.ascontiguousarray(boxes, dtype=np.int32).reshape(-1, 4)
        keypoints = np.ascontiguousarray(keypoints, dtype=np.int32).reshape(-1, 18, 3)
        nf, npose, n = len(boxes), len(keypoints), len(fc)
        pof, fop, links = np.empty(max(nf, 1), np.int32), np.empty(max(npose, 1), np.int32), np.zeros(max(n, 1), np.int32)
        rounds = C.c_int32(0)
        self.check(self.lib.ta_faces_poses_link(self.h, n, ptr(fc) if n else None, ptr(boxes) if nf else None, nf, ptr(pc) if n else None,
                                                ptr(keypoints) if npose else None, npose, int(margin_permille), int(min_inside), ptr(pof),
                                                ptr(fop), ptr(links), C.byref(rounds)))
        return pof[:nf], fop[:npose], links[:n], int(rounds.value)

    def poses_track(self, frames_per_sequence, history_frames, pose_counts, keypoints, closed=None, radius_permille=100, min_shared=3, max_gap=0):
        """ta_poses_track: skeletons followed over the frames of independent sequences (frames_per_sequence, history_frames
        (n_sequences,); pose_counts (n_frames,); keypoints (P, 18, 3) int32; closed (P,) uint8 or None, all concatenated) -> (prev (P,)
        int32, the global row of each skeleton's predecessor or -1; root (P,) int32, the first row of its track; links (n_frames,)
        int32)."""
        fps = np.ascontiguousarray(frames_per_sequence, dtype=np.int32).reshape(-1)
        hist = np.ascontiguousarray(history_frames, dtype=np.int32).reshape(-1)
        if len(fps) != len(hist):
            raise ValueError('poses_track: %d sequences, %d history counts' % (len(fps), len(hist)))
        pc = np.ascontiguousarray(pose_counts, dtype=np.int32).reshape(-1)
        keypoints = np.ascontiguousarray(keypoints, dtype=np.int32).reshape(-1, 18, 3)
        ns, n, npose = len(fps), len(pc), len(keypoints)
        if closed is not None:
            closed = np.ascontiguousarray(closed, dtype=np.uint8).reshape(-1)
            if len(closed) != npose:
                raise ValueError('poses_track: %d closed flags for %d skeletons' % (len(closed), npose))
        prev, root, links = np.empty(max(npose, 1), np.int32), np.empty(max(npose, 1), np.int32), np.zeros(max(n, 1), np.int32)
        self.check(self.lib.ta_poses_track(self.h, ns, ptr(fps) if ns else None, ptr(hist) if ns else None, n, ptr(pc) if n else None,
                                           ptr(keypoints) if npose else None, ptr(closed) if closed is not None and npose else None, npose,
                                           int(radius_permille), int(min_shared), int(max_gap), ptr(prev), ptr(root), ptr(links)))
        return prev[:npose], root[:npose], links[:n]

    def poses_paint(self, frames, pose_counts, keypoints, rgba, radius_permille=(90, 90, 50), min_radius=2, clear=False):
        """ta_poses_paint: the skeletons of the first len(pose_counts) frames of the resident batch `frames` painted into it as
        silhouettes, in place (pose_counts (n_frames,); keypoints (P, 18, 3) int32; rgba (P, 4) uint8 ink and alpha, concatenated;
        radius_permille: head, torso, limb radius in thousandths of a skeleton's size; `clear`: the listed frames are zeroed
        first).  Returns `frames`."""
        pc = np.ascontiguousarray(pose_counts, dtype=np.int32).reshape(-1)
        keypoints = np.ascontiguousarray(keypoints, dtype=np.int32).reshape(-1, 18, 3)
        rgba = np.ascontiguousarray(rgba, dtype=np.uint8).reshape(-1, 4)
        if len(rgba) != len(keypoints):
            raise ValueError('poses_paint: %d inks for %d skeletons' % (len(rgba), len(keypoints)))
        permille = np.ascontiguousarray(radius_permille, dtype=np.int32).reshape(-1)
        if len(permille) != 3:
            raise ValueError('poses_paint: radius_permille is (head, torso, limb), got %r' % (radius_permille,))
        n, npose = len(pc), len(keypoints)
        self.check(self.lib.ta_poses_paint(self.h, frames.h, n, ptr(pc) if n else None, ptr(keypoints) if npose else None,
                                           ptr(rgba) if npose else None, npose, ptr(permille), int(min_radius), int(bool(clear))))
        return frames

    def tracks_fill(self, counts, points, prev, max_gap=5, mark=2):
        """ta_tracks_fill: the tracked rows of consecutive frames (counts (n_frames,); points (R, n_points, 3) int32 (x, y, present);
        prev (R,) int32 as poses_track answers it, frames concatenated) with a synthesized row in every frame a link of 2 ..
        max_gap + 1 frames skips and every absent point interpolated between the chain's nearest rows that have it, at most max_gap
        + 1 frames apart, third value `mark` -> (out_counts (n_frames,) int32, out_points (n_out, n_points, 3) int32, out_source
        (n_out, 2) int32: (r, r) for a real row, (a, b) for a synthesized one)."""
        counts = np.ascontiguousarray(counts, dtype=np.int32).reshape(-1)
        points = np.ascontiguousarray(points, dtype=np.int32)
        if points.ndim != 3 or points.shape[2] != 3:
            raise ValueError('tracks_fill: points must be (rows, n_points, 3) int32, got %s' % (points.shape,))
        prev = np.ascontiguousarray(prev, dtype=np.int32).reshape(-1)
        if len(prev) != len(points):
            raise ValueError('tracks_fill: %d prev entries for %d rows' % (len(prev), len(points)))
        n, rows, npts = len(counts), len(points), points.shape[1]
        # the rows the call will give: a link of d frames, 2 <= d <= max_gap + 1, adds d - 1.  Whatever is wrong with counts or
        # prev the library reports; here such an entry just adds nothing
        cap = rows
        if rows and n and (counts >= 0).all() and int(counts.sum()) == rows:
            frame = np.repeat(np.arange(n), counts)
            linked = (prev >= 0) & (prev < rows)
            d = frame[linked] - frame[prev[linked]]
            cap += int((d[(d >= 2) & (d <= int(max_gap) + 1)] - 1).sum())
        oc, op, src = np.zeros(max(n, 1), np.int32), np.empty((max(cap, 1), npts, 3), np.int32), np.empty((max(cap, 1), 2), np.int32)
        n_out = C.c_int32(0)
        self.check(self.lib.ta_tracks_fill(self.h, n, ptr(counts) if n else None, ptr(points) if rows else None, npts, ptr(prev) if rows else None,
                                           rows, int(max_gap), int(mark), ptr(oc), ptr(op), ptr(src), cap, C.byref(n_out)))
        if n_out.value != cap:
            raise TerranAmdError(E_INVALID, 'tracks_fill: the library gave %d rows, counts and prev give %d' % (n_out.value, cap))
        return oc[:n], op[:cap], src[:cap]

    def cosine_distance(self, a, b):
        a = np.ascontiguousarray(a, dtype=np.float32)
        b = np.ascontiguousarray(b, dtype=np.float32)
        out = np.empty((a.shape[0], b.shape[0]), np.float32)
        self.check(self.lib.ta_cosine_distance(self.h, ptr(a), a.shape[0], ptr(b), b.shape[0], a.shape[1], ptr(out)))
        return out

    def jpeg_decode(self, buffers, threads=0):
        """ta_jpeg_decode: JPEG byte strings -> (list of resident Frames, paths).  One (n,H,W,3) batch when every image
        has the same size, else one (1,H_i,W_i,3) batch per image; paths[i] is JPEG_DEVICE or the fallback reason
        (that image's pixels are zero: the caller fills them).  A TerranAmdError(E_INVALID) carries `.paths`."""
        bufs = [bytes(b) for b in buffers]
        n = len(bufs)
        arrs = [np.frombuffer(b, np.uint8) for b in bufs]
        data = (c_void_p * n)(*[a.ctypes.data for a in arrs])
        sizes = (c_size_t * n)(*[a.size for a in arrs])
        out = (c_void_p * n)()
        paths = np.zeros(n, np.int32)
        req = C.c_int32()
        rc = self.lib.ta_jpeg_decode(self.h, data, sizes, n, int(threads), n, out, paths.ctypes.data_as(P(C.c_int32)),
                                     C.byref(req))
        if rc != OK:
            e = TerranAmdError(rc, self.last_error())
            e.paths = paths                             # TA_E_INVALID: JPEG_INVALID marks the malformed images
            raise e
        return [Frames(self, handle=c_void_p(out[k])) for k in range(req.value)], paths

    def jpeg_stats(self):
        """Figures of the last jpeg_decode: ({host, h2d, idct, color}: ms), {images, blocks, bytes, fallbacks}."""
        ms, cnt = np.zeros(4, np.float64), np.zeros(4, np.int64)
        self.check(self.lib.ta_jpeg_last_stats(self.h, ptr(ms), ptr(cnt)))
        return (dict(zip(('host', 'h2d', 'idct', 'color'), ms.tolist())),
                dict(zip(('images', 'blocks', 'bytes', 'fallbacks'), cnt.tolist())))

    def jpeg_encode(self, frames, quality=75, subsampling=2, optimize=False):
        """ta_jpeg_encode: a resident Frames batch -> list of JPEG files (bytes), Pillow's for the same options; runs on
        this context's stream (ordered after a draw on it).  `optimize`: Pillow's optimize=True, every image coded with
        its own Huffman tables (ta_jpeg_encode_opt)."""
        quality, subsampling = check_jpeg_options(quality, subsampling)
        optimize = check_jpeg_optimize(optimize)
        n = frames.shape[0]
        out = c_void_p()
        sizes = (c_size_t * n)()
        if optimize:
            self.check(self.lib.ta_jpeg_encode_opt(self.h, frames.h, quality, subsampling, 1, C.byref(out), sizes))
        else:
            self.check(self.lib.ta_jpeg_encode(self.h, frames.h, quality, subsampling, C.byref(out), sizes))
        files, at = [], out.value
        for k in range(n):
            files.append(C.string_at(at, sizes[k]))
            at += sizes[k]
        return files

    def jpeg_encode_stats(self):
        """Figures of the last jpeg_encode: ({h2d, coef, length, emit, ffcount, pack, d2h, host; statistics, tables}:
        ms), {images, blocks, bytes, entropy_bytes}.  `statistics` (the symbol-count pass, HIP events) and `tables` (the
        host building tables and headers, wall time) are 0 unless the call had optimize=True."""
        ms, cnt, opt = np.zeros(8, np.float64), np.zeros(4, np.int64), np.zeros(2, np.float64)
        self.check(self.lib.ta_jpeg_encode_last_stats(self.h, ptr(ms), ptr(cnt)))
        self.check(self.lib.ta_jpeg_encode_last_opt_stats(self.h, ptr(opt)))
        return (dict(zip(('h2d', 'coef', 'length', 'emit', 'ffcount', 'pack', 'd2h', 'host', 'statistics', 'tables'),
                         ms.tolist() + opt.tolist())),
                dict(zip(('images', 'blocks', 'bytes', 'entropy_bytes'), cnt.tolist())))

    def conv_variant(self, name):
        """Debug: force every following conv on this context onto one kernel variant ('auto' to release)."""
        self.check(self.lib.ta_debug_conv_variant(self.h, CONV_VARIANTS[name]))

    def conv_counts(self, reset=False):
        """Debug: {variant name: conv launches since the last reset}."""
        c = np.zeros(16, np.int64)
        self.check(self.lib.ta_debug_conv_counts(self.h, ptr(c), int(reset)))
        out = {k: int(c[v]) for k, v in CONV_VARIANTS.items() if v and c[v]}
        if c[15]:
            out['lean_epilogue'] = int(c[15])          # split-role launches that ran the specialised drain
        return out

    def kernel_work(self, reset=False):
        """{kernel instance name: (launches, algorithmic FLOPs, HIP-event ms)} of the dense-conv kernels since the last reset; the
        time covers the launches made while `profile(True)` was on (0.0 otherwise)."""
        buf = C.create_string_buffer(1 << 16)
        self.check(self.lib.ta_debug_kernel_work(self.h, buf, len(buf), int(reset)))
        out = {}
        for line in buf.value.decode().splitlines():
            f = line.split(';')
            out[f[0]] = (int(f[1]), float(f[2]), float(f[3]) if len(f) > 3 else 0.0)
        return out

    def pose_debug(self, n, cap_peaks=1024, cap_conn=1024):
        """Debug taps of the last OpenPose run / grouping on this context -> (peaks, connections):
        peaks[i][part] = (yx (k,2) int32, scores (k,) f32); connections[i][limb] = None (limb skipped) or
        (ij (k,2) int32, scores (k,) f32)."""
        pc = np.zeros((n, 18), np.int32)
        pyx = np.zeros((n, 18, cap_peaks, 2), np.int32)
        psc = np.zeros((n, 18, cap_peaks), np.float32)
        cc = np.zeros((n, 19), np.int32)
        cij = np.zeros((n, 19, cap_conn, 2), np.int32)
        csc = np.zeros((n, 19, cap_conn), np.float32)
        self.check(self.lib.ta_openpose_debug_read(self.h, n, cap_peaks, ptr(pc), ptr(pyx), ptr(psc), cap_conn,
                                                   ptr(cc), ptr(cij), ptr(csc)))
        assert pc.max(initial=0) <= cap_peaks and cc.max(initial=0) <= cap_conn
        peaks = [[(pyx[i, p, :pc[i, p]].copy(), psc[i, p, :pc[i, p]].copy()) for p in range(18)] for i in range(n)]
        conns = [[None if cc[i, l] < 0 else (cij[i, l, :cc[i, l]].copy(), csc[i, l, :cc[i, l]].copy())
                  for l in range(19)] for i in range(n)]
        return peaks, conns

    def pose_debug_capacity(self, n):
        """Debug: rows per part of the work area each image's `pose_debug` taps come from -> [n] ints: 1024 for an image
        the batch pass kept, its own largest peak count for an image that was re-run alone with larger lists."""
        cap = np.zeros(n, np.int32)
        self.check(self.lib.ta_openpose_debug_capacity(self.h, n, ptr(cap)))
        return cap.tolist()

    def pose_stats(self):
        """(peaks, limb connections) of the last OpenPose grouping run on this context."""
        a, b = C.c_int64(), C.c_int64()
        self.check(self.lib.ta_openpose_last_stats(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def bicubic_x8(self, maps):
        maps = np.ascontiguousarray(maps, dtype=np.float32)
        n, c, h, w = maps.shape
        out = np.empty((n, c, 8 * h, 8 * w), np.float32)
        self.check(self.lib.ta_bicubic_x8(self.h, ptr(maps), n, c, h, w, ptr(out)))
        return out


class Frames:
    """uint8 RGB (N,H,W,3) batch resident in HBM."""

    def __init__(self, ctx, images=None, handle=None):
        self.ctx = ctx
        if handle is not None:
            self.h = handle
        else:
            h = c_void_p()
            n, hh, ww = images.shape[:3]
            ctx.check(ctx.lib.ta_frames_upload(ctx.h, ptr(images), n, hh, ww, C.byref(h)))
            self.h = h
        n, hh, ww = c_int(), c_int(), c_int()
        ctx.lib.ta_frames_shape(self.h, C.byref(n), C.byref(hh), C.byref(ww))
        self.shape = (n.value, hh.value, ww.value, 3)

    def __len__(self):
        return self.shape[0]

    @classmethod
    def zeros(cls, ctx, n, h, w):
        hd = c_void_p()
        ctx.check(ctx.lib.ta_frames_alloc(ctx.h, n, h, w, C.byref(hd)))
        return cls(ctx, handle=hd)

    def resize(self, h, w, ctx=None):
        """`ctx`: the context (stream, scratch) the resize runs on and the result belongs to -- the CALLER's, so that a
        batch handed over by another thread's context (video.RawVideoReader) is only ever read here, never driven."""
        ctx = ctx or self.ctx
        hd = c_void_p()
        ctx.check(ctx.lib.ta_frames_resize(ctx.h, self.h, int(h), int(w), C.byref(hd)))
        return Frames(ctx, handle=hd)

    def resize_bicubic(self, h, w, ctx=None):
        ctx = ctx or self.ctx
        hd = c_void_p()
        ctx.check(ctx.lib.ta_frames_resize_bicubic(ctx.h, self.h, int(h), int(w), C.byref(hd)))
        return Frames(ctx, handle=hd)

    def paste(self, src, src_index, dst_index, top, left):
        self.ctx.check(self.ctx.lib.ta_frames_paste(self.ctx.h, src.h, src_index, self.h, dst_index, top, left))

    def draw(self, prims, masks=None, ctx=None):
        """Draw `prims` (a PRIM_DT array, in order) into this batch in place (ta_frames_draw).  `masks`: the uint8 buffer
        that holds the coverage bitmaps of the DRAW_MASK primitives, each at the byte offset its `width` names
        (ta_frames_draw_masks); without it a DRAW_MASK primitive is an unknown kind.  `ctx`: the context the drawing runs
        on -- the CALLER's, as in `resize`."""
        ctx = ctx or self.ctx
        prims, pp, n = _records(prims, PRIM_DT)
        if masks is None:
            ctx.check(ctx.lib.ta_frames_draw(ctx.h, self.h, pp, n))
            return
        masks = np.ascontiguousarray(masks, dtype=np.uint8).reshape(-1)
        ctx.check(ctx.lib.ta_frames_draw_masks(ctx.h, self.h, pp, n, ptr(masks) if len(masks) else None, len(masks)))

    def blur(self, regions, ctx=None):
        """Blur `regions` (a BLUR_DT array, in order) of this batch in place (ta_frames_blur): Pillow's GaussianBlur of each
        half-open box, pasted back under its shape.  `ctx`: the context the blur runs on -- the CALLER's, as in `draw`."""
        ctx = ctx or self.ctx
        regions, p, n = _records(regions, BLUR_DT)
        ctx.check(ctx.lib.ta_frames_blur(ctx.h, self.h, p, n))

    def resample(self, regions, out_h, out_w, filter, ctx=None):
        """A NEW batch (len(regions), out_h, out_w, 3): image i is Pillow's resize((out_w, out_h), filter, box=) of the
        frame and fractional box regions[i] names (a RESAMPLE_DT array; ta_frames_resample), or None without regions.
        `filter`: a TA_RESAMPLE_* / Pillow code.  `ctx`: the context the work runs on and the result belongs to -- the
        CALLER's, as in `resize`."""
        ctx = ctx or self.ctx
        regions, p, n = _records(regions, RESAMPLE_DT)
        hd = c_void_p()
        ctx.check(ctx.lib.ta_frames_resample(ctx.h, self.h, p, n, int(out_h), int(out_w), int(filter), C.byref(hd)))
        return Frames(ctx, handle=hd) if hd.value else None

    def pixelate(self, regions, ctx=None):
        """Pixelate `regions` (a PIXELATE_DT array, in order) of this batch in place (ta_frames_pixelate): each half-open box
        shrunk by its `block` with Pillow's BOX filter and enlarged again with NEAREST, pasted back under its shape.
        `ctx`: the context the work runs on -- the CALLER's, as in `draw`."""
        ctx = ctx or self.ctx
        regions, p, n = _records(regions, PIXELATE_DT)
        ctx.check(ctx.lib.ta_frames_pixelate(ctx.h, self.h, p, n))

    def histogram(self, regions, mode=HIST_RGB, ctx=None):
        """uint32 (len(regions), 3, 256) (HIST_RGB) or (len(regions), 256) (HIST_L): Pillow's histogram of each region of a
        HIST_DT array under its shape (ta_frames_histogram).  The batch is only read.  `ctx`: the CALLER's, as in `blur`."""
        ctx = ctx or self.ctx
        regions, p, n = _records(regions, HIST_DT)
        mode = int(mode)
        hist = np.zeros((n, 3, 256) if mode == HIST_RGB else (n, 256), np.uint32)
        ctx.check(ctx.lib.ta_frames_histogram(ctx.h, self.h, p, n, mode, ptr(hist) if n else None))
        return hist

    def point(self, regions, luts, ctx=None):
        """Apply look-up tables to `regions` (a POINT_DT array, in order) of this batch in place (ta_frames_point): Pillow's
        point() of each half-open box, pasted back under its shape.  `luts`: uint8 (n_luts, 768), R, G and B table of each;
        a region's `lut` names its table."""
        ctx = ctx or self.ctx
        regions, p, n = _records(regions, POINT_DT)
        luts = np.ascontiguousarray(luts, dtype=np.uint8)
        if luts.ndim != 2 or luts.shape[1] != 768:
            raise ValueError('point: luts must be uint8 (n_luts, 768), got %s' % (luts.shape,))
        ctx.check(ctx.lib.ta_frames_point(ctx.h, self.h, p, n, ptr(luts) if len(luts) else None, len(luts)))

    def saturate(self, regions, ctx=None):
        """Blend `regions` (a SATURATE_DT array, in order) of this batch with their own luma in place (ta_frames_saturate):
        Pillow's ImageEnhance.Color(region).enhance(factor), pasted back under its shape."""
        ctx = ctx or self.ctx
        regions, p, n = _records(regions, SATURATE_DT)
        ctx.check(ctx.lib.ta_frames_saturate(ctx.h, self.h, p, n))

    def color(self, regions, ops, tables=None, ctx=None):
        """Convert the colours of `regions` (a COLOR_REGION_DT array, in order) of this batch in place (ta_frames_color):
        Pillow's convert('RGB', matrix), convert('YCbCr' / 'HSV') and back, or filter(Color3DLUT) of each half-open box,
        pasted back under its shape.  `ops`: a COLOR_OP_DT array, a region's `op` names its entry; `tables`: the float32
        array the matrix and 3-D table ops index with `table` (terran_amd.image.color_spec makes both).  The batch has no
        mode: after a conversion to YCbCr or HSV its bytes are those bands.  `ctx`: the CALLER's, as in `blur`."""
        ctx = ctx or self.ctx
        regions, p, n = _records(regions, COLOR_REGION_DT)
        ops, tables = _color_args(ops, tables)
        ctx.check(ctx.lib.ta_frames_color(ctx.h, self.h, p, n, ptr(ops) if len(ops) else None, len(ops),
                                          ptr(tables) if len(tables) else None, len(tables)))

    def filter(self, regions, specs, ctx=None):
        """Filter `regions` (a FILTER_REGION_DT array, in order) of this batch in place (ta_frames_filter): Pillow's
        `crop(box).filter(F)` of each half-open box, pasted back under its shape; F is specs[region['spec']] (a
        FILTER_SPEC_DT array: a convolution kernel, a rank filter or an unsharp mask; terran_amd.image.filter_spec makes
        one from a Pillow filter).  `ctx`: the CALLER's, as in `blur`."""
        ctx = ctx or self.ctx
        regions, p, n = _records(regions, FILTER_REGION_DT)
        specs = np.ascontiguousarray(specs, dtype=FILTER_SPEC_DT).reshape(-1)
        ctx.check(ctx.lib.ta_frames_filter(ctx.h, self.h, p, n, ptr(specs) if len(specs) else None, len(specs)))

    def combine(self, src, regions, masks=None, mask_frames=None, ctx=None):
        """Combine `regions` (a COMBINE_DT array, in order) of this batch with their source boxes in the batch `src`, in
        place (ta_frames_combine): Pillow's paste under a mask, Image.blend or an ImageChops function of each half-open box,
        pasted back under its shape.  `masks`: the uint8 buffer that holds the packed bitmaps of the MASK_BITMAP regions,
        each at the byte offset its `mask_value` names; `mask_frames`: the batch the MASK_FRAMES regions read a band of.
        `src` and `mask_frames` may be this batch when no frame is both written and read.  `ctx`: the CALLER's, as in `blur`."""
        ctx = ctx or self.ctx
        regions, p, n = _records(regions, COMBINE_DT)
        if masks is not None:
            masks = np.ascontiguousarray(masks, dtype=np.uint8).reshape(-1)
        has = masks is not None and len(masks) > 0
        ctx.check(ctx.lib.ta_frames_combine(ctx.h, self.h, src.h, mask_frames.h if mask_frames is not None else None, p, n,
                                            ptr(masks) if has else None, len(masks) if has else 0))

    def transform(self, regions, out_h, out_w, filter, fill=None, ctx=None):
        """A NEW batch (len(regions), out_h, out_w, 3): image i is Pillow's transform((out_w, out_h), method, a,
        resample=filter, fillcolor=fill) of the frame regions[i] names (a TRANSFORM_DT array; ta_frames_transform), or None
        without regions.  `filter`: NEAREST, BILINEAR or BICUBIC; `fill`: None (zeros) or 3 values 0 .. 255.  `ctx`: the
        context the work runs on and the result belongs to -- the CALLER's, as in `resize`."""
        ctx = ctx or self.ctx
        regions, p, n = _records(regions, TRANSFORM_DT)
        rgb = None if fill is None else np.array(fill, np.uint8).reshape(3)
        hd = c_void_p()
        ctx.check(ctx.lib.ta_frames_transform(ctx.h, self.h, p, n, int(out_h), int(out_w), int(filter), ptr(rgb), C.byref(hd)))
        return Frames(ctx, handle=hd) if hd.value else None

    def transform_mesh(self, cells, mesh_first, images, out_h, out_w, filter, fill=None, ctx=None):
        """A NEW batch (len(images), out_h, out_w, 3): image i is Pillow's transform((out_w, out_h), MESH, cells of mesh
        images[i]['mesh'], resample=filter, fillcolor=fill) of the frame images[i]['frame'] (ta_frames_transform_mesh), or
        None without images.  `cells`: a MESH_CELL_DT array, the meshes one after the other; `mesh_first`: their n_meshes + 1
        offsets into it; `images`: a MESH_IMAGE_DT array.  `filter`, `fill`, `ctx`: as in `transform`."""
        ctx = ctx or self.ctx
        cells, pc, nc = _records(cells, MESH_CELL_DT)
        first = np.ascontiguousarray(mesh_first, dtype=np.int32).reshape(-1)
        if len(first) < 1:
            raise ValueError('transform_mesh: mesh_first must hold n_meshes + 1 offsets')
        images, pi, ni = _records(images, MESH_IMAGE_DT)
        rgb = None if fill is None else np.array(fill, np.uint8).reshape(3)
        hd = c_void_p()
        ctx.check(ctx.lib.ta_frames_transform_mesh(ctx.h, self.h, pc, nc, ptr(first), len(first) - 1, pi, ni, int(out_h), int(out_w),
                                                   int(filter), ptr(rgb), C.byref(hd)))
        return Frames(ctx, handle=hd) if hd.value else None

    def transpose(self, op, ctx=None):
        """A NEW batch: Pillow's Image.transpose(op) of every image (ta_frames_transpose).  `op`: FLIP_LEFT_RIGHT ..
        TRANSVERSE, Pillow's codes.  `ctx`: the caller's, as in `resize`."""
        ctx = ctx or self.ctx
        hd = c_void_p()
        ctx.check(ctx.lib.ta_frames_transpose(ctx.h, self.h, int(op), C.byref(hd)))
        return Frames(ctx, handle=hd)

    def encode_jpeg(self, quality=75, subsampling=2, ctx=None, optimize=False):
        """This batch as JPEG files (list of bytes, Pillow's for the same options).  `ctx`: the context the encode runs
        on -- the CALLER's, as in `draw`, so it is ordered after a draw on that context."""
        return (ctx or self.ctx).jpeg_encode(self, quality, subsampling, optimize)

    def to_yuv(self, spec, out=None, ctx=None):
        """ta_frames_to_yuv: this batch as raw YUV frames, a uint8 (n, frame_bytes) array (`out`, if given: contiguous and
        of that shape).  `ctx`: the context the conversion runs on -- the CALLER's, as in `draw`."""
        ctx = ctx or self.ctx
        s = _yuv_spec(spec)
        per = yuv_frame_bytes(s['format'][0], self.shape[1], self.shape[2])
        if out is None:
            out = np.empty((self.shape[0], max(per, 1)), np.uint8)
        elif not (isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.flags['C_CONTIGUOUS'] and per
                  and out.shape == (self.shape[0], per)):
            raise ValueError('to_yuv: out must be a contiguous uint8 array of shape (%d, %d)' % (self.shape[0], per))
        ctx.check(ctx.lib.ta_frames_to_yuv(ctx.h, self.h, ptr(s), ptr(out)))
        return out

    def download(self):
        out = np.empty(self.shape, np.uint8)
        self.ctx.check(self.ctx.lib.ta_frames_download(self.h, ptr(out)))
        return out

    def free(self):
        if getattr(self, 'h', None) and getattr(self.ctx, 'h', None):
            self.ctx.lib.ta_frames_free(self.h)
        self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Gallery:
    """ta_gallery: `dim`-float embeddings resident in HBM, each with an int32 id >= 0, searched by cosine distance."""

    def __init__(self, ctx, dim, reserve=0):
        self.ctx = ctx
        self.dim = int(dim)
        h = c_void_p()
        ctx.check(ctx.lib.ta_gallery_create(ctx.h, self.dim, int(reserve), C.byref(h)))
        self.h = h

    def _rows(self, a, what):
        a = np.ascontiguousarray(a, dtype=np.float32)
        if a.ndim != 2 or a.shape[1] != self.dim:
            raise TerranAmdError(E_INVALID, 'gallery: %s of shape %s are not (n, %d)' % (what, a.shape, self.dim))
        return a

    def add(self, rows, ids, normalize=True):
        rows = self._rows(rows, 'rows')
        ids = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        if len(ids) != len(rows):
            raise TerranAmdError(E_INVALID, 'gallery: %d ids for %d rows' % (len(ids), len(rows)))
        self.ctx.check(self.ctx.lib.ta_gallery_add(self.h, ptr(rows), ptr(ids), len(rows), int(bool(normalize))))

    def remove(self, ids):
        ids = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        removed = C.c_int64()
        self.ctx.check(self.ctx.lib.ta_gallery_remove(self.h, ptr(ids) if len(ids) else None, len(ids), C.byref(removed)))
        return removed.value

    def clear(self):
        self.ctx.check(self.ctx.lib.ta_gallery_clear(self.h))

    def size(self):
        """(rows, live rows)."""
        rows, live = C.c_int64(), C.c_int64()
        self.ctx.check(self.ctx.lib.ta_gallery_size(self.h, C.byref(rows), C.byref(live)))
        return rows.value, live.value

    def download(self):
        """(stored rows (n, dim) float32, ids (n,) int32 with -1 for removed rows)."""
        n = self.size()[0]
        rows, ids = np.empty((n, self.dim), np.float32), np.empty(n, np.int32)
        self.ctx.check(self.ctx.lib.ta_gallery_download(self.h, ptr(rows), ptr(ids)))
        return rows, ids

    def search(self, queries, k=1, normalize=True):
        """(row, id, distance) arrays of shape (nq, k); padded slots are (-1, -1, +inf)."""
        q = self._rows(queries, 'queries')
        k = int(k)
        kk = max(k, 0)
        row, ident = np.empty((len(q), kk), np.int32), np.empty((len(q), kk), np.int32)
        dist = np.empty((len(q), kk), np.float32)
        self.ctx.check(self.ctx.lib.ta_gallery_search(self.h, ptr(q), len(q), k, int(bool(normalize)), ptr(row), ptr(ident), ptr(dist)))
        return row, ident, dist

    def cluster(self, threshold, min_samples=1):
        """ta_gallery_cluster: (labels (rows,) int32 with -1 for noise and removed rows, degree (rows,) int32, number of
        clusters, label propagation rounds run)."""
        n = self.size()[0]
        labels, degree = np.empty(n, np.int32), np.empty(n, np.int32)
        count, rounds = C.c_int32(), C.c_int32()
        self.ctx.check(self.ctx.lib.ta_gallery_cluster(self.h, float(threshold), int(min_samples), ptr(labels), ptr(degree), C.byref(count), C.byref(rounds)))
        return labels, degree, count.value, rounds.value

    def free(self):
        if getattr(self, 'h', None) and getattr(self.ctx, 'h', None):
            self.ctx.lib.ta_gallery_free(self.h)
        self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Model:
    """A packed model on one context."""

    def __init__(self, ctx, program):
        self.ctx = ctx
        self.kind = program.kind
        self.names = dict(program.names)
        blob = program.blob()
        buf = np.frombuffer(blob, dtype=np.uint8)
        h = c_void_p()
        ctx.check(ctx.lib.ta_model_load(ctx.h, program.kind, ptr(buf), len(blob), C.byref(h)))
        self.h = h

    def forward_frames(self, frames):
        self.ctx.check(self.ctx.lib.ta_model_forward_frames(self.h, frames.h))

    def forward_crops(self, crops):
        crops = np.ascontiguousarray(crops, dtype=np.uint8)
        self.ctx.check(self.ctx.lib.ta_model_forward_crops(self.h, ptr(crops), crops.shape[0]))

    def read(self, name):
        """Debug tap: named tensor slice as float32 NCHW."""
        tid, off, ch = self.names[name]
        n, c, h, w = c_int(), c_int(), c_int(), c_int()
        self.ctx.check(self.ctx.lib.ta_model_tensor_shape(self.h, tid, C.byref(n), C.byref(c), C.byref(h), C.byref(w)))
        out = np.empty((n.value, ch, h.value, w.value), np.float32)
        self.ctx.check(self.ctx.lib.ta_model_read_tensor(self.h, tid, off, ch, ptr(out)))
        return out

    def read_tensor(self, tid, ch_off=0, ch=None):
        """Debug tap by tensor id (true values: the activation scale is divided out)."""
        n, c, h, w = c_int(), c_int(), c_int(), c_int()
        self.ctx.check(self.ctx.lib.ta_model_tensor_shape(self.h, tid, C.byref(n), C.byref(c), C.byref(h), C.byref(w)))
        ch = c.value - ch_off if ch is None else ch
        out = np.empty((n.value, ch, h.value, w.value), np.float32)
        self.ctx.check(self.ctx.lib.ta_model_read_tensor(self.h, tid, ch_off, ch, ptr(out)))
        return out

    def tensor_unscale(self, tid, channels):
        """Per-channel factors 2^-a[c] the stored values of tensor `tid` are multiplied with to get the true ones."""
        out = np.empty(channels, np.float32)
        self.ctx.check(self.ctx.lib.ta_model_tensor_unscale(self.h, tid, ptr(out), channels))
        return out

    def amax_collect(self, on=True):
        """Start (zeroed) / stop collecting the largest |x| every conv / dw+pw op stores (ta_model_debug_amax)."""
        self.ctx.check(self.ctx.lib.ta_model_debug_amax(self.h, int(bool(on)), None, 0))

    def graph_probe(self, reps=20):
        """Tools: (gpu_ms_streams, gpu_ms_graph, host_ms_streams, host_ms_graph, capture_ms) of the last forward's op program."""
        out = np.zeros(5, np.float64)
        self.ctx.check(self.ctx.lib.ta_model_graph_probe(self.h, int(reps), ptr(out)))
        return tuple(float(x) for x in out)

    def amax_read(self, n_ops):
        """-> (n_ops, 2) float32 in STORED units: [:, 0] op outputs, [:, 1] depthwise intermediates of dw+pw ops; the
        collection goes on (not zeroed)."""
        out = np.zeros(2 * n_ops, np.float32)
        n = c_int()
        # read without restarting: enable = 1 would zero the slots, so read first through a second call
        self.ctx.check(self.ctx.lib.ta_model_debug_amax(self.h, 2, ptr(out), out.size))
        return out.reshape(n_ops, 2)

    def free(self):
        if getattr(self, 'h', None) and getattr(self.ctx, 'h', None):
            self.ctx.lib.ta_model_free(self.h)
        self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass
