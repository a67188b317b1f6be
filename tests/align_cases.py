"""What tests/test_align_cpu.py and tests/test_gpu_align.py share: the cases of tests/golden/align.npz and the random
similarity matrices of their sweeps.  numpy only."""
import numpy as np

from tests.util import golden


def noise(seed, *shape):
    """Uniform byte noise: the truncation to uint8 of the warp and the clipping of the resamplers only show on busy pixels."""
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def warp_cases():
    """[(name, source (H,W,3), matrix (6,), Pillow's (112,112,3) crop)] of align.npz."""
    g = golden('align.npz')
    return [(str(name), g['warp_src_%d' % k], g['warp_matrix'][k], g['warp_out_%d' % k]) for k, name in enumerate(g['warp_names'])]


def bicubic_cases():
    """[(source (H,W,3), (width, height), Pillow's resize)] of align.npz."""
    g = golden('align.npz')
    return [(g['bicubic_src_%d' % k], tuple(int(v) for v in size), g['bicubic_out_%d' % k]) for k, size in enumerate(g['bicubic_size'])]


# Frames.resize_bicubic on the shared resample kernels (csrc/resample.hip: workgroups of TX = 64 pixels x TY = 4 rows, the
# horizontal pass walks ROWS_PER_GROUP = 16 rows), as batches of 2: [((n, height, width), (out_h, out_w))]
BICUBIC_TILE_EDGES = [((2, 17, 130), (5, 65)), ((2, 16, 128), (4, 64)), ((2, 15, 126), (3, 63))]     # one past, on, one short of a tile
BICUBIC_SKIPS = [((2, 9, 40), (9, 13)), ((2, 9, 40), (4, 40)), ((2, 9, 40), (9, 40))]                # no vertical pass, no horizontal pass, the copy
# ksize = ceil(2 in / out) * 2 + 1 coefficients per output sample: a horizontal workgroup stages 64 rows of them in 8192
# LDS words (ksize <= 128), a vertical one 4 rows (ksize <= 2048); beyond that they are read from global memory
BICUBIC_LDS_SWITCH = [((2, 3, 63), (3, 2)), ((2, 3, 64), (3, 2)), ((2, 1022, 3), (2, 3)), ((2, 1024, 3), (2, 3))]
BICUBIC_EDGE_CASES = BICUBIC_TILE_EDGES + BICUBIC_SKIPS + BICUBIC_LDS_SWITCH


def random_similarity(rng, h, w):
    """6 float64 (crop pixel -> source point of an h x w image): any rotation, scale e^-2 .. e^1.5 source pixels per crop
    pixel, the crop's corner anywhere from 60 pixels before the image to 10 pixels past it."""
    theta = rng.uniform(0.0, 2.0 * np.pi)
    s = np.exp(rng.uniform(-2.0, 1.5))
    return np.array([s * np.cos(theta), -s * np.sin(theta), rng.uniform(-60.0, w + 10.0),
                     s * np.sin(theta), s * np.cos(theta), rng.uniform(-60.0, h + 10.0)])


def bgr_chw(crop):
    """Pillow's (112,112,3) RGB crop as the embedder takes it, (3,112,112) BGR (oracle.arcface_pre.preprocess_face)."""
    return np.ascontiguousarray(crop.transpose(2, 0, 1)[::-1])


WARP_NAMES = ['identity', 'shift_minus_half', 'shift_plus_half', 'corner_top_left', 'corner_top_right', 'corner_bottom_left',
              'corner_bottom_right', 'outside', 'source_1x1', 'source_1x40', 'source_40x1', 'transpose', 'turn_180', 'rotate_45',
              'magnify_20', 'minify_3']

# the many-faces launch: three resident batches of different sizes (n, height, width) and 48 faces over them
MANY_BATCHES = ((2, 37, 53), (1, 113, 111), (3, 1, 64))
MANY_FACES = 48
MANY_SEED = 3              # chosen so that the faces reach every branch (branch_coverage); a condition on the inputs


def many_faces(seed=MANY_SEED):
    """-> (batches [(n,h,w,3) uint8 noise], source_index (48,), frame_index (48,), matrices (48,6)).  The first faces walk
    over every image of every batch, the others draw theirs; then the order is shuffled."""
    rng = np.random.default_rng(seed)
    batches = [noise(400 + k, n, h, w, 3) for k, (n, h, w) in enumerate(MANY_BATCHES)]
    pairs = [(s, f) for s, (n, _, _) in enumerate(MANY_BATCHES) for f in range(n)]
    while len(pairs) < MANY_FACES:
        s = int(rng.integers(len(MANY_BATCHES)))
        pairs.append((s, int(rng.integers(MANY_BATCHES[s][0]))))
    pairs = [pairs[i] for i in rng.permutation(MANY_FACES)]
    matrices = np.stack([random_similarity(rng, *MANY_BATCHES[s][1:]) for s, _ in pairs])
    return batches, np.array([s for s, _ in pairs], np.int32), np.array([f for _, f in pairs], np.int32), matrices


def branch_coverage(source_index, matrices, shapes=MANY_BATCHES):
    """Which branches of the warp these faces reach, from the inputs alone (the kernel's own coordinate arithmetic in
    float64): crops with fill and image pixels both, crops that are all fill, faces with an accepted source point whose
    lower tap row is past the image (y + 1 >= H) on an image of more than one row, faces with an accepted point whose left
    tap is before it (x < 0 after the -0.5 shift)."""
    xin, yin = np.arange(112)[None, :] + 0.5, np.arange(112)[:, None] + 0.5
    mixed = all_fill = last_row = before_left = 0
    for s, a in zip(source_index, matrices):
        _, h, w = shapes[s]
        sx, sy = a[0] * xin + a[1] * yin + a[2], a[3] * xin + a[4] * yin + a[5]
        inside = ~((sx < 0.0) | (sx >= w) | (sy < 0.0) | (sy >= h))
        mixed += bool(inside.any() and not inside.all())
        all_fill += not inside.any()
        last_row += bool(h > 1 and (inside & (np.floor(sy - 0.5) + 1 >= h)).any())
        before_left += bool((inside & (np.floor(sx - 0.5) < 0)).any())
    return dict(mixed=mixed, all_fill=all_fill, last_row=last_row, before_left=before_left)
