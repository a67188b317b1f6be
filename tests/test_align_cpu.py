"""No GPU: the numpy restatements the aligned-crop and frame-resize kernels are held to on the GPU (tests/test_gpu_align.py),
oracle.arcface_pre.pil_affine_bilinear and pil_resize_bicubic, against the recorded Pillow golden (tests/golden/align.npz)
and, where Pillow is installed, against Pillow itself over random similarity transforms.  That equality is what lets the GPU
test use the restatement for cases that are not in the fixture."""
import numpy as np
import pytest

from oracle import arcface_pre
from tests import align_cases

WARP_NAMES = align_cases.WARP_NAMES
SWEEP_SOURCES = ((1, 1), (1, 64), (37, 53), (113, 111), (200, 1), (64, 64))          # (height, width)


def test_the_fixture_holds_the_cases_it_is_there_for():
    cases = align_cases.warp_cases()
    assert [c[0] for c in cases] == WARP_NAMES
    shapes = {name: src.shape for name, src, _, _ in cases}
    assert shapes['identity'] == (112, 112, 3) and shapes['source_1x1'] == (1, 1, 3)
    assert shapes['source_1x40'] == (1, 40, 3) and shapes['source_40x1'] == (40, 1, 3)
    fill = {name: float((crop == 0).all(-1).mean()) for name, _, _, crop in cases}
    assert fill['outside'] == 1.0 and fill['identity'] < 0.01
    assert all(0.4 < fill[n] < 0.6 for n in WARP_NAMES if n.startswith('corner_')), fill
    sizes = [(src.shape[1], src.shape[0], w, h) for src, (w, h), _ in align_cases.bicubic_cases()]
    assert sizes == [(96, 80, 12, 10), (9, 7, 45, 35), (1, 33, 5, 33), (33, 1, 33, 5), (40, 31, 40, 17), (40, 31, 23, 31),
                     (40, 31, 40, 31)]


def test_the_warp_restatement_equals_the_golden():
    for name, src, matrix, crop in align_cases.warp_cases():
        got = arcface_pre.pil_affine_bilinear(src, matrix)
        assert got.dtype == np.uint8 and np.array_equal(got, crop), name


def test_the_bicubic_restatement_equals_the_golden():
    for src, size, expected in align_cases.bicubic_cases():
        got = arcface_pre.pil_resize_bicubic(src, size)
        assert got.dtype == np.uint8 and np.array_equal(got, expected), (src.shape, size)


def test_the_warp_restatement_equals_live_pillow_over_random_similarities():
    """200 matrices from a fixed seed: any rotation, scales e^-2 .. e^1.5, the crop's corner from 60 pixels before the image
    to 10 past it, over sources from 1 x 1 to 200 x 1."""
    pytest.importorskip('PIL')
    from PIL import Image
    rng = np.random.default_rng(20240)
    sources = [align_cases.noise(300 + k, h, w, 3) for k, (h, w) in enumerate(SWEEP_SOURCES)]
    mixed = 0
    for k in range(200):
        src = sources[k % len(sources)]
        matrix = align_cases.random_similarity(rng, *src.shape[:2])
        ref = np.asarray(Image.fromarray(src).transform((112, 112), Image.AFFINE, tuple(matrix), resample=Image.BILINEAR, fillcolor=0))
        got = arcface_pre.pil_affine_bilinear(src, matrix)
        assert np.array_equal(got, ref), (k, src.shape, matrix.tolist())
        mixed += 0 < int(ref.any(-1).sum()) < 112 * 112
    assert mixed >= 50                                   # the sweep does cross image borders


def test_the_many_faces_draw_reaches_every_branch_of_the_warp():
    """The inputs of the 48-face launch of tests/test_gpu_align.py, judged here as well: a draw that stopped reaching a
    branch fails before it gets to a GPU."""
    _, source_index, frame_index, matrices = align_cases.many_faces()
    assert len(matrices) == align_cases.MANY_FACES == 48 and 48 * 112 * 112 > 2048 * 256
    assert {(int(s), int(f)) for s, f in zip(source_index, frame_index)} == \
        {(s, f) for s, (n, _, _) in enumerate(align_cases.MANY_BATCHES) for f in range(n)}
    cover = align_cases.branch_coverage(source_index, matrices)
    assert cover['mixed'] >= 5 and cover['all_fill'] >= 1 and cover['last_row'] >= 1 and cover['before_left'] >= 1, cover
