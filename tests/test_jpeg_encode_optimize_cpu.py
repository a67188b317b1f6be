"""JPEG encode with optimize=True, host side (no GPU): tests/jpeg_encode_optimize_model.py (symbol statistics, libjpeg's
optimal tables, per-image headers) against the Pillow files recorded in tests/golden/jpeg_encode_optimize.npz and 300
seeded live-Pillow encodes; ta_jpeg_optimal_table against the model's tables; tables built from the symbol counts of
ta_jpeg_coefficients of Pillow's own files against the DHT segments of those files; and the `optimize` keyword through
jpeg_options, encode_jpeg's checks and JpegVideoWriter with an injected encoder."""
import io
import os

import numpy as np
import pytest

from tests import jpeg_encode_model as M
from tests import jpeg_encode_optimize_model as O
from tests.test_jpeg_encode_cpu import _code, _random_image

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, 'tests', 'golden')


def golden():
    g = np.load(os.path.join(GOLDEN, 'jpeg_encode_optimize.npz'))
    out = {}
    for name in g['names']:
        name = str(name)
        q, s = (int(x) for x in g['opt_' + name])
        out[name] = dict(px=g['px_' + name], quality=q, subsampling=s, jpg=g['jpg_' + name].tobytes())
    return out


@pytest.fixture(scope='module')
def fx():
    return golden()


@pytest.fixture(scope='module')
def built():
    from terran_amd import build
    build.build()


@pytest.fixture(scope='module')
def hists(fx):
    """name -> (dc, ac) symbol counts of the model's coefficients."""
    out = {}
    for name, f in fx.items():
        s = _code(f['subsampling'])
        H, W = f['px'].shape[:2]
        out[name] = O.histograms(M.coefficients(f['px'], f['quality'], s), H, W, s)
    return out


def _four(h):
    dc, ac = h
    return [dc[0], ac[0], dc[1], ac[1]]


def test_golden_covers_the_contract(fx, hists):
    shapes = {f['px'].shape[:2] for f in fx.values()}
    assert {(1, 1), (17, 9), (250, 33)} <= shapes
    for hw in [(17, 9), (250, 33)]:
        assert {f['subsampling'] for f in fx.values() if f['px'].shape[:2] == hw} >= {0, 1, 2, -1}
    assert {f['quality'] for f in fx.values()} >= {1, 30, 75, 90, 100}
    for kind in ('flat', 'gradient', 'saturated', 'noise', 'rw-1', 'batch', 'deep'):
        assert any(n.startswith(kind) for n in fx), kind
    # a flat image: EOB is the only AC symbol (tables with a single real symbol); DC: each component's first
    # difference, then zeros
    dc, ac = hists['flat_24x40_s0_q100']
    assert [int((t > 0).sum()) for t in (ac[0], ac[1])] == [1, 1] and ac[0][0] and ac[1][0]
    assert int((dc[0] > 0).sum()) <= 2 and int((dc[1] > 0).sum()) <= 3
    assert int(hists['noise_24x40_s0_q100'][1][0].sum()) > 500                       # hundreds of symbols coded
    assert max(int((h[1][t] > 0).sum()) for h in hists.values() for t in (0, 1)) >= 40  # tables of dozens of codes
    # the length limit: a tree deeper than 16 before it, a full 16-bit level after it
    deep = next(n for n in fx if n.startswith('deep'))
    assert max(max(O.unlimited_lengths(t)) for t in _four(hists[deep])) > 16
    assert max(max(O.unlimited_lengths(t)) for n in fx if n != deep for t in _four(hists[n])) <= 16
    # optimized files are never larger than the standard ones
    for name, f in fx.items():
        assert len(f['jpg']) <= len(M.encode(f['px'], f['quality'], _code(f['subsampling']))), name


def test_model_equals_golden_bytes(fx):
    for name, f in fx.items():
        got = O.encode(f['px'], f['quality'], _code(f['subsampling']))
        assert got == f['jpg'], name


def test_model_equals_live_pillow_on_random_encodes():
    Image = pytest.importorskip('PIL.Image')
    rng = np.random.default_rng(2025)
    for t in range(300):
        h, w = int(rng.integers(1, 80)), int(rng.integers(1, 80))
        q, s = int(rng.integers(1, 101)), int(rng.integers(0, 3))
        px = _random_image(rng, t % 4, h, w)
        f = io.BytesIO()
        Image.fromarray(px).save(f, 'JPEG', quality=q, subsampling=s, optimize=True)
        assert O.encode(px, q, s) == f.getvalue(), (t, h, w, q, s)


def test_optimal_table_entry_equals_the_model(built, hists):
    from terran_amd import lib
    tables = 0
    for name, h in hists.items():
        for t in _four(h):
            counts, syms = O.optimal_table(t)
            assert lib.jpeg_optimal_table(t) == (counts, syms), name
            tables += 1
    assert tables == 4 * len(hists)
    rng = np.random.default_rng(6)
    for k in range(60):                                         # ties, sparse and dense tables, big counts, deep trees
        f = np.zeros(257, np.int64)
        n = int(rng.integers(1, 257))
        idx = rng.choice(256, n, replace=False)
        f[idx] = [rng.integers(1, 4, n), rng.integers(1, 10**9 // 257, n),
                  (1.7 ** (rng.permutation(n) % 24)).astype(np.int64)][k % 3]
        f[256] = int(rng.integers(0, 5))                        # ignored: the pseudo-symbol always counts 1
        assert lib.jpeg_optimal_table(f) == O.optimal_table(f), k


def test_optimal_table_entry_refuses_bad_frequencies(built):
    from terran_amd import lib
    for bad in [np.zeros(257, np.int64), np.r_[-1, np.ones(256, np.int64)], np.r_[10**9, np.zeros(256, np.int64)]]:
        with pytest.raises(lib.TerranAmdError):
            lib.jpeg_optimal_table(bad)
    assert lib.jpeg_optimal_table(np.r_[10**9 - 1, np.zeros(256, np.int64)]) == ([1] + [0] * 15, [0])


def test_tables_from_pillows_own_coefficients_equal_its_dht_segments(built, fx):
    """The statistics and the table builder against Pillow alone: the symbol counts over the coefficients the library's
    entropy decoder reads from Pillow's file give, through ta_jpeg_optimal_table, the tables that file carries, in its
    order: DC 0, AC 0, DC 1, AC 1, one DHT segment each."""
    from terran_amd import lib
    for name, f in fx.items():
        s = _code(f['subsampling'])
        H, W = f['px'].shape[:2]
        hdr, coefs = lib.jpeg_coefficients(f['jpg'])
        assert coefs is not None, name
        got = [lib.jpeg_optimal_table(t) for t in _four(O.histograms(coefs, H, W, s))]
        dht = O.parse_dht(f['jpg'])
        assert [d[0] for d in dht] == [0x00, 0x10, 0x01, 0x11], name
        assert f['jpg'].count(b'\xff\xc4') >= 4
        assert [(d[1], d[2]) for d in dht] == got, name


def test_optimize_keyword_is_checked_before_anything_runs():
    from terran_amd import image

    class Boom:
        def __getattr__(self, k):
            raise AssertionError('touched before the options were checked')
    for bad in (1, 0, 'yes', None, 2.0):
        with pytest.raises(ValueError):
            image.jpeg_options(75, -1, bad)
        with pytest.raises(ValueError):
            image.encode_jpeg(Boom(), 75, -1, optimize=bad)
        with pytest.raises(ValueError):
            image.save_images(Boom(), [], optimize=bad)
    assert image.jpeg_options(90, '4:4:4', optimize=True) == (90, 0) == image.jpeg_options(90, 0, False)
    for opt in ('progressive', 'qtables', 'restart_marker_blocks', 'dpi'):
        with pytest.raises(TypeError):
            image.encode_jpeg(np.zeros((8, 8, 3), np.uint8), **{opt: True})


def test_video_writer_passes_optimize_to_the_encoder():
    from terran_amd.video import JpegVideoWriter
    calls = []

    def enc(images, quality, subsampling, **kw):
        calls.append((len(images), quality, subsampling, kw))
        return [b'\xff\xd8' + bytes([k]) + b'\xff\xd9' for k in range(len(images))]

    def enc3(images, quality, subsampling):                     # the hook as it was: three positional arguments
        calls.append((len(images), quality, subsampling, None))
        return [b'\xff\xd8\xff\xd9'] * len(images)
    out = io.BytesIO()
    with JpegVideoWriter(out, quality=90, subsampling='4:2:2', encoder=enc, optimize=True) as w:
        assert w.optimize is True
        w.write_frames([0, 1])
        w.write_frame([5])
    with JpegVideoWriter(out, quality=80, encoder=enc3) as w:
        assert w.optimize is False
        w.write_frames([0, 1, 2])
    with JpegVideoWriter(out, encoder=enc3, optimize=False) as w:
        w.write_frame([0])
    assert calls == [(2, 90, '4:2:2', {'optimize': True}), (1, 90, '4:2:2', {'optimize': True}), (3, 80, -1, None),
                     (1, 75, -1, None)]
    assert out.getvalue().count(b'\xff\xd8') == 7
    for bad in (1, 'yes', None):
        with pytest.raises(ValueError):
            JpegVideoWriter(io.BytesIO(), optimize=bad)
