"""JPEG decode, host half (no GPU): the Huffman decoder behind ta_jpeg_coefficients plus tests/jpeg_model.py (the numpy
restatement of the device kernels' arithmetic) against the reference's open_image pixels (tests/golden/jpeg.npz), the
fallback decisions, malformed input, and -- where Pillow is importable -- a few hundred seeded random encodes."""
import hashlib
import io
import os

import numpy as np
import pytest

from tests import jpeg_model

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, 'tests', 'golden')


def golden():
    g = np.load(os.path.join(GOLDEN, 'jpeg.npz'))
    out = {}
    for name in g['names']:
        name = str(name)
        if 'jpg_' + name in g:
            data = g['jpg_' + name].tobytes()
        else:
            with open(os.path.join(GOLDEN, name + '.jpg'), 'rb') as fh:
                data = fh.read()
        out[name] = dict(data=data, path=int(g['path_' + name]),
                         rgb=g['rgb_' + name] if 'rgb_' + name in g else None,
                         sha=str(g['sha_' + name]) if 'sha_' + name in g else None,
                         rows=g['rows_' + name] if 'rows_' + name in g else None)
    return out


def assert_matches(got, fx, name):
    """got (H, W, 3) uint8 equals the fixture's expected pixels (stored in full, or as sha256 + per-row sums)."""
    if fx['rgb'] is not None:
        assert got.shape == fx['rgb'].shape, (name, got.shape, fx['rgb'].shape)
        bad = np.argwhere((got != fx['rgb']).any(-1))
        assert len(bad) == 0, '%s: %d pixels differ, first %s' % (name, len(bad), bad[:4].tolist())
    else:
        rows = got.reshape(got.shape[0], -1).astype(np.int64).sum(1)
        assert rows.shape == fx['rows'].shape, (name, got.shape)
        bad = np.nonzero(rows != fx['rows'])[0]
        assert len(bad) == 0, '%s: rows %s differ' % (name, bad[:8].tolist())
        assert hashlib.sha256(np.ascontiguousarray(got).tobytes()).hexdigest() == fx['sha'], name


def host_decode(data):
    from terran_amd import lib
    hdr, coefs = lib.jpeg_coefficients(data)
    assert coefs is not None, 'fallback path %d' % hdr['path']
    return jpeg_model.decode(hdr, coefs)


@pytest.fixture(scope='module')
def built():
    from terran_amd import build
    build.build()


def test_golden_fixtures_bit_exact(built):
    fixtures = golden()
    assert len([f for f in fixtures.values() if f['path'] == 0]) >= 29
    for name, fx in fixtures.items():
        if fx['path'] == 0:
            assert_matches(host_decode(fx['data']), fx, name)


def test_fixture_headers(built):
    """The sampling factors and restart intervals the fixtures are meant to cover are what the parser reads."""
    from terran_amd import lib
    fx = golden()
    seen = set()
    for name, f in fx.items():
        hdr, _ = lib.jpeg_coefficients(f['data'], header_only=True)
        assert int(hdr['path']) == f['path'], name
        if f['path'] == 0:
            seen.add((int(hdr['components']), tuple(hdr['h_samp'][:hdr['components']]),
                      tuple(hdr['v_samp'][:hdr['components']])))
            assert (int(hdr['restart_interval']) > 0) == name.startswith('rst_'), name
    assert {(1, (1,), (1,)), (3, (1, 1, 1), (1, 1, 1)), (3, (2, 1, 1), (1, 1, 1)), (3, (2, 1, 1), (2, 1, 1)),
            (3, (1, 1, 1), (2, 1, 1))} <= seen, seen


def test_fallback_paths(built):
    from terran_amd import lib
    fx = golden()
    assert lib.jpeg_coefficients(fx['progressive_40x56']['data'])[1] is None
    hdr, coefs = lib.jpeg_coefficients(fx['cmyk_40x56']['data'])
    assert coefs is None and hdr['path'] == 4 and hdr['components'] == 4
    assert (hdr['width'], hdr['height']) == (56, 40)


def _invalid(data, match=None):
    from terran_amd import lib
    with pytest.raises(lib.TerranAmdError, match=match) as e:
        lib.jpeg_coefficients(data)
    assert e.value.code == lib.E_INVALID


def test_malformed_inputs_are_invalid(built):
    data = golden()['s420_q75_97x203']['data']
    _invalid(b'', 'SOI')
    _invalid(b'\x89PNG\r\n\x1a\n' + bytes(64), 'SOI')
    _invalid(bytes(np.random.default_rng(0).integers(0, 256, 4096, dtype=np.uint8)), 'SOI')
    _invalid(b'\xff\xd8' + bytes(np.random.default_rng(1).integers(0, 256, 4096, dtype=np.uint8)))
    sos = data.index(b'\xff\xda')
    for cut in (3, 40, sos, sos + 20, len(data) // 2, len(data) - 200):
        _invalid(data[:cut])
    _invalid(b'\xff\xd8\xff\xd9', 'EOI')
    # a marker code where the SOF should be: SOF0 rewritten as a second SOI
    sof = data.index(b'\xff\xc0')
    _invalid(data[:sof + 1] + b'\xd8' + data[sof + 2:], 'SOI')
    # the quantisation table a component names is missing
    dqt = data.index(b'\xff\xdb')
    _invalid(data[:dqt + 1] + b'\xfe' + data[dqt + 2:], 'quantisation')
    # a Huffman table whose code set overflows its code space
    dht = data.index(b'\xff\xc4')
    bad = bytearray(data)
    bad[dht + 5:dht + 21] = bytes([2, 2] + [0] * 14)
    _invalid(bytes(bad))
    # corrupt entropy data: the decoder must stop, never read past the buffer
    rng = np.random.default_rng(2)
    for k in range(20):
        bad = bytearray(data)
        for at, v in zip(rng.integers(sos + 20, len(data) - 2, 16), rng.integers(0, 256, 16)):
            bad[int(at)] = int(v)
        from terran_amd import lib
        try:
            lib.jpeg_coefficients(bytes(bad))          # may still decode (garbage pixels) -- or report TA_E_INVALID
        except lib.TerranAmdError as e:
            assert e.code == lib.E_INVALID


def test_grayscale_with_2x2_sampling_decodes_at_full_resolution(built):
    """A single-component scan is not interleaved: whatever sampling factors it declares, its plane is the image."""
    from terran_amd import lib
    f = golden()['gray22_q90_61x77']
    assert f['data'][f['data'].index(b'\xff\xc0') + 11] == 0x22
    hdr, _ = lib.jpeg_coefficients(f['data'], header_only=True)
    assert (hdr['path'], hdr['h_samp'][0], hdr['v_samp'][0], hdr['blocks_w'][0], hdr['blocks_h'][0]) == (0, 1, 1, 10, 8)
    assert_matches(host_decode(f['data']), golden()['gray_q90_61x77'], 'gray22 vs gray11')


def test_standard_tables_and_fill_bytes(built):
    """A frame without DHT decodes with the standard tables; 0xFF fill bytes before RSTn are skipped; a scan naming an
    undefined table 2 or 3 (no standard one) is invalid."""
    fx = golden()
    assert b'\xff\xc4' not in fx['mjpeg_nodht_s422_97x203']['data'].split(b'\xff\xda')[0]
    assert b'\xff\xff\xff\xd0' in fx['rst_fill_s420_97x203']['data']
    data = fx['s420_q75_17x33']['data']
    sos = data.index(b'\xff\xda')
    bad = bytearray(data)
    bad[sos + 6] = 0x22                                          # component 1: DC table 2, AC table 2
    _invalid(bytes(bad), 'Huffman table')


def test_restart_marker_out_of_sequence_is_invalid(built):
    data = bytearray(golden()['rst_blocks5_s420_97x203']['data'])
    i = data.index(b'\xff\xd1')
    data[i + 1] = 0xD3
    _invalid(bytes(data), 'restart')


def test_open_image_equals_reference(tmp_path, built):
    pytest.importorskip('PIL')
    from terran_amd import image
    fx = golden()
    for name in ('s420_q75_17x33', 'gray_q50_9x5', 's440_q90_48x48', 'cmyk_40x56'):
        p = tmp_path / (name + '.jpg')
        p.write_bytes(fx[name]['data'])
        assert_matches(image.open_image(p), fx[name], name)
        assert_matches(image.open_image(str(p)), fx[name], name)
    for name in ('rw-1', 'rw-2'):
        assert_matches(image.open_image(os.path.join(GOLDEN, name + '.jpg')), fx[name], name)


def patch_440(data):
    """4:2:2 -> 4:4:0 (Pillow cannot encode it): the luma sampling byte in SOF0 goes from 0x21 to 0x12."""
    d = bytearray(data)
    luma = d.index(b'\xff\xc0') + 11
    assert d[luma] == 0x21
    d[luma] = 0x12
    return bytes(d)


def strip_dht(data):
    """Drop the DHT segments (Pillow encodes with the standard tables, which the decoder then has to supply)."""
    d = bytearray(data)
    while True:
        i = d.find(b'\xff\xc4')
        if i < 0 or i > d.index(b'\xff\xda'):
            return bytes(d)
        del d[i:i + 2 + ((d[i + 2] << 8) | d[i + 3])]


def test_random_encodes_match_pillow(built):
    """Seeded random sizes, qualities, subsamplings, restart intervals, grayscale (also declaring 2 x 2 sampling) and
    frames without DHT: the host decoder + numpy model equal the installed Pillow's decode bit for bit."""
    Image = pytest.importorskip('PIL.Image')
    from terran_amd import lib, synth
    rng = np.random.default_rng(20261016)
    for t in range(300):
        h, w = int(rng.integers(1, 80)), int(rng.integers(1, 80))
        mode = int(rng.integers(5))
        if mode == 3:
            w = h                       # the patch keeps the MCU count (and so the block stream) only for square images
        img = synth.frames(int(rng.integers(1 << 20)), 1, h, w)[0]
        kw = dict(quality=int(rng.integers(1, 101)))
        if rng.random() < 0.2:
            kw['restart_marker_blocks'] = int(rng.integers(1, 8))
        b = io.BytesIO()
        if mode == 4:
            Image.fromarray(img).convert('L').save(b, 'JPEG', **kw)
        else:
            Image.fromarray(img).save(b, 'JPEG', subsampling=(0, 1, 2, 1)[mode], **kw)
        data = b.getvalue()
        if mode == 3:                                           # 4:4:0 from a 4:2:2 encode (the sampling byte patched)
            data = patch_440(data)
        if mode == 4 and rng.random() < 0.3:                    # grayscale declaring 2 x 2 sampling
            i = data.index(b'\xff\xc0') + 11
            data = data[:i] + b'\x22' + data[i + 1:]
        if rng.random() < 0.2:                                  # Motion-JPEG style: no DHT, the standard tables
            data = strip_dht(data)
        want = np.asarray(Image.open(io.BytesIO(data)).convert('RGB'))
        hdr, coefs = lib.jpeg_coefficients(data)
        got = jpeg_model.decode(hdr, coefs)
        assert np.array_equal(got, want), (t, h, w, mode, kw)
