"""Generate tests/golden/jpeg.npz (+ the two quickstart photos) FROM THE REFERENCE's terran/io/image.py:open_image.

CONTAINER-ONLY (needs the reference tree and Pillow).  The JPEGs are Pillow encodes of synth.frames (4:4:4 / 4:2:2 /
4:2:0, qualities 30..100, odd sizes down to 1 x 1, restart intervals -- one with 0xFF fill bytes before each RSTn --,
grayscale, one declaring 2 x 2 sampling, a frame without DHT that relies on the standard tables), one 4:4:0 file (Pillow cannot encode
4:4:0: a 48 x 48 4:2:2 encode whose SOF0 luma sampling byte is patched from 0x21 to 0x12 -- the block stream is the
same, only its reading changes), and a progressive and a CMYK file for the Pillow fallback.  The expected pixels are the
reference's own `open_image` of each file, stored in full up to 4096 pixels and as the sha256 of the pixel bytes
plus per-row byte sums above that.  The quickstart photos rw-1.jpg / rw-2.jpg are copied next to
this script; their expected output is stored as the sha256 of the pixel bytes plus per-row byte sums.

npz keys: `names`; per name `jpg_<name>` (the file's bytes), `rgb_<name>` (H, W, 3) or `sha_<name>` + `rows_<name>`
(int64 per row) + `shape_<name>`, `path_<name>` (0 = decoded by the library, else the TA_JPEG_FALLBACK_* reason the file must report).

    python tests/golden/make_golden_jpeg.py
"""
import hashlib
import importlib.util
import io
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)

from tests.golden import ref_import as R   # noqa: E402
from terran_amd import synth               # noqa: E402

PHOTOS = ['rw-1.jpg', 'rw-2.jpg']
FULL_PIXELS = 4096          # larger images are stored as sha256 + per-row sums (keeps the file small)


def load_reference_open_image():
    path = os.path.join(R.REF_ROOT, 'terran', 'io', 'image.py')
    spec = importlib.util.spec_from_file_location('terran_io_image', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.open_image


def encode(img, **kw):
    from PIL import Image
    b = io.BytesIO()
    im = Image.fromarray(img)
    mode = kw.pop('mode', None)
    if mode:
        im = im.convert(mode)
    im.save(b, 'JPEG', **kw)
    return b.getvalue()


def patch_440(data):
    """4:2:2 -> 4:4:0: the luma component's sampling byte in SOF0 goes from 0x21 (2 x 1) to 0x12 (1 x 2)."""
    d = bytearray(data)
    sof = d.index(b'\xff\xc0')
    luma = sof + 2 + 2 + 6 + 1                       # marker, length, P Y X Nf, then component 1: id, HV
    assert d[luma] == 0x21, hex(d[luma])
    d[luma] = 0x12
    return bytes(d)


def patch_gray_22(data):
    """A grayscale file whose one component declares 2 x 2 sampling (valid; libjpeg decodes it like 1 x 1)."""
    d = bytearray(data)
    luma = d.index(b'\xff\xc0') + 11
    assert d[luma] == 0x11, hex(d[luma])
    d[luma] = 0x22
    return bytes(d)


def strip_dht(data):
    """Drop every DHT segment: a Motion-JPEG frame that relies on the standard tables (Pillow encodes with them)."""
    d = bytearray(data)
    while True:
        i = d.find(b'\xff\xc4')
        if i < 0 or i > d.index(b'\xff\xda'):
            return bytes(d)
        del d[i:i + 2 + ((d[i + 2] << 8) | d[i + 3])]


def fill_before_restarts(data):
    """Two 0xFF fill bytes in front of every RSTn marker (T.81 B.1.1.2 allows fill bytes before any marker)."""
    d = bytearray(data)
    scan = d.index(b'\xff\xda')
    out, i = d[:scan], scan
    while i < len(d):
        if d[i] == 0xFF and i + 1 < len(d) and 0xD0 <= d[i + 1] <= 0xD7:
            out += b'\xff\xff'
        out.append(d[i])
        i += 1
    return bytes(out)


def fixtures():
    f = {}
    base = synth.frames(11, 1, 97, 203)[0]
    for s, tag in ((0, '444'), (1, '422'), (2, '420')):
        f['s%s_q75_97x203' % tag] = (encode(base, quality=75, subsampling=s), 0)
    for q in (30, 95, 100):
        f['s420_q%d_97x203' % q] = (encode(base, quality=q, subsampling=2), 0)
    f['s444_q100_97x203'] = (encode(base, quality=100, subsampling=0), 0)
    f['s440_q90_48x48'] = (patch_440(encode(synth.frames(12, 1, 48, 48)[0], quality=90, subsampling=1)), 0)
    for h, w in ((1, 1), (7, 9), (17, 33), (250, 33), (33, 250), (2, 3)):
        img = synth.frames(13 + h + w, 1, h, w)[0]
        f['s420_q75_%dx%d' % (h, w)] = (encode(img, quality=75, subsampling=2), 0)
        f['s422_q90_%dx%d' % (h, w)] = (encode(img, quality=90, subsampling=1), 0)
    f['rst_blocks5_s420_97x203'] = (encode(base, quality=85, subsampling=2, restart_marker_blocks=5), 0)
    f['rst_rows2_s422_97x203'] = (encode(base, quality=85, subsampling=1, restart_marker_rows=2), 0)
    f['gray_q90_61x77'] = (encode(synth.frames(14, 1, 61, 77)[0], quality=90, mode='L'), 0)
    f['gray_q50_9x5'] = (encode(synth.frames(15, 1, 9, 5)[0], quality=50, mode='L'), 0)
    f['gray22_q90_61x77'] = (patch_gray_22(encode(synth.frames(14, 1, 61, 77)[0], quality=90, mode='L')), 0)
    f['mjpeg_nodht_s422_97x203'] = (strip_dht(encode(base, quality=80, subsampling=1)), 0)
    f['rst_fill_s420_97x203'] = (fill_before_restarts(encode(base, quality=85, subsampling=2, restart_marker_blocks=5)), 0)
    small = synth.frames(16, 1, 40, 56)[0]
    f['progressive_40x56'] = (encode(small, quality=80, progressive=True), 1)
    f['cmyk_40x56'] = (encode(small, quality=80, mode='CMYK'), 4)
    return f


def row_sums(rgb):
    return rgb.reshape(rgb.shape[0], -1).astype(np.int64).sum(1)


def digest(out, name, rgb):
    out['sha_' + name] = np.array(hashlib.sha256(np.ascontiguousarray(rgb).tobytes()).hexdigest())
    out['rows_' + name] = row_sums(rgb)
    out['shape_' + name] = np.array(rgb.shape, np.int32)


def main():
    open_image = load_reference_open_image()
    out = {}
    names = []
    with tempfile.TemporaryDirectory() as tmp:
        for name, (data, path) in fixtures().items():
            fn = os.path.join(tmp, name + '.jpg')
            with open(fn, 'wb') as fh:
                fh.write(data)
            rgb = open_image(fn)
            assert rgb.dtype == np.uint8 and rgb.ndim == 3 and rgb.shape[2] == 3
            out['jpg_' + name] = np.frombuffer(data, np.uint8)
            if rgb.shape[0] * rgb.shape[1] <= FULL_PIXELS:
                out['rgb_' + name] = rgb
            else:
                digest(out, name, rgb)
            out['path_' + name] = np.int32(path)
            names.append(name)
    for photo in PHOTOS:
        src = os.path.join(R.REF_ROOT, 'docs', 'assets', photo)
        shutil.copyfile(src, os.path.join(HERE, photo))
        rgb = open_image(src)
        name = photo[:-4]
        digest(out, name, rgb)
        out['path_' + name] = np.int32(0)
        names.append(name)
    out['names'] = np.array(names)
    np.savez_compressed(os.path.join(HERE, 'jpeg.npz'), **out)
    print('wrote %d fixtures, %d bytes' % (len(names), os.path.getsize(os.path.join(HERE, 'jpeg.npz'))))


if __name__ == '__main__':
    main()
