"""numpy / Python restatement of libjpeg's optimized Huffman coding (`save(..., 'JPEG', optimize=True)`), on top of
tests/jpeg_encode_model.py: what ta_jpeg_encode_opt computes with optimize = 1.

Test infrastructure (the yardstick of tests/test_jpeg_encode_optimize_cpu.py), pinned black-box against the installed
Pillow by that test's random encodes:

  statistics     per table class (0: Y, 1: Cb and Cr together) the DC categories and the AC symbols (run << 4) | size,
                 0xF0 per ZRL, 0x00 per EOB, of every coded block, dummy blocks included (jchuff.c htest_one_block)
  table          jchuff.c jpeg_gen_optimal_table (Annex K.2 with libjpeg's choices): the pseudo-symbol 256 counts 1;
                 the two least frequent entries are merged, of equals the one with the LARGER symbol first; lengths over
                 16 are shortened pairwise; the pseudo-symbol leaves the longest length; symbols by length, then value
  header         as the standard one, the four DHT segments (DC 0, AC 0, DC 1, AC 1) holding the image's tables

`encode(rgb, quality, subsampling)` returns the file `Image.fromarray(rgb).save(f, 'JPEG', quality=quality,
subsampling=subsampling, optimize=True)` writes.
"""
import numpy as np

from tests import jpeg_encode_model as M

MAX_CLEN = 32


def block_symbols(blk, pred):
    """One block in zigzag order -> (DC category, [AC symbols]) as the entropy coder emits them."""
    dc = M._category(int(blk[0]) - pred)
    ac, run = [], 0
    for k in range(1, 64):
        a = int(blk[k])
        if a == 0:
            run += 1
            continue
        while run > 15:
            ac.append(0xF0)
            run -= 16
        ac.append((run << 4) | M._category(a))
        run = 0
    if run:
        ac.append(0x00)
    return dc, ac


def histograms(coefs, H, W, subsampling):
    """`coefficients` output (or ta_jpeg_coefficients of a file) -> (dc (2, 257), ac (2, 257)) int64 symbol counts per
    table class; entry 256 is left 0."""
    comps, _ = M.layout(H, W, subsampling)
    dc, ac = np.zeros((2, 257), np.int64), np.zeros((2, 257), np.int64)
    off = 0
    for c, (h, v, gw, gh, _, _) in enumerate(comps):
        t = 0 if c == 0 else 1
        z = coefs[off:off + gw * gh].astype(np.int64)[:, M.ZIGZAG]
        off += gw * gh
        # DC differences follow the scan order inside the component: MCU raster, inside an MCU the blocks in raster
        grid = z[:, 0].reshape(gh // v, v, gw // h, h).transpose(0, 2, 1, 3).reshape(-1)
        diff = np.diff(np.concatenate([[0], grid]))
        for d in diff:
            dc[t, M._category(d)] += 1
        for blk in z:
            for s in block_symbols(blk, int(blk[0]))[1]:
                ac[t, s] += 1
    return dc, ac


def unlimited_lengths(freq):
    """Huffman's procedure as jpeg_gen_optimal_table runs it -> codesize[257] before any limiting."""
    freq = [int(x) for x in freq[:256]] + [1]
    codesize, others = [0] * 257, [-1] * 257
    while True:
        c1, v = -1, 1000000000
        for i in range(257):
            if freq[i] and freq[i] <= v:
                v, c1 = freq[i], i
        c2, v = -1, 1000000000
        for i in range(257):
            if freq[i] and freq[i] <= v and i != c1:
                v, c2 = freq[i], i
        if c2 < 0:
            return codesize
        freq[c1] += freq[c2]
        freq[c2] = 0
        codesize[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            codesize[c1] += 1
        others[c1] = c2
        codesize[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            codesize[c2] += 1


def optimal_table(freq):
    """257 frequencies (entry 256 ignored) -> (counts of codes of length 1..16, symbols in code order)."""
    codesize = unlimited_lengths(freq)
    bits = [0] * (MAX_CLEN + 1)
    for cs in codesize:
        if cs:
            assert cs <= MAX_CLEN
            bits[cs] += 1
    i = MAX_CLEN
    while i > 16:
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
        i -= 1
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1
    vals = [j for length in range(1, MAX_CLEN + 1) for j in range(256) if codesize[j] == length]
    return bits[1:17], vals


def tables(coefs, H, W, subsampling):
    """-> [DC 0, AC 0, DC 1, AC 1] as (counts, symbols), the order of the DHT segments."""
    dc, ac = histograms(coefs, H, W, subsampling)
    return [optimal_table(dc[0]), optimal_table(ac[0]), optimal_table(dc[1]), optimal_table(ac[1])]


def header(H, W, quality, subsampling, tabs):
    std = M.header(H, W, quality, subsampling)
    at = len(std) - 432 - 14                          # the standard DHT segments (33 + 183 + 33 + 183 bytes), then SOS
    assert std[at:at + 2] == b'\xff\xc4' and std[-14:-12] == b'\xff\xda'
    out = std[:at]
    for cls_idx, (counts, syms) in zip((0x00, 0x10, 0x01, 0x11), tabs):
        out += M._segment(0xC4, bytes([cls_idx]) + bytes(counts) + bytes(syms))
    return out + std[-14:]


def scan_bytes(coefs, H, W, subsampling, tabs):
    saved = M.DC_LUMA, M.AC_LUMA, M.DC_CHROMA, M.AC_CHROMA
    try:                                              # the standard model's scan with this image's tables
        M.DC_LUMA, M.AC_LUMA, M.DC_CHROMA, M.AC_CHROMA = tabs
        return M.scan_bytes(coefs, H, W, subsampling)
    finally:
        M.DC_LUMA, M.AC_LUMA, M.DC_CHROMA, M.AC_CHROMA = saved


def encode(rgb, quality=75, subsampling=2):
    rgb = np.asarray(rgb, np.uint8)
    H, W = rgb.shape[:2]
    coefs = M.coefficients(rgb, quality, subsampling)
    tabs = tables(coefs, H, W, subsampling)
    return header(H, W, quality, subsampling, tabs) + scan_bytes(coefs, H, W, subsampling, tabs) + b'\xff\xd9'


def parse_dht(data):
    """The DHT segments of a file, in file order: [(class << 4 | index, counts[16], symbols)]."""
    out, at = [], 2
    while True:
        assert data[at] == 0xFF
        marker, length = data[at + 1], int.from_bytes(data[at + 2:at + 4], 'big')
        seg, k = data[at + 4:at + 2 + length], 0
        if marker == 0xC4:
            while k < len(seg):
                counts = list(seg[k + 1:k + 17])
                out.append((seg[k], counts, list(seg[k + 17:k + 17 + sum(counts)])))
                k += 17 + sum(counts)
        at += 2 + length
        if marker == 0xDA:
            return out
