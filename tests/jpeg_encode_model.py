"""numpy restatement of libjpeg-turbo's default baseline encode (what terran_amd/csrc/jpeg_encode.hip computes).

Test infrastructure (the yardstick of tests/test_jpeg_encode_cpu.py), written from the JPEG standard and libjpeg's
documented integer arithmetic, and pinned black-box against the installed Pillow by that test's random encodes:

  quant tables   Annex K.1 tables, jcparam.c quality scaling (q < 50: 5000 / q, else 200 - 2 q), (b s + 50) / 100
                 clamped to 1..255 (force_baseline)
  colour         jccolor.c RGB -> YCbCr, SCALEBITS 16 tables; Cb / Cr carry ONE_HALF - 1 and CENTERJSAMPLE << 16
  edges          jcsample.c / jcprepct.c: the last column replicated out to the padded component width (times the
                 downsampling ratio), the last row down to a whole row group, the last downsampled row down to the
                 iMCU row
  downsample     h2v1: (a + b + bias) >> 1, bias 0, 1, 0, 1 ... across output columns; h2v2: (a + b + c + d + bias) >> 2,
                 bias 1, 2, 1, 2 ...  (smoothing off)
  forward DCT    jfdctint.c islow: CONST_BITS 13, PASS1_BITS 2, input level-shifted by -128, output scaled by 8
  quantise       round half away from zero of x / 8Q (jcdctmgr.c's reciprocal multiply: quant_reciprocal shows
                 it is this division)
  dummy blocks   jccoefct.c: blocks of an MCU past the component's block grid have zero AC and the DC of the block
                 coded before them
  Huffman        the K.3 standard tables, DC prediction per component in scan order, ZRL / EOB, negative values as
                 value - 1 in their low bits, 0xFF stuffed with 0x00, the last byte padded with 1 bits

`encode(rgb, quality, subsampling)` returns the file `Image.fromarray(rgb).save(f, 'JPEG', quality=quality,
subsampling=subsampling)` writes (subsampling 0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0).
"""
import numpy as np

LUMA_Q = np.array([
    16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
    14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
    49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99], np.int64)
CHROMA_Q = np.array([
    17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
    47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32, np.int64)

ZIGZAG = np.array([                       # jpeg_natural_order: zigzag position k -> natural (row-major) index
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
    28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
    54, 47, 55, 62, 63], np.int64)

# K.3 standard Huffman tables: (counts of codes of length 1..16, symbols)
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14,
    0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09,
    0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a,
    0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65,
    0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88,
    0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9,
    0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca,
    0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea,
    0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32,
    0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16,
    0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39,
    0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64,
    0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86,
    0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7,
    0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8,
    0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9,
    0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])

SAMPLING = {0: (1, 1), 1: (2, 1), 2: (2, 2)}     # subsampling -> luma (h, v); chroma is always 1 x 1


def quant_tables(quality):
    """(2, 64) int64 natural order: jpeg_set_quality(quality, force_baseline=TRUE)."""
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.stack([np.clip((b * scale + 50) // 100, 1, 255) for b in (LUMA_Q, CHROMA_Q)])


def quant_reciprocal(x, q):
    """jcdctmgr.c (libjpeg-turbo, 16-bit DCTELEM): compute_reciprocal(8 q) and quantize() applied to the DCT outputs
    x (int64, |x| < 2^15).  The tests show it equals `quantise`."""
    d = 8 * int(q)
    b = d.bit_length() - 1
    r = 16 + b
    fq, fr = divmod(1 << r, d)
    c = d // 2
    if fr == 0:
        fq >>= 1
        r -= 1
    elif fr <= d // 2:
        c += 1
    else:
        fq += 1
    # product = (UDCTELEM2)(|x| + corr) * recip, >> (shift + 16) with shift = r - 16 (the SIMD form multiplies by
    # scale = 2^(32 - r) and takes the high halves twice: the same floor)
    ax = np.abs(np.asarray(x, np.int64))
    res = ((ax + c) * fq) >> r
    return np.where(x < 0, -res, res)


def quantise(x, q):
    """x / 8q rounded half away from zero."""
    d = 8 * np.asarray(q, np.int64)
    r = (np.abs(x) + d // 2) // d
    return np.where(x < 0, -r, r)


def rgb_to_ycc(rgb):
    """(H, W, 3) uint8 -> three (H, W) int64 planes, jccolor.c rgb_ycc_convert."""
    def fix(x):
        return int(x * 65536 + 0.5)
    r, g, b = (rgb[..., k].astype(np.int64) for k in range(3))
    half, cbcr = 1 << 15, 128 << 16
    y = (fix(0.29900) * r + fix(0.58700) * g + fix(0.11400) * b + half) >> 16
    cb = (-fix(0.16874) * r - fix(0.33126) * g + fix(0.5) * b + cbcr + half - 1) >> 16
    cr = (fix(0.5) * r - fix(0.41869) * g - fix(0.08131) * b + cbcr + half - 1) >> 16
    return y, cb, cr


def _pad(p, rows, cols):
    """Replicate the last row / column of p out to (rows, cols) (never crops)."""
    return np.pad(p, ((0, max(0, rows - p.shape[0])), (0, max(0, cols - p.shape[1]))), mode='edge')


def component_plane(full, H, W, h, v, hmax, vmax, mcus_y):
    """One component's padded, downsampled sample plane: (mcus_y * 8 v, bw * 8) int64, bw its real block width."""
    bw = -(-W * h // (8 * hmax))
    rh, rv = hmax // h, vmax // v
    p = _pad(full, -(-H // vmax) * vmax, bw * 8 * rh)[:, :bw * 8 * rh]
    if rh == 2 and rv == 1:
        bias = np.tile([0, 1], bw * 4)
        p = (p[:, 0::2] + p[:, 1::2] + bias) >> 1
    elif rh == 2 and rv == 2:
        bias = np.tile([1, 2], bw * 4)
        p = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
    return _pad(p, mcus_y * 8 * v, p.shape[1])


def fdct_islow(blocks):
    """(B, 8, 8) int64 samples (0..255) -> (B, 8, 8) DCT outputs scaled by 8 (jfdctint.c)."""
    def pass_(d, first):
        t0, t7 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7]
        t1, t6 = d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
        t2, t5 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5]
        t3, t4 = d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
        t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
        n = 11 if first else 15                  # CONST_BITS - PASS1_BITS, then CONST_BITS + PASS1_BITS

        def ds(x, s):
            return (x + (1 << (s - 1))) >> s
        o = [None] * 8
        if first:
            o[0], o[4] = (t10 + t11) << 2, (t10 - t11) << 2
        else:
            o[0], o[4] = ds(t10 + t11, 2), ds(t10 - t11, 2)
        z1 = (t12 + t13) * 4433
        o[2] = ds(z1 + t13 * 6270, n)
        o[6] = ds(z1 - t12 * 15137, n)
        z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
        z5 = (z3 + z4) * 9633
        t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
        z1, z2 = z1 * -7373, z2 * -20995
        z3, z4 = z3 * -16069 + z5, z4 * -3196 + z5
        o[7] = ds(t4 + z1 + z3, n)
        o[5] = ds(t5 + z2 + z4, n)
        o[3] = ds(t6 + z2 + z3, n)
        o[1] = ds(t7 + z1 + z4, n)
        return np.stack(o, axis=-1)
    d = blocks.astype(np.int64) - 128
    d = pass_(d, True)                                              # rows
    d = np.swapaxes(pass_(np.swapaxes(d, 1, 2), False), 1, 2)      # columns
    return d


def layout(H, W, subsampling):
    """Per component: (h, v, blocks_w, blocks_h of the MCU grid, real blocks_w, real blocks_h); and (mcus_x, mcus_y)."""
    hl, vl = SAMPLING[subsampling]
    mx, my = -(-W // (8 * hl)), -(-H // (8 * vl))
    comps = []
    for h, v in ((hl, vl), (1, 1), (1, 1)):
        comps.append((h, v, mx * h, my * v, -(-W * h // (8 * hl)), -(-H * v // (8 * vl))))
    return comps, (mx, my)


def coefficients(rgb, quality, subsampling):
    """Quantised coefficients as ta_jpeg_coefficients returns them: (blocks, 64) int16 natural order, component after
    component, each component's MCU block grid (dummy blocks included) in raster order."""
    H, W = rgb.shape[:2]
    comps, (mx, my) = layout(H, W, subsampling)
    hmax, vmax = comps[0][0], comps[0][1]
    qt = quant_tables(quality)
    out = []
    for c, full in enumerate(rgb_to_ycc(rgb)):
        h, v, gw, gh, bw, bh = comps[c]
        p = component_plane(full, H, W, h, v, hmax, vmax, my)
        blocks = p[:bh * 8].reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3).reshape(-1, 8, 8)
        q = quantise(fdct_islow(blocks).reshape(-1, 64), qt[0 if c == 0 else 1]).reshape(bh, bw, 64)
        grid = np.zeros((gh, gw, 64), np.int64)
        grid[:bh, :bw] = q
        # dummy blocks, in the MCU order the encoder codes them: right of the real grid, then whole dummy rows
        for by in range(gh):
            for bx in range(gw):
                if by < bh and bx < bw:
                    continue
                mcu_x = bx // h
                if by >= bh:                    # jccoefct.c: a dummy row takes the DC of the MCU's last block above
                    sx, sy = min(mcu_x * h + h - 1, bw - 1), bh - 1
                else:
                    sx, sy = bw - 1, by
                grid[by, bx, 0] = grid[sy, sx, 0]
        out.append(grid.reshape(-1, 64))
    return np.concatenate(out).astype(np.int16)


class _Bits:
    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def put(self, code, size):
        self.acc = (self.acc << size) | (code & ((1 << size) - 1))
        self.n += size
        while self.n >= 8:
            self.n -= 8
            byte = (self.acc >> self.n) & 0xFF
            self.out.append(byte)
            if byte == 0xFF:
                self.out.append(0)
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put(0x7F, 8 - self.n)


def huff_codes(table):
    """(counts, symbols) -> {symbol: (code, length)} (Annex C)."""
    counts, syms = table
    codes, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            codes[syms[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return codes


def _category(x):
    return int(abs(int(x))).bit_length()


def scan_bytes(coefs, H, W, subsampling):
    """Entropy-coded segment (stuffed, padded) from `coefficients` output."""
    comps, (mx, my) = layout(H, W, subsampling)
    tabs = [(huff_codes(DC_LUMA), huff_codes(AC_LUMA)), (huff_codes(DC_CHROMA), huff_codes(AC_CHROMA))]
    grids, off = [], 0
    for h, v, gw, gh, _, _ in comps:
        grids.append(coefs[off:off + gw * gh].reshape(gh, gw, 64).astype(np.int64))
        off += gw * gh
    bits = _Bits()
    pred = [0, 0, 0]
    for my_ in range(my):
        for mx_ in range(mx):
            for c, (h, v, _, _, _, _) in enumerate(comps):
                dc_t, ac_t = tabs[0 if c == 0 else 1]
                for yy in range(v):
                    for xx in range(h):
                        blk = grids[c][my_ * v + yy, mx_ * h + xx][ZIGZAG]
                        d = int(blk[0]) - pred[c]
                        pred[c] = int(blk[0])
                        s = _category(d)
                        bits.put(*dc_t[s])
                        if s:
                            bits.put(d - 1 if d < 0 else d, s)
                        run = 0
                        for k in range(1, 64):
                            a = int(blk[k])
                            if a == 0:
                                run += 1
                                continue
                            while run > 15:
                                bits.put(*ac_t[0xF0])
                                run -= 16
                            s = _category(a)
                            bits.put(*ac_t[(run << 4) | s])
                            bits.put(a - 1 if a < 0 else a, s)
                            run = 0
                        if run:
                            bits.put(*ac_t[0x00])
    bits.flush()
    return bytes(bits.out)


def _segment(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, 'big') + payload


def header(H, W, quality, subsampling):
    """SOI .. SOS, as Pillow / libjpeg-turbo writes it."""
    qt = quant_tables(quality)
    hl, vl = SAMPLING[subsampling]
    out = b'\xff\xd8'
    out += _segment(0xE0, b'JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00')
    for t in range(2):
        out += _segment(0xDB, bytes([t]) + bytes(qt[t][ZIGZAG].astype(np.uint8)))
    out += _segment(0xC0, bytes([8]) + H.to_bytes(2, 'big') + W.to_bytes(2, 'big') + bytes(
        [3, 1, (hl << 4) | vl, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for cls_idx, table in ((0x00, DC_LUMA), (0x10, AC_LUMA), (0x01, DC_CHROMA), (0x11, AC_CHROMA)):
        out += _segment(0xC4, bytes([cls_idx]) + bytes(table[0]) + bytes(table[1]))
    out += _segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    return out


def encode(rgb, quality=75, subsampling=2):
    rgb = np.asarray(rgb, np.uint8)
    H, W = rgb.shape[:2]
    coefs = coefficients(rgb, quality, subsampling)
    return header(H, W, quality, subsampling) + scan_bytes(coefs, H, W, subsampling) + b'\xff\xd9'
