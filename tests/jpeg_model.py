"""numpy restatement of the pixel half of libjpeg-turbo's default decode (what terran_amd/csrc/jpeg.hip computes).

Test infrastructure (the yardstick of tests/test_jpeg_cpu.py), written from the JPEG standard and libjpeg's documented
integer arithmetic, and pinned black-box against the installed Pillow by that test's random encodes:

  dequantise + islow IDCT   jidctint.c: CONST_BITS 13, PASS1_BITS 2, descale by 11 then 18, then the range-limit table
                            (its C code's integer widths: see idct_blocks)
  upsample                  jdsample.c fancy upsampling: h2v1 / h1v2 triangle filters (bias 1 / 2), h2v2 (bias 8 / 7),
                            edges replicated over the real downsampled size; h2v1 / h2v2 box replication when that
                            width is <= 2
  colour                    jdcolor.c YCbCr -> RGB, SCALEBITS 16

`decode(header, coefs)` takes what `lib.jpeg_coefficients` returns and gives the (H, W, 3) uint8 RGB image
`np.asarray(Image.open(f).convert('RGB'))` gives.
"""
import numpy as np

FIX = dict(f0298=2446, f0390=3196, f0541=4433, f0765=6270, f0899=7373, f1175=9633, f1501=12299, f1847=15137,
           f1961=16069, f2053=16819, f2562=20995, f3072=25172)


def _idct_1d(v, shift):
    """v: (..., 8) int64 along the last axis -> (..., 8) descaled by `shift`."""
    f = FIX
    c = [v[..., k] for k in range(8)]
    z1 = (c[2] + c[6]) * f['f0541']
    tmp2 = z1 - c[6] * f['f1847']
    tmp3 = z1 + c[2] * f['f0765']
    tmp0 = (c[0] + c[4]) << 13
    tmp1 = (c[0] - c[4]) << 13
    t10, t13, t11, t12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    o0, o1, o2, o3 = c[7], c[5], c[3], c[1]
    z1, z2, z3, z4 = o0 + o3, o1 + o2, o0 + o2, o1 + o3
    z5 = (z3 + z4) * f['f1175']
    o0, o1, o2, o3 = o0 * f['f0298'], o1 * f['f2053'], o2 * f['f3072'], o3 * f['f1501']
    z1, z2 = z1 * -f['f0899'], z2 * -f['f2562']
    z3, z4 = z3 * -f['f1961'] + z5, z4 * -f['f0390'] + z5
    o0, o1, o2, o3 = o0 + z1 + z3, o1 + z2 + z4, o2 + z2 + z3, o3 + z1 + z4
    r = 1 << (shift - 1)
    out = [t10 + o3, t11 + o2, t12 + o1, t13 + o0, t13 - o0, t12 - o1, t11 - o2, t10 - o3]
    return np.stack([(x + r) >> shift for x in out], axis=-1)


def range_limit(x):
    """libjpeg's post-IDCT table, indexed by x & 1023."""
    x = x & 1023
    return np.where(x < 128, x + 128, np.where(x < 512, 255, np.where(x < 896, 0, x - 896))).astype(np.uint8)


def _int32(x):
    """C's (int) of a 64-bit value (two's-complement wrap)."""
    return ((x + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def idct_blocks(coefs, quant):
    """coefs (B, 64) int16 natural order, quant (64,) -> (B, 8, 8) uint8 samples.  jidctint.c's C arithmetic: 16-bit
    signed dequantisation multipliers, 64-bit sums, the pass-1 workspace and the range-limit index taken as int (all
    three only matter for coefficients no 8-bit image produces)."""
    q = quant.astype(np.uint16).view(np.int16).astype(np.int64)
    d = (coefs.astype(np.int64) * q).reshape(-1, 8, 8)
    cols = _int32(_idct_1d(np.swapaxes(d, 1, 2), 11))          # pass 1 over columns: (B, col, row)
    rows = _idct_1d(np.swapaxes(cols, 1, 2), 18)               # pass 2 over rows
    return range_limit(rows)


def plane(header, coefs, c):
    """Component c's sample plane, (blocks_h * 8, blocks_w * 8) uint8."""
    bw, bh, off = int(header['blocks_w'][c]), int(header['blocks_h'][c]), int(header['block_offset'][c])
    q = header['quant'][int(header['quant_index'][c])]
    blocks = idct_blocks(coefs[off:off + bw * bh], q).reshape(bh, bw, 8, 8)
    return blocks.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


def _h2(p, dw, bias_lo, bias_hi, shift, scale):
    """Horizontal doubling of the rows of p (..., dw) with the triangle filter: out[2i] = (3 s[i] + s[i-1] + lo) >> shift,
    out[2i+1] = (3 s[i] + s[i+1] + hi) >> shift, where s = scale-weighted sums (edges replicated)."""
    s = p[:, :dw]
    left = np.concatenate([s[:, :1], s[:, :-1]], axis=1)
    right = np.concatenate([s[:, 1:], s[:, -1:]], axis=1)
    out = np.empty((s.shape[0], 2 * dw), np.int64)
    out[:, 0::2] = (3 * s + left + bias_lo) >> shift
    out[:, 1::2] = (3 * s + right + bias_hi) >> shift
    return out


def upsample(p, dw, dh, rh, rv, H, W):
    """jdsample.c on a plane whose real size is dh x dw -> (H, W) int64."""
    p = p[:dh, :dw].astype(np.int64)
    if rh == 1 and rv == 1:
        return p[:H, :W]
    if rv == 1:
        if dw <= 2:
            return np.repeat(p, 2, axis=1)[:H, :W]
        return _h2(p, dw, 1, 2, 2, 1)[:H, :W]
    up = np.concatenate([p[:1], p[:-1]], axis=0)
    down = np.concatenate([p[1:], p[-1:]], axis=0)
    if rh == 1:
        out = np.empty((2 * dh, dw), np.int64)
        out[0::2] = (3 * p + up + 1) >> 2
        out[1::2] = (3 * p + down + 2) >> 2
        return out[:H, :W]
    if dw <= 2:
        return np.repeat(np.repeat(p, 2, axis=0), 2, axis=1)[:H, :W]
    out = np.empty((2 * dh, 2 * dw), np.int64)
    out[0::2] = _h2(3 * p + up, dw, 8, 7, 4, 1)
    out[1::2] = _h2(3 * p + down, dw, 8, 7, 4, 1)
    return out[:H, :W]


def ycc_to_rgb(y, cb, cr):
    cb, cr = cb - 128, cr - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-46802 * cr - 22554 * cb + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def decode(header, coefs):
    H, W, nc = int(header['height']), int(header['width']), int(header['components'])
    if nc == 1:
        y = plane(header, coefs, 0)[:H, :W]
        return np.repeat(y[..., None], 3, axis=2)
    hs, vs = [int(x) for x in header['h_samp']], [int(x) for x in header['v_samp']]
    hmax, vmax = max(hs), max(vs)
    comps = []
    for c in range(3):
        dw = -(-W * hs[c] // hmax)
        dh = -(-H * vs[c] // vmax)
        comps.append(upsample(plane(header, coefs, c), dw, dh, hmax // hs[c], vmax // vs[c], H, W))
    return ycc_to_rgb(*comps)
