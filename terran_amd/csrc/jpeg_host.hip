// Baseline JPEG, host half: marker parser and Huffman decoder (ITU-T T.81, annexes B, C, F).  No HIP call: this file is
// also what ta_jpeg_coefficients runs on a machine without a GPU.  The device half (dequantisation, IDCT, upsampling,
// colour) is jpeg.hip.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "jpeg.h"

namespace {

// zig-zag position -> natural (row-major) position; 16 extra entries so that a corrupt run length past 63 lands on
// coefficient 63 as it does in libjpeg (it keeps the same guard)
const uint8_t kNatural[64 + 16] = {
    0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13,
    6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31,
    39, 46, 53, 60, 61, 54, 47, 55, 62, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63};

// The standard Huffman tables of annex K.3: counts per code length (DC luminance, DC chrominance, AC luminance, AC
// chrominance) and symbols
const uint8_t kStdBits[4][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0},
                                 {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0},
                                 {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125},
                                 {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
const uint8_t kStdDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const uint8_t kStdAcLuma[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07,
    0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0,
    0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49,
    0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
    0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7,
    0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5,
    0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
    0xf9, 0xfa,};
const uint8_t kStdAcChroma[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71,
    0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0,
    0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
    0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5,
    0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
    0xf9, 0xfa,};

int fail(std::string* err, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
int fail(std::string* err, const char* fmt, ...) {
  if (err) {
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    *err = buf;
  }
  return TA_E_INVALID;
}

inline int be16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

// Builds the decoding tables of one DHT table (annex C); false for a code set that overflows its code space.
bool build_huff(ta_jpeg_huff* h, const uint8_t counts[16], const uint8_t* vals, int nvals) {
  memset(h->look, 0, sizeof(h->look));
  memcpy(h->vals, vals, nvals);
  int code = 0, k = 0;
  for (int l = 1; l <= 16; ++l) {
    const int c = counts[l - 1];
    h->valoff[l] = k - code;
    if (code + c >= (1 << l)) return false;   // libjpeg refuses a set that reaches the all-ones code as well
    for (int i = 0; i < c; ++i, ++k, ++code)
      if (l <= 9)
        for (int j = 0; j < (1 << (9 - l)); ++j) h->look[(code << (9 - l)) | j] = (uint16_t)((l << 8) | vals[k]);
    h->maxcode[l] = c ? code - 1 : -1;
    code <<= 1;
  }
  h->maxcode[0] = -1;
  h->maxcode[17] = 0x7fffffff;
  h->present = true;
  return true;
}

// Bit reader over entropy-coded data: removes stuffed zero bytes, stops at a marker and feeds zero bits after it (as
// libjpeg does).  Consuming such a made-up bit means the data ended early: `overrun` then reports corrupt data.
struct bits {
  const uint8_t* p;
  const uint8_t* end;
  uint64_t acc = 0;      // next bits at the top
  int n = 0;             // valid bits in acc
  int pad = 0;           // of those, made-up zero bits at the bottom
  bool at_marker = false;

  void fill() {
    while (n <= 56) {
      int b = 0;
      if (!at_marker) {
        if (p >= end) {
          at_marker = true;
        } else if (p[0] != 0xFF) {
          b = *p++;
        } else if (p + 1 < end && p[1] == 0x00) {
          b = 0xFF;
          p += 2;
        } else {
          at_marker = true;                 // p stays on the marker's 0xFF
        }
      }
      if (at_marker) pad += 8;
      acc |= (uint64_t)b << (56 - n);
      n += 8;
    }
  }
  inline int peek(int k) { return (int)(acc >> (64 - k)); }
  inline void skip(int k) {
    acc <<= k;
    n -= k;
  }
  inline bool overrun() const { return n < pad; }
  inline int get(int k) {                     // k in 1..16, enough bits buffered
    const int v = peek(k);
    skip(k);
    return v;
  }
};

// One Huffman symbol; -1 for a code no table entry matches.  Needs >= 16 bits buffered.
inline int decode_sym(bits& b, const ta_jpeg_huff& h) {
  const int look = h.look[b.peek(9)];
  if (look) {
    b.skip(look >> 8);
    return look & 0xFF;
  }
  int l = 10;
  int code = b.peek(10);
  while (code > h.maxcode[l]) {
    ++l;
    if (l > 16) return -1;
    code = b.peek(l);
  }
  b.skip(l);
  return h.vals[(h.valoff[l] + code) & 0xFF];
}

inline int extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

}  // namespace

int ta_jpeg_parse(const uint8_t* data, size_t size, ta_jpeg_parsed* p, std::string* err) {
  ta_jpeg_header& h = p->hdr;
  memset(&h, 0, sizeof(h));
  for (auto& t : p->dc) t.present = false;
  for (auto& t : p->ac) t.present = false;
  if (!data || size < 4 || data[0] != 0xFF || data[1] != 0xD8) return fail(err, "not a JPEG (no SOI marker)");
  const uint8_t* q = data + 2;
  const uint8_t* end = data + size;
  bool saw_jfif = false, saw_adobe = false, saw_sof = false, sequential = false;
  int adobe_transform = -1;
  bool q_defined[4] = {false, false, false, false};
  int comp_id[3] = {0, 0, 0};
  int fallback = TA_JPEG_DEVICE;
  p->end = end;
  for (;;) {
    // next marker: 0xFF, any 0xFF fill bytes, then the code
    if (q >= end) return fail(err, "truncated before the scan");
    if (*q != 0xFF) return fail(err, "expected a marker at byte %zu, found 0x%02x", (size_t)(q - data), *q);
    while (q < end && *q == 0xFF) ++q;
    if (q >= end) return fail(err, "truncated before the scan");
    const int m = *q++;
    if (m == 0xD8) return fail(err, "second SOI marker");
    if (m == 0xD9) return fail(err, "EOI before any scan");
    if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) return fail(err, "marker 0x%02x outside a scan", m);
    if (m == 0x00) return fail(err, "stray 0xFF00 before the scan");
    if (end - q < 2) return fail(err, "truncated marker segment");
    const int len = be16(q);
    if (len < 2 || len > end - q) return fail(err, "marker 0x%02x: bad segment length %d", m, len);
    const uint8_t* s = q + 2;
    const int n = len - 2;
    q += len;
    if (m >= 0xC0 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC) {         // SOFn
      if (saw_sof) return fail(err, "second SOF marker");
      saw_sof = true;
      if (n < 6) return fail(err, "SOF too short");
      h.height = be16(s + 1);
      h.width = be16(s + 3);
      h.components = s[5];
      if (m == 0xC0 || m == 0xC1) sequential = true;
      else if (m >= 0xC9) fallback = TA_JPEG_FALLBACK_ARITHMETIC;
      else fallback = TA_JPEG_FALLBACK_PROCESS;                                   // progressive, lossless, hierarchical
      if (n < 6 + 3 * h.components) return fail(err, "SOF too short for %d components", h.components);
      if (h.width == 0) return fail(err, "image width 0");
      if (h.height == 0) return fail(err, "image height 0 (DNL marker not supported)");
      if (h.components == 0) return fail(err, "no components");
      if (fallback != TA_JPEG_DEVICE) continue;
      if (s[0] != 8) { fallback = TA_JPEG_FALLBACK_PRECISION; continue; }
      if (h.components != 1 && h.components != 3) { fallback = TA_JPEG_FALLBACK_COMPONENTS; continue; }
      for (int c = 0; c < h.components; ++c) {
        comp_id[c] = s[6 + 3 * c];
        h.h_samp[c] = s[7 + 3 * c] >> 4;
        h.v_samp[c] = s[7 + 3 * c] & 15;
        h.quant_index[c] = s[8 + 3 * c];
        if (h.h_samp[c] < 1 || h.h_samp[c] > 4 || h.v_samp[c] < 1 || h.v_samp[c] > 4)
          return fail(err, "component %d: bad sampling factors", c);
        if (h.quant_index[c] > 3) return fail(err, "component %d: quantisation table %d", c, h.quant_index[c]);
      }
    } else if (m == 0xC4) {                                                        // DHT
      const uint8_t* t = s;
      while (t < s + n) {
        if (s + n - t < 17) return fail(err, "DHT too short");
        const int tc = t[0] >> 4, th = t[0] & 15;
        if (tc > 1 || th > 3) return fail(err, "DHT: bad table class / id 0x%02x", t[0]);
        int total = 0;
        for (int i = 0; i < 16; ++i) total += t[1 + i];
        if (total > 256 || s + n - t < 17 + total) return fail(err, "DHT: bad symbol count");
        if (!build_huff(tc ? &p->ac[th] : &p->dc[th], t + 1, t + 17, total)) return fail(err, "DHT: code set overflows");
        t += 17 + total;
      }
    } else if (m == 0xDB) {                                                        // DQT
      const uint8_t* t = s;
      while (t < s + n) {
        const int pq = t[0] >> 4, tq = t[0] & 15;
        if (pq > 1 || tq > 3) return fail(err, "DQT: bad precision / id 0x%02x", t[0]);
        const int bytes = pq ? 128 : 64;
        if (s + n - t < 1 + bytes) return fail(err, "DQT too short");
        for (int k = 0; k < 64; ++k) h.quant[tq][kNatural[k]] = (uint16_t)(pq ? be16(t + 1 + 2 * k) : t[1 + k]);
        q_defined[tq] = true;
        t += 1 + bytes;
      }
    } else if (m == 0xDD) {                                                        // DRI
      if (n < 2) return fail(err, "DRI too short");
      h.restart_interval = be16(s);
    } else if (m == 0xE0) {
      if (n >= 5 && !memcmp(s, "JFIF\0", 5)) saw_jfif = true;
    } else if (m == 0xEE) {
      if (n >= 12 && !memcmp(s, "Adobe", 5)) {
        saw_adobe = true;
        adobe_transform = s[11];
      }
    } else if (m == 0xDA) {                                                        // SOS
      if (!saw_sof) return fail(err, "SOS before SOF");
      if (fallback != TA_JPEG_DEVICE) break;
      if (n < 1) return fail(err, "SOS too short");
      const int ns = s[0];
      if (n < 4 + 2 * ns || ns < 1 || ns > 4) return fail(err, "SOS: bad length");
      if (ns != h.components) { fallback = TA_JPEG_FALLBACK_SCANS; break; }
      for (int k = 0; k < ns; ++k) {
        int c = 0;
        while (c < h.components && comp_id[c] != s[1 + 2 * k]) ++c;
        if (c == h.components) return fail(err, "SOS: unknown component id %d", s[1 + 2 * k]);
        for (int j = 0; j < k; ++j)
          if (p->scan_order[j] == c) return fail(err, "SOS: component %d listed twice", c);
        p->scan_order[k] = c;
        p->dc_sel[c] = s[2 + 2 * k] >> 4;
        p->ac_sel[c] = s[2 + 2 * k] & 15;
        if (p->dc_sel[c] > 3 || p->ac_sel[c] > 3) return fail(err, "SOS: bad table selector");
      }
      const uint8_t* t = s + 1 + 2 * ns;
      if (t[0] != 0 || t[1] != 63 || t[2] != 0) return fail(err, "SOS: spectral selection %d..%d / %d in a sequential scan", t[0], t[1], t[2]);
      p->scan = q;
      break;
    }
    // APPn, COM, DAC and the rest: skipped
  }
  (void)sequential;
  if (fallback != TA_JPEG_DEVICE) {
    h.path = fallback;
    return TA_OK;
  }
  // colour space, as libjpeg decides it by default (jdapimin.c: JFIF, then Adobe's transform, then component ids)
  if (h.components == 3) {
    bool rgb = false;
    if (saw_jfif) rgb = false;
    else if (saw_adobe) rgb = adobe_transform == 0;
    else rgb = comp_id[0] == 'R' && comp_id[1] == 'G' && comp_id[2] == 'B';
    if (rgb) { h.path = TA_JPEG_FALLBACK_COLOR; return TA_OK; }
  }
  int hmax = 1, vmax = 1, blocks_in_mcu = 0;
  for (int c = 0; c < h.components; ++c) {
    hmax = h.h_samp[c] > hmax ? h.h_samp[c] : hmax;
    vmax = h.v_samp[c] > vmax ? h.v_samp[c] : vmax;
    blocks_in_mcu += h.h_samp[c] * h.v_samp[c];
  }
  if (h.components > 1 && blocks_in_mcu > 10) return fail(err, "sampling factors too large for an interleaved scan");
  if (h.components == 1) {
    // a single-component scan is not interleaved: MCU = one block and the plane is the image, whatever the sampling
    // factors say (libjpeg decodes a 2x2 grayscale file like a 1x1 one)
    hmax = vmax = 1;
  } else {
    for (int c = 0; c < h.components; ++c) {
      const int rh = hmax / h.h_samp[c], rv = vmax / h.v_samp[c];
      if (hmax % h.h_samp[c] || vmax % h.v_samp[c] || rh > 2 || rv > 2) { h.path = TA_JPEG_FALLBACK_SAMPLING; return TA_OK; }
    }
  }
  // Motion-JPEG frames usually carry no DHT: like libjpeg, undefined tables 0 and 1 are the standard ones (annex K.3)
  for (int k = 0; k < 2; ++k) {
    if (!p->dc[k].present) build_huff(&p->dc[k], kStdBits[k], kStdDcVals, 12);
    if (!p->ac[k].present) build_huff(&p->ac[k], kStdBits[2 + k], k ? kStdAcChroma : kStdAcLuma, 162);
  }
  for (int c = 0; c < h.components; ++c) {
    if (!q_defined[h.quant_index[c]]) return fail(err, "quantisation table %d is not defined", h.quant_index[c]);
    if (!p->dc[p->dc_sel[c]].present || !p->ac[p->ac_sel[c]].present)
      return fail(err, "Huffman table %d / %d is not defined", p->dc_sel[c], p->ac_sel[c]);
  }
  p->hmax = hmax;
  p->vmax = vmax;
  int64_t off = 0;
  if (h.components == 1) {
    p->mcus_x = (h.width + 7) / 8;
    p->mcus_y = (h.height + 7) / 8;
    h.h_samp[0] = h.v_samp[0] = 1;           // reported as what the decode does: full resolution
    h.blocks_w[0] = p->mcus_x;
    h.blocks_h[0] = p->mcus_y;
    h.blocks_total = (int64_t)p->mcus_x * p->mcus_y;
  } else {
    p->mcus_x = (h.width + 8 * hmax - 1) / (8 * hmax);
    p->mcus_y = (h.height + 8 * vmax - 1) / (8 * vmax);
    for (int c = 0; c < h.components; ++c) {
      h.blocks_w[c] = p->mcus_x * h.h_samp[c];
      h.blocks_h[c] = p->mcus_y * h.v_samp[c];
      h.block_offset[c] = off;
      off += (int64_t)h.blocks_w[c] * h.blocks_h[c];
    }
    h.blocks_total = off;
  }
  h.path = TA_JPEG_DEVICE;
  return TA_OK;
}

int ta_jpeg_entropy_decode(const ta_jpeg_parsed* p, int16_t* coefs, std::string* err) {
  const ta_jpeg_header& h = p->hdr;
  bits b;
  b.p = p->scan;
  b.end = p->end;
  const int nc = h.components;
  int pred[3] = {0, 0, 0};
  const int64_t mcus = (int64_t)p->mcus_x * p->mcus_y;
  const int ri = h.restart_interval;
  int64_t left = ri;
  int next_rst = 0;
  // per MCU: the blocks of each scan component in order, each with its destination
  for (int64_t mcu = 0; mcu < mcus; ++mcu) {
    if (ri && left == 0) {
      // restart: the rest of the byte is padding, then RSTn, then fresh bits and DC predictions
      if (b.n - b.pad >= 8) return fail(err, "restart marker expected after MCU %lld", (long long)mcu);
      while (b.p + 1 < b.end && b.p[0] == 0xFF && b.p[1] == 0xFF) ++b.p;   // fill bytes may precede any marker (B.1.1.2)
      if (b.p + 1 >= b.end || b.p[0] != 0xFF || b.p[1] != 0xD0 + next_rst)
        return fail(err, "missing restart marker RST%d before MCU %lld", next_rst, (long long)mcu);
      b.p += 2;
      b.acc = 0;
      b.n = b.pad = 0;
      b.at_marker = false;
      next_rst = (next_rst + 1) & 7;
      pred[0] = pred[1] = pred[2] = 0;
      left = ri;
    }
    --left;
    const int mx = (int)(mcu % p->mcus_x), my = (int)(mcu / p->mcus_x);
    for (int k = 0; k < nc; ++k) {
      const int c = p->scan_order[k];
      const ta_jpeg_huff& dc = p->dc[p->dc_sel[c]];
      const ta_jpeg_huff& ac = p->ac[p->ac_sel[c]];
      const int hs = nc == 1 ? 1 : h.h_samp[c], vs = nc == 1 ? 1 : h.v_samp[c];
      for (int v = 0; v < vs; ++v)
        for (int u = 0; u < hs; ++u) {
          const int64_t bx = (int64_t)mx * hs + u, by = (int64_t)my * vs + v;
          int16_t* blk = coefs + (h.block_offset[c] + by * h.blocks_w[c] + bx) * 64;
          memset(blk, 0, 64 * sizeof(int16_t));
          b.fill();
          int s = decode_sym(b, dc);
          if (s < 0) return fail(err, "bad Huffman code (DC, MCU %lld)", (long long)mcu);
          s &= 15;
          int diff = 0;
          if (s) {
            if (b.n < 32) b.fill();
            diff = extend(b.get(s), s);
          }
          pred[c] = (int)((unsigned)pred[c] + (unsigned)diff);      // a corrupt stream wraps instead of overflowing
          blk[0] = (int16_t)pred[c];
          for (int kk = 1; kk < 64; ++kk) {
            if (b.n < 32) b.fill();
            const int rs = decode_sym(b, ac);
            if (rs < 0) return fail(err, "bad Huffman code (AC, MCU %lld)", (long long)mcu);
            const int r = rs >> 4, sz = rs & 15;
            if (sz) {
              kk += r;
              blk[kNatural[kk]] = (int16_t)extend(b.get(sz), sz);
            } else if (r == 15) {
              kk += 15;
            } else {
              break;
            }
          }
          if (b.overrun()) return fail(err, "entropy-coded data ends early (MCU %lld of %lld)", (long long)mcu, (long long)mcus);
        }
    }
  }
  return TA_OK;
}

extern "C" int ta_jpeg_coefficients(const uint8_t* data, size_t size, ta_jpeg_header* header, int16_t* coefs,
                                    int64_t capacity_blocks, char* err, int err_capacity) {
  std::string msg;
  auto out_err = [&](int rc) {
    if (err && err_capacity > 0) snprintf(err, (size_t)err_capacity, "%s", msg.c_str());
    return rc;
  };
  if (!header) {
    msg = "null header";
    return out_err(TA_E_INVALID);
  }
  ta_jpeg_parsed* p = new ta_jpeg_parsed();
  int rc = ta_jpeg_parse(data, size, p, &msg);
  if (rc == TA_OK) {
    *header = p->hdr;
    if (p->hdr.path == TA_JPEG_DEVICE && coefs) {
      if (capacity_blocks < p->hdr.blocks_total) {
        msg = "capacity_blocks below blocks_total";
        rc = TA_E_CAPACITY;
      } else {
        rc = ta_jpeg_entropy_decode(p, coefs, &msg);
      }
    }
  }
  delete p;
  return out_err(rc);
}
