// Baseline JPEG encoder: resident uint8 RGB frames -> complete JFIF files, byte for byte what Pillow (libjpeg-turbo,
// default options: islow DCT, standard Huffman tables, no smoothing, no restart markers) writes for the same quality
// and subsampling.  Every stage runs on the device; only the finished files cross PCIe.  Pure integer code:
// tests/jpeg_encode_model.py restates it and tests/test_jpeg_encode_cpu.py pins that against Pillow.
//
// Passes (each covers every image of the call; a batch's images share one block layout):
//   E1 je_coef_kernel   colour conversion, edge replication, downsampling, islow FDCT, quantisation -> int16
//                       coefficients in zigzag order, one 128-byte block per SLOT.  Slots are numbered in scan order
//                       (MCU raster, inside an MCU the Y blocks in H x V raster, then Cb, then Cr); every image owns a
//                       whole number of 256-slot chunks, the tail slots are unused.
//   E2 je_len_kernel    bit length of every block (DC difference to the previous block of its component in scan order,
//                       AC run / size codes, ZRL, EOB) and the total of each 256-slot chunk
//   S  je_scan_kernel   per image: exclusive scan of the chunk totals -> chunk bit offsets, the image's total bits;
//                       the totals go to the host, which sizes the bit-word buffer exactly
//   E3 je_emit_kernel   each block writes its codes at its bit offset into the zeroed word buffer: words only it
//                       touches with plain stores, the first and last (shared with its neighbours) with atomicOr --
//                       OR does not depend on arrival order, so the stream is bitwise deterministic.  Bit order: stream
//                       bit p is bit 7 - (p & 7) of byte p >> 3, the bytes in memory order (each 32-bit word is
//                       assembled big-endian and byte-swapped before it is written)
//   E4a je_ffcount_kernel  0xFF bytes per 4 KB chunk of each stream (after the final byte's padding with 1 bits)
//   S  je_scan_kernel   per image: chunk offsets of the stuffing zeros, the image's total; to the host again
//   E4b je_pack_kernel  header, stuffed stream and EOI of every image, back to back, into one packed buffer
// then ONE device-to-host copy of the packed files into the context's pinned output.
//
// optimize = 1 (Pillow's optimize=True: per-image Huffman tables) adds, between E1 and E2,
//   ES je_stat_kernel   symbol counts of every image per table class (0: Y, 1: Cb and Cr): DC categories, AC
//                       (run << 4) | size, ZRL, EOB -- the symbols E2 / E3 code, from the same walk_block
// whose histograms (JE_TABLE_WORDS uint32 an image) go to the host.  It builds every table as libjpeg's
// jpeg_gen_optimal_table does (optimal_table below), the code words E2 / E3 read (one table set per image) and every
// image's own header (its DHT segments differ in length), and sends both back.  With optimize = 0 E2 / E3 read the one
// standard table set (stride 0) and every image's header entry names the one shared header.
#include <string.h>

#include <chrono>
#include <vector>

#include "ta_internal.h"

namespace {

#define JE_SLOTS 256                     // slots per chunk (= E2 / E3 workgroup)
#define JE_FF_CHUNK 4096                 // stream bytes per E4 workgroup: 256 threads x 16 bytes
#define JE_LDS_STRIDE 72                 // ints per block in LDS (E1), as in the decoder's IDCT kernel
#define JE_TABLE_WORDS 544               // one table set: dc [2][16], ac [2][256]; code words and histograms alike
#define JE_HEADER_STRIDE 1024            // room for one optimized header (at most 191 + 2 x (37 + 277) bytes)
#define JE_MAX_COUNT 1000000000ll        // jpeg_gen_optimal_table's "infinite" frequency

struct je_params {
  const uint8_t* src;                    // (n, h, w, 3) uint8
  int32_t n, h, w;
  int32_t hl, vl;                        // luma sampling factors (chroma is 1 x 1)
  int32_t bpm;                           // blocks per MCU
  int32_t mcus_x, mcus_y;
  int32_t nblocks;                       // blocks per image
  int32_t spi;                           // slots per image (nblocks rounded up to JE_SLOTS)
  int32_t bw[3], bh[3];                  // real block grid of each component (without dummy blocks)
};

__constant__ uint8_t je_zigzag[64] = {   // zigzag position -> natural index
    0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// K.1 tables (natural order) and K.3 Huffman tables (counts of lengths 1..16, symbols)
const uint8_t kLumaQ[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,
                            14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
                            18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                            49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
const uint8_t kChromaQ[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                              99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                              99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
const uint8_t kDcLumaBits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
const uint8_t kDcChromaBits[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
const uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const uint8_t kAcLumaBits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
const uint8_t kAcLumaVals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14,
    0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09,
    0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a,
    0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65,
    0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88,
    0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9,
    0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca,
    0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea,
    0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
const uint8_t kAcChromaBits[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
const uint8_t kAcChromaVals[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32,
    0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16,
    0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39,
    0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64,
    0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86,
    0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7,
    0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8,
    0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9,
    0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};

// jpeg_set_quality(quality, force_baseline = TRUE): table t (0 luma, 1 chroma), natural order
void quant_table(int quality, int t, uint16_t* out) {
  const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  const uint8_t* base = t ? kChromaQ : kLumaQ;
  for (int i = 0; i < 64; ++i) {
    int v = (base[i] * scale + 50) / 100;
    out[i] = (uint16_t)(v < 1 ? 1 : (v > 255 ? 255 : v));
  }
}

// Annex C: symbol -> (length << 16) | code
void huff_codes(const uint8_t* bits, const uint8_t* vals, uint32_t* out, int n_out) {
  memset(out, 0, sizeof(uint32_t) * n_out);
  uint32_t code = 0;
  int k = 0;
  for (int len = 1; len <= 16; ++len) {
    for (int i = 0; i < bits[len - 1]; ++i) out[vals[k++]] = (uint32_t)len << 16 | code++;
    code <<= 1;
  }
}

void put_segment(std::vector<uint8_t>& o, uint8_t marker, const std::vector<uint8_t>& payload) {
  o.push_back(0xFF);
  o.push_back(marker);
  const size_t len = payload.size() + 2;
  o.push_back((uint8_t)(len >> 8));
  o.push_back((uint8_t)len);
  o.insert(o.end(), payload.begin(), payload.end());
}

struct je_huff {                         // one table as a DHT segment holds it
  uint8_t bits[17];                      // [1..16]: codes of each length
  uint8_t vals[256];
  int nvals;
};

// SOI .. SOS as libjpeg-turbo writes them for Pillow's defaults; opt: the image's own tables (DC 0, AC 0, DC 1, AC 1)
// in place of the standard ones
std::vector<uint8_t> make_header(int h, int w, int quality, int subsampling, const je_huff* opt = nullptr) {
  std::vector<uint8_t> o = {0xFF, 0xD8};
  put_segment(o, 0xE0, {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
  for (int t = 0; t < 2; ++t) {
    uint16_t q[64];
    quant_table(quality, t, q);
    std::vector<uint8_t> p = {(uint8_t)t};
    for (int k = 0; k < 64; ++k) p.push_back((uint8_t)q[kZigzag[k]]);
    put_segment(o, 0xDB, p);
  }
  const uint8_t luma = subsampling == 0 ? 0x11 : (subsampling == 1 ? 0x21 : 0x22);
  put_segment(o, 0xC0, {8, (uint8_t)(h >> 8), (uint8_t)h, (uint8_t)(w >> 8), (uint8_t)w, 3, 1, luma, 0, 2, 0x11, 1, 3,
                        0x11, 1});
  const struct {
    uint8_t id;
    const uint8_t *bits, *vals;
    int nv;
  } dht[4] = {{0x00, kDcLumaBits, kDcVals, 12},
              {0x10, kAcLumaBits, kAcLumaVals, 162},
              {0x01, kDcChromaBits, kDcVals, 12},
              {0x11, kAcChromaBits, kAcChromaVals, 162}};
  for (int k = 0; k < 4; ++k) {
    const auto& d = dht[k];
    std::vector<uint8_t> p = {d.id};
    if (opt) {
      p.insert(p.end(), opt[k].bits + 1, opt[k].bits + 17);
      p.insert(p.end(), opt[k].vals, opt[k].vals + opt[k].nvals);
    } else {
      p.insert(p.end(), d.bits, d.bits + 16);
      p.insert(p.end(), d.vals, d.vals + d.nv);
    }
    put_segment(o, 0xC4, p);
  }
  put_segment(o, 0xDA, {3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0});
  return o;
}

// jchuff.c jpeg_gen_optimal_table (Annex K.2 with libjpeg's choices, which Pillow's files show): freq[0..255] symbol
// counts below JE_MAX_COUNT, not all zero; freq[256] is the pseudo-symbol that keeps the all-ones code free
// false: a code longer than 32 bits (libjpeg's JERR_HUFF_CLEN_OVERFLOW)
bool optimal_table(const int64_t* counts, je_huff* out) {
  const int kMaxLen = 32;
  int64_t freq[257];
  int codesize[257], others[257];
  uint8_t bits[kMaxLen + 1] = {};
  for (int i = 0; i < 256; ++i) freq[i] = counts[i];
  freq[256] = 1;
  for (int i = 0; i < 257; ++i) {
    codesize[i] = 0;
    others[i] = -1;
  }
  for (;;) {
    // the two least frequent entries; of equal ones the larger symbol first
    int c1 = -1, c2 = -1;
    int64_t v = JE_MAX_COUNT;
    for (int i = 0; i <= 256; ++i)
      if (freq[i] && freq[i] <= v) {
        v = freq[i];
        c1 = i;
      }
    v = JE_MAX_COUNT;
    for (int i = 0; i <= 256; ++i)
      if (freq[i] && freq[i] <= v && i != c1) {
        v = freq[i];
        c2 = i;
      }
    if (c2 < 0) break;
    freq[c1] += freq[c2];
    freq[c2] = 0;
    for (++codesize[c1]; others[c1] >= 0;) ++codesize[c1 = others[c1]];
    others[c1] = c2;
    for (++codesize[c2]; others[c2] >= 0;) ++codesize[c2 = others[c2]];
  }
  for (int i = 0; i <= 256; ++i) {
    if (codesize[i] > kMaxLen) return false;
    if (codesize[i]) ++bits[codesize[i]];
  }
  int i = kMaxLen;
  for (; i > 16; --i)                                          // no code longer than 16: shorten in pairs
    while (bits[i] > 0) {
      int j = i - 2;
      while (bits[j] == 0) --j;
      bits[i] -= 2;
      ++bits[i - 1];
      bits[j + 1] += 2;
      --bits[j];
    }
  while (bits[i] == 0) --i;                                    // the pseudo-symbol leaves the longest length
  --bits[i];
  memcpy(out->bits, bits, 17);
  int p = 0;
  for (int len = 1; len <= kMaxLen; ++len)
    for (int j = 0; j < 256; ++j)
      if (codesize[j] == len) out->vals[p++] = (uint8_t)j;
  out->nvals = p;
  return true;
}

inline int64_t align_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

// ---- device helpers ---------------------------------------------------------------------------------------------

// exclusive scan of one uint32 per thread over a 256-thread workgroup (4 waves of 64); lds: 4 words
__device__ __forceinline__ uint32_t wg_exclusive_scan(uint32_t v, uint32_t* lds, uint32_t* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t y = __shfl_up(x, o, 64);
    if (lane >= o) x += y;
  }
  if (lane == 63) lds[wave] = x;
  __syncthreads();
  uint32_t base = 0, tot = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t s = lds[k];
    base += k < wave ? s : 0;
    tot += s;
  }
  __syncthreads();                                         // lds is reused by the caller's next scan
  *total = tot;
  return base + x - v;
}

// jccolor.c rgb_ycc_convert (SCALEBITS 16): component c of one pixel
__device__ __forceinline__ int ycc(const uint8_t* __restrict__ p, int c) {
  const int r = p[0], g = p[1], b = p[2];
  if (c == 0) return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
  if (c == 1) return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
  return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

// jfdctint.c, one 1-D pass over 8 values in place; pass 1 (rows) scales up by PASS1_BITS, pass 2 (columns) descales
template <bool FIRST>
__device__ __forceinline__ void fdct8(int d[8]) {
  const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
  const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  const int n = FIRST ? 11 : 15, r = 1 << (n - 1);
  if (FIRST) {
    d[0] = (t10 + t11) * 4;
    d[4] = (t10 - t11) * 4;
  } else {
    d[0] = (t10 + t11 + 2) >> 2;
    d[4] = (t10 - t11 + 2) >> 2;
  }
  int z1 = (t12 + t13) * 4433;
  d[2] = (z1 + t13 * 6270 + r) >> n;
  d[6] = (z1 - t12 * 15137 + r) >> n;
  z1 = t4 + t7;
  int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int z5 = (z3 + z4) * 9633;
  z1 *= -7373;
  z2 *= -20995;
  z3 = z3 * -16069 + z5;
  z4 = z4 * -3196 + z5;
  d[7] = (t4 * 2446 + z1 + z3 + r) >> n;
  d[5] = (t5 * 16819 + z2 + z4 + r) >> n;
  d[3] = (t6 * 25172 + z2 + z3 + r) >> n;
  d[1] = (t7 * 12299 + z1 + z4 + r) >> n;
}

// where slot `local` of an image sits: component, block coordinates in that component's MCU grid
struct je_pos {
  int c, bx, by, mcu;
};

__device__ __forceinline__ je_pos slot_pos(const je_params& p, int local) {
  je_pos r;
  r.mcu = local / p.bpm;
  const int k = local - r.mcu * p.bpm, my = r.mcu / p.mcus_x, mx = r.mcu - my * p.mcus_x, ny = p.hl * p.vl;
  if (k < ny) {
    r.c = 0;
    r.by = my * p.vl + k / p.hl;
    r.bx = mx * p.hl + k % p.hl;
  } else {
    r.c = 1 + k - ny;
    r.by = my;
    r.bx = mx;
  }
  return r;
}

// ---- E1 ---------------------------------------------------------------------------------------------------------
// Thread t of a workgroup: slot t / 8 of the workgroup's 32, lane j = t % 8 owns row j of that block: it builds the
// row's 8 samples from the RGB frame (each chroma sample from its 1, 2 or 4 full-resolution pixels, coordinates
// clamped = jcsample.c / jcprepct.c edge replication), runs the row pass, then (after an LDS transpose) the column
// pass on column j, quantises, and stores zigzag positions 8 j .. 8 j + 7 as one 16-byte store.  A dummy block
// (past the component's real grid) is computed from the block jccoefct.c takes its DC from; its AC are stored as 0.
__global__ void __launch_bounds__(256) je_coef_kernel(je_params p, const uint16_t* __restrict__ quant,
                                                      int16_t* __restrict__ coefs) {
  __shared__ int ws[32 * JE_LDS_STRIDE];
  const int t = threadIdx.x, lb = t >> 3, j = t & 7;
  const int64_t slot = (int64_t)blockIdx.x * 32 + lb;
  const int img = (int)(slot / p.spi), local = (int)(slot - (int64_t)img * p.spi);
  const bool live = img < p.n && local < p.nblocks;
  int* w = ws + lb * JE_LDS_STRIDE;
  je_pos pos = {0, 0, 0, 0};
  bool dummy = false;
  if (live) {
    pos = slot_pos(p, local);
    const int c = pos.c, bw = p.bw[c], bh = p.bh[c];
    const int hc = c ? 1 : p.hl;
    dummy = pos.bx >= bw || pos.by >= bh;
    const int sy = min(pos.by, bh - 1);
    const int mx = pos.bx / hc;
    const int sx = pos.by >= bh ? min(mx * hc + hc - 1, bw - 1) : min(pos.bx, bw - 1);
    const uint8_t* base = p.src + (int64_t)img * p.h * p.w * 3;
    const int rh = c ? p.hl : 1, rv = c ? p.vl : 1;
    int cy = sy * 8 + j;
    if (c) cy = min(cy, (p.h + rv - 1) / rv - 1);              // downsampled rows past the image: the last one
    const uint8_t* row0 = base + (int64_t)min(cy * rv, p.h - 1) * p.w * 3;
    const uint8_t* row1 = base + (int64_t)min(cy * rv + rv - 1, p.h - 1) * p.w * 3;
    int d[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int cx = sx * 8 + i;
      int s;
      if (rh == 1) {
        s = ycc(row0 + min(cx, p.w - 1) * 3, c);
      } else {
        const int x0 = min(2 * cx, p.w - 1) * 3, x1 = min(2 * cx + 1, p.w - 1) * 3;
        if (rv == 1) s = (ycc(row0 + x0, c) + ycc(row0 + x1, c) + (i & 1)) >> 1;
        else s = (ycc(row0 + x0, c) + ycc(row0 + x1, c) + ycc(row1 + x0, c) + ycc(row1 + x1, c) + 1 + (i & 1)) >> 2;
      }
      d[i] = s - 128;
    }
    fdct8<true>(d);
#pragma unroll
    for (int i = 0; i < 8; ++i) w[j * 8 + i] = d[i];
  }
  __syncthreads();
  if (live) {
    int d[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) d[i] = w[i * 8 + j];
    fdct8<false>(d);
    const uint16_t* q = quant + (pos.c ? 64 : 0);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int dv = 8 * q[i * 8 + j];                         // round half away from zero of d / 8Q
      const int a = (abs(d[i]) + (dv >> 1)) / dv;
      d[i] = d[i] < 0 ? -a : a;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) w[i * 8 + j] = d[i];
  }
  __syncthreads();
  if (live) {
    uint32_t pk[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      int a = w[je_zigzag[j * 8 + 2 * k]], b = w[je_zigzag[j * 8 + 2 * k + 1]];
      if (dummy) {
        a = (j == 0 && k == 0) ? a : 0;
        b = 0;
      }
      pk[k] = (uint32_t)(uint16_t)a | (uint32_t)(uint16_t)b << 16;
    }
    *reinterpret_cast<uint4*>(coefs + slot * 64 + j * 8) = make_uint4(pk[0], pk[1], pk[2], pk[3]);
  }
}

// ---- E2 / E3: the Huffman walk of one block ---------------------------------------------------------------------

// DC of the block coded before this one in the same component (0 for the first), scan order
__device__ __forceinline__ int pred_dc(const je_params& p, const int16_t* __restrict__ img_coefs, int local,
                                       const je_pos& pos) {
  const int ny = p.hl * p.vl, k = local - pos.mcu * p.bpm;
  int prev = -1;
  if (pos.c == 0) prev = k > 0 ? local - 1 : (pos.mcu > 0 ? local - p.bpm + ny - 1 : -1);
  else prev = pos.mcu > 0 ? local - p.bpm : -1;
  return prev < 0 ? 0 : img_coefs[(int64_t)prev * 64];
}

__device__ __forceinline__ int category(int v) { return v ? 32 - __clz(abs(v)) : 0; }

// The one walk E2, E3 and the statistics pass share: calls sym(ac, symbol, value bits, size) for every code of the
// block -- ac 0: the DC table, symbol = size = the category of the difference to pred; ac 1: the AC table, symbol
// (run << 4) | size, 0xF0 (ZRL) or 0x00 (EOB) with no value bits
template <class F>
__device__ __forceinline__ void walk_block(const int16_t* __restrict__ blk, int pred, F&& sym) {
  uint64_t nz = 0;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const uint4 v = *reinterpret_cast<const uint4*>(blk + q * 8);
    const uint32_t wv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      nz |= (uint64_t)((wv[k] & 0xFFFFu) != 0) << (q * 8 + 2 * k);
      nz |= (uint64_t)((wv[k] >> 16) != 0) << (q * 8 + 2 * k + 1);
    }
  }
  const int diff = blk[0] - pred;
  int s = category(diff);
  sym(0, s, (uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << s) - 1), s);
  nz &= ~1ull;
  int last = 0;
  while (nz) {
    const int k = __ffsll((unsigned long long)nz) - 1;
    nz &= nz - 1;
    int run = k - last - 1;
    for (; run > 15; run -= 16) sym(1, 0xF0, 0u, 0);
    const int a = blk[k];
    s = category(a);
    sym(1, (run << 4) | s, (uint32_t)(a < 0 ? a - 1 : a) & ((1u << s) - 1), s);
    last = k;
  }
  if (last != 63) sym(1, 0x00, 0u, 0);
}

// where table class t (0: Y, 1: Cb / Cr) keeps symbol `symbol` in one table set (code words or histogram)
__device__ __forceinline__ int table_word(int t, int ac, int symbol) {
  return (ac ? 32 + 256 * t : 16 * t) + symbol;
}

// tables: dc codes [2][16], ac codes [2][256] ((length << 16) | code); image i reads the set at i * table_stride words
// (0: one set for every image)
__global__ void __launch_bounds__(256) je_len_kernel(je_params p, const int16_t* __restrict__ coefs,
                                                     const uint32_t* __restrict__ tables, int table_stride,
                                                     uint32_t* __restrict__ lens, uint32_t* __restrict__ chunk_tot) {
  __shared__ uint32_t lds[4];
  const int64_t slot = (int64_t)blockIdx.x * JE_SLOTS + threadIdx.x;
  const int img = (int)(slot / p.spi), local = (int)(slot - (int64_t)img * p.spi);
  uint32_t bits = 0;
  if (img < p.n && local < p.nblocks) {
    const je_pos pos = slot_pos(p, local);
    const int16_t* ic = coefs + (int64_t)img * p.spi * 64;
    const int t = pos.c ? 1 : 0;
    const uint32_t* tab = tables + (int64_t)img * table_stride;
    walk_block(ic + (int64_t)local * 64, pred_dc(p, ic, local, pos),
               [&](int ac, int symbol, uint32_t, int size) { bits += (tab[table_word(t, ac, symbol)] >> 16) + size; });
  }
  lens[slot] = bits;
  uint32_t tot;
  (void)wg_exclusive_scan(bits, lds, &tot);
  if (threadIdx.x == 0) chunk_tot[blockIdx.x] = tot;
}

// One workgroup per segment i: out[k] = sum of vals[seg[i] .. k), total[i] = the segment's sum
__global__ void __launch_bounds__(256) je_scan_kernel(const uint32_t* __restrict__ vals, const int64_t* __restrict__ seg,
                                                      uint64_t* __restrict__ out, uint64_t* __restrict__ total) {
  __shared__ uint32_t lds[4];
  const int64_t b = seg[blockIdx.x], e = seg[blockIdx.x + 1];
  uint64_t carry = 0;
  for (int64_t base = b; base < e; base += 256) {
    const int64_t k = base + threadIdx.x;
    const uint32_t v = k < e ? vals[k] : 0;
    uint32_t tot;
    const uint32_t ex = wg_exclusive_scan(v, lds, &tot);
    if (k < e) out[k] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) total[blockIdx.x] = carry;
}

// Writes stream words [w0, ...) of one block: `first` is the word it shares with the block before it
struct je_writer {
  uint32_t* words;
  int64_t w, first;
  uint64_t acc;
  int nacc;
  __device__ __forceinline__ void flush_word(uint32_t v) {
    v = __builtin_bswap32(v);
    if (w == first) atomicOr(words + w, v);
    else words[w] = v;
    ++w;
  }
  __device__ __forceinline__ void put(uint32_t code, int len) {
    acc = acc << len | code;
    nacc += len;
    if (nacc >= 32) {
      nacc -= 32;
      flush_word((uint32_t)(acc >> nacc));
      acc &= (1ull << nacc) - 1;
    }
  }
  __device__ __forceinline__ void finish() {
    if (nacc) atomicOr(words + w, __builtin_bswap32((uint32_t)(acc << (32 - nacc))));
  }
};

__global__ void __launch_bounds__(256) je_emit_kernel(je_params p, const int16_t* __restrict__ coefs,
                                                      const uint32_t* __restrict__ tables, int table_stride,
                                                      const uint32_t* __restrict__ lens,
                                                      const uint64_t* __restrict__ chunk_off,
                                                      const uint64_t* __restrict__ word0, uint32_t* __restrict__ words) {
  __shared__ uint32_t lds[4];
  const int64_t slot = (int64_t)blockIdx.x * JE_SLOTS + threadIdx.x;
  const int img = (int)(slot / p.spi), local = (int)(slot - (int64_t)img * p.spi);
  const uint32_t len = lens[slot];
  uint32_t tot;
  const uint32_t ex = wg_exclusive_scan(len, lds, &tot);
  if (img >= p.n || local >= p.nblocks) return;
  const uint64_t bit = chunk_off[blockIdx.x] + ex;
  je_writer wr;
  wr.words = words + word0[img];
  wr.w = wr.first = (int64_t)(bit >> 5);
  wr.acc = 0;
  wr.nacc = (int)(bit & 31);
  const je_pos pos = slot_pos(p, local);
  const int16_t* ic = coefs + (int64_t)img * p.spi * 64;
  const int t = pos.c ? 1 : 0;
  const uint32_t* tab = tables + (int64_t)img * table_stride;
  walk_block(ic + (int64_t)local * 64, pred_dc(p, ic, local, pos), [&](int ac, int symbol, uint32_t value, int size) {
    const uint32_t e = tab[table_word(t, ac, symbol)];
    wr.put(((e & 0xFFFF) << size) | value, (int)(e >> 16) + size);
  });
  wr.finish();
}

// ---- ES: symbol statistics (optimize) ---------------------------------------------------------------------------
// One thread per slot, E2's geometry: an image owns whole 256-slot chunks, so a workgroup counts for ONE image.  It
// counts into its own histogram in LDS (LDS atomics) and then adds the bins it touched to the image's histogram
// (hist: [n][JE_TABLE_WORDS], zeroed before the launch, laid out like a table set).  Integer sums: the result does not
// depend on the order of arrival.
__global__ void __launch_bounds__(256) je_stat_kernel(je_params p, const int16_t* __restrict__ coefs,
                                                      uint32_t* __restrict__ hist) {
  __shared__ uint32_t h[JE_TABLE_WORDS];
  for (int k = threadIdx.x; k < JE_TABLE_WORDS; k += 256) h[k] = 0;
  __syncthreads();
  const int64_t slot = (int64_t)blockIdx.x * JE_SLOTS + threadIdx.x;
  const int img = (int)(slot / p.spi), local = (int)(slot - (int64_t)img * p.spi);
  if (img < p.n && local < p.nblocks) {
    const je_pos pos = slot_pos(p, local);
    const int16_t* ic = coefs + (int64_t)img * p.spi * 64;
    const int t = pos.c ? 1 : 0;
    walk_block(ic + (int64_t)local * 64, pred_dc(p, ic, local, pos),
               [&](int ac, int symbol, uint32_t, int) { atomicAdd(&h[table_word(t, ac, symbol)], 1u); });
  }
  __syncthreads();
  const int wimg = (int)((int64_t)blockIdx.x * JE_SLOTS / p.spi);   // the workgroup's image (p.spi is a multiple of 256)
  if (wimg >= p.n) return;
  for (int k = threadIdx.x; k < JE_TABLE_WORDS; k += 256) {
    const uint32_t v = h[k];
    if (v) atomicAdd(hist + (int64_t)wimg * JE_TABLE_WORDS + k, v);
  }
}

// ---- E4 ---------------------------------------------------------------------------------------------------------
struct je_stream {
  const uint32_t* words;                 // image's first word
  int64_t bytes;                         // entropy-coded bytes before stuffing
  int pad;                               // 1 bits the final byte is padded with (0..7)
};

__device__ __forceinline__ int find_image(const int64_t* __restrict__ seg, int n, int64_t chunk) {
  int lo = 0, hi = n - 1;                                      // last image with seg[i] <= chunk
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (seg[mid] <= chunk) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// this thread's 16 stream bytes (chunk-relative offset `at`), padded, zero past the end; returns how many are real
__device__ __forceinline__ int load16(const uint32_t* __restrict__ words, const uint64_t* __restrict__ bits, int img,
                                      int64_t at, uint8_t b[16]) {
  const uint64_t nb = bits[img];
  const int64_t bytes = (int64_t)((nb + 7) >> 3);
  const int real = (int)max((int64_t)0, min((int64_t)16, bytes - at));
  uint4 v = make_uint4(0, 0, 0, 0);
  if (real > 0) v = *reinterpret_cast<const uint4*>(words + at / 4);
  const uint32_t wv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int k = 0; k < 16; ++k) b[k] = k < real ? (uint8_t)(wv[k >> 2] >> (8 * (k & 3))) : 0;
  const int pad = (int)((8 - (nb & 7)) & 7);
  const int64_t lastk = bytes - 1 - at;                        // the final byte, if it is one of these 16
#pragma unroll
  for (int k = 0; k < 16; ++k)
    if (k == lastk) b[k] |= (uint8_t)((1u << pad) - 1);
  return real;
}

__global__ void __launch_bounds__(256) je_ffcount_kernel(const uint32_t* __restrict__ words,
                                                         const uint64_t* __restrict__ word0,
                                                         const uint64_t* __restrict__ bits,
                                                         const int64_t* __restrict__ seg, int n,
                                                         uint32_t* __restrict__ ff_cnt) {
  __shared__ uint32_t lds[4];
  const int64_t chunk = blockIdx.x;
  const int img = find_image(seg, n, chunk);
  const int64_t at = (chunk - seg[img]) * JE_FF_CHUNK + threadIdx.x * 16;
  uint8_t b[16];
  const int real = load16(words + word0[img], bits, img, at, b);
  uint32_t cnt = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k) cnt += (k < real && b[k] == 0xFF) ? 1 : 0;
  uint32_t tot;
  (void)wg_exclusive_scan(cnt, lds, &tot);                     // per-wave sums first, one write per workgroup
  if (threadIdx.x == 0) ff_cnt[chunk] = tot;
}

__global__ void __launch_bounds__(256) je_pack_kernel(const uint32_t* __restrict__ words,
                                                      const uint64_t* __restrict__ word0,
                                                      const uint64_t* __restrict__ bits,
                                                      const int64_t* __restrict__ seg, int n,
                                                      const uint64_t* __restrict__ ff_off,
                                                      const uint64_t* __restrict__ ff_tot,
                                                      const uint64_t* __restrict__ file_off,
                                                      const uint8_t* __restrict__ headers,
                                                      const uint2* __restrict__ header_tab,
                                                      uint8_t* __restrict__ out) {
  __shared__ uint32_t lds[4];
  const int64_t chunk = blockIdx.x;
  const int img = find_image(seg, n, chunk);
  const int64_t rel = chunk - seg[img];
  const int64_t at = rel * JE_FF_CHUNK + threadIdx.x * 16;
  const uint2 hd = header_tab[img];                            // the image's header: byte offset in `headers`, length
  const uint8_t* header = headers + hd.x;
  const int header_len = (int)hd.y;
  uint8_t b[16];
  const int real = load16(words + word0[img], bits, img, at, b);
  uint32_t cnt = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k) cnt += (k < real && b[k] == 0xFF) ? 1 : 0;
  uint32_t tot;
  const uint32_t ex = wg_exclusive_scan(cnt, lds, &tot);
  uint8_t* file = out + file_off[img];
  uint8_t* dst = file + header_len + at + ff_off[chunk] + ex;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    if (k < real) {
      *dst++ = b[k];
      if (b[k] == 0xFF) *dst++ = 0;
    }
  }
  if (rel == 0)
    for (int k = threadIdx.x; k < header_len; k += 256) file[k] = header[k];
  if (chunk + 1 == seg[img + 1] && threadIdx.x == 0) {
    uint8_t* end = file + header_len + (int64_t)((bits[img] + 7) >> 3) + ff_tot[img];
    end[0] = 0xFF;
    end[1] = 0xD9;
  }
}

}  // namespace

extern "C" int ta_jpeg_encode_header(int h, int w, int quality, int subsampling, uint8_t* out, size_t capacity,
                                     size_t* size) {
  if (h < 1 || w < 1 || h > 65535 || w > 65535 || quality < 1 || quality > 100 || subsampling < 0 || subsampling > 2 ||
      !size)
    return TA_E_INVALID;
  const std::vector<uint8_t> hd = make_header(h, w, quality, subsampling);
  *size = hd.size();
  if (!out || capacity < hd.size()) return TA_E_CAPACITY;
  memcpy(out, hd.data(), hd.size());
  return TA_OK;
}

extern "C" int ta_jpeg_optimal_table(const int64_t* freq, uint8_t* bits, uint8_t* vals, int* nvals) {
  if (!freq || !bits || !vals || !nvals) return TA_E_INVALID;
  bool any = false;
  for (int i = 0; i < 256; ++i) {
    if (freq[i] < 0 || freq[i] >= JE_MAX_COUNT) return TA_E_INVALID;
    any |= freq[i] != 0;
  }
  je_huff t;
  if (!any || !optimal_table(freq, &t)) return TA_E_INVALID;
  memcpy(bits, t.bits, 17);
  memcpy(vals, t.vals, (size_t)t.nvals);
  *nvals = t.nvals;
  return TA_OK;
}

static int jpeg_encode(ta_ctx* ctx, const ta_frames* frames, int quality, int subsampling, bool optimize,
                       const uint8_t** out, size_t* sizes) {
  if (!ctx) return TA_E_INVALID;
  ta_enter(ctx);
  if (!frames || !out || !sizes) return ta_fail(ctx, TA_E_INVALID, "jpeg_encode: bad arguments");
  if (quality < 1 || quality > 100) return ta_fail(ctx, TA_E_INVALID, "jpeg_encode: quality %d not in 1..100", quality);
  if (subsampling < 0 || subsampling > 2)
    return ta_fail(ctx, TA_E_INVALID, "jpeg_encode: subsampling %d not 0 (4:4:4), 1 (4:2:2) or 2 (4:2:0)", subsampling);
  const int n = frames->n, h = frames->h, w = frames->w;
  if (n < 1 || h < 1 || w < 1 || h > 65535 || w > 65535)
    return ta_fail(ctx, TA_E_INVALID, "jpeg_encode: frames of %d x %d x %d cannot be encoded (1..65535 each side)", n, h,
                   w);
  const auto t_host = std::chrono::steady_clock::now();
  je_params p = {};
  p.src = frames->dev;
  p.n = n;
  p.h = h;
  p.w = w;
  p.hl = subsampling == 0 ? 1 : 2;
  p.vl = subsampling == 2 ? 2 : 1;
  p.bpm = p.hl * p.vl + 2;
  p.mcus_x = (w + 8 * p.hl - 1) / (8 * p.hl);
  p.mcus_y = (h + 8 * p.vl - 1) / (8 * p.vl);
  for (int c = 0; c < 3; ++c) {
    const int hc = c ? 1 : p.hl, vc = c ? 1 : p.vl;
    p.bw[c] = (int)(((int64_t)w * hc + 8 * p.hl - 1) / (8 * p.hl));
    p.bh[c] = (int)(((int64_t)h * vc + 8 * p.vl - 1) / (8 * p.vl));
  }
  const int64_t nblocks = (int64_t)p.mcus_x * p.mcus_y * p.bpm;
  if (nblocks > (1ll << 30)) return ta_fail(ctx, TA_E_INVALID, "jpeg_encode: image too large");
  if (optimize && nblocks * 64 >= JE_MAX_COUNT)
    return ta_fail(ctx, TA_E_INVALID, "jpeg_encode: %lld blocks an image are too many for optimize (symbol counts must "
                   "stay below 10^9)", (long long)nblocks);
  p.nblocks = (int)nblocks;
  p.spi = (int)align_up(nblocks, JE_SLOTS);
  const int64_t slots = (int64_t)n * p.spi, chunks = slots / JE_SLOTS;
  const std::vector<uint8_t> header = make_header(h, w, quality, subsampling);
  const int header_len = (int)header.size();

  // phase 1 staging: [quant 2x64 u16][dc codes 2x16 u32, ac codes 2x256 u32][header][header table n x (offset, length)
  // u32][block segments n+1 i64]
  const int64_t off_tables = 256, off_header = off_tables + JE_TABLE_WORDS * 4;
  const int64_t off_htab = align_up(off_header + header_len, 8);
  const int64_t off_seg = align_up(off_htab + (int64_t)n * 8, 256);
  const int64_t staged = align_up(off_seg + (int64_t)(n + 1) * 8, 256);
  // pinned after the staging: image bit totals, then phase 2 [word0 n][ff segments n+1], ff totals, file offsets
  const int64_t pin_bits = staged, pin_w0 = pin_bits + align_up(8 * n, 256);
  const int64_t pin_ffseg = pin_w0 + align_up(8 * n, 256), pin_fftot = pin_ffseg + align_up(8 * (n + 1), 256);
  const int64_t pin_foff = pin_fftot + align_up(8 * n, 256), pin_end = pin_foff + align_up(8 * n, 256);
  // optimize: the histograms come here; the per-image [code words][headers][header table] go back in one copy
  const int64_t set_bytes = (int64_t)JE_TABLE_WORDS * 4;
  const int64_t pin_hist = pin_end, pin_otab = pin_hist + align_up(n * set_bytes, 256);
  const int64_t pin_ohdr = pin_otab + align_up(n * set_bytes, 256);
  const int64_t pin_ohtab = pin_ohdr + (int64_t)n * JE_HEADER_STRIDE;
  const int64_t pin_all = optimize ? pin_ohtab + align_up(8 * n, 256) : pin_end;
  void* pin = nullptr;
  TA_TRY(ta_pinned(ctx, (size_t)pin_all, &pin));
  uint8_t* host = (uint8_t*)pin;
  quant_table(quality, 0, (uint16_t*)host);
  quant_table(quality, 1, (uint16_t*)host + 64);
  uint32_t* tab = (uint32_t*)(host + off_tables);
  huff_codes(kDcLumaBits, kDcVals, tab, 16);
  huff_codes(kDcChromaBits, kDcVals, tab + 16, 16);
  huff_codes(kAcLumaBits, kAcLumaVals, tab + 32, 256);
  huff_codes(kAcChromaBits, kAcChromaVals, tab + 32 + 256, 256);
  memcpy(host + off_header, header.data(), header.size());
  uint32_t* htab = (uint32_t*)(host + off_htab);               // every image: the one shared header
  for (int i = 0; i < n; ++i) {
    htab[2 * i] = 0;
    htab[2 * i + 1] = (uint32_t)header_len;
  }
  int64_t* seg = (int64_t*)(host + off_seg);
  for (int i = 0; i <= n; ++i) seg[i] = (int64_t)i * (p.spi / JE_SLOTS);

  // device scratch: [staging][coefficients slots x 128][lens slots x 4][chunk totals][chunk offsets][image bits]
  const int64_t d_coef = staged, d_lens = d_coef + slots * 128, d_ctot = align_up(d_lens + slots * 4, 256);
  const int64_t d_coff = align_up(d_ctot + chunks * 4, 256), d_bits = align_up(d_coff + chunks * 8, 256);
  const int64_t d_p2 = d_bits + align_up(8 * n, 256);   // phase 2 copies of pin_w0 .. pin_end
  const int64_t d_hist = d_p2 + (pin_end - pin_w0);     // optimize: histograms, then the copies of pin_otab .. pin_all
  const int64_t d_opt = d_hist + (pin_otab - pin_hist);
  const int64_t d_end = optimize ? d_opt + (pin_all - pin_otab) : d_hist;
  void* scr = nullptr;
  TA_TRY(ta_scratch(ctx, (size_t)d_end, &scr));
  uint8_t* dev = (uint8_t*)scr;
  const uint16_t* d_quant = (const uint16_t*)dev;
  const uint32_t* d_tables = (const uint32_t*)(optimize ? dev + d_opt : dev + off_tables);
  const int table_stride = optimize ? JE_TABLE_WORDS : 0;
  const uint8_t* d_headers = optimize ? dev + d_opt + (pin_ohdr - pin_otab) : dev + off_header;
  const uint2* d_htab = (const uint2*)(optimize ? dev + d_opt + (pin_ohtab - pin_otab) : dev + off_htab);
  if (optimize) htab = (uint32_t*)(host + pin_ohtab);
  const int header_cap = optimize ? JE_HEADER_STRIDE : header_len;
  uint64_t* d_bits_p = (uint64_t*)(dev + d_bits);
  auto p2 = [&](int64_t pin_off) { return dev + d_p2 + (pin_off - pin_w0); };

  // HIP events around each pass while profiling: [0] H2D staging, [1] E1, [2] E2 + scan, [3] E3, [4] E4a + scan,
  // [5] E4b, [6] D2H of the files; [7] the statistics pass (optimize)
  hipEvent_t ev[16] = {};
  double opt_ms[2] = {0, 0};
  const bool timed = ctx->profiling;
  if (timed)
    for (auto& e : ev)
      if (hipEventCreate(&e) != hipSuccess) e = nullptr;
  auto mark = [&](int k) {
    if (timed && ev[k]) (void)hipEventRecord(ev[k], ctx->stream);
  };
  auto done = [&](hipError_t e) {
    double ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (timed) {
      for (int k = 0; k < (optimize ? 8 : 7); ++k) {
        float f = 0;
        if (e == hipSuccess && ev[2 * k] && ev[2 * k + 1] && hipEventElapsedTime(&f, ev[2 * k], ev[2 * k + 1]) == hipSuccess)
          (k < 7 ? ms[k] : opt_ms[0]) = f;
      }
      for (auto& x : ev)
        if (x) (void)hipEventDestroy(x);
    }
    ms[7] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_host).count();
    memcpy(ctx->jpeg_enc_ms, ms, sizeof(ms));
    memcpy(ctx->jpeg_enc_opt_ms, opt_ms, sizeof(opt_ms));
    return e;
  };

  // E1, E2, block scan; the bit totals to the host
  mark(0);
  hipError_t e = hipMemcpyAsync(dev, host, (size_t)staged, hipMemcpyHostToDevice, ctx->stream);
  mark(1);
  mark(2);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(je_coef_kernel, dim3((unsigned)(slots / 32)), dim3(256), 0, ctx->stream, p, d_quant,
                       (int16_t*)(dev + d_coef));
    e = hipGetLastError();
  }
  mark(3);
  if (optimize) {
    // ES: the histograms to the host, which builds every image's tables and header and sends them back
    uint32_t* d_hist_p = (uint32_t*)(dev + d_hist);
    mark(14);
    if (e == hipSuccess) e = hipMemsetAsync(d_hist_p, 0, (size_t)(n * set_bytes), ctx->stream);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(je_stat_kernel, dim3((unsigned)chunks), dim3(256), 0, ctx->stream, p,
                         (const int16_t*)(dev + d_coef), d_hist_p);
      e = hipGetLastError();
    }
    mark(15);
    if (e == hipSuccess)
      e = hipMemcpyAsync(host + pin_hist, d_hist_p, (size_t)(n * set_bytes), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return ta_fail(ctx, TA_E_DEVICE, "jpeg_encode: %s", hipGetErrorString(done(e)));
    const auto t_tab = std::chrono::steady_clock::now();
    for (int i = 0; i < n; ++i) {
      const uint32_t* hist = (const uint32_t*)(host + pin_hist) + (int64_t)i * JE_TABLE_WORDS;
      uint32_t* codes = (uint32_t*)(host + pin_otab) + (int64_t)i * JE_TABLE_WORDS;
      je_huff huff[4];                                         // DC 0, AC 0, DC 1, AC 1: the order of the DHT segments
      for (int k = 0; k < 4; ++k) {
        const int t = k >> 1, ac = k & 1, nsym = ac ? 256 : 16, at = ac ? 32 + 256 * t : 16 * t;
        int64_t freq[257] = {};
        for (int s = 0; s < nsym; ++s) freq[s] = hist[at + s];
        if (!optimal_table(freq, &huff[k])) {
          (void)done(hipSuccess);
          return ta_fail(ctx, TA_E_INVALID, "jpeg_encode: image %d needs a Huffman code longer than 32 bits", i);
        }
        huff_codes(huff[k].bits + 1, huff[k].vals, codes + at, nsym);
      }
      const std::vector<uint8_t> hd = make_header(h, w, quality, subsampling, huff);
      if (hd.size() > JE_HEADER_STRIDE) {
        (void)done(hipSuccess);
        return ta_fail(ctx, TA_E_INVALID, "jpeg_encode: header of %zu bytes", hd.size());
      }
      memcpy(host + pin_ohdr + (int64_t)i * JE_HEADER_STRIDE, hd.data(), hd.size());
      htab[2 * i] = (uint32_t)(i * JE_HEADER_STRIDE);
      htab[2 * i + 1] = (uint32_t)hd.size();
    }
    opt_ms[1] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_tab).count();
    e = hipMemcpyAsync(dev + d_opt, host + pin_otab, (size_t)(pin_all - pin_otab), hipMemcpyHostToDevice, ctx->stream);
  }
  mark(4);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(je_len_kernel, dim3((unsigned)chunks), dim3(256), 0, ctx->stream, p,
                       (const int16_t*)(dev + d_coef), d_tables, table_stride, (uint32_t*)(dev + d_lens),
                       (uint32_t*)(dev + d_ctot));
    e = hipGetLastError();
  }
  if (e == hipSuccess) {
    hipLaunchKernelGGL(je_scan_kernel, dim3((unsigned)n), dim3(256), 0, ctx->stream, (const uint32_t*)(dev + d_ctot),
                       (const int64_t*)(dev + off_seg), (uint64_t*)(dev + d_coff), d_bits_p);
    e = hipGetLastError();
  }
  mark(5);
  if (e == hipSuccess) e = hipMemcpyAsync(host + pin_bits, d_bits_p, 8 * n, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) return ta_fail(ctx, TA_E_DEVICE, "jpeg_encode: %s", hipGetErrorString(done(e)));

  // exact stream sizes -> word buffer and 4 KB stuffing chunks; every image's words start 16-byte aligned
  const uint64_t* bits = (const uint64_t*)(host + pin_bits);
  uint64_t* w0 = (uint64_t*)(host + pin_w0);
  int64_t* ffseg = (int64_t*)(host + pin_ffseg);
  int64_t words = 0, ffchunks = 0, entropy_bytes = 0;
  for (int i = 0; i < n; ++i) {
    const int64_t bytes = (int64_t)((bits[i] + 7) >> 3);
    entropy_bytes += bytes;
    w0[i] = (uint64_t)words;
    words += align_up(bytes, JE_FF_CHUNK) / 4;                  // E4 reads whole 16-byte groups of whole chunks
    ffseg[i] = ffchunks;
    ffchunks += (bytes + JE_FF_CHUNK - 1) / JE_FF_CHUNK;
  }
  ffseg[n] = ffchunks;
  // second device block: [words][ff counts][ff offsets][ff totals][packed files, worst case: every byte stuffed]
  const int64_t e_ffc = words * 4, e_ffo = align_up(e_ffc + ffchunks * 4, 256);
  const int64_t e_fft = align_up(e_ffo + ffchunks * 8, 256), e_out = e_fft + align_up(8 * n, 256);
  const int64_t e_end = e_out + 2 * entropy_bytes + (int64_t)n * (header_cap + 2);
  if ((size_t)e_end > ctx->jpeg_enc_dev_bytes) {
    if (ctx->jpeg_enc_dev) (void)hipFree(ctx->jpeg_enc_dev);  // the stream is idle: synchronised above
    ctx->jpeg_enc_dev = nullptr;
    ctx->jpeg_enc_dev_bytes = 0;
    const size_t want = (size_t)e_end + (size_t)e_end / 4 + (1 << 20);
    e = hipMalloc(&ctx->jpeg_enc_dev, want);
    if (e != hipSuccess) return ta_fail(ctx, TA_E_DEVICE, "jpeg_encode: %s", hipGetErrorString(done(e)));
    ctx->jpeg_enc_dev_bytes = want;
  }
  uint8_t* eb = (uint8_t*)ctx->jpeg_enc_dev;
  uint32_t* d_words = (uint32_t*)eb;
  const uint64_t* d_w0 = (const uint64_t*)p2(pin_w0);
  const int64_t* d_ffseg = (const int64_t*)p2(pin_ffseg);

  // E3, E4a, stuffing scan; the stuffing totals to the host
  e = hipMemcpyAsync(p2(pin_w0), host + pin_w0, (size_t)(pin_fftot - pin_w0), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemsetAsync(d_words, 0, (size_t)words * 4, ctx->stream);
  mark(6);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(je_emit_kernel, dim3((unsigned)chunks), dim3(256), 0, ctx->stream, p,
                       (const int16_t*)(dev + d_coef), d_tables, table_stride, (const uint32_t*)(dev + d_lens),
                       (const uint64_t*)(dev + d_coff), d_w0, d_words);
    e = hipGetLastError();
  }
  mark(7);
  mark(8);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(je_ffcount_kernel, dim3((unsigned)ffchunks), dim3(256), 0, ctx->stream, d_words, d_w0, d_bits_p,
                       d_ffseg, n, (uint32_t*)(eb + e_ffc));
    e = hipGetLastError();
  }
  if (e == hipSuccess) {
    hipLaunchKernelGGL(je_scan_kernel, dim3((unsigned)n), dim3(256), 0, ctx->stream, (const uint32_t*)(eb + e_ffc),
                       d_ffseg, (uint64_t*)(eb + e_ffo), (uint64_t*)(eb + e_fft));
    e = hipGetLastError();
  }
  mark(9);
  if (e == hipSuccess) e = hipMemcpyAsync(host + pin_fftot, eb + e_fft, 8 * n, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) return ta_fail(ctx, TA_E_DEVICE, "jpeg_encode: %s", hipGetErrorString(done(e)));

  // file sizes and offsets; E4b packs, one copy brings the files home
  const uint64_t* fftot = (const uint64_t*)(host + pin_fftot);
  uint64_t* foff = (uint64_t*)(host + pin_foff);
  int64_t total = 0;
  for (int i = 0; i < n; ++i) {
    sizes[i] = (size_t)((int64_t)htab[2 * i + 1] + (int64_t)((bits[i] + 7) >> 3) + (int64_t)fftot[i] + 2);
    foff[i] = (uint64_t)total;
    total += (int64_t)sizes[i];
  }
  if ((size_t)total > ctx->jpeg_enc_out_bytes) {
    if (ctx->jpeg_enc_out) (void)hipHostFree(ctx->jpeg_enc_out);
    ctx->jpeg_enc_out = nullptr;
    ctx->jpeg_enc_out_bytes = 0;
    const size_t want = (size_t)total + (size_t)total / 4 + (1 << 16);
    e = hipHostMalloc((void**)&ctx->jpeg_enc_out, want, hipHostMallocDefault);
    if (e != hipSuccess) return ta_fail(ctx, TA_E_DEVICE, "jpeg_encode: %s", hipGetErrorString(done(e)));
    ctx->jpeg_enc_out_bytes = want;
  }
  e = hipMemcpyAsync(p2(pin_foff), host + pin_foff, 8 * n, hipMemcpyHostToDevice, ctx->stream);
  mark(10);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(je_pack_kernel, dim3((unsigned)ffchunks), dim3(256), 0, ctx->stream, d_words, d_w0, d_bits_p,
                       d_ffseg, n, (const uint64_t*)(eb + e_ffo), (const uint64_t*)(eb + e_fft),
                       (const uint64_t*)p2(pin_foff), d_headers, d_htab, eb + e_out);
    e = hipGetLastError();
  }
  mark(11);
  mark(12);
  if (e == hipSuccess)
    e = hipMemcpyAsync(ctx->jpeg_enc_out, eb + e_out, (size_t)total, hipMemcpyDeviceToHost, ctx->stream);
  mark(13);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) return ta_fail(ctx, TA_E_DEVICE, "jpeg_encode: %s", hipGetErrorString(done(e)));
  (void)done(e);
  ctx->jpeg_enc_counts[0] = n;
  ctx->jpeg_enc_counts[1] = (int64_t)n * nblocks;
  ctx->jpeg_enc_counts[2] = total;
  ctx->jpeg_enc_counts[3] = entropy_bytes;
  *out = ctx->jpeg_enc_out;
  return TA_OK;
}

extern "C" int ta_jpeg_encode(ta_ctx* ctx, const ta_frames* frames, int quality, int subsampling, const uint8_t** out,
                              size_t* sizes) {
  return jpeg_encode(ctx, frames, quality, subsampling, false, out, sizes);
}

extern "C" int ta_jpeg_encode_opt(ta_ctx* ctx, const ta_frames* frames, int quality, int subsampling, int optimize,
                                  const uint8_t** out, size_t* sizes) {
  if (ctx && optimize != 0 && optimize != 1) {
    ta_enter(ctx);
    return ta_fail(ctx, TA_E_INVALID, "jpeg_encode: optimize %d not 0 or 1", optimize);
  }
  return jpeg_encode(ctx, frames, quality, subsampling, optimize == 1, out, sizes);
}

extern "C" int ta_jpeg_encode_last_opt_stats(const ta_ctx* ctx, double* ms) {
  if (!ctx || !ms) return TA_E_INVALID;
  memcpy(ms, ctx->jpeg_enc_opt_ms, sizeof(ctx->jpeg_enc_opt_ms));
  return TA_OK;
}

extern "C" int ta_jpeg_encode_last_stats(const ta_ctx* ctx, double* ms, int64_t* counts) {
  if (!ctx) return TA_E_INVALID;
  if (ms) memcpy(ms, ctx->jpeg_enc_ms, sizeof(ctx->jpeg_enc_ms));
  if (counts) memcpy(counts, ctx->jpeg_enc_counts, sizeof(ctx->jpeg_enc_counts));
  return TA_OK;
}
