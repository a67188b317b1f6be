// Baseline JPEG: the host half (marker parser + Huffman decoder, jpeg_host.hip) and what the device half (jpeg.hip)
// needs from it.  Plain C++: no HIP call is made by anything declared here.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>

#include "../../include/terran_amd.h"

// One parsed image.  `hdr` is what ta_jpeg_coefficients hands out; the rest is the decoder's private state.
struct ta_jpeg_huff {
  bool present = false;
  uint16_t look[512];         // 9-bit lookahead: (length << 8) | symbol, 0 = longer code (slow path)
  int32_t maxcode[18];        // largest code of each length (-1: none); maxcode[17] sentinel
  int32_t valoff[17];         // symbol index of a length's first code minus that code
  uint8_t vals[256];
};

struct ta_jpeg_parsed {
  ta_jpeg_header hdr;
  int hmax = 1, vmax = 1;
  int mcus_x = 0, mcus_y = 0;
  int scan_order[3] = {0, 1, 2};   // component index of the scan's k-th component (MCU interleave order)
  int dc_sel[3] = {0, 0, 0}, ac_sel[3] = {0, 0, 0};
  ta_jpeg_huff dc[4], ac[4];
  const uint8_t* scan = nullptr;   // first byte of entropy-coded data
  const uint8_t* end = nullptr;    // end of the buffer
};

// Parses markers up to the start of the scan.  TA_OK with hdr.path == TA_JPEG_DEVICE (decodable here) or a
// TA_JPEG_FALLBACK_* reason (the header facts that could be read are filled in), or TA_E_INVALID with `err` set.
int ta_jpeg_parse(const uint8_t* data, size_t size, ta_jpeg_parsed* p, std::string* err);
// Entropy-decodes a parsed TA_JPEG_DEVICE image into hdr.blocks_total blocks of 64 int16 (natural order, quantised),
// component after component, each component's block grid in raster order.  TA_OK or TA_E_INVALID with `err` set.
int ta_jpeg_entropy_decode(const ta_jpeg_parsed* p, int16_t* coefs, std::string* err);
