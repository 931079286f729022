// The quantiser of the JPEG encoder (include/rtm3d_hip.h, "JPEG encoding", step 5), shared by the device stage (jpeg_enc.hip)
// and by a stand-alone host program (tests/jpeg_quant_main.cpp) that proves it exhaustively.  Integer code only.
//
// The rule is a = (|c| + 4 q) / (8 q), truncating.  The division is one multiplication: with d = 8 q <= 2040 < 2^11 and
// x = |c| + 4 q <= 32767 + 1020 < 2^16, m = floor(2^32 / d) + 1 gives floor(x / d) = (x * m) >> 32 for every such x
// (Granlund & Montgomery: m d = 2^32 + e with 0 < e <= d, so x m / 2^32 = x / d + x e / (d 2^32), and the second term is
// below 2^16 / 2^32 < 1 / d, too small to reach the next integer).  The host computes m once per table entry and passes it
// by value; the test walks all 255 * 32768 cases.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define JPG_QUANT_FN __host__ __device__ __forceinline__
#else
#define JPG_QUANT_FN inline
#endif

// the multiplier of a table entry q (1..255)
JPG_QUANT_FN uint32_t jpeg_quant_multiplier(uint32_t q) { return (uint32_t)(0x100000000ull / (8u * q)) + 1u; }

// the quantised coefficient; c is the forward DCT's output (|c| <= 32767), m = jpeg_quant_multiplier(q)
JPG_QUANT_FN int32_t jpeg_quantise(int32_t c, uint32_t q, uint32_t m) {
    const uint32_t x = (uint32_t)(c < 0 ? -c : c) + 4u * q;
    const int32_t a = (int32_t)(uint32_t)(((uint64_t)x * m) >> 32);
    return c < 0 ? -a : a;
}
