// The store of a run of packed RGB pixels, shared by the kernels that write tightly packed uint8 (h, w, 3) frames
// (frames_convert.hip: frames_convert_kernel, runs of 8 pixels; lens.hip: frames_remap_kernel, runs of 4; augment.hip: out_mode 2,
// runs of 4).  Integer code only:
// it compiles the same with and without -ffp-contract=off.
//
// Any byte address is legal.  The 3 * PX output bytes of a full run leave as aligned dwords - 8 bytes at a time where the run
// holds an even number of dwords and the address allows it; shifted by the destination's misalignment, with a byte-wise head
// and tail, where the address is no multiple of 4 - and a partial run (the row's last) byte by byte: a run writes exactly
// 3 * n bytes, so a frame exactly h * w * 3.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// ---- the run's 3 * PX output bytes (n pixels of them valid) to q; pix[i] = c0 | c1 << 8 | c2 << 16, bits 24-31 zero
template <int PX>
__device__ __forceinline__ void store_rgb_run(uint8_t* q, const uint32_t (&pix)[PX], int n) {
    static_assert(PX % 4 == 0, "four pixels fill three dwords");
    constexpr int ND = 3 * PX / 4;                                // dwords of a full run
    uint32_t v[ND];
#pragma unroll
    for (int g = 0; g < PX / 4; ++g) {
        const uint32_t* px = pix + 4 * g;
        v[3 * g] = px[0] | (px[1] << 24); v[3 * g + 1] = (px[1] >> 8) | (px[2] << 16); v[3 * g + 2] = (px[2] >> 16) | (px[3] << 8);
    }
    const int a = (int)((uintptr_t)q & 3);
    if (n == PX && a == 0) {
        if (ND % 2 == 0 && ((uintptr_t)q & 7) == 0) {
#pragma unroll
            for (int i = 0; i < ND / 2; ++i) ((uint2*)q)[i] = make_uint2(v[2 * i], v[2 * i + 1]);
        } else {
#pragma unroll
            for (int i = 0; i < ND; ++i) ((uint32_t*)q)[i] = v[i];
        }
    } else if (n == PX) {
        const int hb = 4 - a, lo = 8 * hb, hi = 8 * a;            // hb = 1..3 head bytes reach the next dword boundary
#pragma unroll
        for (int i = 0; i < 3; ++i)
            if (i < hb) q[i] = (uint8_t)(v[0] >> (8 * i));
        uint32_t* d = (uint32_t*)(q + hb);
#pragma unroll
        for (int i = 0; i < ND - 1; ++i) d[i] = (v[i] >> lo) | (v[i + 1] << hi);
        const uint32_t t = v[ND - 1] >> lo;
#pragma unroll
        for (int i = 0; i < 3; ++i)
            if (i < a) q[hb + 4 * (ND - 1) + i] = (uint8_t)(t >> (8 * i));
    } else {
#pragma unroll
        for (int i = 0; i < 3 * PX; ++i)
            if (i < 3 * n) q[i] = (uint8_t)(v[i >> 2] >> (8 * (i & 3)));
    }
}
