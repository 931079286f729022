// Host side of the camera-frame entry points (include/rtm3d_hip.h, "camera frames"): the normalisation tables and the
// Resize / letterbox geometry of a batch of frames, restated from rtm3d_amd/preprocess.py (normalize_lut, device_luts,
// resized_size, the pad rule of preprocess_batch) so that a C caller gets the reference's numbers bit for bit.  No device
// access: these run on a machine without a GPU.
#include <stdint.h>
#include <string.h>

#include "../../include/rtm3d_hip.h"

extern void rt_set_error(const char* fmt, ...);

namespace {

// float32 -> IEEE binary16, round to nearest even (what numpy's astype(float16) and the device cast do)
uint16_t half_bits(float f) {
    union { float f; uint32_t u; } v, magic;
    v.f = f;
    const uint32_t sign = v.u & 0x80000000u;
    v.u ^= sign;
    uint16_t o;
    if (v.u >= (uint32_t)(127 + 16) << 23) {
        o = v.u > (uint32_t)255 << 23 ? 0x7e00 : 0x7c00;          // NaN : overflow / infinity
    } else if (v.u < (uint32_t)113 << 23) {
        magic.u = (uint32_t)((127 - 15) + (23 - 10) + 1) << 23;    // subnormal half: the float addition does the rounding
        v.f += magic.f;
        o = (uint16_t)(v.u - magic.u);
    } else {
        const uint32_t odd = (v.u >> 13) & 1;
        v.u += ((uint32_t)(15 - 127) << 23) + 0xfff;
        v.u += odd;
        o = (uint16_t)(v.u >> 13);
    }
    return (uint16_t)(o | (sign >> 16));
}

}  // namespace

// Normalize + ToTensor (preprocess/transforms.py:110-120, 312-317): float32((v / 255. - mean[c]) / std[c]) evaluated in
// float64 with float32 mean / std
extern "C" int rtm3d_normalize_luts(const float mean[3], const float std[3], float* h_lut32, uint16_t* h_lut16) {
    if (!mean || !std || (!h_lut32 && !h_lut16)) { rt_set_error("normalize_luts: null argument"); return 1; }
    for (int c = 0; c < 3; ++c)
        for (int v = 0; v < 256; ++v) {
            const float r = (float)(((double)v / 255.0 - (double)mean[c]) / (double)std[c]);
            if (h_lut32) h_lut32[c * 256 + v] = r;
            if (h_lut16) h_lut16[c * 256 + v] = half_bits(r);
        }
    return 0;
}

// transforms.Resize with an int size (preprocess/transforms.py:484-490) and the centred letterbox
// (datasets/dataset_reader.py:175-195)
extern "C" int rtm3d_frame_geometry(int B, const int* h_hw, int resize_to, int H, int W, rtm3d_frame_geom* out) {
    if (B < 1 || !h_hw || !out || resize_to < 0 || H < 1 || W < 1) { rt_set_error("frame_geometry: bad arguments"); return 1; }
    for (int b = 0; b < B; ++b) {
        const int h = h_hw[2 * b], w = h_hw[2 * b + 1];
        int rh = h, rw = w;
        if (h >= 1 && w >= 1 && resize_to) {
            const double rate = (double)resize_to / (double)(h > w ? h : w);
            rh = (int)((double)h * rate);
            rw = (int)((double)w * rate);
        }
        if (h < 1 || w < 1 || rh < 1 || rw < 1 || rh > H || rw > W) {
            rt_set_error("frame_geometry: frame %d (%dx%d -> %dx%d) does not fit the %dx%d canvas", b, h, w, rh, rw, H, W);
            return 1;
        }
        rtm3d_frame_geom g;
        g.h = h; g.w = w; g.rh = rh; g.rw = rw;
        g.pad_w = (W - rw) / 2; g.pad_h = (H - rh) / 2;
        out[b] = g;
    }
    return 0;
}
