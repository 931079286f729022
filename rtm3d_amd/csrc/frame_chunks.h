// Host side shared by the frame stages (frames_convert, demosaic, jpeg, jpeg_enc, lens, augment): a batch of B frames goes to
// the device in chunks of FRAME_CHUNK - one launch each, the per-frame descriptors by value - and every stage refuses the same
// malformed batches in the same words.  Host code only: no kernel reads anything here but FRAME_CHUNK, the length of the
// descriptor arrays.
#pragma once

#define FRAME_CHUNK 32

extern void rt_set_error(const char* fmt, ...);          // (runtime.hip; the one declaration for these files)

// for (const FrameChunk c : frame_chunks(B)): frames c.b0 .. c.b0 + c.nb - 1 are chunk number c.k, 1 <= c.nb <= FRAME_CHUNK;
// no chunk for B < 1
struct FrameChunk { int b0, nb, k; };
struct FrameChunks {
    int B;
    struct It {
        int b0, B;
        FrameChunk operator*() const { return FrameChunk{b0, B - b0 < FRAME_CHUNK ? B - b0 : FRAME_CHUNK, b0 / FRAME_CHUNK}; }
        It& operator++() { b0 += (**this).nb; return *this; }             // (ends at B exactly: no sum beyond it)
        bool operator!=(const It& o) const { return b0 != o.b0; }
    };
    It begin() const { return It{0, B}; }
    It end() const { return It{B < 0 ? 0 : B, B}; }
};
static inline FrameChunks frame_chunks(int B) { return FrameChunks{B}; }

// ---- the refusals every stage words alike: each sets the error and returns true when it refuses
static inline bool refuse_count(const char* who, int B) {
    if (B < 1) rt_set_error("%s: B = %d", who, B);
    return B < 1;
}
static inline bool refuse_null(const char* who, const void* p) {
    if (!p) rt_set_error("%s: null pointer", who);
    return !p;
}
static inline bool refuse_order(const char* who, const char* name, int order) {         // name: dst_order, src_order
    if (order != 0 && order != 1) rt_set_error("%s: %s %d (0 R G B, 1 B G R)", who, name, order);
    return order != 0 && order != 1;
}
static inline bool refuse_side(const char* who, int b, int h, int w, int lo, int hi) {
    const bool bad = h < lo || w < lo || h > hi || w > hi;
    if (bad) rt_set_error("%s: frame %d is %d x %d; a side must lie in %d..%d", who, b, h, w, lo, hi);
    return bad;
}
static inline bool refuse_reserved(const char* who, int b, int reserved) {
    if (reserved != 0) rt_set_error("%s: frame %d: reserved = %d, not 0", who, b, reserved);
    return reserved != 0;
}
static inline bool refuse_null_dst(const char* who, int b, const void* dst) {
    if (!dst) rt_set_error("%s: frame %d: the destination is a NULL pointer", who, b);
    return !dst;
}

#ifdef __HIPCC__
// after the last launch of an entry point: its return value
static inline int launch_ok(const char* who) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { rt_set_error("%s launch: %s", who, hipGetErrorString(e)); return 1; }
    return 0;
}
#endif
