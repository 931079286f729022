// Engine files (include/rtm3d_hip.h, "engine files"; writer: rtm3d_amd/engine.py): host-only loader and the one-call
// detect step.  The loader checks the whole file before it touches a device, then replays the recorded calls through the
// same C entry points the Python recorder (rtm3d_amd/plan.py: RealizedPlan) calls, so the context holds the same launches.
#include <hip/hip_runtime_api.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>

#include "../../include/rtm3d_hip.h"

extern void rt_set_error(const char* fmt, ...);
extern void rt_ctx_attach_engine(rtm3d_ctx* ctx, void* engine, void (*engine_free)(void*));
extern void* rt_ctx_engine(rtm3d_ctx* ctx);

namespace {

const size_t HEADER_BYTES = 256, META_BYTES = 496, ALIGN = 256;

// ---- SHA-256 (FIPS 180-4)
struct Sha256 {
    uint32_t h[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
    uint8_t buf[64];
    size_t nbuf = 0;
    uint64_t total = 0;
    static uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
    void block(const uint8_t* p) {
        static const uint32_t k[64] = {
            0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01,
            0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc,
            0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147,
            0x06ca6351, 0x14292967, 0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
            0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08,
            0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208,
            0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
        uint32_t w[64];
        for (int i = 0; i < 16; ++i) w[i] = (uint32_t)p[4 * i] << 24 | (uint32_t)p[4 * i + 1] << 16 | (uint32_t)p[4 * i + 2] << 8 | p[4 * i + 3];
        for (int i = 16; i < 64; ++i) {
            uint32_t s0 = rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3);
            uint32_t s1 = rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10);
            w[i] = w[i - 16] + s0 + w[i - 7] + s1;
        }
        uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
        for (int i = 0; i < 64; ++i) {
            uint32_t t1 = hh + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + k[i] + w[i];
            uint32_t t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
            hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
        }
        h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
    }
    void update(const uint8_t* p, size_t n) {
        total += n;
        while (n) {
            if (nbuf == 0 && n >= 64) { block(p); p += 64; n -= 64; continue; }
            size_t k = 64 - nbuf < n ? 64 - nbuf : n;
            memcpy(buf + nbuf, p, k); nbuf += k; p += k; n -= k;
            if (nbuf == 64) { block(buf); nbuf = 0; }
        }
    }
    void final(uint8_t out[32]) {
        uint64_t bits = total * 8;
        uint8_t pad = 0x80, zero = 0;
        update(&pad, 1);
        while (nbuf != 56) update(&zero, 1);
        uint8_t len[8];
        for (int i = 0; i < 8; ++i) len[i] = (uint8_t)(bits >> (56 - 8 * i));
        update(len, 8);
        for (int i = 0; i < 8; ++i) for (int j = 0; j < 4; ++j) out[4 * i + j] = (uint8_t)(h[i] >> (24 - 8 * j));
    }
};

enum Opcode {
    OPC_TENSOR = 1, OPC_TENSOR_MX8 = 2, OPC_BLOB = 3,
    OPC_INPUT4 = 16, OPC_CONV = 17, OPC_STEM = 18, OPC_CONV32S2 = 19, OPC_CONV64_ROOT = 20, OPC_HEADOUT = 21, OPC_MAXPOOL = 22,
    OPC_MAXPOOL_S2D = 23, OPC_SOFTMAX = 24, OPC_QUANT_MX8 = 25, OPC_CONV_MX8 = 26,
};

const char* op_name(uint32_t op) {
    switch (op) {
    case OPC_TENSOR: return "tensor_create";
    case OPC_TENSOR_MX8: return "tensor_create_mx8";
    case OPC_BLOB: return "blob_create";
    case OPC_INPUT4: return "op_input_nhwc4";
    case OPC_CONV: return "op_conv";
    case OPC_STEM: return "op_stem_fused";
    case OPC_CONV32S2: return "op_conv32s2_fused";
    case OPC_CONV64_ROOT: return "op_conv64_root";
    case OPC_HEADOUT: return "op_headout";
    case OPC_MAXPOOL: return "op_maxpool";
    case OPC_MAXPOOL_S2D: return "op_maxpool_s2d";
    case OPC_SOFTMAX: return "op_softmax_fuse";
    case OPC_QUANT_MX8: return "op_quant_mx8";
    case OPC_CONV_MX8: return "op_conv_mx8";
    default: return nullptr;
    }
}

// payload bytes of an opcode (int32 records), 0 for the descriptor / blob records
size_t int_args(uint32_t op) {
    switch (op) {
    case OPC_TENSOR: case OPC_TENSOR_MX8: return 6;
    case OPC_INPUT4: return 1;
    case OPC_STEM: return 9;
    case OPC_CONV32S2: return 10;
    case OPC_CONV64_ROOT: return 16;
    case OPC_HEADOUT: return 8;
    case OPC_MAXPOOL: return 8;
    case OPC_MAXPOOL_S2D: return 5;
    case OPC_SOFTMAX: return 6;
    case OPC_QUANT_MX8: return 5;
    default: return 0;
    }
}

struct Record { uint32_t op; const uint8_t* p; uint32_t n; };

struct Parsed {
    std::vector<uint8_t> file;
    rtm3d_engine_info info;
    std::vector<Record> recs;
    const uint8_t* blobs = nullptr;
    uint64_t blob_area = 0;
};

template <class T> T rd(const uint8_t* p) { T v; memcpy(&v, p, sizeof(T)); return v; }

#define EFAIL(...) do { rt_set_error(__VA_ARGS__); return 1; } while (0)

// tensor (kind 'T'), MX8 tensor ('M') or blob ('B') id used by record i: created before it; `opt`: -1 (none) is allowed
struct Ids {
    int tensors = 0, mx8 = 0, blobs = 0;
    bool ok(char kind, int id, bool opt) const {
        if (opt && id == -1) return true;
        int n = kind == 'T' ? tensors : kind == 'M' ? mx8 : blobs;
        return id >= 0 && id < n;
    }
};

int check_ids(const Record& r, size_t i, const Ids& ids, const char* what) {
    auto arg = [&](size_t k) { return rd<int32_t>(r.p + 4 * k); };
    // (kind, argument index, optional) per opcode
    struct Use { char kind; int k; bool opt; };
    std::vector<Use> uses;
    switch (r.op) {
    case OPC_INPUT4: uses = {{'T', 0, false}}; break;
    case OPC_STEM: uses = {{'T', 0, false}, {'T', 1, false}, {'B', 3, false}, {'B', 4, false}, {'B', 5, false}, {'B', 6, false},
                           {'B', 7, true}, {'B', 8, true}}; break;
    case OPC_CONV32S2: uses = {{'T', 0, false}, {'T', 2, false}, {'T', 4, false}, {'B', 6, false}, {'B', 7, false}, {'B', 8, false},
                               {'B', 9, false}}; break;
    case OPC_CONV64_ROOT: uses = {{'T', 0, false}, {'T', 2, false}, {'B', 5, false}, {'B', 6, false}, {'B', 7, false}, {'B', 8, false},
                                  {'T', 9, true}, {'T', 12, true}, {'T', 14, true}}; break;
    case OPC_HEADOUT: uses = {{'T', 0, false}, {'B', 1, false}, {'B', 2, false}}; break;
    case OPC_MAXPOOL: uses = {{'T', 0, false}, {'T', 2, false}}; break;
    case OPC_MAXPOOL_S2D: uses = {{'T', 0, false}, {'T', 2, false}}; break;
    case OPC_SOFTMAX: {
        int n_u = arg(2);
        if (n_u < 1 || n_u > 3) EFAIL("%s: record %zu (op_softmax_fuse): n_u = %d", what, i, n_u);
        uses = {{'T', 0, false}, {'T', 1, false}};
        for (int u = 0; u < n_u; ++u) uses.push_back({'T', 3 + u, false});
        break;
    }
    case OPC_QUANT_MX8: uses = {{'T', 0, false}, {'M', 2, false}}; break;
    case OPC_CONV: {
        rtm3d_conv_desc d;
        memcpy(&d, r.p + 4, sizeof d);
        if (!ids.ok('T', d.in_tensor, false) || !ids.ok('T', d.out_tensor, true) || !ids.ok('T', d.res_tensor, true) ||
            !(d.s2d_tensor == 0 || ids.ok('T', d.s2d_tensor - 1, false)))
            EFAIL("%s: record %zu (op_conv): tensor id out of range (in %d, out %d, res %d, s2d %d; %d tensors created before it)", what, i,
                  d.in_tensor, d.out_tensor, d.res_tensor, d.s2d_tensor - 1, ids.tensors);
        if (!ids.ok('B', d.w_blob, false) || !ids.ok('B', d.bias_blob, false))
            EFAIL("%s: record %zu (op_conv): blob id out of range (w %d, bias %d; %d blobs created before it)", what, i, d.w_blob, d.bias_blob, ids.blobs);
        return 0;
    }
    case OPC_CONV_MX8: {
        rtm3d_conv_mx8_desc d;
        memcpy(&d, r.p + 4, sizeof d);
        if (!ids.ok('M', d.in_tensor, false) || !ids.ok(d.out_fp16 ? 'T' : 'M', d.out_tensor, false))
            EFAIL("%s: record %zu (op_conv_mx8): tensor id out of range (in %d, out %d)", what, i, d.in_tensor, d.out_tensor);
        if (!ids.ok('B', d.w_blob, false) || !ids.ok('B', d.wscale_blob, false) || !ids.ok('B', d.bias_blob, false))
            EFAIL("%s: record %zu (op_conv_mx8): blob id out of range", what, i);
        return 0;
    }
    default: return 0;
    }
    for (const Use& u : uses) {
        int id = arg(u.k);
        if (!ids.ok(u.kind, id, u.opt))
            EFAIL("%s: record %zu (%s): %s id %d (argument %d) out of range (%d created before it)", what, i, op_name(r.op),
                  u.kind == 'B' ? "blob" : u.kind == 'M' ? "mx8 tensor" : "tensor", id, u.k,
                  u.kind == 'B' ? ids.blobs : u.kind == 'M' ? ids.mx8 : ids.tensors);
    }
    return 0;
}

int parse(const char* path, Parsed& P, const char* what) {
    if (!path) EFAIL("%s: null path", what);
    FILE* f = fopen(path, "rb");
    if (!f) EFAIL("%s: cannot open %s", what, path);
    if (fseek(f, 0, SEEK_END) != 0) { fclose(f); EFAIL("%s: cannot seek %s", what, path); }
    long size = ftell(f);
    if (size < 0) { fclose(f); EFAIL("%s: cannot size %s", what, path); }
    P.file.resize((size_t)size);
    rewind(f);
    size_t got = size ? fread(P.file.data(), 1, (size_t)size, f) : 0;
    fclose(f);
    if (got != (size_t)size) EFAIL("%s: short read of %s", what, path);
    const uint8_t* d = P.file.data();
    const size_t n = P.file.size();
    rtm3d_engine_info& I = P.info;
    memset(&I, 0, sizeof I);
    I.file_bytes = n;

    // ---- header
    if (n < HEADER_BYTES) EFAIL("%s: truncated header (%zu bytes, the header is %zu)", what, n, HEADER_BYTES);
    if (memcmp(d, "RTM3DENG", 8) != 0) EFAIL("%s: bad magic (not an engine file)", what);
    I.format_version = (int)rd<uint32_t>(d + 8);
    I.abi_version = (int)rd<uint32_t>(d + 12);
    if (I.format_version != RTM3D_ENGINE_FORMAT) EFAIL("%s: format version %d, this library reads %d", what, I.format_version, RTM3D_ENGINE_FORMAT);
    if (I.abi_version != RTM3D_ABI_VERSION) EFAIL("%s: written for ABI %d, this library is ABI %d", what, I.abi_version, RTM3D_ABI_VERSION);
    memcpy(I.arch, d + 16, 15);
    memcpy(I.state_digest, d + 32, 64);
    if (strcmp(I.arch, "gfx950") != 0) EFAIL("%s: target arch '%s', this library is built for gfx950", what, I.arch);
    const uint8_t* sha = d + 96;
    const uint64_t nbody = rd<uint64_t>(d + 128);
    if (nbody != n - HEADER_BYTES)
        EFAIL("%s: the header announces a %llu-byte body, the file holds %zu bytes after the header (truncated or padded)", what,
              (unsigned long long)nbody, n - HEADER_BYTES);
    const uint8_t* b = d + HEADER_BYTES;
    uint8_t h[32];
    Sha256 s;
    s.update(b, (size_t)nbody);
    s.final(h);
    if (memcmp(h, sha, 32) != 0) EFAIL("%s: sha256 of the body does not match the header (file corrupted)", what);

    // ---- metadata
    if (nbody < META_BYTES + 16) EFAIL("%s: truncated metadata", what);
    I.B = rd<int32_t>(b); I.H = rd<int32_t>(b + 4); I.W = rd<int32_t>(b + 8);
    memcpy(I.backbone, b + 12, 15);
    I.head_precision = rd<int32_t>(b + 28); I.header_num_conv = rd<int32_t>(b + 32); I.num_classes = rd<int32_t>(b + 36);
    for (int k = 0; k < 4; ++k) I.head_channels[k] = rd<int32_t>(b + 40 + 4 * k);
    I.topk = rd<int32_t>(b + 56);
    I.down_sample = rd<float>(b + 60); I.score_thresh = rd<float>(b + 64);
    I.n_dim_ref = rd<int32_t>(b + 68);
    memcpy(I.dim_ref, b + 72, sizeof I.dim_ref);
    memcpy(I.ref_loc, b + 456, sizeof I.ref_loc);
    I.solver_form = rd<int32_t>(b + 480); I.use_graph = rd<int32_t>(b + 484);
    I.fun_accept = rd<double>(b + 488);
    if (I.B <= 0 || I.H <= 0 || I.W <= 0 || I.H % 32 || I.W % 32 || I.topk <= 0 || I.num_classes < 1 || I.num_classes > RTM3D_ENGINE_MAX_CLASSES ||
        I.n_dim_ref < I.num_classes || I.n_dim_ref > RTM3D_ENGINE_MAX_CLASSES || I.head_channels[0] != I.num_classes ||
        I.head_channels[1] != 16 || I.head_channels[2] != 2 || I.head_channels[3] != 2 || (I.head_precision != 0 && I.head_precision != 1) ||
        (I.solver_form != RTM3D_SOLVER_DIRECT && I.solver_form != RTM3D_SOLVER_PUBLISHED))
        EFAIL("%s: metadata out of range (B %d, H %d, W %d, topk %d, classes %d, dim_ref rows %d)", what, I.B, I.H, I.W, I.topk,
              I.num_classes, I.n_dim_ref);

    // ---- records
    const uint32_t n_records = rd<uint32_t>(b + META_BYTES), n_blobs = rd<uint32_t>(b + META_BYTES + 4);
    const uint64_t rbytes = rd<uint64_t>(b + META_BYTES + 8);
    const uint64_t rbeg = META_BYTES + 16;
    if (rbytes > nbody - rbeg || nbody - rbeg - rbytes < 16)
        EFAIL("%s: the records section (%llu bytes) runs past the end of the file", what, (unsigned long long)rbytes);
    const uint64_t rend = rbeg + rbytes;
    const uint64_t boff = rd<uint64_t>(b + rend), bbytes = rd<uint64_t>(b + rend + 8);
    if (boff % ALIGN || boff < rend + 16 || boff > nbody || bbytes != nbody - boff)
        EFAIL("%s: blob area [%llu, +%llu) does not end at the end of the file (%llu body bytes)", what, (unsigned long long)boff,
              (unsigned long long)bbytes, (unsigned long long)nbody);
    P.blobs = b + boff;
    P.blob_area = bbytes;
    Ids ids;
    uint64_t pos = rbeg;
    for (size_t i = 0; i < n_records; ++i) {
        if (rend - pos < 8) EFAIL("%s: record %zu: header past the end of the records section", what, i);
        Record r{rd<uint32_t>(b + pos), b + pos + 8, rd<uint32_t>(b + pos + 4)};
        pos += 8;
        if (r.n > rend - pos) EFAIL("%s: record %zu: %u payload bytes run past the end of the records section", what, i, r.n);
        pos += r.n;
        const char* name = op_name(r.op);
        if (!name) EFAIL("%s: record %zu: unknown opcode %u", what, i, r.op);
        if (r.op == OPC_CONV || r.op == OPC_CONV_MX8) {
            const uint32_t want = r.op == OPC_CONV ? (uint32_t)sizeof(rtm3d_conv_desc) : (uint32_t)sizeof(rtm3d_conv_mx8_desc);
            const uint32_t size = r.n >= 4 ? rd<uint32_t>(r.p) : 0;
            if (r.n < 4 || size != want || r.n != 4 + want)
                EFAIL("%s: record %zu (%s): descriptor of %u bytes, this library's is %u", what, i, name, size, want);
        } else if (r.op == OPC_BLOB) {
            if (r.n != 24) EFAIL("%s: record %zu (blob_create): payload of %u bytes, expected 24", what, i, r.n);
            const uint64_t nb = rd<uint64_t>(r.p), off = rd<uint64_t>(r.p + 8);
            if (nb == 0 || off % ALIGN || off > bbytes || nb > bbytes - off)
                EFAIL("%s: record %zu (blob_create): %llu bytes at offset %llu run past the end of the file (blob area %llu bytes)", what, i,
                      (unsigned long long)nb, (unsigned long long)off, (unsigned long long)bbytes);
        } else if (r.n != 4 * int_args(r.op)) {
            EFAIL("%s: record %zu (%s): payload of %u bytes, expected %zu", what, i, name, r.n, 4 * int_args(r.op));
        }
        if (check_ids(r, i, ids, what)) return 1;
        if (r.op == OPC_TENSOR || r.op == OPC_TENSOR_MX8 || r.op == OPC_BLOB) {
            int& next = r.op == OPC_TENSOR ? ids.tensors : r.op == OPC_TENSOR_MX8 ? ids.mx8 : ids.blobs;
            const int id = r.op == OPC_BLOB ? rd<int32_t>(r.p + 16) : rd<int32_t>(r.p + 20);
            if (id != next) EFAIL("%s: record %zu (%s): id %d, the runtime hands out %d", what, i, name, id, next);
            ++next;
            if (r.op == OPC_BLOB) I.blob_bytes += rd<uint64_t>(r.p);
        } else {
            I.n_launches++;
        }
        P.recs.push_back(r);
    }
    if (pos != rend) EFAIL("%s: %llu bytes after the last record of the records section", what, (unsigned long long)(rend - pos));
    if ((int)n_blobs != ids.blobs) EFAIL("%s: %d blob records, the counts say %u", what, ids.blobs, n_blobs);
    I.n_records = (int)n_records;
    I.n_tensors = ids.tensors;
    I.n_mx8_tensors = ids.mx8;
    I.n_blobs = ids.blobs;
    return 0;
}

int replay(rtm3d_ctx* ctx, const Parsed& P) {
    for (size_t i = 0; i < P.recs.size(); ++i) {
        const Record& r = P.recs[i];
        int v[16] = {0};
        const size_t na = int_args(r.op);
        for (size_t k = 0; k < na; ++k) v[k] = rd<int32_t>(r.p + 4 * k);
        int rc = 0, id = -1, want = -1;
        switch (r.op) {
        case OPC_TENSOR: rc = rtm3d_tensor_create(ctx, v[0], v[1], v[2], v[3], v[4], &id); want = v[5]; break;
        case OPC_TENSOR_MX8: rc = rtm3d_tensor_create_mx8(ctx, v[0], v[1], v[2], v[3], v[4], &id); want = v[5]; break;
        case OPC_BLOB:
            rc = rtm3d_blob_create(ctx, P.blobs + rd<uint64_t>(r.p + 8), (size_t)rd<uint64_t>(r.p), &id);
            want = rd<int32_t>(r.p + 16);
            break;
        case OPC_INPUT4: rc = rtm3d_op_input_nhwc4(ctx, v[0]); break;
        case OPC_CONV: {
            rtm3d_conv_desc d;
            memcpy(&d, r.p + 4, sizeof d);
            rc = rtm3d_op_conv(ctx, &d);
            break;
        }
        case OPC_STEM: rc = rtm3d_op_stem_fused(ctx, v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8]); break;
        case OPC_CONV32S2: rc = rtm3d_op_conv32s2_fused(ctx, v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9]); break;
        case OPC_CONV64_ROOT:
            rc = rtm3d_op_conv64_root(ctx, v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9], v[10], v[11], v[12], v[13], v[14], v[15]);
            break;
        case OPC_HEADOUT: rc = rtm3d_op_headout(ctx, v[0], v[1], v[2], v[3], v + 4); break;
        case OPC_MAXPOOL: rc = rtm3d_op_maxpool(ctx, v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]); break;
        case OPC_MAXPOOL_S2D: rc = rtm3d_op_maxpool_s2d(ctx, v[0], v[1], v[2], v[3], v[4]); break;
        case OPC_SOFTMAX: rc = rtm3d_op_softmax_fuse(ctx, v[0], v[1], v[2], v + 3); break;
        case OPC_QUANT_MX8: rc = rtm3d_op_quant_mx8(ctx, v[0], v[1], v[2], v[3], v[4]); break;
        case OPC_CONV_MX8: {
            rtm3d_conv_mx8_desc d;
            memcpy(&d, r.p + 4, sizeof d);
            rc = rtm3d_op_conv_mx8(ctx, &d);
            break;
        }
        default: EFAIL("engine_load: record %zu: unknown opcode %u", i, r.op);
        }
        if (rc != 0) {
            std::string why = rtm3d_last_error();
            EFAIL("engine_load: record %zu (%s) refused by the runtime: %s", i, op_name(r.op), why.c_str());
        }
        if (want >= 0 && id != want) EFAIL("engine_load: record %zu (%s): the runtime handed out id %d, the file says %d", i, op_name(r.op), id, want);
    }
    return 0;
}

// what rtm3d_engine_detect needs besides the replayed plan
struct EngineState {
    rtm3d_engine_info info;
    const double* d_dim_ref = nullptr;   // blobs of the context
    const double* d_ref_loc = nullptr;
    // camera-frame steps (rtm3d_engine_set_frame_params): the normalisation tables (blobs too) and the per-call geometry
    bool frames = false;
    int resize_to = 0;
    const float* d_lut32 = nullptr;
    const uint16_t* d_lut16 = nullptr;
    std::vector<rtm3d_frame_geom> geom;
    std::vector<int> resized_hw;
    std::vector<int> src_hw;             // (h, w) of the sources of rtm3d_engine_detect_frames_src / _raw
    std::vector<int> rect_hw;            // (ho, wo) of the maps of rtm3d_engine_detect_frames_lens
};

void free_state(void* p) { delete (EngineState*)p; }

size_t align_up(size_t v) { return (v + ALIGN - 1) / ALIGN * ALIGN; }

// the workspace of a detect step: four logit maps, the decode2d workspace, the slots of decode2d and of the solver
struct Layout {
    size_t logits[4], ws2d, n, cls, score, mproj, verts, bbox, x, fun, nit, status, total;
};

Layout layout(const rtm3d_engine_info& I) {
    Layout L;
    size_t o = 0;
    const size_t hw = (size_t)(I.H / 4) * (I.W / 4), N = (size_t)I.B * I.topk;
    auto take = [&](size_t bytes) { size_t at = o; o = align_up(o + bytes); return at; };
    for (int k = 0; k < 4; ++k) L.logits[k] = take((size_t)I.B * I.head_channels[k] * hw * sizeof(float));
    L.ws2d = take(rtm3d_decode2d_workspace_bytes(I.B, I.num_classes, I.H / 4, I.W / 4));
    L.n = take((size_t)I.B * sizeof(int32_t));
    L.cls = take(N * sizeof(int64_t));
    L.score = take(N * sizeof(float));
    L.mproj = take(N * 2 * sizeof(float));
    L.verts = take(N * 16 * sizeof(float));
    L.bbox = take(N * 4 * sizeof(float));
    L.x = take(N * 8 * sizeof(double));
    L.fun = take(N * sizeof(double));
    L.nit = take(N * sizeof(int32_t));
    L.status = take(N * sizeof(int32_t));
    L.total = o;
    return L;
}

template <class T> int device_blob(rtm3d_ctx* ctx, const void* h, size_t bytes, const T** d) {
    int id = -1;
    void* p = nullptr;
    if (rtm3d_blob_create(ctx, h, bytes, &id) || rtm3d_blob_address(ctx, id, &p, nullptr)) return 1;
    *d = (const T*)p;
    return 0;
}

// the workspace of a frames step: the detect workspace, then the channel sums of the letterbox and the canvas intrinsics
struct FramesLayout { size_t sums, K_net, total; };

FramesLayout frames_layout(const rtm3d_engine_info& I) {
    FramesLayout F;
    F.sums = layout(I).total;
    F.K_net = align_up(F.sums + (size_t)I.B * 3 * sizeof(unsigned long long));
    F.total = align_up(F.K_net + (size_t)I.B * 9 * sizeof(double));
    return F;
}

}  // namespace

extern "C" int rtm3d_engine_inspect(const char* path, rtm3d_engine_info* info) {
    Parsed P;
    if (parse(path, P, "engine_inspect")) return 1;
    if (info) *info = P.info;
    return 0;
}

extern "C" int rtm3d_engine_load(const char* path, int device, rtm3d_ctx** out, rtm3d_engine_info* info) {
    if (!out) EFAIL("engine_load: null out");
    *out = nullptr;
    Parsed P;
    if (parse(path, P, "engine_load")) return 1;
    hipDeviceProp_t prop;
    hipError_t e = hipGetDeviceProperties(&prop, device);
    if (e != hipSuccess) EFAIL("engine_load: device %d: %s", device, hipGetErrorString(e));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0 || (prop.gcnArchName[6] != 0 && prop.gcnArchName[6] != ':'))
        EFAIL("engine_load: device %d is %s, the engine is built for gfx950", device, prop.gcnArchName);
    rtm3d_ctx* ctx = nullptr;
    if (rtm3d_ctx_create(device, &ctx)) return 1;
    EngineState* st = new EngineState();
    st->info = P.info;
    rt_ctx_attach_engine(ctx, st, free_state);
    if (replay(ctx, P) || device_blob(ctx, P.info.dim_ref, sizeof(double) * 3 * P.info.n_dim_ref, &st->d_dim_ref) ||
        device_blob(ctx, P.info.ref_loc, sizeof P.info.ref_loc, &st->d_ref_loc) || rtm3d_ctx_set_graph(ctx, P.info.use_graph)) {
        std::string why = rtm3d_last_error();
        rtm3d_ctx_destroy(ctx);
        EFAIL("%s", why.c_str());
    }
    if (info) *info = P.info;
    *out = ctx;
    return 0;
}

extern "C" size_t rtm3d_engine_workspace_bytes(rtm3d_ctx* ctx) {
    EngineState* st = (EngineState*)rt_ctx_engine(ctx);
    return st ? layout(st->info).total : 0;
}

// forward -> decode2d -> decode3d_slots -> pack_records on the workspace; d_in == nullptr: the plan's input tensor is filled
static int detect_step(rtm3d_ctx* ctx, EngineState* st, void* stream, const float* d_in, const double* d_K_per_image, float* d_rec,
                       void* d_workspace) {
    const rtm3d_engine_info& I = st->info;
    const Layout L = layout(I);
    char* w = (char*)d_workspace;
    float* logits[4];
    for (int k = 0; k < 4; ++k) logits[k] = (float*)(w + L.logits[k]);
    int32_t* n = (int32_t*)(w + L.n);
    int64_t* cls = (int64_t*)(w + L.cls);
    float *score = (float*)(w + L.score), *mproj = (float*)(w + L.mproj), *verts = (float*)(w + L.verts), *bbox = (float*)(w + L.bbox);
    double *x = (double*)(w + L.x), *fun = (double*)(w + L.fun);
    int32_t *nit = (int32_t*)(w + L.nit), *status = (int32_t*)(w + L.status);
    if (rtm3d_forward(ctx, stream, d_in, logits)) return 1;
    if (rtm3d_decode2d(stream, logits[0], logits[1], logits[2], I.B, I.num_classes, I.H / 4, I.W / 4, I.score_thresh, I.topk,
                       I.down_sample, w + L.ws2d, n, cls, score, mproj, verts, bbox))
        return 1;
    if (rtm3d_decode3d_slots(stream, I.B, I.topk, n, cls, verts, d_K_per_image, st->d_dim_ref, I.n_dim_ref, st->d_ref_loc, x, fun, nit,
                             status, I.solver_form))
        return 1;
    return rtm3d_pack_records(stream, I.B, I.topk, n, cls, score, mproj, verts, bbox, x, fun, status, I.fun_accept, d_rec);
}

extern "C" int rtm3d_engine_detect(rtm3d_ctx* ctx, void* stream, const float* d_in, const double* d_K_per_image, float* d_rec,
                                   void* d_workspace) {
    EngineState* st = (EngineState*)rt_ctx_engine(ctx);
    if (!st) EFAIL("engine_detect: the context was not made by rtm3d_engine_load");
    if (!d_in || !d_K_per_image || !d_rec || !d_workspace) EFAIL("engine_detect: null argument");
    return detect_step(ctx, st, stream, d_in, d_K_per_image, d_rec, d_workspace);
}

extern "C" int rtm3d_engine_set_frame_params(rtm3d_ctx* ctx, const rtm3d_frame_params* params) {
    EngineState* st = (EngineState*)rt_ctx_engine(ctx);
    if (!st) EFAIL("engine_set_frame_params: the context was not made by rtm3d_engine_load");
    if (!params) EFAIL("engine_set_frame_params: null argument");
    if (st->frames) EFAIL("engine_set_frame_params: the frame parameters of this context are already set");
    if (params->resize_to < 0) EFAIL("engine_set_frame_params: resize_to = %d", params->resize_to);
    float lut32[3 * 256];
    uint16_t lut16[3 * 256];
    if (rtm3d_normalize_luts(params->mean, params->std, lut32, lut16)) return 1;
    void* base = nullptr;
    int B, H, W, border;
    if (rtm3d_input_tensor(ctx, &base, &B, &H, &W, &border)) return 1;      // a plan that cannot be fed in place is refused here
    if (B != st->info.B || H != st->info.H || W != st->info.W)
        EFAIL("engine_set_frame_params: the plan's input tensor is %dx%dx%d, the engine's batch %dx%dx%d", B, H, W, st->info.B,
              st->info.H, st->info.W);
    if (device_blob(ctx, lut32, sizeof lut32, &st->d_lut32) || device_blob(ctx, lut16, sizeof lut16, &st->d_lut16)) return 1;
    st->resize_to = params->resize_to;
    st->geom.resize((size_t)st->info.B);
    st->resized_hw.resize((size_t)st->info.B * 2);
    st->frames = true;
    return 0;
}

extern "C" size_t rtm3d_engine_frames_workspace_bytes(rtm3d_ctx* ctx) {
    EngineState* st = (EngineState*)rt_ctx_engine(ctx);
    return st ? frames_layout(st->info).total : 0;
}

// the opening of every camera-frame entry: the engine state of the context, nullptr after one of the three refusals
static EngineState* frames_state(rtm3d_ctx* ctx, const char* who, bool null_argument) {
    EngineState* st = (EngineState*)rt_ctx_engine(ctx);
    if (!st) rt_set_error("%s: the context was not made by rtm3d_engine_load", who);
    else if (null_argument) rt_set_error("%s: null argument", who);
    else if (!st->frames) rt_set_error("%s: call rtm3d_engine_set_frame_params first", who);
    else return st;
    return nullptr;
}

// size_of(b, hw) writes (h, w) of frame b or refuses it; then the frames' place on the canvas
template <class F> static int place_frames(EngineState* st, std::vector<int>& hw, F size_of) {
    const rtm3d_engine_info& I = st->info;
    hw.resize((size_t)I.B * 2);
    for (int b = 0; b < I.B; ++b)
        if (size_of(b, &hw[2 * b])) return 1;
    return rtm3d_frame_geometry(I.B, hw.data(), st->resize_to, I.H, I.W, st->geom.data());
}

extern "C" int rtm3d_engine_detect_frames(rtm3d_ctx* ctx, void* stream, const uint8_t* const* h_imgs, const int* h_hw,
                                          const double* d_K_camera, float* d_rec, double* d_kitti, void* d_workspace) {
    EngineState* st = frames_state(ctx, "engine_detect_frames", !h_imgs || !h_hw || !d_K_camera || !d_rec || !d_workspace);
    if (!st) return 1;
    const rtm3d_engine_info& I = st->info;
    for (int b = 0; b < I.B; ++b)
        if (!h_imgs[b]) EFAIL("engine_detect_frames: frame %d is a null pointer", b);
    rtm3d_frame_geom* geom = st->geom.data();
    if (rtm3d_frame_geometry(I.B, h_hw, st->resize_to, I.H, I.W, geom)) return 1;
    for (int b = 0; b < I.B; ++b) { st->resized_hw[2 * b] = geom[b].rh; st->resized_hw[2 * b + 1] = geom[b].rw; }
    void* base = nullptr;
    int tB, tH, tW, border;
    if (rtm3d_input_tensor(ctx, &base, &tB, &tH, &tW, &border)) return 1;
    const FramesLayout F = frames_layout(I);
    const Layout L = layout(I);
    char* w = (char*)d_workspace;
    double* K_net = (double*)(w + F.K_net);
    if (rtm3d_preprocess_batch(stream, I.B, h_imgs, h_hw, st->resized_hw.data(), base, 1, I.H, I.W, border, st->d_lut32, st->d_lut16,
                               (unsigned long long*)(w + F.sums)))
        return 1;
    if (rtm3d_frames_adjust_k(stream, I.B, geom, d_K_camera, K_net)) return 1;
    if (detect_step(ctx, st, stream, nullptr, K_net, d_rec, d_workspace)) return 1;
    return rtm3d_records_to_camera(stream, I.B, I.topk, geom, d_rec, d_K_camera, (const double*)(w + L.x), (const double*)(w + L.fun),
                                   (const int32_t*)(w + L.status), I.fun_accept, d_kitti);
}

extern "C" int rtm3d_engine_detect_frames_src(rtm3d_ctx* ctx, void* stream, const rtm3d_frame_src* h_src, uint8_t* const* h_packed,
                                              int dst_order, const double* d_K_camera, float* d_rec, double* d_kitti, void* d_workspace) {
    EngineState* st = frames_state(ctx, "engine_detect_frames_src", !h_src || !h_packed || !d_K_camera || !d_rec || !d_workspace);
    if (!st) return 1;
    const rtm3d_engine_info& I = st->info;
    // everything either step would refuse, before the first launch: the sources, then the frames' place on the canvas
    if (rtm3d_frames_convert_check(I.B, h_src, h_packed, dst_order)) return 1;
    if (place_frames(st, st->src_hw, [&](int b, int* hw) { hw[0] = h_src[b].h; hw[1] = h_src[b].w; return 0; })) return 1;
    if (rtm3d_frames_convert(stream, I.B, h_src, h_packed, dst_order)) return 1;
    return rtm3d_engine_detect_frames(ctx, stream, h_packed, st->src_hw.data(), d_K_camera, d_rec, d_kitti, d_workspace);
}

extern "C" int rtm3d_engine_detect_frames_raw(rtm3d_ctx* ctx, void* stream, const rtm3d_raw_src* h_src, uint8_t* const* h_packed,
                                              int method, int dst_order, const double* d_K_camera, float* d_rec, double* d_kitti,
                                              void* d_workspace) {
    EngineState* st = frames_state(ctx, "engine_detect_frames_raw", !h_src || !h_packed || !d_K_camera || !d_rec || !d_workspace);
    if (!st) return 1;
    const rtm3d_engine_info& I = st->info;
    // everything either step would refuse, before the first launch: the sources, then the frames' place on the canvas
    if (rtm3d_frames_demosaic_check(I.B, h_src, h_packed, method, dst_order)) return 1;
    if (place_frames(st, st->src_hw, [&](int b, int* hw) { hw[0] = h_src[b].h; hw[1] = h_src[b].w; return 0; })) return 1;
    if (rtm3d_frames_demosaic(stream, I.B, h_src, h_packed, method, dst_order)) return 1;
    return rtm3d_engine_detect_frames(ctx, stream, h_packed, st->src_hw.data(), d_K_camera, d_rec, d_kitti, d_workspace);
}

extern int rt_jpeg_info(const uint8_t* data, size_t bytes, rtm3d_jpeg_stream_info* out, char* msg, size_t msg_len);

extern "C" int rtm3d_engine_detect_frames_jpeg(rtm3d_ctx* ctx, void* stream, const uint8_t* const* h_data, const size_t* h_bytes,
                                               int16_t* h_stage, int16_t* d_coef, size_t capacity, uint8_t* const* h_packed,
                                               const size_t* h_packed_bytes, int dst_order, int n_threads, const double* d_K_camera,
                                               float* d_rec, double* d_kitti, void* d_workspace) {
    EngineState* st = frames_state(ctx, "engine_detect_frames_jpeg", !h_data || !h_bytes || !h_stage || !d_coef || !h_packed || !h_packed_bytes ||
                                                                          !d_K_camera || !d_rec || !d_workspace);
    if (!st) return 1;
    const rtm3d_engine_info& I = st->info;
    // the frames' place on the canvas, before anything is decoded or launched; rtm3d_frames_jpeg refuses the rest before its first launch
    const auto header_size = [&](int b, int* hw) {
        rtm3d_jpeg_stream_info J;
        char msg[200];
        if (rt_jpeg_info(h_data[b], h_bytes[b], &J, msg, sizeof(msg))) EFAIL("engine_detect_frames_jpeg: frame %d: %s", b, msg);
        hw[0] = J.h; hw[1] = J.w;
        return 0;
    };
    if (place_frames(st, st->src_hw, header_size)) return 1;
    if (rtm3d_frames_jpeg(stream, I.B, h_data, h_bytes, h_stage, d_coef, capacity, h_packed, h_packed_bytes, dst_order, n_threads)) return 1;
    return rtm3d_engine_detect_frames(ctx, stream, h_packed, st->src_hw.data(), d_K_camera, d_rec, d_kitti, d_workspace);
}

extern "C" int rtm3d_engine_detect_frames_lens(rtm3d_ctx* ctx, void* stream, const rtm3d_frame_src* h_src, uint8_t* const* h_packed,
                                               const int* h_hw, int dst_order, const rtm3d_lens_map* h_maps, uint8_t* const* h_rect,
                                               const uint8_t fill[3], const double* d_K_rect, float* d_rec, double* d_kitti,
                                               void* d_workspace) {
    EngineState* st = frames_state(ctx, "engine_detect_frames_lens",
                                   !h_packed || (!h_src && !h_hw) || !h_maps || !h_rect || !fill || !d_K_rect || !d_rec || !d_workspace);
    if (!st) return 1;
    const rtm3d_engine_info& I = st->info;
    // everything the three steps would refuse, before the first launch: the sources, the maps and both sets of buffers, then
    // the rectified frames' place on the canvas
    if (h_src && rtm3d_frames_convert_check(I.B, h_src, h_packed, dst_order)) return 1;
    st->src_hw.resize((size_t)I.B * 2);
    for (int b = 0; b < I.B; ++b) {
        st->src_hw[2 * b] = h_src ? h_src[b].h : h_hw[2 * b];
        st->src_hw[2 * b + 1] = h_src ? h_src[b].w : h_hw[2 * b + 1];
    }
    if (rtm3d_frames_remap_check(I.B, h_packed, st->src_hw.data(), h_maps, h_rect, fill)) return 1;
    if (place_frames(st, st->rect_hw, [&](int b, int* hw) { hw[0] = h_maps[b].ho; hw[1] = h_maps[b].wo; return 0; })) return 1;
    if (h_src && rtm3d_frames_convert(stream, I.B, h_src, h_packed, dst_order)) return 1;
    if (rtm3d_frames_remap(stream, I.B, h_packed, st->src_hw.data(), h_maps, h_rect, fill)) return 1;
    return rtm3d_engine_detect_frames(ctx, stream, h_rect, st->rect_hw.data(), d_K_rect, d_rec, d_kitti, d_workspace);
}
