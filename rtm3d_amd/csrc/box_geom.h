// The rotated-box intersection shared by box_overlap.hip (pairwise overlaps, 3D NMS) and track.hip (association of detections to
// tracks): one definition, so both translation units run the same fp64 operation sequence (include/rtm3d_hip.h, "box overlaps").
// Both are compiled with -ffp-contract=off (Makefile).  The polygon buffers are the caller's LDS: [vertex][lane], BO_LANES lanes.
#pragma once
#include "common.h"

#define BO_LANES 256
#define BO_MAXV 8

struct BoxP {                       // a box made ready for pairing
    double X, Z, c, s, hl, hw, y0, y1, area, h;
    bool valid;
};

__device__ __forceinline__ BoxP box_prepare(double h, double w, double l, double X, double Y, double Z, double ry) {
    BoxP p;
    p.valid = h > 0.0 && w > 0.0 && l > 0.0 && __builtin_isfinite(h) && __builtin_isfinite(w) && __builtin_isfinite(l) &&
              __builtin_isfinite(X) && __builtin_isfinite(Y) && __builtin_isfinite(Z) && __builtin_isfinite(ry);
    p.X = X; p.Z = Z; p.h = h;
    p.c = cos(ry); p.s = sin(ry);
    p.hl = l / 2.0; p.hw = w / 2.0;
    p.y0 = Y - h / 2.0; p.y1 = Y + h / 2.0;
    p.area = l * w;
    return p;
}

typedef double2 (*PolyBuf)[BO_LANES];          // [vertex][lane]

// Keep the part of `in` (n vertices) with  sign * coordinate[axis] <= bound;  returns the new vertex count (<= BO_MAXV).
template <int AXIS>
__device__ __forceinline__ int clip_halfplane(PolyBuf in, int n, PolyBuf out, int lane, double sign, double bound) {
    if (n == 0) return 0;
    int m = 0;
    double2 prev = in[n - 1][lane];
    double dprev = bound - sign * (AXIS == 0 ? prev.x : prev.y);
    for (int i = 0; i < n; ++i) {
        const double2 cur = in[i][lane];
        const double dcur = bound - sign * (AXIS == 0 ? cur.x : cur.y);
        if ((dcur >= 0.0) != (dprev >= 0.0)) {          // the edge prev -> cur crosses the line: d is linear along it
            const double t = dprev / (dprev - dcur);
            double2 q;
            if (AXIS == 0) { q.x = sign * bound; q.y = prev.y + t * (cur.y - prev.y); }
            else { q.y = sign * bound; q.x = prev.x + t * (cur.x - prev.x); }
            if (m < BO_MAXV) out[m++][lane] = q;
        }
        if (dcur >= 0.0 && m < BO_MAXV) out[m++][lane] = cur;
        prev = cur; dprev = dcur;
    }
    return m;
}

// BEV intersection area and vertical overlap length of two prepared boxes (the footprint areas are a.area, b.area).
// p0 / p1: the lane's two polygon buffers.
__device__ __forceinline__ void box_pair(const BoxP& a, const BoxP& b, PolyBuf p0, PolyBuf p1, int lane, double& inter, double& ov) {
    inter = 0.0; ov = 0.0;
    if (!a.valid || !b.valid) return;
    const double top = fmax(a.y0, b.y0), bot = fmin(a.y1, b.y1);
    ov = fmax(bot - top, 0.0);
    // corners of A, counter-clockwise in its own (x, z): world offset from B's centre, then B's local coordinates
    const double dX = a.X - b.X, dZ = a.Z - b.Z;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double lx = (k == 0 || k == 3) ? a.hl : -a.hl;
        const double lz = (k < 2) ? a.hw : -a.hw;
        const double wx = (a.c * lx + a.s * lz) + dX;
        const double wz = (a.c * lz - a.s * lx) + dZ;
        double2 q;
        q.x = b.c * wx - b.s * wz;             // R_b^T: local x = c * x - s * z, local z = s * x + c * z
        q.y = b.s * wx + b.c * wz;
        p0[k][lane] = q;
    }
    int n = clip_halfplane<0>(p0, 4, p1, lane, 1.0, b.hl);
    n = clip_halfplane<0>(p1, n, p0, lane, -1.0, b.hl);
    n = clip_halfplane<1>(p0, n, p1, lane, 1.0, b.hw);
    n = clip_halfplane<1>(p1, n, p0, lane, -1.0, b.hw);
    if (n < 3) return;
    double2 prev = p0[n - 1][lane];
    double sum = 0.0;
    for (int i = 0; i < n; ++i) {
        const double2 cur = p0[i][lane];
        sum = sum + (prev.x * cur.y - prev.y * cur.x);
        prev = cur;
    }
    inter = fabs(sum) / 2.0;
}

// criterion 0: inter / (sa + sb - inter), 1: inter / sa, 2: inter / sb; a denominator that is not positive gives 0
__device__ __forceinline__ double overlap_ratio(double inter, double sa, double sb, int criterion) {
    const double den = criterion == 0 ? (sa + sb) - inter : (criterion == 1 ? sa : sb);
    double r = den > 0.0 ? inter / den : 0.0;
    if (!(r == r)) r = 0.0;                    // inf / inf of boxes whose size overflows
    return r;
}

__device__ __forceinline__ BoxP box_load(const double* __restrict__ v) {
    return box_prepare(v[0], v[1], v[2], v[3], v[4], v[5], v[6]);
}
