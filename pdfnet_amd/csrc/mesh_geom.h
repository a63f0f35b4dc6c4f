// The geometry of the two hand meshes of a sample (verts [..., 2, n, 3], faces [2, Fc, 3]), shared by every kernel that stages them in LDS and
// walks them triangle by triangle: metrics.hip (penetration metric), icp.hip (ICP and the cloud-to-mesh loss), meshcloud.hip, penetration.hip,
// render.hip and silhouette.hip.  One copy of the limits, the index clamp, the staging loops, the separately rounded forms, the winding
// number's solid angle, the closest-point walk, the fixed-order block sum and the corner-gradient gather.  A function whose roundings two
// kernels must share carries `#pragma clang fp contract(off)` in its own body, so every kernel that inlines it rounds alike whatever the
// compiler makes of the code around it.
#pragma once
#include "common.h"

#define HAND_MAXN 1024                                         // vertices of a hand
#define HAND_MAXF 2048                                         // faces of a hand
#define HAND_MAXP 1024                                         // sensor points of a hand

#define ICP_T 1024
#define ICP_W (ICP_T / 64)

// p q - r s from separately rounded products (no fma): exactly negated when (p, r) or (q, s) change places, so a cross product built from it
// is exactly zero for equal vectors (a triangle with two equal corners, or with collinear corners whose edges are exact multiples of each
// other, has the normal 0) and exactly negated when the two vectors change places
__device__ __forceinline__ float geo_det2(float p, float q, float r, float s) {
#pragma clang fp contract(off)
    return p * q - r * s;
}

// a face index clamped into [0, n): it must not leave the staged vertices
__device__ __forceinline__ int geo_index(const long long* f, int n) { return (int)min(max(*f, 0LL), (long long)(n - 1)); }

// faces fo [Fc][3] (global) -> 16-bit triples tri [Fc] (LDS), clamped
__device__ __forceinline__ void geo_stage_faces(const long long* __restrict__ fo, int Fc, int n, ushort4* tri) {
    for (int g = threadIdx.x; g < Fc; g += blockDim.x)
        tri[g] = make_ushort4((unsigned short)geo_index(fo + 3 * g, n), (unsigned short)geo_index(fo + 3 * g + 1, n),
                              (unsigned short)geo_index(fo + 3 * g + 2, n), 0);
}

// row [n][3] (global) -> planes x, y, z [n] (LDS); consecutive lanes read consecutive floats
__device__ __forceinline__ void geo_stage_planes(const float* __restrict__ row, int n, float* x, float* y, float* z) {
    for (int e = threadIdx.x; e < 3 * n; e += blockDim.x) {
        const int i = e / 3, k = e - 3 * i;
        (k == 0 ? x : k == 1 ? y : z)[i] = row[e];
    }
}

// The associations below are written with their fused multiply-adds spelled out and contraction off: with contraction left to the compiler
// two kernels chose different operands to fuse, and a near-tie between two triangles then fell to different sides.  The forms are the ones
// mesh_icp_kernel has always run.
// x0 x1 + y0 y1 + z0 z1 as fma(y0, y1, x0 x1) + z0 z1: the facing test
__device__ __forceinline__ float icp_dot3(float x0, float x1, float y0, float y1, float z0, float z1) {
#pragma clang fp contract(off)
    return __builtin_fmaf(y0, y1, x0 * x1) + z0 * z1;
}
// u . v as fma(uz, vz, fma(ux, vx, uy vy)): the walk's d1 .. d6 and |q - p|^2
__device__ __forceinline__ float icp_dot(float ux, float uy, float uz, float vx, float vy, float vz) {
#pragma clang fp contract(off)
    return __builtin_fmaf(uz, vz, __builtin_fmaf(ux, vx, uy * vy));
}

// does triangle (a, b, c), oriented outwards, face the camera at the origin: n . (a + b + c) < 0 with n = (b - a) x (c - a)
__device__ __forceinline__ bool geo_faces_camera(float ax, float ay, float az, float bx, float by, float bz, float cx, float cy, float cz) {
    const float e1x = bx - ax, e1y = by - ay, e1z = bz - az, e2x = cx - ax, e2y = cy - ay, e2z = cz - az;
    const float nx = geo_det2(e1y, e2z, e1z, e2y), ny = geo_det2(e1z, e2x, e1x, e2z), nz = geo_det2(e1x, e2y, e1y, e2x);
    return icp_dot3(nx, ax + bx + cx, ny, ay + by + cy, nz, az + bz + cz) < 0.f;
}

// (x, y, 1/Z, Z) of a camera-space point under the pinhole camera K9 (row-major 3 x 3): x = fx X / Z + cx, y = fy Y / Z + cy
__device__ __forceinline__ float4 geo_project(const float* __restrict__ K9, float X, float Y, float Z) {
    return make_float4(K9[0] * X / Z + K9[2], K9[4] * Y / Z + K9[5], 1.f / Z, Z);
}

// Numerator and denominator of a triangle's Van Oosterom-Strackee solid angle, a, b, c the corners relative to the query:
//   det = a . (b x c),  den = |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|
// The winding number of mesh_penetration_kernel (metrics.hip) and of penetration_loss_kernel (penetration.hip) is made of these, and both call
// this function: every product that is fused and every one that is rounded on its own is written down, b x c is from separately rounded
// products (exactly 0 for a collapsed triangle), so the loss's `inside` is the metric's wind > 0.5 bit for bit.
__device__ __forceinline__ void geo_solid_angle(float ax, float ay, float az, float bx, float by, float bz, float cx, float cy, float cz,
                                                float& det, float& den) {
#pragma clang fp contract(off)
    const float la = sqrtf(__builtin_fmaf(ay, ay, ax * ax) + az * az);
    const float lb = sqrtf(__builtin_fmaf(by, by, bx * bx) + bz * bz);
    const float lc = sqrtf(__builtin_fmaf(cx, cx, cy * cy) + cz * cz);
    const float ab = __builtin_fmaf(az, bz, __builtin_fmaf(ay, by, ax * bx));
    const float bc = bz * cz + __builtin_fmaf(by, cy, bx * cx);
    const float ca = __builtin_fmaf(ax, cx, ay * cy) + az * cz;
    const float ux = by * cz - bz * cy, uy = bz * cx - bx * cz, uz = bx * cy - by * cx;      // b x c from separately rounded products
    det = az * uz + __builtin_fmaf(ay, uy, ax * ux);
    den = lb * ca + __builtin_fmaf(la, bc, __builtin_fmaf(ab, lc, (la * lb) * lc));
}

// v[0..K) summed over a block of ICP_T lanes in a fixed order -> out[0..K) in LDS (ends in a barrier): the xor butterfly per wave, then
// thread k adds the 16 wave partials of sum k as a balanced tree
template <int K>
__device__ __forceinline__ void icp_block_sum(double* v, double* sm, double* out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double r = wave_sum_d(v[k]);
        if (lane == 0) sm[wave * K + k] = r;
    }
    __syncthreads();
    if (threadIdx.x < K) {
        double p[ICP_W];
#pragma unroll
        for (int w = 0; w < ICP_W; ++w) p[w] = sm[w * K + threadIdx.x];
#pragma unroll
        for (int m = ICP_W / 2; m > 0; m /= 2) {
#pragma unroll
            for (int w = 0; w < m; ++w) p[w] = p[2 * w] + p[2 * w + 1];
        }
        out[threadIdx.x] = p[0];
    }
    __syncthreads();
}

// ---- the closest-point walk (icp.hip and penetration.hip) ---------------------------------------------------------------------------------
#define ICP_TINY 1e-37f
#define ICP_K 17                                               // count, sum p [3], sum q [3], sum q p^T [9], sum |p - q|^2

// v ab + w ac - ap as fma(ac, w, ab v) - ap: a coordinate of q - p
__device__ __forceinline__ float icp_comb(float v, float ab, float w, float ac, float ap) {
#pragma clang fp contract(off)
    return __builtin_fmaf(ac, w, ab * v) - ap;
}

struct IcpShared {                                             // (the small members first: their addresses fit a DS instruction's 16-bit offset)
    double red[ICP_W * ICP_K], sum[ICP_K];                     // wave partials; the inlier sums of the last association
    double xf[12];                                             // R row-major, then t
    double svd[4][3][3];                                       // the one-lane solve works here, not in registers: H, G, U, V
    int wave_n[ICP_W];
    int stop;
    float vx[HAND_MAXN], vy[HAND_MAXN], vz[HAND_MAXN];
    ushort4 tri[HAND_MAXF];
    float4 ca[HAND_MAXF], cb[HAND_MAXF], cc[HAND_MAXF];        // corners of the listed triangles (icp.hip: the camera-facing ones); ca.w carries the face index
};

// closest point of the listed triangles to (px, py, pz): squared distance, the point and the face index (-1: the list is empty).
// BARY: also the weights (wa, wb, wc) of that triangle's corners in q = wa a + wb b + wc c: one-hot in a vertex region, the opposite corner's
// exactly 0 in an edge region, all in [0, 1].  They are kept beside (v, w) and feed nothing that the distance is made of, so both
// instantiations choose the same triangle and the same q.
template <bool BARY>
__device__ __forceinline__ void icp_walk(const IcpShared& s, int count, float px, float py, float pz, float& best, float& qx, float& qy, float& qz,
                                         int& face, float& wa, float& wb, float& wc) {
    best = 3.0e38f; qx = qy = qz = 0.f; face = -1;
    wa = wb = wc = 0.f;
    for (int j = 0; j < count; ++j) {
        const float4 a = s.ca[j], b = s.cb[j], c = s.cc[j];
        const float abx = b.x - a.x, aby = b.y - a.y, abz = b.z - a.z, acx = c.x - a.x, acy = c.y - a.y, acz = c.z - a.z;
        const float apx = px - a.x, apy = py - a.y, apz = pz - a.z;
        const float bpx = px - b.x, bpy = py - b.y, bpz = pz - b.z;
        const float cpx = px - c.x, cpy = py - c.y, cpz = pz - c.z;
        const float d1 = icp_dot(abx, aby, abz, apx, apy, apz), d2 = icp_dot(acx, acy, acz, apx, apy, apz);
        const float d3 = icp_dot(abx, aby, abz, bpx, bpy, bpz), d4 = icp_dot(acx, acy, acz, bpx, bpy, bpz);
        const float d5 = icp_dot(abx, aby, abz, cpx, cpy, cpz), d6 = icp_dot(acx, acy, acz, cpx, cpy, cpz);
        const float vc = geo_det2(d1, d4, d3, d2), vb = geo_det2(d5, d2, d1, d6), va = geo_det2(d3, d6, d5, d4);
        // q = a + v ab + w ac; the face first, then the regions from the last of the order to the first, so the first that holds wins
        const float inv = __frcp_rn(fmaxf(va + vb + vc, ICP_TINY));
        float v = fminf(fmaxf(vb * inv, 0.f), 1.f), w = fminf(fmaxf(vc * inv, 0.f), 1.f);
        bool near_a = true;                                    // a carries weight: false on edge BC and at the vertices B and C
        if (va <= 0.f && d4 - d3 >= 0.f && d5 - d6 >= 0.f) {                                   // edge BC
            w = fminf((d4 - d3) * __frcp_rn(fmaxf((d4 - d3) + (d5 - d6), ICP_TINY)), 1.f);
            v = 1.f - w;
            near_a = false;
        }
        if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f) { v = 0.f; w = fminf(d2 * __frcp_rn(fmaxf(d2 - d6, ICP_TINY)), 1.f); near_a = true; }      // edge AC
        if (d6 >= 0.f && d5 <= d6) { v = 0.f; w = 1.f; near_a = false; }                       // vertex C
        if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f) { v = fminf(d1 * __frcp_rn(fmaxf(d1 - d3, ICP_TINY)), 1.f); w = 0.f; near_a = true; }      // edge AB
        if (d3 >= 0.f && d4 <= d3) { v = 1.f; w = 0.f; near_a = false; }                       // vertex B
        if (d1 <= 0.f && d2 <= 0.f) { v = 0.f; w = 0.f; near_a = true; }                       // vertex A
        const float rx = icp_comb(v, abx, w, acx, apx), ry = icp_comb(v, aby, w, acy, apy), rz = icp_comb(v, abz, w, acz, apz);      // q - p
        const float dd = icp_dot(rx, ry, rz, rx, ry, rz);
        if (dd < best) {
            best = dd; qx = px + rx; qy = py + ry; qz = pz + rz; face = __float_as_int(a.w);
            if (BARY) { wa = near_a ? fmaxf(1.f - v - w, 0.f) : 0.f; wb = v; wc = w; }        // (1 - (1 - w) - w is not 0 for every w: hence near_a)
        }
    }
}

// Gather of corner gradients without atomics, for a kernel whose lane t holds a query with its closest point q = wa a + wb b + wc c on
// triangle `face` of s.tri (-1: the query contributes nothing) and a vector (gx, gy, gz) that corner k of the triangle receives w_k times.
// The corner list is dead (the caller's block sum has ended in a barrier), so lane t < records writes its record over the head of the list:
// s.ca[t] = (wa, wb, wc, corner indices 0 and 1 as 16-bit halves), s.cb[t] = (g, corner index 2); no face writes the index 0xffff, which is
// no vertex.  Behind a barrier lane t < n reads the records front to back, every lane the same record (two broadcast 16-byte reads), and
// adds those that name vertex t, in double, in ascending record order.  Returns that sum (0 for a lane t >= n).  Every lane of the block calls.
__device__ __forceinline__ double3 geo_corner_gather(IcpShared& s, float wa, float wb, float wc, float gx, float gy, float gz, int face, int records,
                                                     int n) {
    const int t = threadIdx.x;
    if (t < records) {
        ushort4 f = make_ushort4(0xffff, 0xffff, 0xffff, 0);
        if (face >= 0) f = s.tri[face];                        // face < Fc: it came out of the list
        s.ca[t] = make_float4(wa, wb, wc, __int_as_float((int)f.x | ((int)f.y << 16)));
        s.cb[t] = make_float4(gx, gy, gz, __int_as_float((int)f.z));
    }
    __syncthreads();
    double sx = 0.0, sy = 0.0, sz = 0.0;
    if (t < n) {
        for (int j = 0; j < records; ++j) {
            const float4 ra = s.ca[j], rb = s.cb[j];
            const int i01 = __float_as_int(ra.w), i2 = __float_as_int(rb.w);
            if ((i01 & 0xffff) == t) { sx += (double)(ra.x * rb.x); sy += (double)(ra.x * rb.y); sz += (double)(ra.x * rb.z); }
            if (((i01 >> 16) & 0xffff) == t) { sx += (double)(ra.y * rb.x); sy += (double)(ra.y * rb.y); sz += (double)(ra.y * rb.z); }
            if (i2 == t) { sx += (double)(ra.z * rb.x); sy += (double)(ra.z * rb.y); sz += (double)(ra.z * rb.z); }
        }
    }
    return make_double3(sx, sy, sz);
}

// geo_corner_gather with a fourth sum and exact products: .x .y .z = the sum of w_k g with every product taken in double (exact: two fp32
// factors), added in double in ascending record order, and .w = the sum of the weights w_k themselves over the records that name vertex t.
// A query with face = -1 adds to neither.
__device__ __forceinline__ double4 geo_corner_gather_w(IcpShared& s, float wa, float wb, float wc, float gx, float gy, float gz, int face,
                                                       int records, int n) {
    const int t = threadIdx.x;
    if (t < records) {
        ushort4 f = make_ushort4(0xffff, 0xffff, 0xffff, 0);
        if (face >= 0) f = s.tri[face];                        // face < Fc: it came out of the list
        s.ca[t] = make_float4(wa, wb, wc, __int_as_float((int)f.x | ((int)f.y << 16)));
        s.cb[t] = make_float4(gx, gy, gz, __int_as_float((int)f.z));
    }
    __syncthreads();
    double sx = 0.0, sy = 0.0, sz = 0.0, sw = 0.0;
    if (t < n) {
        for (int j = 0; j < records; ++j) {
            const float4 ra = s.ca[j], rb = s.cb[j];
            const int i01 = __float_as_int(ra.w), i2 = __float_as_int(rb.w);
            if ((i01 & 0xffff) == t) { sx += (double)ra.x * (double)rb.x; sy += (double)ra.x * (double)rb.y; sz += (double)ra.x * (double)rb.z; sw += (double)ra.x; }
            if (((i01 >> 16) & 0xffff) == t) { sx += (double)ra.y * (double)rb.x; sy += (double)ra.y * (double)rb.y; sz += (double)ra.y * (double)rb.z; sw += (double)ra.y; }
            if (i2 == t) { sx += (double)ra.z * (double)rb.x; sy += (double)ra.z * (double)rb.y; sz += (double)ra.z * (double)rb.z; sw += (double)ra.z; }
        }
    }
    return make_double4(sx, sy, sz, sw);
}
