// What the kernels that compare the hand meshes with the sensor point cloud share (icp.hip, meshcloud.hip): the workgroup shape, the
// separately rounded forms of the facing test, and the fixed-order block sum; and, with penetration.hip, the workgroup's LDS layout and the
// closest-point walk.  The functions were moved here from icp.hip unchanged.
#pragma once
#include "common.h"
#include "svd3.h"                                               // wave_sum_d

#define ICP_T 1024
#define ICP_W (ICP_T / 64)
#define ICP_MAXN 1024
#define ICP_MAXF 2048
#define ICP_MAXP 1024

// p q - r s from separately rounded products (no fma): the normal of a triangle with two equal corners, or with collinear corners whose
// edges are exact multiples of each other, is exactly zero
__device__ __forceinline__ float icp_det2(float p, float q, float r, float s) {
#pragma clang fp contract(off)
    return p * q - r * s;
}

// The association is written with its fused multiply-adds spelled out and contraction off, so that every kernel that inlines it rounds alike
// whatever the compiler makes of the code around it: with contraction left to the compiler two kernels chose different operands to fuse,
// and a near-tie between two triangles then fell to different sides.  The forms are the ones mesh_icp_kernel has always run.
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

// v[0..K) summed over the block in a fixed order -> out[0..K) in LDS (ends in a barrier): the xor butterfly per wave, then thread k
// adds the 16 wave partials of sum k as a balanced tree
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

// ---- the closest-point walk (shared by icp.hip and penetration.hip; moved here from icp.hip unchanged) ------------------------------------
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
    float vx[ICP_MAXN], vy[ICP_MAXN], vz[ICP_MAXN];
    ushort4 tri[ICP_MAXF];
    float4 ca[ICP_MAXF], cb[ICP_MAXF], cc[ICP_MAXF];           // corners of the listed triangles (icp.hip: the camera-facing ones); ca.w carries the face index
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
        const float vc = icp_det2(d1, d4, d3, d2), vb = icp_det2(d5, d2, d1, d6), va = icp_det2(d3, d6, d5, d4);
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
