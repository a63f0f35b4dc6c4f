// What the kernels that compare the hand meshes with the sensor point cloud share (icp.hip, meshcloud.hip): the workgroup shape, the
// separately rounded forms of the facing test, and the fixed-order block sum.  The functions were moved here from icp.hip unchanged.
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
