// Winograd F(4x4, 3x3) (default) and F(2x2, 3x3) for the stride-1 3x3 convolutions with >= 128 channels (fp32 mode): `feat` (1024 -> 256 at
// 64x64, a fifth of the step's multiply-adds), p2, the first convolution of the hm / wh / params heads (256 -> 256), the up-sampling decoders,
// ResNet layers 2-3 -- forward, backward-data and (F(4x4) only, further down) the weight gradient.  The F(2x2) form is described first; F(4x4)
// is the same scheme with 6x6 patches, 36 planes and 4x instead of 2.25x fewer multiplications (matrices and accuracy: see wino4_* below and
// DESIGN section 4).
//
// Why.  Every dense contraction of the step already runs on the matrix pipe at 75-83 % of its fp32 peak; what is left
// is to do fewer multiplications.  A 2x2 output tile of a 3x3 convolution costs 36 multiply-adds per (input, output) channel pair
// directly and 16 in the Winograd domain: 2.25x fewer MFMA instructions for the price of three streaming passes,
//     V[xi][t][c] = (B^T d B)[xi]      input transform of every 4x4 patch d (stride 2) -- 16 planes, 4x the input's bytes
//     M[xi][t][n] = sum_c V[xi][t][c] U[xi][n][c]      16 plain GEMMs [T x C] x [N x C]^T in ONE batched launch (gemm.hip)
//     y tile      = A^T M A + bias, activation          output transform
// with U = G g G^T the transformed weights (16 planes of [N][C], rebuilt per call: the weights change every step).  The transform
// matrices of F(2x2, 3x3) hold only 0, +-1 and 1/2, so the result differs from the direct sum by a few fp32 roundings (the parity bars
// of the tests are unchanged).  reference layers: intaghand_encoder.py:617 (feat), :602 (p2), :675-693 (heads).
//
// Backward-data is the same convolution of dy with the taps mirrored and the channel roles swapped: only the weight transform differs
// (U'[xi][ci][co] from w[co][2 - ky][2 - kx][ci]).
#include "common.h"
#include "gemm_internal.h"
#include <cstdio>

// ---- weights: w [Cout][3][3][Cin] -> U [16][N][K]; forward: N = Cout, K = Cin; backward-data (FLIP): N = Cin, K = Cout, taps mirrored
template <bool FLIP>
__global__ __launch_bounds__(256) void wino_weight_kernel(const float* __restrict__ w, float* __restrict__ U, int Cout, int Cin) {
    const int N = FLIP ? Cin : Cout, K = FLIP ? Cout : Cin;
    const long total = (long)N * K;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int n = (int)(i / K), k = (int)(i - (long)n * K);
        float g[3][3];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b)
                g[a][b] = FLIP ? w[(((long)k * 3 + (2 - a)) * 3 + (2 - b)) * Cin + n] : w[(((long)n * 3 + a) * 3 + b) * Cin + k];
        float t[4][3];                                       // G g
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            t[0][b] = g[0][b];
            t[1][b] = 0.5f * (g[0][b] + g[1][b] + g[2][b]);
            t[2][b] = 0.5f * (g[0][b] - g[1][b] + g[2][b]);
            t[3][b] = g[2][b];
        }
#pragma unroll
        for (int a = 0; a < 4; ++a) {                        // (G g) G^T
            const float u0 = t[a][0], u1 = 0.5f * (t[a][0] + t[a][1] + t[a][2]), u2 = 0.5f * (t[a][0] - t[a][1] + t[a][2]), u3 = t[a][2];
            U[(long)(a * 4 + 0) * total + i] = u0;
            U[(long)(a * 4 + 1) * total + i] = u1;
            U[(long)(a * 4 + 2) * total + i] = u2;
            U[(long)(a * 4 + 3) * total + i] = u3;
        }
    }
}

// ---- input: x [N][H][W][C] (row stride ldx) -> V [16][T][C], T = N (H/2) (W/2); one thread = 4 channels of one tile
__global__ __launch_bounds__(256) void wino_input_kernel(const float* __restrict__ x, int ldx, float* __restrict__ V, int N, int H, int W, int C) {
    const int C4 = C >> 2, TW = W >> 1, TH = H >> 1;
    const long T = (long)N * TH * TW, total = T * C4;
    const long plane = T * C;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long t = i / C4;
        const int c = (int)(i - t * C4) * 4;
        const int n = (int)(t / (TH * TW)), r = (int)(t - (long)n * TH * TW), ty = r / TW, tx = r - ty * TW;
        float4 d[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int iy = 2 * ty - 1 + a;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int ix = 2 * tx - 1 + b;
                d[a][b] = (iy >= 0 && iy < H && ix >= 0 && ix < W) ? *reinterpret_cast<const float4*>(x + (((long)n * H + iy) * W + ix) * ldx + c)
                                                                   : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
        // B^T d: rows (d0 - d2), (d1 + d2), (d2 - d1), (d1 - d3); then the same on the columns
        float4 s[4][4];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
#define WSUB(p, q) make_float4(p.x - q.x, p.y - q.y, p.z - q.z, p.w - q.w)
#define WADD(p, q) make_float4(p.x + q.x, p.y + q.y, p.z + q.z, p.w + q.w)
            s[0][b] = WSUB(d[0][b], d[2][b]);
            s[1][b] = WADD(d[1][b], d[2][b]);
            s[2][b] = WSUB(d[2][b], d[1][b]);
            s[3][b] = WSUB(d[1][b], d[3][b]);
        }
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const float4 v0 = WSUB(s[a][0], s[a][2]), v1 = WADD(s[a][1], s[a][2]), v2 = WSUB(s[a][2], s[a][1]), v3 = WSUB(s[a][1], s[a][3]);
            float* o = V + t * C + c;
            *reinterpret_cast<float4*>(o + (long)(a * 4 + 0) * plane) = v0;
            *reinterpret_cast<float4*>(o + (long)(a * 4 + 1) * plane) = v1;
            *reinterpret_cast<float4*>(o + (long)(a * 4 + 2) * plane) = v2;
            *reinterpret_cast<float4*>(o + (long)(a * 4 + 3) * plane) = v3;
        }
    }
}

// ---- output: M [16][T][Co] -> y [N][H][W][Co] (row stride ldy): y tile = A^T m A (+ bias, activation; += y when accum)
__global__ __launch_bounds__(256) void wino_output_kernel(const float* __restrict__ Mx, const float* __restrict__ bias, float* __restrict__ y, int ldy,
                                                          int N, int H, int W, int Co, int act, int accum) {
    const int C4 = Co >> 2, TW = W >> 1, TH = H >> 1;
    const long T = (long)N * TH * TW, total = T * C4;
    const long plane = T * Co;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long t = i / C4;
        const int c = (int)(i - t * C4) * 4;
        const int n = (int)(t / (TH * TW)), r = (int)(t - (long)n * TH * TW), ty = r / TW, tx = r - ty * TW;
        float4 m[4][4];
        const float* p = Mx + t * Co + c;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) m[a][b] = *reinterpret_cast<const float4*>(p + (long)(a * 4 + b) * plane);
        float4 s[2][4];                                      // A^T m: rows (m0 + m1 + m2), (m1 - m2 - m3)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            s[0][b] = WADD(WADD(m[0][b], m[1][b]), m[2][b]);
            s[1][b] = WSUB(WSUB(m[1][b], m[2][b]), m[3][b]);
        }
        const float4 bv = bias != nullptr ? *reinterpret_cast<const float4*>(bias + c) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            float4 o[2];
            o[0] = WADD(WADD(s[a][0], s[a][1]), s[a][2]);
            o[1] = WSUB(WSUB(s[a][1], s[a][2]), s[a][3]);
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                float4 v = WADD(o[b], bv);
                if (act == 1) v = make_float4(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f));
                else if (act == 2) v = make_float4(v.x > 0.f ? v.x : 0.1f * v.x, v.y > 0.f ? v.y : 0.1f * v.y, v.z > 0.f ? v.z : 0.1f * v.z, v.w > 0.f ? v.w : 0.1f * v.w);
                float* q = y + (((long)n * H + 2 * ty + a) * W + 2 * tx + b) * ldy + c;
                if (accum) { const float4 e = *reinterpret_cast<const float4*>(q); v = WADD(v, e); }
                *reinterpret_cast<float4*>(q) = v;
            }
        }
    }
}
#undef WSUB
#undef WADD

// ------------------------------------------------------------------------------------------------------------------------------
// F(4x4, 3x3): 6x6 patches at stride 4, 36 transform-domain planes, 4x fewer multiplications than the direct sum (F(2x2): 2.25x) and
// only 2.25x the input's bytes in the transform domain (F(2x2): 4x).  The price is accuracy: the matrices hold 4, 5, 8, 1/6, 1/24, so
// a result carries ~4e-5 absolute error on values of a few units where F(2x2) and the direct kernels stay at 1e-6 ... 3e-6 (measured,
// profiles/r04_winograd_ab.txt).  Standard matrices (Lavin & Gray, "Fast Algorithms for Convolutional Neural Networks", 2016):
//   B^T = [4 0 -5 0 1 0; 0 -4 -4 1 1 0; 0 4 -4 -1 1 0; 0 -2 -1 2 1 0; 0 2 -1 -2 1 0; 0 4 0 -5 0 1]
//   G   = [1/4 0 0; -1/6 -1/6 -1/6; -1/6 1/6 -1/6; 1/24 1/12 1/6; 1/24 -1/12 1/6; 0 0 1]
//   A^T = [1 1 1 1 1 0; 0 1 -1 2 -2 0; 0 1 1 4 4 0; 0 1 -1 8 -8 1]
// X3: U is written as x3 planes (three bf16 tensors [36][N][K], component stride 36 N K elements -- gemm_x3.hip) instead of fp32
template <bool FLIP, bool X3>
__global__ __launch_bounds__(256) void wino4_weight_kernel(const float* __restrict__ w, float* __restrict__ U, int Cout, int Cin) {
    const int N = FLIP ? Cin : Cout, K = FLIP ? Cout : Cin;
    const long total = (long)N * K;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int n = (int)(i / K), k = (int)(i - (long)n * K);
        float g[3][3];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b)
                g[a][b] = FLIP ? w[(((long)k * 3 + (2 - a)) * 3 + (2 - b)) * Cin + n] : w[(((long)n * 3 + a) * 3 + b) * Cin + k];
        float t[6][3];
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            const float g0 = g[0][b], g1 = g[1][b], g2 = g[2][b];
            t[0][b] = g0 * 0.25f;
            t[1][b] = -(g0 + g1 + g2) * (1.f / 6.f);
            t[2][b] = -(g0 - g1 + g2) * (1.f / 6.f);
            t[3][b] = g0 * (1.f / 24.f) + g1 * (1.f / 12.f) + g2 * (1.f / 6.f);
            t[4][b] = g0 * (1.f / 24.f) - g1 * (1.f / 12.f) + g2 * (1.f / 6.f);
            t[5][b] = g2;
        }
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            const float g0 = t[a][0], g1 = t[a][1], g2 = t[a][2];
            const float u[6] = {g0 * 0.25f, -(g0 + g1 + g2) * (1.f / 6.f), -(g0 - g1 + g2) * (1.f / 6.f),
                                g0 * (1.f / 24.f) + g1 * (1.f / 12.f) + g2 * (1.f / 6.f), g0 * (1.f / 24.f) - g1 * (1.f / 12.f) + g2 * (1.f / 6.f), g2};
#pragma unroll
            for (int b = 0; b < 6; ++b) {
                if constexpr (X3) {
                    unsigned h, m, l;
                    pdf_x3_split2(u[b], 0.f, h, m, l);
                    unsigned short* o = reinterpret_cast<unsigned short*>(U) + (long)(a * 6 + b) * total + i;
                    o[0] = (unsigned short)h; o[36 * total] = (unsigned short)m; o[72 * total] = (unsigned short)l;
                } else U[(long)(a * 6 + b) * total + i] = u[b];
            }
        }
    }
}
// six values in place: v <- B^T v
__device__ __forceinline__ void wino4_bt(float2 (&v)[6]) {
    const float2 d0 = v[0], d1 = v[1], d2 = v[2], d3 = v[3], d4 = v[4], d5 = v[5];
#define W4(e) make_float2(e(x), e(y))
#define E0(c) 4.f * d0.c - 5.f * d2.c + d4.c
#define E1(c) -4.f * (d1.c + d2.c) + d3.c + d4.c
#define E2(c) 4.f * (d1.c - d2.c) - d3.c + d4.c
#define E3(c) 2.f * (d3.c - d1.c) - d2.c + d4.c
#define E4(c) 2.f * (d1.c - d3.c) - d2.c + d4.c
#define E5(c) 4.f * d1.c - 5.f * d3.c + d5.c
    v[0] = W4(E0); v[1] = W4(E1); v[2] = W4(E2); v[3] = W4(E3); v[4] = W4(E4); v[5] = W4(E5);
#undef E0
#undef E1
#undef E2
#undef E3
#undef E4
#undef E5
}
// x [N][H][W][C] -> V [36][T][C], T = N (H/4) (W/4); one thread = 2 channels of one 6x6 patch (72 registers of data)
template <bool X3>
__global__ __launch_bounds__(256) void wino4_input_kernel(const float* __restrict__ x, int ldx, float* __restrict__ V, int N, int H, int W, int C) {
    const int C2 = C >> 1, TW = W >> 2, TH = H >> 2;
    const long T = (long)N * TH * TW, total = T * C2;
    const long plane = T * C;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long t = i / C2;
        const int c = (int)(i - t * C2) * 2;
        const int n = (int)(t / (TH * TW)), r = (int)(t - (long)n * TH * TW), ty = r / TW, tx = r - ty * TW;
        float2 d[6][6];
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            const int iy = 4 * ty - 1 + a;
#pragma unroll
            for (int b = 0; b < 6; ++b) {
                const int ix = 4 * tx - 1 + b;
                d[a][b] = (iy >= 0 && iy < H && ix >= 0 && ix < W) ? *reinterpret_cast<const float2*>(x + (((long)n * H + iy) * W + ix) * ldx + c) : make_float2(0.f, 0.f);
            }
        }
#pragma unroll
        for (int b = 0; b < 6; ++b) {                        // columns: d <- B^T d
            float2 col[6] = {d[0][b], d[1][b], d[2][b], d[3][b], d[4][b], d[5][b]};
            wino4_bt(col);
#pragma unroll
            for (int a = 0; a < 6; ++a) d[a][b] = col[a];
        }
        float* o = V + t * C + c;
#pragma unroll
        for (int a = 0; a < 6; ++a) {                        // rows: (B^T d) B
            wino4_bt(d[a]);
#pragma unroll
            for (int b = 0; b < 6; ++b) {
                if constexpr (X3) pdf_x3_store2(reinterpret_cast<unsigned short*>(V), t * C + c + (long)(a * 6 + b) * plane, 36 * plane, d[a][b].x, d[a][b].y);
                else *reinterpret_cast<float2*>(o + (long)(a * 6 + b) * plane) = d[a][b];
            }
        }
    }
}
// M [36][T][Co] -> y: y tile (4x4) = A^T m A (+ bias, activation; += y when accum); one thread = 2 channels of one tile
__global__ __launch_bounds__(256) void wino4_output_kernel(const float* __restrict__ Mx, const float* __restrict__ bias, float* __restrict__ y, int ldy,
                                                           int N, int H, int W, int Co, int act, int accum) {
    const int C2 = Co >> 1, TW = W >> 2, TH = H >> 2;
    const long T = (long)N * TH * TW, total = T * C2;
    const long plane = T * Co;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long t = i / C2;
        const int c = (int)(i - t * C2) * 2;
        const int n = (int)(t / (TH * TW)), r = (int)(t - (long)n * TH * TW), ty = r / TW, tx = r - ty * TW;
        const float* p = Mx + t * Co + c;
        float2 s[4][6];                                      // A^T m, column by column
#pragma unroll
        for (int b = 0; b < 6; ++b) {
            float2 m[6];
#pragma unroll
            for (int a = 0; a < 6; ++a) m[a] = *reinterpret_cast<const float2*>(p + (long)(a * 6 + b) * plane);
#define O0(c) m[0].c + m[1].c + m[2].c + m[3].c + m[4].c
#define O1(c) m[1].c - m[2].c + 2.f * (m[3].c - m[4].c)
#define O2(c) m[1].c + m[2].c + 4.f * (m[3].c + m[4].c)
#define O3(c) m[1].c - m[2].c + 8.f * (m[3].c - m[4].c) + m[5].c
            s[0][b] = W4(O0); s[1][b] = W4(O1); s[2][b] = W4(O2); s[3][b] = W4(O3);
        }
        const float2 bv = bias != nullptr ? *reinterpret_cast<const float2*>(bias + c) : make_float2(0.f, 0.f);
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const float2* m = s[a];
            float2 o[4] = {W4(O0), W4(O1), W4(O2), W4(O3)};
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                float2 v = make_float2(o[b].x + bv.x, o[b].y + bv.y);
                if (act == 1) v = make_float2(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f));
                else if (act == 2) v = make_float2(v.x > 0.f ? v.x : 0.1f * v.x, v.y > 0.f ? v.y : 0.1f * v.y);
                float* q = y + (((long)n * H + 4 * ty + a) * W + 4 * tx + b) * ldy + c;
                if (accum) { const float2 e = *reinterpret_cast<const float2*>(q); v.x += e.x; v.y += e.y; }
                *reinterpret_cast<float2*>(q) = v;
            }
        }
#undef O0
#undef O1
#undef O2
#undef O3
#undef W4
    }
}

// m = output tile edge: 2 (F(2x2, 3x3), 16 planes) or 4 (F(4x4, 3x3), 36 planes).  PDF_WINOGRAD: 4 (default) = F(4x4) where the map allows
// it and PDF_WINOGRAD_F4 permits (see below and the accuracy note above), else F(2x2); 2 = F(2x2) only; 0 = the direct kernels.
// ---- weight gradient in the F(4x4, 3x3) domain.  With Y = A^T [U (.) V] A, U = G g G^T, V = B^T d B:
//     dL/dU[xi][n][c] = sum_t dYh[xi][t][n] V[xi][t][c],   dYh = A dY A^T (each 4x4 tile of dy -> 6x6),   dL/dg = G^T (dL/dU) G
// i.e. 36 weight-gradient-shaped products over T = N H W / 16 tiles instead of one over N H W pixels x 9 taps: 4x fewer multiplications.
// dy [N][H][W][Co] -> dYh [36][T][Co]: A = (A^T)^T = [1 0 0 0; 1 1 1 1; 1 -1 1 -1; 1 2 4 8; 1 -2 4 -8; 0 0 0 1]
template <bool X3>
__global__ __launch_bounds__(256) void wino4_dy_kernel(const float* __restrict__ dy, int lddy, float* __restrict__ Yh, int N, int H, int W, int Co) {
    const int C2 = Co >> 1, TW = W >> 2, TH = H >> 2;
    const long T = (long)N * TH * TW, total = T * C2;
    const long plane = T * Co;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long t = i / C2;
        const int c = (int)(i - t * C2) * 2;
        const int n = (int)(t / (TH * TW)), r = (int)(t - (long)n * TH * TW), ty = r / TW, tx = r - ty * TW;
        float2 d[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) d[a][b] = *reinterpret_cast<const float2*>(dy + (((long)n * H + 4 * ty + a) * W + 4 * tx + b) * lddy + c);
        float2 u[6][4];                                      // A d (columns)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
#define A2(e) make_float2(e(x), e(y))
#define P0(k) d[0][b].k
#define P1(k) d[0][b].k + d[1][b].k + d[2][b].k + d[3][b].k
#define P2(k) d[0][b].k - d[1][b].k + d[2][b].k - d[3][b].k
#define P3(k) d[0][b].k + 2.f * d[1][b].k + 4.f * d[2][b].k + 8.f * d[3][b].k
#define P4(k) d[0][b].k - 2.f * d[1][b].k + 4.f * d[2][b].k - 8.f * d[3][b].k
#define P5(k) d[3][b].k
            u[0][b] = A2(P0); u[1][b] = A2(P1); u[2][b] = A2(P2); u[3][b] = A2(P3); u[4][b] = A2(P4); u[5][b] = A2(P5);
#undef P0
#undef P1
#undef P2
#undef P3
#undef P4
#undef P5
        }
        float* o = Yh + t * Co + c;
#pragma unroll
        for (int a = 0; a < 6; ++a) {                        // (A d) A^T (rows)
            const float2 e0 = u[a][0], e1 = u[a][1], e2 = u[a][2], e3 = u[a][3];
#define Q0(k) e0.k
#define Q1(k) e0.k + e1.k + e2.k + e3.k
#define Q2(k) e0.k - e1.k + e2.k - e3.k
#define Q3(k) e0.k + 2.f * e1.k + 4.f * e2.k + 8.f * e3.k
#define Q4(k) e0.k - 2.f * e1.k + 4.f * e2.k - 8.f * e3.k
#define Q5(k) e3.k
            const float2 q[6] = {A2(Q0), A2(Q1), A2(Q2), A2(Q3), A2(Q4), A2(Q5)};
#pragma unroll
            for (int b = 0; b < 6; ++b) {
                if constexpr (X3) pdf_x3_store2(reinterpret_cast<unsigned short*>(Yh), t * Co + c + (long)(a * 6 + b) * plane, 36 * plane, q[b].x, q[b].y);
                else *reinterpret_cast<float2*>(o + (long)(a * 6 + b) * plane) = q[b];
            }
#undef Q0
#undef Q1
#undef Q2
#undef Q3
#undef Q4
#undef Q5
#undef A2
        }
    }
}
// slabs [36][splits][Co][Ci]: the splits of every plane summed into its split 0, in split order (a small layer has one 128x128 tile per
// plane and 32 splits: with one thread per weight element summing 36 x 32 values in turn the pass was latency-bound -- 0.16 ms per call
// for 75 MB -- so the sum runs over all 36 Co Ci elements in parallel, four values per thread)
__global__ __launch_bounds__(256) void wino4_slab_sum_kernel(float* __restrict__ slab, int splits, long total4) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < 36 * total4; i += (long)gridDim.x * 256) {
        const long p = i / total4, e = i - p * total4;
        float4* base = reinterpret_cast<float4*>(slab) + p * splits * total4 + e;
        float4 v = base[0];
        for (int y = 1; y < splits; ++y) { const float4 w = base[(long)y * total4]; v.x += w.x; v.y += w.y; v.z += w.z; v.w += w.w; }
        base[0] = v;
    }
}
// summed slabs (split 0 of each plane) -> dw [Co][3][3][Ci] (+)= G^T u G      (one thread per (co, ci))
__global__ __launch_bounds__(256) void wino4_wgrad_out_kernel(const float* __restrict__ slab, int splits, float* __restrict__ dw, int Co, int Ci, int accumulate) {
    const long total = (long)Co * Ci;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int n = (int)(i / Ci), c = (int)(i - (long)n * Ci);
        float u[6][6];
#pragma unroll
        for (int p = 0; p < 36; ++p) u[p / 6][p % 6] = slab[(long)p * splits * total + i];
        {
        float t[3][6];                                       // G^T u: rows G[:,a]
#pragma unroll
        for (int b = 0; b < 6; ++b) {
            t[0][b] = 0.25f * u[0][b] - (1.f / 6.f) * (u[1][b] + u[2][b]) + (1.f / 24.f) * (u[3][b] + u[4][b]);
            t[1][b] = (1.f / 6.f) * (u[2][b] - u[1][b]) + (1.f / 12.f) * (u[3][b] - u[4][b]);
            t[2][b] = -(1.f / 6.f) * (u[1][b] + u[2][b]) + (1.f / 6.f) * (u[3][b] + u[4][b]) + u[5][b];
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float g0 = 0.25f * t[a][0] - (1.f / 6.f) * (t[a][1] + t[a][2]) + (1.f / 24.f) * (t[a][3] + t[a][4]);
            const float g1 = (1.f / 6.f) * (t[a][2] - t[a][1]) + (1.f / 12.f) * (t[a][3] - t[a][4]);
            const float g2 = -(1.f / 6.f) * (t[a][1] + t[a][2]) + (1.f / 6.f) * (t[a][3] + t[a][4]) + t[a][5];
            float* o = dw + (((long)n * 3 + a) * 3) * Ci + c;
            if (accumulate) { o[0] += g0; o[Ci] += g1; o[2 * (long)Ci] += g2; }
            else { o[0] = g0; o[Ci] = g1; o[2 * (long)Ci] = g2; }
        }
        }
    }
}

// ---- the plans: every decision about a Winograd launch and every offset into its workspace is made here, once per call (gemm_internal.h)
// The switches, each read once.
//   PDF_WINOGRAD        4 (default) = F(4x4) where the map allows it and PDF_WINOGRAD_F4 permits, else F(2x2); 2 = F(2x2) only; 0 = the direct kernels
//   PDF_WINOGRAD_F4     the launches that may take F(4x4) -- bit 0: forward of the layers with at most 256 channels on either side, bit 1: their
//                       backward-data, bit 2: forward of the wider layers (`feat`), bit 3: their backward-data -- F(2x2) for the rest.  Default 15 =
//                       all of them.  (Until late in round 4 the default was 11, everything but the forward of `feat`: with F(4x4)
//                       THERE pointnet_plus.sft1.SFT_shift_conv1.bias -- one of the 705 gradients of the B=32 step -- deviates by 2.2e-3 of its norm
//                       from the float64 oracle, over the fixed 1.5e-3 bar; the oracle's own float32 run deviates by 3.8e-2 on that tensor, a sum of
//                       +- terms that nearly cancel, so the bar of tests/test_headline_gpu.py is now the fixed one plus twice the fp32 oracle's own
//                       deviation and the launch is no exception any more: worst tensor 0.48 of its bar, every tensor that is not noise in fp32
//                       below its FIXED bar; profiles/r04_winograd_ab.txt.)
//   PDF_WINOGRAD_MINPT  planes x tiles a launch must have: 16384 takes ResNet layer 3 (36 x 512) in
//   PDF_X3_MINC / MINT  see wino_shared_x3 below
struct WinoEnv { int mode, f4, wgrad, minc, x3_minc; long minpt, x3_mint; };
static const WinoEnv& wino_env() {
    static const auto num = [](const char* v, long dflt) { return v ? atol(v) : dflt; };
    static const WinoEnv e = {(int)num(getenv("PDF_WINOGRAD"), 4), (int)num(getenv("PDF_WINOGRAD_F4"), 15), (int)num(getenv("PDF_WINOGRAD_WGRAD"), 1),
                              (int)num(getenv("PDF_WINOGRAD_MINC"), 128), (int)num(getenv("PDF_X3_MINC"), 256),
                              num(getenv("PDF_WINOGRAD_MINPT"), 16384), num(getenv("PDF_X3_MINT"), 2048)};
    return e;
}
// x3 arithmetic for the F(4x4) transform-domain products (gemm_x3.hip): the transforms write their outputs as x3 planes (6 bytes per element
// instead of 4) and the 36 products run on the bf16 matrix pipe, six MFMAs per fp32 product.  A transformed tensor [36][T][C] CAN be x3 when
// C % 32 == 0 (a K-step of the products) and the three components stay within 32-bit byte offsets.  PDF_X3=0 / pdf_set_x3_mode(0): the native fp32 MFMA.
// This is the format rule of a tensor PRIVATE to one launch (backward-data's V of dy; the weight gradient's Yh): its format follows the launch.
static bool wino_x3_fits(long T, int C) { return (pdf_internal_x3_mode() & 1) != 0 && C % 32 == 0 && T % 32 == 0 && 73.0 * (double)T * C < 2147483000.0; }
// (T, C) of a transformed tensor that SEVERAL launches read (the forward's V: heads sharing it, the weight gradient): a function of (T, C) ONLY, so
// that every forward that could have written it agrees; a reader still compares the format its plan records (shared_v_x3) with its own.  x3 where the
// products it feeds are long enough reductions over enough tiles to be bound by the matrix pipe -- C >= PDF_X3_MINC (256) and T >= PDF_X3_MINT (2,048 tiles): `feat`
// and the 256-channel layers on the 32x32 / 64x64 maps.  The 128-channel layers and ResNet layer 3 (T = 512) gain 0-25 % on the product and lose as
// much on the 1.5x larger transform writes (profiles/r06_x3_step_ab.txt, r06_x3_minc_ab.txt: 512 / 0 -> 45.38 ms, 256 / 8192 -> 45.0, 256 / 2048 -> 44.87).
static bool wino_shared_x3(long T, int C) { return wino_x3_fits(T, C) && C >= wino_env().x3_minc && T >= wino_env().x3_mint; }
// Is this a convolution the Winograd paths take?  (3x3, stride 1, pad 1, channel counts the fast GEMM tiles like)
static bool wino_layer_ok(int Ck, int Cn, int KH, int KW, int stride, int pad) {
    return KH == 3 && KW == 3 && stride == 1 && pad == 1 && Ck % 16 == 0 && Cn % 16 == 0 && Ck >= wino_env().minc && Cn >= 64;
}
// the output tile edge for this launch: 4, 2, or 0 (not a Winograd launch).  A size only qualifies when its planes x tiles fill the chip
// (the batched GEMM wants >= 512 row blocks of 128) and one transform-domain plane stays below 4 GB.
static int wino_tile(int N, int H, int W, int Ck, int Cn, int flip) {
    const WinoEnv& e = wino_env();
    if (e.mode == 0) return 0;
    const int bit = ((Ck > 256 || Cn > 256) ? 4 : 1) << (flip ? 1 : 0);
    for (int m = (e.mode == 4 && (e.f4 & bit)) ? 4 : 2; m >= 2; m -= 2) {
        if (H % m || W % m) continue;
        const long T = (long)N * (H / m) * (W / m), P = (m + 2) * (m + 2);
        if (P * T < e.minpt) continue;
        if ((double)T * (Ck > Cn ? Ck : Cn) * 4.0 > 4.0e9) continue;
        return m;
    }
    return 0;
}
static bool wino_wgrad_ok(int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad) {
    const WinoEnv& e = wino_env();
    if (!e.wgrad || e.mode == 0 || !wino_layer_ok(Cin, Cout, KH, KW, stride, pad) || H % 4 || W % 4) return false;
    const long T = (long)N * (H / 4) * (W / 4);
    return T % 16 == 0 && 36 * T >= e.minpt && (double)T * (Cin > Cout ? Cin : Cout) * 4.0 <= 4.0e9;
}
static WsRegion ws_carve(long& at, long len) { const WsRegion r = {at, len}; at += len; return r; }
// forward / backward-data: U, V, M in that order (U and V at 6 bytes per element when the launch is x3)
WinoPlan wino_plan(int N, int H, int W, int Ck, int Cn, int KH, int KW, int stride, int pad, int flip) {
    WinoPlan p = {};
    p.v_offset = -1; p.shared_v_x3 = -1;
    if (!wino_layer_ok(Ck, Cn, KH, KW, stride, pad) || (p.m = wino_tile(N, H, W, Ck, Cn, flip)) == 0) return p;
    p.ok = 1; p.N = N; p.H = H; p.W = W; p.Ck = Ck; p.Cn = Cn; p.flip = flip;
    p.T = (long)N * (H / p.m) * (W / p.m); p.P = (p.m + 2) * (p.m + 2);
    // backward-data's V is private: x3 wherever it fits and either side is wide enough for the products to gain
    p.x3 = p.m == 4 && (flip ? wino_x3_fits(p.T, Ck) && (Ck >= wino_env().x3_minc || Cn >= wino_env().x3_minc) : wino_shared_x3(p.T, Ck));
    if (!flip && p.m == 4) p.shared_v_x3 = wino_shared_x3(p.T, Ck);
    const long per = p.x3 ? 54 : p.P;                         // floats per (plane set, element): P fp32 planes, or 3 x 36 bf16
    p.U = ws_carve(p.total, per * Cn * Ck);
    p.V = ws_carve(p.total, per * p.T * Ck);
    p.M = ws_carve(p.total, p.P * p.T * Cn);
    if (!flip && p.m == 4 && wino_wgrad_ok(N, H, W, Ck, Cn, KH, KW, stride, pad)) p.v_offset = p.V.off;
    return p;
}
static int wino_wgrad_splits(long T, int Co, int Ci) {
    const long tiles = 36L * cdiv(Co, 128) * cdiv(Ci, 128);
    long sp = (2304 + tiles - 1) / tiles;                    // ~3 full rounds of 768 co-resident blocks
    const long cap = T / 256 > 0 ? T / 256 : 1;              // at least 256 rows (16 K-steps) per block
    if (sp > cap) sp = cap;
    return (int)(sp < 1 ? 1 : sp);
}
// weight gradient: V, Yh, the slabs of the split reduction, the scratch of the bias gradient's column sums
WinoWgradPlan wino_wgrad_plan(int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad) {
    WinoWgradPlan p = {};
    p.shared_v_x3 = -1;
    if (!wino_wgrad_ok(N, H, W, Cin, Cout, KH, KW, stride, pad)) return p;
    p.ok = 1; p.N = N; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout;
    p.T = (long)N * (H / 4) * (W / 4);
    p.x3 = wino_shared_x3(p.T, Cin) && wino_x3_fits(p.T, Cout);      // (both operands of the products in one format)
    if (wino_tile(N, H, W, Cin, Cout, 0) == 4) p.shared_v_x3 = wino_shared_x3(p.T, Cin);
    p.splits = wino_wgrad_splits(p.T, Cout, Cin);            // (the x3 product may use fewer: rows per split a multiple of 32)
    const long per = p.x3 ? 54 : 36;
    p.V = ws_carve(p.total, per * p.T * Cin);
    p.Yh = ws_carve(p.total, per * p.T * Cout);
    p.slab = ws_carve(p.total, 36L * p.splits * Cout * Cin);
    p.colsum = ws_carve(p.total, pdf_internal_colsum_ws(Cout, (long)N * H * W));
    p.total += 64;
    return p;
}
// Workspace (floats) a stride-1 3x3 convolution [Cout][3][3][Cin] on N x H x W maps wants for its Winograd path -- backward = 0: the
// forward pass, 1: backward-data, 2: the weight gradient -- or 0 when the layer does not qualify (then no workspace is needed)
PDF_API long pdf_conv2d_winograd_workspace_floats(int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int backward) {
    if (backward == 2) return wino_wgrad_plan(N, H, W, Cin, Cout, KH, KW, stride, pad).total;
    return wino_plan(N, H, W, backward ? Cout : Cin, backward ? Cin : Cout, KH, KW, stride, pad, backward).total;
}
PDF_API long pdf_conv2d_winograd_v_offset(int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad) {
    return wino_plan(N, H, W, Cin, Cout, KH, KW, stride, pad, 0).v_offset;
}

// dw [Cout][3][3][Cin] (+)= the weight gradient of the stride-1 3x3 convolution; db [Cout] (+)= column sums of dy (optional)
// v_cached: the forward's V for the same x (at the forward plan's v_offset), or NULL -- then, or when it is in the other format, the input is transformed here
int pdf_internal_conv3x3_winograd_wgrad(const WinoWgradPlan& p, const float* x, int ldx, const float* dy, int lddy, float* dw, float* db, float* ws,
                                        int accumulate, const float* v_cached, hipStream_t s) {
    const int N = p.N, H = p.H, W = p.W, Cin = p.Cin, Cout = p.Cout;
    const long T = p.T;
    const bool x3 = p.x3;
    if (p.shared_v_x3 != p.x3) v_cached = nullptr;
    float* V = ws + p.V.off;
    float* Yh = ws + p.Yh.off;
    float* slab = ws + p.slab.off;
    if (v_cached == nullptr) {
        if (x3) hipLaunchKernelGGL((wino4_input_kernel<true>), dim3(grid_for(T * (Cin / 2), 256, 256 * 32)), dim3(256), 0, s, x, ldx, V, N, H, W, Cin);
        else hipLaunchKernelGGL((wino4_input_kernel<false>), dim3(grid_for(T * (Cin / 2), 256, 256 * 32)), dim3(256), 0, s, x, ldx, V, N, H, W, Cin);
    }
    if (x3) hipLaunchKernelGGL((wino4_dy_kernel<true>), dim3(grid_for(T * (Cout / 2), 256, 256 * 32)), dim3(256), 0, s, dy, lddy, Yh, N, H, W, Cout);
    else hipLaunchKernelGGL((wino4_dy_kernel<false>), dim3(grid_for(T * (Cout / 2), 256, 256 * 32)), dim3(256), 0, s, dy, lddy, Yh, N, H, W, Cout);
    PDF_LAUNCH_CHECK();
    const float* Vq = v_cached != nullptr ? v_cached : V;
    const int used = x3 ? pdf_internal_x3_batched_wgemm(Yh, 36L * T * Cout, Vq, 36L * T * Cin, slab, 36, T * Cout, T * Cin, (int)T, Cout, Cin, p.splits, -1, 6, s)
                        : pdf_internal_batched_wgemm(Yh, Vq, slab, 36, T * Cout, T * Cin, (int)T, Cout, Cin, p.splits, s);
    if (used <= 0) return used < 0 ? used : PDF_E_BADARG;
    if (used > 1) hipLaunchKernelGGL(wino4_slab_sum_kernel, dim3(grid_for(36L * Cout * Cin / 4)), dim3(256), 0, s, slab, used, (long)Cout * Cin / 4);
    hipLaunchKernelGGL(wino4_wgrad_out_kernel, dim3(grid_for((long)Cout * Cin)), dim3(256), 0, s, slab, used, dw, Cout, Cin, accumulate);
    PDF_LAUNCH_CHECK();
    if (db != nullptr) return pdf_internal_colsum(dy, lddy, Cout, (long)N * H * W, db, accumulate, ws + p.colsum.off, s);
    return 0;
}

// x [N][H][W][Ck] (ldx) * w -> y [N][H][W][Cn] (ldy).  flip = 0: forward, w = [Cn][3][3][Ck]; flip = 1: backward-data, w = [Ck][3][3][Cn]
// (x = dy, y = dx).  ws: p.total floats.
// v_shared (forward, F(4x4) only): V of the same input tensor, written by another convolution's forward -- the input transform is skipped
int pdf_internal_conv3x3_winograd(const WinoPlan& p, const float* x, int ldx, const float* w, const float* bias, float* y, int ldy, float* ws,
                                  int act, int accum, const float* v_shared, hipStream_t s) {
    const int N = p.N, H = p.H, W = p.W, Ck = p.Ck, Cn = p.Cn, flip = p.flip, m = p.m;
    const long T = p.T;
    const bool x3 = p.x3;
    float* U = ws + p.U.off;
    float* Vown = ws + p.V.off;
    const float* V = Vown;
    float* Mx = ws + p.M.off;
    const int gw = grid_for((long)Cn * Ck);
    if (m == 4) {
        if (x3 && flip) hipLaunchKernelGGL((wino4_weight_kernel<true, true>), dim3(gw), dim3(256), 0, s, w, U, Ck, Cn);
        else if (x3) hipLaunchKernelGGL((wino4_weight_kernel<false, true>), dim3(gw), dim3(256), 0, s, w, U, Cn, Ck);
        else if (flip) hipLaunchKernelGGL((wino4_weight_kernel<true, false>), dim3(gw), dim3(256), 0, s, w, U, Ck, Cn);
        else hipLaunchKernelGGL((wino4_weight_kernel<false, false>), dim3(gw), dim3(256), 0, s, w, U, Cn, Ck);
        if (v_shared != nullptr && p.shared_v_x3 == p.x3) V = v_shared;
        else if (x3) hipLaunchKernelGGL((wino4_input_kernel<true>), dim3(grid_for(T * (Ck / 2), 256, 256 * 32)), dim3(256), 0, s, x, ldx, Vown, N, H, W, Ck);
        else hipLaunchKernelGGL((wino4_input_kernel<false>), dim3(grid_for(T * (Ck / 2), 256, 256 * 32)), dim3(256), 0, s, x, ldx, Vown, N, H, W, Ck);
    } else {
        if (flip) hipLaunchKernelGGL((wino_weight_kernel<true>), dim3(gw), dim3(256), 0, s, w, U, Ck, Cn);        // w [Cout = Ck][3][3][Cin = Cn]
        else hipLaunchKernelGGL((wino_weight_kernel<false>), dim3(gw), dim3(256), 0, s, w, U, Cn, Ck);
        hipLaunchKernelGGL(wino_input_kernel, dim3(grid_for(T * (Ck / 4), 256, 256 * 32)), dim3(256), 0, s, x, ldx, Vown, N, H, W, Ck);
    }
    PDF_LAUNCH_CHECK();
    if (x3) {
        if (int rc = pdf_internal_x3_batched_gemm(V, 36L * T * Ck, U, 36L * Cn * Ck, Mx, 36, T * Ck, (long)Cn * Ck, T * Cn, (int)T, Cn, Ck, -1, 6, s)) return rc;
    } else if (int rc = pdf_internal_batched_gemm(V, U, Mx, (int)p.P, T * Ck, (long)Cn * Ck, T * Cn, (int)T, Cn, Ck, s)) return rc;
    if (m == 4) hipLaunchKernelGGL(wino4_output_kernel, dim3(grid_for(T * (Cn / 2), 256, 256 * 32)), dim3(256), 0, s, Mx, bias, y, ldy, N, H, W, Cn, act, accum);
    else hipLaunchKernelGGL(wino_output_kernel, dim3(grid_for(T * (Cn / 4), 256, 256 * 32)), dim3(256), 0, s, Mx, bias, y, ldy, N, H, W, Cn, act, accum);
    PDF_LAUNCH_CHECK();
    return 0;
}
