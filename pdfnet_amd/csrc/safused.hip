// Fused PointNet++ set-abstraction MLP with recomputation:
//   y1 = u[idx] - v[s]  ->  BN1 + ReLU  ->  1x1 conv W2  ->  BN2 + ReLU  ->  1x1 conv W3  ->  BN3 + ReLU  ->  max over the K neighbours
// with train-mode batch statistics, WITHOUT any [rows][C] activation in HBM: every pass rebuilds the neighbour rows of one centroid
// (a tile of K rows) in LDS from the O(points) inputs u, v, idx and the layer weights, on fp32 MFMA (v_mfma_f32_16x16x4_f32).
//
// Forward (training): P1 statistics of y1 -> P2 statistics of z2 -> P3 statistics of z3 and, per (centroid, channel), the max and
// the min of z3 over k with their (first) k -> out = relu(scale3 * ((zmax or zmin) - mean3) + beta3): BN3 + ReLU is monotone in z3 (increasing
// for scale3 >= 0, decreasing otherwise), so that is the max over k of the activation.  Eval: one pass with the running statistics.
// Backward: the layer-3 gradient is non-zero at the selected (s, k*, c) only, so its two BatchNorm sums come from O(S C3) data; then
// Q1 (rebuild -> dz3 -> dW3 / db3, da2 -> BN2 sums), Q2 (rebuild -> dz2 -> dW2 / db2, da1 -> BN1 sums), Q3 (rebuild -> dz1, written
// to the caller's transient buffer for the deterministic gather_sub backward).
//
// Deterministic: no float atomics.  Each workgroup walks a fixed contiguous range of tiles and writes ONE partial per quantity
// (statistics as (mean, M2) merged with Chan's formula; sums; weight gradients accumulated in registers across its tiles); small
// finishing kernels combine the partials in workgroup order.
#include "common.h"
#include <mutex>

typedef float sa_f32x4 __attribute__((ext_vector_type(4)));

#define SA_T 256
#define SA_MAXC 256         // C1, C2, C3 <= 256: 16-column blocks, at most 4 per wave
#define SA_MAXJC 4
#define SA_MAXJW 32         // weight-gradient 16 x 16 blocks per wave: Cout * Cin <= 4 * 32 * 256
#define SA_MAXG 512

enum { SA_P1 = 1, SA_P2, SA_P3, SA_EVAL, SA_Q1, SA_Q2, SA_Q3 };

struct SaArgs {
    const float* u; const float* v; const int* idx;
    int N, S, K, C1, C2, C3; long ntiles;
    const float* w2; const float* b2; const float* w3; const float* b3;
    const float* saved;     // per layer i: mean, rstd, scale = gamma rstd, beta [C_i] each (layer 1 at 0, layer 2 at 4 C1, layer 3 at 4 (C1 + C2))
    const float* bcoef;     // backward, per layer: c1, c2 [C_i] each (dz = scale (dy - c1 - xhat c2)); layer 1 at 0, 2 at 2 C1, 3 at 2 (C1 + C2)
    const float* dout; const float* out; const int* arg;     // Q passes: the layer-3 selection
    float* part;            // per-workgroup partials, stride pstride floats
    long pstride;
    float* zmm;             // P3: zmax, zmin, kmax, kmin (as int bits) [ntiles][C3] each
    float* y;               // EVAL: out [ntiles][C3];  Q3: dz1 [ntiles * K][C1]
};

__device__ __forceinline__ sa_f32x4 sa_mfma4(const float4 a, const float4 b, sa_f32x4 c) {
    // lane l holds A[row l & 15][k0 + 4 (l >> 4) + i] and B[k0 + 4 (l >> 4) + i][col l & 15] in component i: MFMA i sums over the
    // four lane groups, the four MFMAs over i -- the 16 k of the step in a permuted order
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, c, 0, 0, 0);
    return c;
}

// acc[mb] = D[mb 16 .. +16][n0 .. n0 + 16] for mb < nmb, D = A B over kd (kd % 16 == 0).  C/D map: col = n0 + (l & 15),
// row = mb 16 + 4 (l >> 4) + r for component r.
template <class LA, class LB>
__device__ __forceinline__ void sa_colblock(int nmb, int kd, int n0, const LA& la, const LB& lb, sa_f32x4 (&acc)[4]) {
    const int l = threadIdx.x & 63, lr = l & 15, kq = (l >> 4) * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = sa_f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < kd; k0 += 16) {
        const float4 b = lb(k0 + kq, n0 + lr);
#pragma unroll
        for (int mb = 0; mb < 4; ++mb)
            if (mb < nmb) acc[mb] = sa_mfma4(la(mb * 16 + lr, k0 + kq), b, acc[mb]);
    }
}

__device__ __forceinline__ float sa_colred(float v) {      // sum over the four lanes that hold one column of a C/D block
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}
__device__ __forceinline__ double sa_colred(double v) {
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}
__device__ __forceinline__ void sa_pick(float& v, int& k, bool want_max) {   // arg-extreme over the four lanes of a column, first k wins
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) {
        const float ov = __shfl_xor(v, o, 64);
        const int ok = __shfl_xor(k, o, 64);
        if ((want_max ? ov > v : ov < v) || (ov == v && ok < k)) { v = ov; k = ok; }
    }
}
// BatchNorm + ReLU as relu(scale (z - mean) + beta): the mean is subtracted FIRST.  The folded form fma(z, scale, beta - mean scale) cancels
// catastrophically when the channel mean is large against its spread (level 1: rstd ~ 300 on tight clouds, |mean scale| ~ 60 for O(1)
// results -- an error of ulp(60) ~ 4e-6 on every activation, enough to flip near-tied maxima)
__device__ __forceinline__ float sa_bnr(float z, float m, float sc, float be) { return fmaxf(fmaf(z - m, sc, be), 0.f); }
__device__ __forceinline__ float4 sa_relu_aff(float4 z, const float* mn, const float* sc, const float* be, int k) {
    const float4 m = *reinterpret_cast<const float4*>(mn + k), a = *reinterpret_cast<const float4*>(sc + k), b = *reinterpret_cast<const float4*>(be + k);
    return make_float4(sa_bnr(z.x, m.x, a.x, b.x), sa_bnr(z.y, m.y, a.y, b.y), sa_bnr(z.z, m.z, a.z, b.z), sa_bnr(z.w, m.w, a.w, b.w));
}
// Chan's merge of a tile's (K rows, mean m, M2 q) into the range's running (n, mean, M2), in fp64
__device__ __forceinline__ void sa_chan(double& n, double& mean, double& m2, int K, float m, float q) {
    const double nn = n + (double)K, d = (double)m - mean;
    mean += d * (double)K / nn;
    m2 += (double)q + d * d * n * (double)K / nn;
    n = nn;
}

template <int MODE>
__global__ __launch_bounds__(SA_T) void sa_pass_kernel(const SaArgs a) {
    constexpr int NJW = (MODE == SA_Q1 || MODE == SA_Q2) ? SA_MAXJW : 1;
    extern __shared__ float sa_lds[];
    __shared__ int sidx[64];
    const int K = a.K, C1 = a.C1, C2 = a.C2, C3 = a.C3, nmb = K / 16;
    const int LD1 = C1 + 4, LD2 = C2 + 4, LD3 = C3 + 4;          // (+4: the 16 rows of an A fragment fall on distinct banks)
    float* z1s = sa_lds;                                          // y1 = z1 [K][LD1]
    float* z2s = z1s + K * LD1;                                   // z2 [K][LD2]; Q2 / Q3: overwritten in place by dz2
    float* dz3s = z2s + K * LD2;                                  // Q: dz3 [K][LD3]
    const int tid = threadIdx.x, wave = tid >> 6, l = tid & 63, lr = l & 15, lq = l >> 4;
    const int g = blockIdx.x, G = gridDim.x;
    const long t0 = (long)g * a.ntiles / G, t1 = (long)(g + 1) * a.ntiles / G;
    const float* sv1 = a.saved;
    const float* sv2 = sv1 + 4 * C1;
    const float* sv3 = sv2 + 4 * C2;
    const float *sc1 = sv1 + 2 * C1, *be1 = sv1 + 3 * C1, *sc2 = sv2 + 2 * C2, *be2 = sv2 + 3 * C2, *sc3 = sv3 + 2 * C3, *be3 = sv3 + 3 * C3;
    const float* bc1 = a.bcoef;
    const float* bc2 = bc1 + 2 * C1;
    const float* bc3 = bc2 + 2 * C2;

    // per-workgroup accumulators, carried across the tiles of the range (fixed ownership: deterministic)
    double cnt = 0.0, smean = 0.0, sm2 = 0.0;                     // P1: column tid
    double jcnt[SA_MAXJC], jmean[SA_MAXJC], jm2[SA_MAXJC];        // P2 / P3: column block wave + 4 j, column lr
    float jsa[SA_MAXJC], jsb[SA_MAXJC], jdb[SA_MAXJC];            // Q: BatchNorm sums of the lower layer, bias gradient
#pragma unroll
    for (int j = 0; j < SA_MAXJC; ++j) { jcnt[j] = jmean[j] = jm2[j] = 0.0; jsa[j] = jsb[j] = jdb[j] = 0.f; }
    sa_f32x4 accW[NJW];
#pragma unroll
    for (int j = 0; j < NJW; ++j) accW[j] = sa_f32x4{0.f, 0.f, 0.f, 0.f};

    for (long t = t0; t < t1; ++t) {
        const long b = t / a.S, s = t - b * a.S;
        __syncthreads();                                          // the previous tile is done with the LDS
        if (tid < K) {
            const int p = a.idx[t * K + tid];
            sidx[tid] = min(max(p, 0), a.N - 1);
        }
        __syncthreads();
        {   // gather y1 = u[idx] - v[s]
            const int cq = C1 / 4;
            const float* vb = a.v + (b * a.S + s) * C1;
            for (int i = tid; i < K * cq; i += SA_T) {
                const int r = i / cq, c = (i - r * cq) * 4;
                const float4 x = *reinterpret_cast<const float4*>(a.u + (b * a.N + sidx[r]) * (long)C1 + c);
                const float4 y = *reinterpret_cast<const float4*>(vb + c);
                *reinterpret_cast<float4*>(z1s + r * LD1 + c) = make_float4(x.x - y.x, x.y - y.y, x.z - y.z, x.w - y.w);
            }
        }
        __syncthreads();
        if constexpr (MODE == SA_P1) {
            if (tid < C1) {                                       // tile (mean, M2), Chan-merged into the range's
                double sum = 0.0;                                 // (fp64: the tile mean is exact to fp32 rounding)
                for (int r = 0; r < K; ++r) sum += z1s[r * LD1 + tid];
                const float m = (float)(sum / K);
                float q = 0.f;
                for (int r = 0; r < K; ++r) { const float d = z1s[r * LD1 + tid] - m; q = fmaf(d, d, q); }
                sa_chan(cnt, smean, sm2, K, m, q);
            }
            continue;
        } else {
            // ---- z2 = a1 W2^T + b2, a1 = relu(sc1 (y1 - mean1) + beta1)
            auto la1 = [&](int m, int k) { return sa_relu_aff(*reinterpret_cast<const float4*>(z1s + m * LD1 + k), sv1, sc1, be1, k); };
            auto lw2 = [&](int k, int n) { return *reinterpret_cast<const float4*>(a.w2 + (long)n * C1 + k); };
#pragma unroll
            for (int j = 0; j < SA_MAXJC; ++j) {
                const int cb = wave + 4 * j;
                if (cb * 16 >= C2) break;
                sa_f32x4 acc[4];
                sa_colblock(nmb, C1, cb * 16, la1, lw2, acc);
                const int c = cb * 16 + lr;
                const float bias = a.b2[c];
                if constexpr (MODE == SA_P2) {
                    double sum = 0.0;
#pragma unroll
                    for (int mb = 0; mb < 4; ++mb) {
                        if (mb >= nmb) break;
#pragma unroll
                        for (int r = 0; r < 4; ++r) { acc[mb][r] += bias; sum += acc[mb][r]; }
                    }
                    const float m = (float)(sa_colred(sum) / K);
                    float q = 0.f;
#pragma unroll
                    for (int mb = 0; mb < 4; ++mb) {
                        if (mb >= nmb) break;
#pragma unroll
                        for (int r = 0; r < 4; ++r) { const float d = acc[mb][r] - m; q = fmaf(d, d, q); }
                    }
                    sa_chan(jcnt[j], jmean[j], jm2[j], K, m, sa_colred(q));
                } else {
#pragma unroll
                    for (int mb = 0; mb < 4; ++mb) {
                        if (mb >= nmb) break;
#pragma unroll
                        for (int r = 0; r < 4; ++r) z2s[(mb * 16 + lq * 4 + r) * LD2 + c] = acc[mb][r] + bias;
                    }
                }
            }
            if constexpr (MODE == SA_P2) continue;
            else {
                __syncthreads();
                // ---- z3 = a2 W3^T + b3, a2 = relu(sc2 (z2 - mean2) + beta2)
                auto la2 = [&](int m, int k) { return sa_relu_aff(*reinterpret_cast<const float4*>(z2s + m * LD2 + k), sv2, sc2, be2, k); };
                auto lw3 = [&](int k, int n) { return *reinterpret_cast<const float4*>(a.w3 + (long)n * C2 + k); };
#pragma unroll
                for (int j = 0; j < SA_MAXJC; ++j) {
                    const int cb = wave + 4 * j;
                    if (cb * 16 >= C3) break;
                    sa_f32x4 acc[4];
                    sa_colblock(nmb, C2, cb * 16, la2, lw3, acc);
                    const int c = cb * 16 + lr;
                    const float bias = a.b3[c];
                    if constexpr (MODE == SA_P3) {
                        double sum = 0.0;
                        float vmax = -INFINITY, vmin = INFINITY;
                        int kmax = 0, kmin = 0;
#pragma unroll
                        for (int mb = 0; mb < 4; ++mb) {
                            if (mb >= nmb) break;
#pragma unroll
                            for (int r = 0; r < 4; ++r) {                   // rows ascending within the lane: strict compares keep the first k
                                const float z = acc[mb][r] + bias;
                                acc[mb][r] = z;
                                sum += z;
                                const int k = mb * 16 + lq * 4 + r;
                                if (z > vmax) { vmax = z; kmax = k; }
                                if (z < vmin) { vmin = z; kmin = k; }
                            }
                        }
                        const float m = (float)(sa_colred(sum) / K);
                        float q = 0.f;
#pragma unroll
                        for (int mb = 0; mb < 4; ++mb) {
                            if (mb >= nmb) break;
#pragma unroll
                            for (int r = 0; r < 4; ++r) { const float d = acc[mb][r] - m; q = fmaf(d, d, q); }
                        }
                        sa_chan(jcnt[j], jmean[j], jm2[j], K, m, sa_colred(q));
                        sa_pick(vmax, kmax, true);
                        sa_pick(vmin, kmin, false);
                        if (lq == 0) {
                            const long o = t * C3 + c, plane = a.ntiles * C3;
                            a.zmm[o] = vmax;
                            a.zmm[plane + o] = vmin;
                            a.zmm[2 * plane + o] = __int_as_float(kmax);
                            a.zmm[3 * plane + o] = __int_as_float(kmin);
                        }
                    } else if constexpr (MODE == SA_EVAL) {
                        const float m3 = sv3[c], s3 = sc3[c], h3 = be3[c];
                        float best = -1.f;                                   // the relu output is >= 0: the first k always beats -1
                        int kb = 0;
#pragma unroll
                        for (int mb = 0; mb < 4; ++mb) {
                            if (mb >= nmb) break;
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const float z = sa_bnr(acc[mb][r] + bias, m3, s3, h3);
                                if (z > best) { best = z; kb = mb * 16 + lq * 4 + r; }
                            }
                        }
                        sa_pick(best, kb, true);
                        if (lq == 0) a.y[t * C3 + c] = best;
                    } else {                                          // Q: dz3 = scale3 (dy3 - c1 - xhat3 c2), dy3 at the selected k only
                        const long o = t * C3 + c;
                        const int ksel = a.arg[o];
                        const float gsel = a.out[o] > 0.f ? a.dout[o] : 0.f;
                        const float mean = sv3[c], rstd = sv3[C3 + c], s3 = sc3[c], k1 = bc3[c], k2 = bc3[C3 + c];
#pragma unroll
                        for (int mb = 0; mb < 4; ++mb) {
                            if (mb >= nmb) break;
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const int row = mb * 16 + lq * 4 + r;
                                const float xh = (acc[mb][r] + bias - mean) * rstd;
                                const float dz = s3 * ((row == ksel ? gsel : 0.f) - k1 - xh * k2);
                                dz3s[row * LD3 + c] = dz;
                                if constexpr (MODE == SA_Q1) jdb[j] += dz;
                            }
                        }
                    }
                }
                if constexpr (MODE == SA_P3 || MODE == SA_EVAL) continue;
                else {
                    __syncthreads();
                    if constexpr (MODE == SA_Q1) {                    // dW3[c3][c2] += sum_rows dz3[row][c3] a2[row][c2]
                        const int nbn = C2 / 16, nblk = (C3 / 16) * nbn;
#pragma unroll
                        for (int j = 0; j < NJW; ++j) {
                            const int bid = wave + 4 * j;
                            if (bid >= nblk) break;
                            const int m = (bid / nbn) * 16 + lr, n = (bid % nbn) * 16 + lr;
                            const float m2 = sv2[n], s2 = sc2[n], h2 = be2[n];
                            for (int k0 = 0; k0 < K; k0 += 16) {
                                const int k = k0 + lq * 4;
                                const float4 av = make_float4(dz3s[k * LD3 + m], dz3s[(k + 1) * LD3 + m], dz3s[(k + 2) * LD3 + m], dz3s[(k + 3) * LD3 + m]);
                                const float4 bv = make_float4(sa_bnr(z2s[k * LD2 + n], m2, s2, h2), sa_bnr(z2s[(k + 1) * LD2 + n], m2, s2, h2),
                                                              sa_bnr(z2s[(k + 2) * LD2 + n], m2, s2, h2), sa_bnr(z2s[(k + 3) * LD2 + n], m2, s2, h2));
                                accW[j] = sa_mfma4(av, bv, accW[j]);
                            }
                        }
                    }
                    // ---- da2 = dz3 W3 -> dy2 (ReLU mask of layer 2); Q1: BN2 sums; Q2 / Q3: dz2, in place of z2 (each element is read and
                    // written by the same lane; nothing else reads z2 in this phase)
                    auto ld3 = [&](int m, int k) { return *reinterpret_cast<const float4*>(dz3s + m * LD3 + k); };
                    auto lw3t = [&](int k, int n) { return make_float4(a.w3[(long)k * C2 + n], a.w3[(long)(k + 1) * C2 + n], a.w3[(long)(k + 2) * C2 + n], a.w3[(long)(k + 3) * C2 + n]); };
#pragma unroll
                    for (int j = 0; j < SA_MAXJC; ++j) {
                        const int cb = wave + 4 * j;
                        if (cb * 16 >= C2) break;
                        sa_f32x4 acc[4];
                        sa_colblock(nmb, C3, cb * 16, ld3, lw3t, acc);
                        const int c = cb * 16 + lr;
                        const float mean = sv2[c], rstd = sv2[C2 + c], s2 = sc2[c], h2 = be2[c], k1 = bc2[c], k2 = bc2[C2 + c];
#pragma unroll
                        for (int mb = 0; mb < 4; ++mb) {
                            if (mb >= nmb) break;
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                float* zp = z2s + (mb * 16 + lq * 4 + r) * LD2 + c;
                                const float z = *zp;
                                const float dy = fmaf(z - mean, s2, h2) > 0.f ? acc[mb][r] : 0.f;
                                const float xh = (z - mean) * rstd;
                                if constexpr (MODE == SA_Q1) { jsa[j] += dy; jsb[j] = fmaf(dy, xh, jsb[j]); }
                                else {
                                    const float dz = s2 * (dy - k1 - xh * k2);
                                    *zp = dz;
                                    if constexpr (MODE == SA_Q2) jdb[j] += dz;
                                }
                            }
                        }
                    }
                    if constexpr (MODE == SA_Q1) continue;
                    else {
                        __syncthreads();
                        if constexpr (MODE == SA_Q2) {                // dW2[c2][c1] += sum_rows dz2[row][c2] a1[row][c1]
                            const int nbn = C1 / 16, nblk = (C2 / 16) * nbn;
#pragma unroll
                            for (int j = 0; j < NJW; ++j) {
                                const int bid = wave + 4 * j;
                                if (bid >= nblk) break;
                                const int m = (bid / nbn) * 16 + lr, n = (bid % nbn) * 16 + lr;
                                const float m1 = sv1[n], s1 = sc1[n], h1 = be1[n];
                                for (int k0 = 0; k0 < K; k0 += 16) {
                                    const int k = k0 + lq * 4;
                                    const float4 av = make_float4(z2s[k * LD2 + m], z2s[(k + 1) * LD2 + m], z2s[(k + 2) * LD2 + m], z2s[(k + 3) * LD2 + m]);
                                    const float4 bv = make_float4(sa_bnr(z1s[k * LD1 + n], m1, s1, h1), sa_bnr(z1s[(k + 1) * LD1 + n], m1, s1, h1),
                                                                  sa_bnr(z1s[(k + 2) * LD1 + n], m1, s1, h1), sa_bnr(z1s[(k + 3) * LD1 + n], m1, s1, h1));
                                    accW[j] = sa_mfma4(av, bv, accW[j]);
                                }
                            }
                        }
                        // ---- da1 = dz2 W2 -> dy1; Q2: BN1 sums; Q3: dz1 -> HBM
                        auto ld2 = [&](int m, int k) { return *reinterpret_cast<const float4*>(z2s + m * LD2 + k); };
                        auto lw2t = [&](int k, int n) { return make_float4(a.w2[(long)k * C1 + n], a.w2[(long)(k + 1) * C1 + n], a.w2[(long)(k + 2) * C1 + n], a.w2[(long)(k + 3) * C1 + n]); };
#pragma unroll
                        for (int j = 0; j < SA_MAXJC; ++j) {
                            const int cb = wave + 4 * j;
                            if (cb * 16 >= C1) break;
                            sa_f32x4 acc[4];
                            sa_colblock(nmb, C2, cb * 16, ld2, lw2t, acc);
                            const int c = cb * 16 + lr;
                            const float mean = sv1[c], rstd = sv1[C1 + c], s1 = sc1[c], h1 = be1[c], k1 = bc1[c], k2 = bc1[C1 + c];
#pragma unroll
                            for (int mb = 0; mb < 4; ++mb) {
                                if (mb >= nmb) break;
#pragma unroll
                                for (int r = 0; r < 4; ++r) {
                                    const int row = mb * 16 + lq * 4 + r;
                                    const float z = z1s[row * LD1 + c];
                                    const float dy = fmaf(z - mean, s1, h1) > 0.f ? acc[mb][r] : 0.f;
                                    const float xh = (z - mean) * rstd;
                                    if constexpr (MODE == SA_Q2) { jsa[j] += dy; jsb[j] = fmaf(dy, xh, jsb[j]); }
                                    else a.y[(t * K + row) * C1 + c] = s1 * (dy - k1 - xh * k2);
                                }
                            }
                        }
                    }
                }
            }
        }
    }

    // ---- the range's partials
    float* P = a.part + (long)g * a.pstride;
    if constexpr (MODE == SA_P1) {
        if (tid < C1) { P[2 * tid] = (float)smean; P[2 * tid + 1] = (float)sm2; }
    } else if constexpr (MODE == SA_P2 || MODE == SA_P3) {
        const int C = MODE == SA_P2 ? C2 : C3;
#pragma unroll
        for (int j = 0; j < SA_MAXJC; ++j) {
            const int cb = wave + 4 * j;
            if (cb * 16 >= C) break;
            if (lq == 0) { P[2 * (cb * 16 + lr)] = (float)jmean[j]; P[2 * (cb * 16 + lr) + 1] = (float)jm2[j]; }
        }
    } else if constexpr (MODE == SA_Q1 || MODE == SA_Q2) {
        // layout: dW [Cout][Cin], db [Cout], BatchNorm sums of the lower layer [Cin][2]
        const int Co = MODE == SA_Q1 ? C3 : C2, Ci = MODE == SA_Q1 ? C2 : C1;
        const int nbn = Ci / 16, nblk = (Co / 16) * nbn;
#pragma unroll
        for (int j = 0; j < NJW; ++j) {
            const int bid = wave + 4 * j;
            if (bid >= nblk) break;
            const int m0 = (bid / nbn) * 16 + lq * 4, n = (bid % nbn) * 16 + lr;
#pragma unroll
            for (int r = 0; r < 4; ++r) P[(long)(m0 + r) * Ci + n] = accW[j][r];
        }
        float* Pb = P + (long)Co * Ci;
        float* Ps = Pb + Co;
#pragma unroll
        for (int j = 0; j < SA_MAXJC; ++j) {
            const int cb = wave + 4 * j;
            const float db = sa_colred(jdb[j]), sa = sa_colred(jsa[j]), sb = sa_colred(jsb[j]);
            if (lq == 0 && cb * 16 < Co) Pb[cb * 16 + lr] = db;
            if (lq == 0 && cb * 16 < Ci) { Ps[2 * (cb * 16 + lr)] = sa; Ps[2 * (cb * 16 + lr) + 1] = sb; }
        }
    }
}

// statistics partials (mean, M2) of the G tile ranges -> Chan merge in fp64, workgroup order -> mean / rstd / scale / beta, running update
__global__ __launch_bounds__(256) void sa_stats_finalize_kernel(const float* __restrict__ part, long pstride, int G, long ntiles, int K, int C,
                                                                const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                float* __restrict__ rmean, float* __restrict__ rvar, float momentum, float eps,
                                                                float* __restrict__ sv /* mean, rstd, scale, beta [C] */) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double n = 0.0, mean = 0.0, m2 = 0.0;
    for (int g = 0; g < G; ++g) {
        const double nb = (double)(((long)(g + 1) * ntiles / G - (long)g * ntiles / G) * K);
        if (nb <= 0.0) continue;
        const double mb = part[g * pstride + 2 * c], qb = part[g * pstride + 2 * c + 1];
        const double nn = n + nb, d = mb - mean;
        mean += d * nb / nn;
        m2 += qb + d * d * n * nb / nn;
        n = nn;
    }
    double var = m2 / n;
    if (var < 0.0) var = 0.0;
    const float rstd = (float)(1.0 / sqrt(var + (double)eps));
    sv[c] = (float)mean;
    sv[C + c] = rstd;
    if (rmean != nullptr) {
        rmean[c] = (1.f - momentum) * rmean[c] + momentum * (float)mean;
        const double unb = n > 1.0 ? m2 / (n - 1.0) : var;
        rvar[c] = (1.f - momentum) * rvar[c] + momentum * (float)unb;
    }
    const float sc = gamma[c] * rstd;
    sv[2 * C + c] = sc;
    sv[3 * C + c] = beta[c];
}

__global__ void sa_eval_coeff_kernel(int C, const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ rm,
                                     const float* __restrict__ rv, float eps, float* __restrict__ sv) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    sv[c] = rm[c];
    sv[C + c] = 1.f / sqrtf(rv[c] + eps);
    sv[2 * C + c] = gamma[c] / sqrtf(rv[c] + eps);
    sv[3 * C + c] = beta[c];
}

// out = relu(scale3 (z - mean3) + beta3) at z = zmax (scale3 >= 0) or zmin (scale3 < 0); arg = its k; zsel = z (for the backward)
__global__ __launch_bounds__(256) void sa_out_kernel(const float* __restrict__ zmm, long ntiles, int C, const float* __restrict__ sv3,
                                                     float* __restrict__ out, int* __restrict__ arg, float* __restrict__ zsel) {
    const long total = ntiles * C;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const float sc = sv3[2 * C + c];
        const bool up = sc >= 0.f;
        const float z = up ? zmm[i] : zmm[total + i];
        out[i] = sa_bnr(z, sv3[c], sc, sv3[3 * C + c]);
        arg[i] = __float_as_int(up ? zmm[2 * total + i] : zmm[3 * total + i]);
        zsel[i] = z;
    }
}

// layer-3 BatchNorm sums from the selection: sum dy3, sum dy3 xhat3 over the tiles of range g -> part[g][C][2]
__global__ __launch_bounds__(256) void sa_bn3_bwd_partial_kernel(const float* __restrict__ dout, const float* __restrict__ out,
                                                                 const float* __restrict__ zsel, const float* __restrict__ sv3, long ntiles, int C,
                                                                 float* __restrict__ part) {
    const int g = blockIdx.x, G = gridDim.x;
    const long t0 = (long)g * ntiles / G, t1 = (long)(g + 1) * ntiles / G;
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        const float mean = sv3[c], rstd = sv3[C + c];
        float sa = 0.f, sb = 0.f;
        for (long t = t0; t < t1; ++t) {
            const long o = t * C + c;
            const float dy = out[o] > 0.f ? dout[o] : 0.f;
            sa += dy;
            sb = fmaf(dy, (zsel[o] - mean) * rstd, sb);
        }
        part[((long)g * C + c) * 2] = sa;
        part[((long)g * C + c) * 2 + 1] = sb;
    }
}

// BatchNorm backward sums (part + g * pstride)[c][2] -> dbeta = sum dy, dgamma = sum dy xhat, c1 / c2 = those over the row count
__global__ __launch_bounds__(256) void sa_bwd_finalize_kernel(const float* __restrict__ part, long pstride, int G, int C, double rows,
                                                              float* __restrict__ dgamma, float* __restrict__ dbeta, float* __restrict__ bc) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double sa = 0.0, sb = 0.0;
    for (int g = 0; g < G; ++g) { sa += part[g * pstride + 2 * c]; sb += part[g * pstride + 2 * c + 1]; }
    dbeta[c] = (float)sa;
    dgamma[c] = (float)sb;
    bc[c] = (float)(sa / rows);
    bc[C + c] = (float)(sb / rows);
}

// weight / bias gradient partials: out[i] = sum_g part[g * pstride + i] (fp64, workgroup order); i < nw -> dw, else db
__global__ __launch_bounds__(256) void sa_sum_partials_kernel(const float* __restrict__ part, long pstride, int G, long nw, long nb,
                                                              float* __restrict__ dw, float* __restrict__ db) {
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (i >= nw + nb) return;
    double s = 0.0;
    for (int g = 0; g < G; ++g) s += part[g * pstride + i];
    if (i < nw) dw[i] = (float)s;
    else db[i - nw] = (float)s;
}

// ---------------------------------------------------------------------------------------------------------------------------------
#define SA_MAX_LDS (159L * 1024)   // dynamic LDS per workgroup (+ 256 B of static LDS: the 160 KiB of a CU)
static long sa_lds_bytes(int K, int C1, int C2, int C3, int mode) {
    long f = (long)K * (C1 + 4);
    if (mode >= SA_P2) f += (long)K * (C2 + 4);
    if (mode >= SA_Q1) f += (long)K * (C3 + 4);
    return f * 4;
}
static bool sa_shape_ok(int Bc, int N, int S, int K, int C1, int C2, int C3) {
    if (Bc <= 0 || N <= 0 || S <= 0 || S > N || K < 16 || K > 64 || K % 16) return false;
    for (int c : {C1, C2, C3})
        if (c <= 0 || c % 16 || c > SA_MAXC) return false;
    // the backward's LDS (the largest: y1, z2 and dz3 of one centroid) must fit the dynamic LDS the launches allow
    return (long)C3 * C2 <= 4L * SA_MAXJW * 256 && (long)C2 * C1 <= 4L * SA_MAXJW * 256 && sa_lds_bytes(K, C1, C2, C3, SA_Q1) <= SA_MAX_LDS;
}
static int sa_grid(long ntiles, int K, int C1, int C2, int C3) {
    // one range of tiles per workgroup; two workgroups per CU where the backward's LDS allows it
    const long g = sa_lds_bytes(K, C1, C2, C3, SA_Q1) <= 80 * 1024 ? SA_MAXG : SA_MAXG / 2;
    return (int)(ntiles < g ? ntiles : g);
}
static long sa_part_floats(int C1, int C2, int C3) {
    const long p1 = 2L * SA_MAXC;
    const long q1 = (long)C3 * C2 + C3 + 2L * C2, q2 = (long)C2 * C1 + C2 + 2L * C1;
    return p1 > q1 ? (p1 > q2 ? p1 : q2) : (q1 > q2 ? q1 : q2);
}

PDF_API long pdf_sa_fused_workspace_floats(int Bc, int S, int K, int C1, int C2, int C3) {
    if (Bc <= 0 || S <= 0 || K <= 0 || C1 <= 0 || C2 <= 0 || C3 <= 0) return 0;
    const long ntiles = (long)Bc * S;
    return 2L * (C1 + C2 + C3) + (long)sa_grid(ntiles, K, C1, C2, C3) * sa_part_floats(C1, C2, C3) + 4L * ntiles * C3;
}

template <int MODE>
static int sa_launch(const SaArgs& a, int G, hipStream_t s) {
    static std::once_flag once;
    std::call_once(once, [] { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(sa_pass_kernel<MODE>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)SA_MAX_LDS); });
    hipLaunchKernelGGL(sa_pass_kernel<MODE>, dim3(G), dim3(SA_T), sa_lds_bytes(a.K, a.C1, a.C2, a.C3, MODE), s, a);
    PDF_LAUNCH_CHECK();
    return 0;
}

PDF_API int pdf_sa_fused_fwd(const float* u, const float* v, const int* idx, int Bc, int N, int S, int K, int C1, int C2, int C3,
                             const float* w2, const float* b2, const float* w3, const float* b3,
                             const float* gamma1, const float* beta1, const float* gamma2, const float* beta2, const float* gamma3, const float* beta3,
                             float* rmean1, float* rvar1, float* rmean2, float* rvar2, float* rmean3, float* rvar3, float momentum, float eps, int training,
                             float* out, int* arg, float* zsel, float* saved, float* ws, long ws_floats, void* stream) {
    if (!sa_shape_ok(Bc, N, S, K, C1, C2, C3)) return PDF_E_BADARG;
    if (!u || !v || !idx || !w2 || !b2 || !w3 || !b3 || !gamma1 || !beta1 || !gamma2 || !beta2 || !gamma3 || !beta3 || !out || !saved || !ws) return PDF_E_BADARG;
    if (training ? (!arg || !zsel) : (!rmean1 || !rvar1 || !rmean2 || !rvar2 || !rmean3 || !rvar3)) return PDF_E_BADARG;
    if (ws_floats < pdf_sa_fused_workspace_floats(Bc, S, K, C1, C2, C3)) return PDF_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const long ntiles = (long)Bc * S;
    const int G = sa_grid(ntiles, K, C1, C2, C3);
    SaArgs a = {};
    a.u = u; a.v = v; a.idx = idx; a.N = N; a.S = S; a.K = K; a.C1 = C1; a.C2 = C2; a.C3 = C3; a.ntiles = ntiles;
    a.w2 = w2; a.b2 = b2; a.w3 = w3; a.b3 = b3; a.saved = saved; a.bcoef = ws;
    a.part = ws + 2L * (C1 + C2 + C3);
    a.pstride = sa_part_floats(C1, C2, C3);
    a.zmm = a.part + (long)G * a.pstride;
    float* sv[3] = {saved, saved + 4 * C1, saved + 4 * (C1 + C2)};
    const int Cs[3] = {C1, C2, C3};
    const float* gm[3] = {gamma1, gamma2, gamma3};
    const float* bt[3] = {beta1, beta2, beta3};
    float* rm[3] = {rmean1, rmean2, rmean3};
    float* rv[3] = {rvar1, rvar2, rvar3};
    if (!training) {
        for (int i = 0; i < 3; ++i) {
            hipLaunchKernelGGL(sa_eval_coeff_kernel, dim3(cdiv(Cs[i], 256)), dim3(256), 0, s, Cs[i], gm[i], bt[i], rm[i], rv[i], eps, sv[i]);
            PDF_LAUNCH_CHECK();
        }
        a.y = out;
        return sa_launch<SA_EVAL>(a, G, s);
    }
    for (int i = 0; i < 3; ++i) {
        const int rc = i == 0 ? sa_launch<SA_P1>(a, G, s) : i == 1 ? sa_launch<SA_P2>(a, G, s) : sa_launch<SA_P3>(a, G, s);
        if (rc) return rc;
        hipLaunchKernelGGL(sa_stats_finalize_kernel, dim3(cdiv(Cs[i], 256)), dim3(256), 0, s, a.part, a.pstride, G, ntiles, K, Cs[i], gm[i], bt[i],
                           rm[i], rv[i], momentum, eps, sv[i]);
        PDF_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(sa_out_kernel, dim3(grid_for(ntiles * C3)), dim3(256), 0, s, a.zmm, ntiles, C3, sv[2], out, arg, zsel);
    PDF_LAUNCH_CHECK();
    return 0;
}

PDF_API int pdf_sa_fused_bwd(const float* dout, const float* u, const float* v, const int* idx, int Bc, int N, int S, int K, int C1, int C2, int C3,
                             const float* w2, const float* b2, const float* w3, const float* b3,
                             const float* out, const int* arg, const float* zsel, const float* saved,
                             float* dz1, float* dw2, float* db2, float* dw3, float* db3,
                             float* dgamma1, float* dbeta1, float* dgamma2, float* dbeta2, float* dgamma3, float* dbeta3,
                             float* ws, long ws_floats, void* stream) {
    if (!sa_shape_ok(Bc, N, S, K, C1, C2, C3)) return PDF_E_BADARG;
    if (!dout || !u || !v || !idx || !w2 || !b2 || !w3 || !b3 || !out || !arg || !zsel || !saved || !dz1 || !dw2 || !db2 || !dw3 || !db3 ||
        !dgamma1 || !dbeta1 || !dgamma2 || !dbeta2 || !dgamma3 || !dbeta3 || !ws) return PDF_E_BADARG;
    if (ws_floats < pdf_sa_fused_workspace_floats(Bc, S, K, C1, C2, C3)) return PDF_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const long ntiles = (long)Bc * S;
    const double rows = (double)ntiles * K;
    const int G = sa_grid(ntiles, K, C1, C2, C3);
    SaArgs a = {};
    a.u = u; a.v = v; a.idx = idx; a.N = N; a.S = S; a.K = K; a.C1 = C1; a.C2 = C2; a.C3 = C3; a.ntiles = ntiles;
    a.w2 = w2; a.b2 = b2; a.w3 = w3; a.b3 = b3; a.saved = saved; a.bcoef = ws;
    a.dout = dout; a.out = out; a.arg = arg;
    a.part = ws + 2L * (C1 + C2 + C3);
    a.pstride = sa_part_floats(C1, C2, C3);
    float* bc = ws;
    const float* sv3 = saved + 4 * (C1 + C2);
    // layer 3: its two sums from the selection only
    hipLaunchKernelGGL(sa_bn3_bwd_partial_kernel, dim3(G), dim3(256), 0, s, dout, out, zsel, sv3, ntiles, C3, a.part);
    PDF_LAUNCH_CHECK();
    hipLaunchKernelGGL(sa_bwd_finalize_kernel, dim3(cdiv(C3, 256)), dim3(256), 0, s, a.part, 2L * C3, G, C3, rows, dgamma3, dbeta3, bc + 2 * (C1 + C2));
    PDF_LAUNCH_CHECK();
    // Q1: dW3, db3, BN2 sums
    if (int rc = sa_launch<SA_Q1>(a, G, s)) return rc;
    hipLaunchKernelGGL(sa_sum_partials_kernel, dim3(cdiv((long)C3 * C2 + C3, 256)), dim3(256), 0, s, a.part, a.pstride, G, (long)C3 * C2, (long)C3, dw3, db3);
    PDF_LAUNCH_CHECK();
    hipLaunchKernelGGL(sa_bwd_finalize_kernel, dim3(cdiv(C2, 256)), dim3(256), 0, s, a.part + (long)C3 * C2 + C3, a.pstride, G, C2, rows, dgamma2, dbeta2, bc + 2 * C1);
    PDF_LAUNCH_CHECK();
    // Q2: dW2, db2, BN1 sums
    if (int rc = sa_launch<SA_Q2>(a, G, s)) return rc;
    hipLaunchKernelGGL(sa_sum_partials_kernel, dim3(cdiv((long)C2 * C1 + C2, 256)), dim3(256), 0, s, a.part, a.pstride, G, (long)C2 * C1, (long)C2, dw2, db2);
    PDF_LAUNCH_CHECK();
    hipLaunchKernelGGL(sa_bwd_finalize_kernel, dim3(cdiv(C1, 256)), dim3(256), 0, s, a.part + (long)C2 * C1 + C2, a.pstride, G, C1, rows, dgamma1, dbeta1, bc);
    PDF_LAUNCH_CHECK();
    // Q3: dz1 into the caller's transient buffer
    a.y = dz1;
    return sa_launch<SA_Q3>(a, G, s);
}
