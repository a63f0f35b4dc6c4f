// Normalisation kernels on row-major [rows][channels] (NHWC) activations: BatchNorm (train/eval,
// fused ReLU / residual), LayerNorm, L2Norm.  All HBM-bound: each is a column- or row-reduction plus
// one streaming pass; channels are the contiguous axis so every access is coalesced.
#include "common.h"
#include <initializer_list>
#include <cstdlib>

// ---------------------------------------------------------------------------------------------
// BatchNorm2d / BatchNorm1d over rows.  Statistics are accumulated as shifted sums
// sum(x - x0), sum((x - x0)^2) (x0 = first row) in fp32 per thread, combined in fp64.
//
// Every column pass (reduction or streaming) is ONE body in two instantiations over V, the channels a thread owns: a block is
// 64 channels = BN_TX(V) = 64 / V channel groups x BN_TY(V) = 256 / BN_TX(V) row lanes.
//   V = 4: 16 channel quads x 16 row lanes, 16-byte accesses, 4 rows in flight per thread (the scalar form moved 1.1-1.6 TB/s:
//          one 4-byte load in flight per thread)
//   V = 1: 64 channels x 4 row lanes -- C % 4 != 0, an odd leading dimension or an unaligned pointer (v4_ok)
// A block walks its own contiguous chunk of rows_per_chunk rows: rows r0 + ty, r0 + ty + BN_TY, ...
#define BN_CT 64   // channels per block
#define BN_TX(V) (BN_CT / (V))
#define BN_TY(V) (256 / BN_TX(V))
template <int V> using vf = float __attribute__((ext_vector_type(V)));      // V floats, component-wise arithmetic, 4 V bytes aligned
template <int V> __device__ __forceinline__ vf<V> vld(const float* p) { return *reinterpret_cast<const vf<V>*>(p); }
template <int V> __device__ __forceinline__ void vst(float* p, vf<V> v) { *reinterpret_cast<vf<V>*>(p) = v; }
template <int V> __device__ __forceinline__ vf<V> vfma(vf<V> a, vf<V> b, vf<V> c) {
    vf<V> r;
#pragma unroll
    for (int i = 0; i < V; ++i) r[i] = fmaf(a[i], b[i], c[i]);
    return r;
}
__device__ __forceinline__ float add_rounded_product(float acc, float p, float q) {                // acc + p * q, never fused
#pragma clang fp contract(off)
    const float pq = p * q;
    return acc + pq;
}
__device__ __forceinline__ float sum_of_rounded_products(float a, float b, float c, float d) {      // a * b + c * d, never fused
#pragma clang fp contract(off)
    const float ab = a * b, cd = c * d;
    return ab + cd;
}
// acc + p * q in a running sum.  The two forms have always rounded this differently: the float4 kernels fuse it, the scalar kernels
// round the product first (the compiler paired their two accumulators into one packed add before it could contract).  Each keeps
// its rounding, spelled out here so that it no longer depends on what the compiler makes of the loop.
template <int V> __device__ __forceinline__ vf<V> bn_acc(vf<V> acc, vf<V> p, vf<V> q) {
    if constexpr (V == 1) { vf<1> r; r[0] = add_rounded_product(acc[0], p[0], q[0]); return r; }
    else return vfma<V>(p, q, acc);
}
template <int V> __device__ __forceinline__ vf<V> vrsqrt_eps(vf<V> var, float eps) {
    vf<V> r;
#pragma unroll
    for (int i = 0; i < V; ++i) r[i] = 1.f / sqrtf(var[i] + eps);
    return r;
}
__device__ __forceinline__ void vst_bf16(unsigned short* p, vf<4> v) {     // the bf16 shadow of four floats: one 8-byte store
    *reinterpret_cast<uint2*>(p) = uint2{pdf_pk_bf16(v[0], v[1]), pdf_pk_bf16(v[2], v[3])};
}
__device__ __forceinline__ vf<4> as_vf(float4 v) { return vf<4>{v.x, v.y, v.z, v.w}; }
// bf16 storage mode: the BatchNorm input x (a conv output nobody else reads) may come as bf16 (X16): 4 channels = one 8-byte load
template <int V, bool X16>
__device__ __forceinline__ vf<V> ld_x(const float* __restrict__ x, long idx) {
    if constexpr (X16) {
        static_assert(V == 4, "bf16 input: float4 form only");
        const uint2 u = *reinterpret_cast<const uint2*>(reinterpret_cast<const unsigned short*>(x) + idx);
        return vf<4>{__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16), __uint_as_float(u.y & 0xffff0000u)};
    } else {
        return vld<V>(x + idx);
    }
}
// the row lanes of a block summed in lane order 0, 1, ... -> part[blockIdx.y][c0 .. c0 + V)[2]  (two == false: the second sum is 0)
template <int V>
__device__ __forceinline__ void bn_block_reduce(vf<V> a, vf<V> b, vf<V> (&sa)[BN_TY(V)][BN_TX(V)], vf<V> (&sb)[BN_TY(V)][BN_TX(V)],
                                                float* __restrict__ part, int C, int c0, bool two) {
    const int tx = threadIdx.x & (BN_TX(V) - 1), ty = threadIdx.x / BN_TX(V);
    sa[ty][tx] = a;
    if (two) sb[ty][tx] = b;
    __syncthreads();
    if (ty == 0 && c0 < C) {
        vf<V> x = sa[0][tx], y = {};
        if (two) y = sb[0][tx];
        for (int j = 1; j < BN_TY(V); ++j) { x += sa[j][tx]; if (two) y += sb[j][tx]; }
        float* o = part + ((long)blockIdx.y * C + c0) * 2;
#pragma unroll
        for (int i = 0; i < V; ++i) { o[2 * i] = x[i]; o[2 * i + 1] = two ? y[i] : 0.f; }
    }
}
// g = dy under the ReLU of the forward.  relu 0: none; 1: mask from the saved output y; 2: no residual went into the ReLU, so its
// mask is recomputed from x as fmaf(x, scale, shift) > 0 -- the exact expression of the forward -- and y is not read at all
template <int V>
__device__ __forceinline__ vf<V> bn_masked_grad(vf<V> g, int relu, const float* __restrict__ y_at, vf<V> xv, vf<V> sc, vf<V> sh) {
    if (relu) {
        const vf<V> yv = relu == 2 ? vfma<V>(xv, sc, sh) : vld<V>(y_at);
#pragma unroll
        for (int i = 0; i < V; ++i) if (!(yv[i] > 0.f)) g[i] = 0.f;
    }
    return g;
}

template <int V, bool X16>
__global__ __launch_bounds__(256) void bn_partial_kernel(const float* __restrict__ x, int ldx, int C, long R, long rows_per_chunk,
                                                         float* __restrict__ part /*[chunks][C][2]*/, float* __restrict__ shift0) {
    __shared__ vf<V> sa[BN_TY(V)][BN_TX(V)], sb[BN_TY(V)][BN_TX(V)];
    const int tx = threadIdx.x & (BN_TX(V) - 1), ty = threadIdx.x / BN_TX(V);
    const int c0 = blockIdx.x * BN_CT + tx * V;
    const long r0 = blockIdx.y * rows_per_chunk, r1 = min(R, r0 + rows_per_chunk);
    vf<V> a = {}, b = {};
    if (c0 < C) {
        const vf<V> sh = ld_x<V, X16>(x, c0);
        if (X16 && blockIdx.y == 0 && ty == 0) vst<V>(shift0 + c0, sh);      // (the finaliser's `x[c]`: row 0 as floats)
#pragma unroll 4
        for (long r = r0 + ty; r < r1; r += BN_TY(V)) {
            const vf<V> v = ld_x<V, X16>(x, r * ldx + c0) - sh;
            a += v; b = bn_acc<V>(b, v, v);
        }
    }
    bn_block_reduce<V>(a, b, sa, sb, part, C, c0, true);
}

// sum the per-chunk partials part[chunk][C][2] for channel c: 64 channels x 16 chunk-lanes per block
// (a serial 512-iteration loop per channel was latency-bound: ~50 us for a kernel that moves a few KB)
#define FIN_TX 64
#define FIN_TY 16
__device__ __forceinline__ void reduce_chunks(const float* __restrict__ part, int chunks, int C, int c, int ty,
                                              double (&s1)[FIN_TY][FIN_TX], double (&s2)[FIN_TY][FIN_TX], double& a, double& b) {
    a = 0.0; b = 0.0;
    if (c < C) {
        const float2* p2 = reinterpret_cast<const float2*>(part) + c;
#pragma unroll 4
        for (int k = ty; k < chunks; k += FIN_TY) { const float2 v = p2[(long)k * C]; a += v.x; b += v.y; }
    }
    const int tx = threadIdx.x;
    s1[ty][tx] = a; s2[ty][tx] = b;
    __syncthreads();
    a = 0.0; b = 0.0;
    for (int j = 0; j < FIN_TY; ++j) { a += s1[j][tx]; b += s2[j][tx]; }
}

// what the statistics of channel c turn into: save_mean / save_rstd for the backward, the running statistics, and the
// coefficients scale / shift of the apply pass.  `var` is the biased variance over R rows.
struct BnFin {
    const float* gamma; const float* beta; float* running_mean; float* running_var; float momentum, eps;
    float* save_mean; float* save_rstd; float* scale; float* shift;
};
__device__ __forceinline__ void bn_finish_channel(int c, double mean, double var, long R, const BnFin& f) {
    if (var < 0.0) var = 0.0;
    const double n = (double)R;
    const float rstd = (float)(1.0 / sqrt(var + (double)f.eps));
    f.save_mean[c] = (float)mean;
    f.save_rstd[c] = rstd;
    // (roundings spelled out -- two rounded products and a rounded sum for the running statistics, one fused step for shift -- so
    // that they do not depend on whether the compiler pairs the two products into one packed multiply or contracts one of them)
    if (f.running_mean != nullptr) {
        const float keep = 1.f - f.momentum;
        f.running_mean[c] = sum_of_rounded_products(keep, f.running_mean[c], f.momentum, (float)mean);
        const double unb = R > 1 ? var * n / (n - 1.0) : var;
        f.running_var[c] = sum_of_rounded_products(keep, f.running_var[c], f.momentum, (float)unb);
    }
    const float sc = f.gamma[c] * rstd;
    f.scale[c] = sc;
    f.shift[c] = fmaf(-(float)mean, sc, f.beta[c]);
}

// x0: the row the partial kernel shifted by (row 0 of x; of a bf16 x, its copy as floats)
__global__ __launch_bounds__(FIN_TX * FIN_TY) void bn_finalize_kernel(const float* __restrict__ part, int chunks, const float* __restrict__ x0, int C, long R,
                                                                      const BnFin f) {
    __shared__ double s1[FIN_TY][FIN_TX], s2[FIN_TY][FIN_TX];
    const int c = blockIdx.x * FIN_TX + threadIdx.x;
    double a, b;
    reduce_chunks(part, chunks, C, c, threadIdx.y, s1, s2, a, b);
    if (c >= C || threadIdx.y != 0) return;
    const double n = (double)R;
    const double dm = a / n;
    bn_finish_channel(c, dm + (double)x0[c], b / n - dm * dm, R, f);
}

// Statistics that arrive as per-row-block (mean, M2) pairs out of the producing GEMM's epilogue (IGemm::stat, gemm_common.h):
// part[(t * C + c) * 2 + {0, 1}], block t covers rows [t rpt, min(R, (t + 1) rpt)).  Combined in fp64 in block order
// (deterministic): mean = sum n_t mean_t / R, M2 = sum (M2_t + n_t mean_t^2) - R mean^2.
#define FT_C 16                                              // channels per block
#define FT_L 64                                              // tile lanes per channel
__global__ __launch_bounds__(FT_C * FT_L) void bn_finalize_tiles_kernel(const float* __restrict__ part, int tiles, long rpt, int C, long R, const BnFin f) {
    // 16 channels x 64 tile lanes per block (C / 16 blocks): with 64 channels per block a 64-channel layer was ONE block walking
    // 1,024 row blocks 16 at a time -- 15 us per call of pure latency, 78 calls per step
    __shared__ double s1[FT_L][FT_C], s2[FT_L][FT_C];
    const int tx = threadIdx.x & (FT_C - 1), ty = threadIdx.x / FT_C;
    const int c = blockIdx.x * FT_C + tx;
    double a = 0.0, b = 0.0;
    if (c < C) {
        const float2* p2 = reinterpret_cast<const float2*>(part) + c;
#pragma unroll 4
        for (int t = ty; t < tiles; t += FT_L) {
            const float2 v = p2[(long)t * C];
            const double n = (double)min(rpt, R - (long)t * rpt), m = (double)v.x;
            a += n * m; b += (double)v.y + n * m * m;
        }
    }
    s1[ty][tx] = a; s2[ty][tx] = b;
    __syncthreads();
    for (int h = FT_L / 2; h >= 1; h >>= 1) {                // fixed tree: deterministic
        if (ty < h) { s1[ty][tx] += s1[ty + h][tx]; s2[ty][tx] += s2[ty + h][tx]; }
        __syncthreads();
    }
    if (c >= C || ty != 0) return;
    a = s1[0][tx]; b = s2[0][tx];
    const double n = (double)R;
    const double mean = a / n;
    bn_finish_channel(c, mean, b / n - mean * mean, R, f);
}
struct TileStats { const float* part; long tiles, rows; };

__global__ void bn_eval_coeff_kernel(int C, const float* __restrict__ gamma, const float* __restrict__ beta,
                                     const float* __restrict__ rm, const float* __restrict__ rv, float eps,
                                     float* __restrict__ scale, float* __restrict__ shift) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const float sc = gamma[c] / sqrtf(rv[c] + eps);
    scale[c] = sc;
    shift[c] = beta[c] - rm[c] * sc;
}

// y = act(scale*x + shift (+ res)).  A streaming pass on the block shape of the reductions: per-channel coefficients live in
// registers, no index division, 4 independent loads per operand in flight per thread.
// y16 (bf16 mode, optional, V = 4): the same values rounded to bf16 beside y, same leading dimension -- the shadow the bf16 GEMMs read
template <int V, bool X16>
__global__ __launch_bounds__(256) void affine_apply_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ scale,
                                                           const float* __restrict__ shift, const float* __restrict__ res, int ldr,
                                                           float* __restrict__ y, int ldy, int C, long R, long rows_per_chunk, int relu,
                                                           unsigned short* __restrict__ y16) {
    const int tx = threadIdx.x & (BN_TX(V) - 1), ty = threadIdx.x / BN_TX(V);
    const int c0 = blockIdx.x * BN_CT + tx * V;
    if (c0 >= C) return;
    const long r0 = blockIdx.y * rows_per_chunk, r1 = min(R, r0 + rows_per_chunk);
    const vf<V> sc = vld<V>(scale + c0), sh = vld<V>(shift + c0);
#pragma unroll 4
    for (long r = r0 + ty; r < r1; r += BN_TY(V)) {
        vf<V> v = vfma<V>(ld_x<V, X16>(x, r * ldx + c0), sc, sh);
        if (res != nullptr) v += vld<V>(res + r * ldr + c0);
        if (relu) {
#pragma unroll
            for (int i = 0; i < V; ++i) v[i] = fmaxf(v[i], 0.f);
        }
        vst<V>(y + r * ldy + c0, v);
        if constexpr (V == 4) if (y16 != nullptr) vst_bf16(y16 + r * ldy + c0, v);
    }
}

// row chunks for the streaming passes: ~4096 blocks, >= 64 rows each
static long apply_rows_per_chunk(int C, long R) {
    static const long blocks = getenv("PDF_BN_APPLY_BLOCKS") ? atol(getenv("PDF_BN_APPLY_BLOCKS")) : 4096;
    long want = blocks / ((C + BN_CT - 1) / BN_CT);
    if (want < 1) want = 1;
    long rpc = (R + want - 1) / want;
    if (rpc < 64) rpc = 64;
    return (rpc + BN_TY(4) - 1) / BN_TY(4) * BN_TY(4);
}
static bool v4_ok(int C, std::initializer_list<int> lds, std::initializer_list<const void*> ptrs) {
    if (C % 4) return false;
    for (int l : lds) if (l % 4) return false;
    for (const void* p : ptrs) if (p != nullptr && (reinterpret_cast<uintptr_t>(p) & 15)) return false;
    return true;
}
// kern<V, X16> in the instantiation the operands allow: <4, true> (bf16 input; the caller checked v4_ok), <4, false>, <1, false>
#define BN_LAUNCH(kern, vec, x16, grid, s, ...)                                                           \
    do {                                                                                                  \
        if (x16) hipLaunchKernelGGL((kern<4, true>), grid, dim3(256), 0, s, __VA_ARGS__);                 \
        else if (vec) hipLaunchKernelGGL((kern<4, false>), grid, dim3(256), 0, s, __VA_ARGS__);           \
        else hipLaunchKernelGGL((kern<1, false>), grid, dim3(256), 0, s, __VA_ARGS__);                    \
    } while (0)

static void launch_affine_apply(const float* x, int ldx, const float* scale, const float* shift, const float* res, int ldr,
                                float* y, int ldy, int C, long R, int relu, hipStream_t s, void* y16 = nullptr, const void* x16 = nullptr) {
    const bool vec = x16 != nullptr || v4_ok(C, {ldx, ldy, res ? ldr : 0}, {x, y, res, scale, shift});      // (x16: the caller checked v4_ok)
    const long rpc = apply_rows_per_chunk(C, R);
    BN_LAUNCH(affine_apply_kernel, vec, x16 != nullptr, dim3(cdiv(C, BN_CT), (unsigned)((R + rpc - 1) / rpc)), s,
              x16 != nullptr ? reinterpret_cast<const float*>(x16) : x, ldx, scale, shift, res, ldr, y, ldy, C, R, rpc, relu, reinterpret_cast<unsigned short*>(y16));
}

// Training forward.  ws: >= pdf_bn_workspace_floats(C, R) floats.  scale/shift [C] are outputs the
// caller keeps for backward-free reuse; save_mean/save_rstd [C] feed the backward.
static long bn_chunks(int C, long R) {
    static const long blocks = getenv("PDF_BN_PARTIAL_BLOCKS") ? atol(getenv("PDF_BN_PARTIAL_BLOCKS")) : 1024;
    static const long cap_env = getenv("PDF_BN_PARTIAL_CAP") ? atol(getenv("PDF_BN_PARTIAL_CAP")) : 0;
    const long ctiles = (C + BN_CT - 1) / BN_CT;
    long want = blocks / ctiles;                            // ~1024 blocks over (channel tiles x chunks)
    // at most 256 chunks -- but at least 512 blocks: a 64-channel tensor (one channel tile: the stem's 1M-row BatchNorm) ran its
    // statistics passes on 256 blocks, one per CU, at 4.3 TB/s; 512 chunks: 5.2 (profiles/r04_bn_chunks_ab.txt; 1024+ lose again)
    const long cap = cap_env > 0 ? cap_env : (512 / ctiles > 256 ? 512 / ctiles : 256);
    if (want > cap) want = cap;
    long by_rows = (R + 63) / 64;                           // at least 64 rows per chunk
    if (want > by_rows) want = by_rows;
    if (want < 1) want = 1;
    return want;
}
// the row chunks of a reduction pass over R rows: `chunks` blocks of `rpc` rows (the last one may be short), none empty
struct BnSplit { long rpc, chunks; };
static BnSplit bn_split(int C, long R) {
    const long want = bn_chunks(C, R);
    const long rpc = (R + want - 1) / want;
    return {rpc, (R + rpc - 1) / rpc};
}
PDF_API long pdf_bn_workspace_floats(int C, long R) {
    long chunks = bn_chunks(C, R);
    return chunks * C * 2 + C;                              // (+ C: row 0 of a bf16 input as floats, the `shift0` of bn_partial_kernel)
}
// bf16 storage mode (PdfCallOpts::bn_x_bf16): pdf_bn_train_fwd / pdf_bn_train_bwd read their input x from a bf16 tensor (same shape and
// leading dimension in elements) instead of the fp32 pointer they are given

static int pdf_bn_train_fwd_impl(const float* x, int ldx, int C, long R, const float* gamma, const float* beta,
                             float* running_mean, float* running_var, float momentum, float eps,
                             const float* res, int ldr, int relu, float* y, int ldy,
                             float* save_mean, float* save_rstd, float* scale, float* shift, float* ws, void* stream, PdfCallOpts& co) {
    hipStream_t s = (hipStream_t)stream;
    void* y16 = co.out_bf16;                                 // bf16 shadow of y, vectorised path only
    const TileStats ts = {co.tile_stats, co.tile_n, co.tile_rows};
    const void* x16 = co.bn_x_bf16;
    if (R <= 0 || C <= 0) return 0;
    if (x16 != nullptr && !v4_ok(C, {ldx, ldy, res ? ldr : 0}, {x16, y, res, scale, shift})) return PDF_E_BADARG;
    const BnFin fin = {gamma, beta, running_mean, running_var, momentum, eps, save_mean, save_rstd, scale, shift};
    const bool from_tiles = ts.part != nullptr;              // statistics came out of the producing GEMM's epilogue: no pass over x
    if (from_tiles) {
        if (ts.tiles * ts.rows < R || (ts.tiles - 1) * ts.rows >= R) return PDF_E_BADARG;
        hipLaunchKernelGGL(bn_finalize_tiles_kernel, dim3(cdiv(C, FT_C)), dim3(FT_C * FT_L), 0, s, ts.part, (int)ts.tiles, ts.rows, C, R, fin);
    } else {
        const BnSplit sp = bn_split(C, R);
        float* shift0 = ws + bn_chunks(C, R) * C * 2;        // X16: row 0 of x as floats, written by the partial kernel
        const bool vec = x16 != nullptr || v4_ok(C, {ldx}, {x});
        BN_LAUNCH(bn_partial_kernel, vec, x16 != nullptr, dim3(cdiv(C, BN_CT), (unsigned)sp.chunks), s,
                  x16 != nullptr ? reinterpret_cast<const float*>(x16) : x, ldx, C, R, sp.rpc, ws, shift0);
        PDF_LAUNCH_CHECK();
        hipLaunchKernelGGL(bn_finalize_kernel, dim3(cdiv(C, FIN_TX)), dim3(FIN_TX, FIN_TY), 0, s, ws, (int)sp.chunks, x16 != nullptr ? shift0 : x, C, R, fin);
    }
    PDF_LAUNCH_CHECK();
    if (y == nullptr) return res == nullptr && y16 == nullptr ? 0 : PDF_E_BADARG;      // statistics and coefficients only: the consumer applies them (pdf_set_input_affine_relu)
    if (x16 == nullptr && y16 != nullptr && !v4_ok(C, {ldx, ldy, res ? ldr : 0}, {x, y, res, scale, shift, y16})) return PDF_E_BADARG;
    launch_affine_apply(x, ldx, scale, shift, res, ldr, y, ldy, C, R, relu, s, y16, x16);
    PDF_LAUNCH_CHECK();
    return 0;
}
PDF_API int pdf_bn_train_fwd_x(const float* x, int ldx, int C, long R, const float* gamma, const float* beta,
                             float* running_mean, float* running_var, float momentum, float eps,
                             const float* res, int ldr, int relu, float* y, int ldy,
                             float* save_mean, float* save_rstd, float* scale, float* shift, float* ws, void* stream, PdfCallOpts* opts) {
    return pdf_call_x(opts, pdf_bn_train_fwd_impl, x, ldx, C, R, gamma, beta, running_mean, running_var, momentum, eps, res, ldr, relu, y, ldy,
                      save_mean, save_rstd, scale, shift, ws, stream);
}
PDF_API int pdf_bn_train_fwd(const float* x, int ldx, int C, long R, const float* gamma, const float* beta,
                             float* running_mean, float* running_var, float momentum, float eps,
                             const float* res, int ldr, int relu, float* y, int ldy,
                             float* save_mean, float* save_rstd, float* scale, float* shift, float* ws, void* stream) {
    return pdf_call_plain(pdf_bn_train_fwd_impl, x, ldx, C, R, gamma, beta, running_mean, running_var, momentum, eps, res, ldr, relu, y, ldy,
                          save_mean, save_rstd, scale, shift, ws, stream);
}


PDF_API int pdf_bn_eval_fwd(const float* x, int ldx, int C, long R, const float* gamma, const float* beta,
                            const float* running_mean, const float* running_var, float eps,
                            const float* res, int ldr, int relu, float* y, int ldy, float* scale, float* shift, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (R <= 0 || C <= 0) return 0;
    hipLaunchKernelGGL(bn_eval_coeff_kernel, dim3(cdiv(C, 128)), dim3(128), 0, s, C, gamma, beta, running_mean, running_var, eps, scale, shift);
    PDF_LAUNCH_CHECK();
    launch_affine_apply(x, ldx, scale, shift, res, ldr, y, ldy, C, R, relu, s);
    PDF_LAUNCH_CHECK();
    return 0;
}

// backward partials: sum(g), sum(g * xhat) with g = dy * (y > 0 if relu)
template <int V, bool X16>
__global__ __launch_bounds__(256) void bn_bwd_partial_kernel(const float* __restrict__ dy, int lddy, const float* __restrict__ y, int ldy, int relu,
                                                             const float* __restrict__ x, int ldx, const float* __restrict__ mean,
                                                             const float* __restrict__ rstd, const float* __restrict__ scale,
                                                             const float* __restrict__ shift, int C, long R, long rows_per_chunk,
                                                             float* __restrict__ part) {
    __shared__ vf<V> sa[BN_TY(V)][BN_TX(V)], sb[BN_TY(V)][BN_TX(V)];
    const int tx = threadIdx.x & (BN_TX(V) - 1), ty = threadIdx.x / BN_TX(V);
    const int c0 = blockIdx.x * BN_CT + tx * V;
    const long r0 = blockIdx.y * rows_per_chunk, r1 = min(R, r0 + rows_per_chunk);
    vf<V> a = {}, b = {};
    if (c0 < C) {
        const vf<V> m = vld<V>(mean + c0), rs = vld<V>(rstd + c0);
        vf<V> sc = {}, sh = {};
        if (relu == 2) { sc = vld<V>(scale + c0); sh = vld<V>(shift + c0); }
#pragma unroll 4
        for (long r = r0 + ty; r < r1; r += BN_TY(V)) {
            vf<V> g = vld<V>(dy + r * lddy + c0);
            const vf<V> xv = ld_x<V, X16>(x, r * ldx + c0);
            g = bn_masked_grad<V>(g, relu, y + r * ldy + c0, xv, sc, sh);
            a += g; b = bn_acc<V>(b, g * (xv - m), rs);
        }
    }
    bn_block_reduce<V>(a, b, sa, sb, part, C, c0, true);
}

__global__ __launch_bounds__(FIN_TX * FIN_TY) void bn_bwd_finalize_kernel(const float* __restrict__ part, int chunks, int C, long R, const float* __restrict__ gamma,
                                       const float* __restrict__ rstd, float* __restrict__ dgamma, float* __restrict__ dbeta, int accumulate,
                                       float* __restrict__ coef /*[3][C]: a, c1, c2*/) {
    __shared__ double s1[FIN_TY][FIN_TX], s2[FIN_TY][FIN_TX];
    const int c = blockIdx.x * FIN_TX + threadIdx.x;
    double a, b;
    reduce_chunks(part, chunks, C, c, threadIdx.y, s1, s2, a, b);
    if (c >= C || threadIdx.y != 0) return;
    if (accumulate) { dbeta[c] += (float)a; dgamma[c] += (float)b; }
    else { dbeta[c] = (float)a; dgamma[c] = (float)b; }
    coef[c] = gamma[c] * rstd[c];
    coef[C + c] = (float)(a / (double)R);
    coef[2 * C + c] = (float)(b / (double)R);
}

// dx = a * (g - c1 - xhat * c2);  dres = g (optional);  dx16 (optional, V = 4): dx rounded to bf16
template <int V, bool X16>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const float* __restrict__ dy, int lddy, const float* __restrict__ y, int ldy, int relu,
                                                           const float* __restrict__ x, int ldx, const float* __restrict__ mean,
                                                           const float* __restrict__ rstd, const float* __restrict__ coef,
                                                           const float* __restrict__ scale, const float* __restrict__ shift, int C, long R,
                                                           long rows_per_chunk, float* __restrict__ dx, int lddx, float* __restrict__ dres, int lddr,
                                                           unsigned short* __restrict__ dx16) {
    const int tx = threadIdx.x & (BN_TX(V) - 1), ty = threadIdx.x / BN_TX(V);
    const int c0 = blockIdx.x * BN_CT + tx * V;
    if (c0 >= C) return;
    const long r0 = blockIdx.y * rows_per_chunk, r1 = min(R, r0 + rows_per_chunk);
    const vf<V> m = vld<V>(mean + c0), rs = vld<V>(rstd + c0);
    const vf<V> ka = vld<V>(coef + c0), k1 = vld<V>(coef + C + c0), k2 = vld<V>(coef + 2 * C + c0);
    vf<V> sc = {}, sh = {};
    if (relu == 2) { sc = vld<V>(scale + c0); sh = vld<V>(shift + c0); }
#pragma unroll 4
    for (long r = r0 + ty; r < r1; r += BN_TY(V)) {
        vf<V> g = vld<V>(dy + r * lddy + c0);
        const vf<V> xv = ld_x<V, X16>(x, r * ldx + c0);
        g = bn_masked_grad<V>(g, relu, y + r * ldy + c0, xv, sc, sh);
        if (dres != nullptr) vst<V>(dres + r * lddr + c0, g);
        const vf<V> o = ka * (g - k1 - (xv - m) * rs * k2);
        if (dx != nullptr) vst<V>(dx + r * lddx + c0, o);
        if constexpr (V == 4) if (dx16 != nullptr) vst_bf16(dx16 + r * lddx + c0, o);
    }
}

// ws: pdf_bn_workspace_floats(C,R) + 3*C floats
// relu: 0 none; 1 ReLU, mask from the saved output y; 2 ReLU without residual, mask recomputed from x with the forward's
// scale / shift (y may be NULL: two fewer full-tensor reads)
static int pdf_bn_train_bwd_impl(const float* dy, int lddy, const float* y, int ldy, int relu, const float* x, int ldx,
                             const float* save_mean, const float* save_rstd, const float* gamma,
                             const float* scale, const float* shift, int C, long R,
                             float* dx, int lddx, float* dres, int lddr, float* dgamma, float* dbeta, int accumulate,
                             float* ws, void* stream, PdfCallOpts& co) {
    hipStream_t s = (hipStream_t)stream;
    void* dx16 = co.out_bf16;                                  // bf16 shadow of dx
    const void* x16 = co.bn_x_bf16;                         // bf16 storage mode: x comes as bf16; dx == NULL: only the bf16 gradient is written
    if (R <= 0 || C <= 0) return 0;
    if ((relu == 1 && y == nullptr) || (relu == 2 && (scale == nullptr || shift == nullptr || dres != nullptr))) return PDF_E_BADARG;
    if (dx == nullptr && dx16 == nullptr) return PDF_E_BADARG;
    const BnSplit sp = bn_split(C, R);
    float* coef = ws + pdf_bn_workspace_floats(C, R);
    const float* xin = x16 != nullptr ? reinterpret_cast<const float*>(x16) : x;
    const bool vec = v4_ok(C, {lddy, ldx, lddx, relu == 1 ? ldy : 0, dres ? lddr : 0},
                           {dy, xin, dx, dres, relu == 1 ? y : nullptr, save_mean, save_rstd, coef, relu == 2 ? scale : nullptr, relu == 2 ? shift : nullptr});
    if ((x16 != nullptr || dx == nullptr) && !vec) return PDF_E_BADARG;
    BN_LAUNCH(bn_bwd_partial_kernel, vec, x16 != nullptr, dim3(cdiv(C, BN_CT), (unsigned)sp.chunks), s, dy, lddy, y, ldy, relu, xin, ldx,
              save_mean, save_rstd, scale, shift, C, R, sp.rpc, ws);
    PDF_LAUNCH_CHECK();
    hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(cdiv(C, FIN_TX)), dim3(FIN_TX, FIN_TY), 0, s, ws, (int)sp.chunks, C, R, gamma, save_rstd, dgamma, dbeta, accumulate, coef);
    PDF_LAUNCH_CHECK();
    if (!vec && dx16 != nullptr) return PDF_E_BADARG;
    const long arpc = apply_rows_per_chunk(C, R);
    BN_LAUNCH(bn_bwd_apply_kernel, vec, x16 != nullptr, dim3(cdiv(C, BN_CT), (unsigned)((R + arpc - 1) / arpc)), s, dy, lddy, y, ldy, relu,
              xin, ldx, save_mean, save_rstd, coef, scale, shift, C, R, arpc, dx, lddx, dres, lddr, reinterpret_cast<unsigned short*>(dx16));
    PDF_LAUNCH_CHECK();
    return 0;
}
PDF_API int pdf_bn_train_bwd_x(const float* dy, int lddy, const float* y, int ldy, int relu, const float* x, int ldx,
                             const float* save_mean, const float* save_rstd, const float* gamma,
                             const float* scale, const float* shift, int C, long R,
                             float* dx, int lddx, float* dres, int lddr, float* dgamma, float* dbeta, int accumulate,
                             float* ws, void* stream, PdfCallOpts* opts) {
    return pdf_call_x(opts, pdf_bn_train_bwd_impl, dy, lddy, y, ldy, relu, x, ldx, save_mean, save_rstd, gamma, scale, shift, C, R, dx, lddx, dres,
                      lddr, dgamma, dbeta, accumulate, ws, stream);
}
PDF_API int pdf_bn_train_bwd(const float* dy, int lddy, const float* y, int ldy, int relu, const float* x, int ldx,
                             const float* save_mean, const float* save_rstd, const float* gamma,
                             const float* scale, const float* shift, int C, long R,
                             float* dx, int lddx, float* dres, int lddr, float* dgamma, float* dbeta, int accumulate,
                             float* ws, void* stream) {
    return pdf_call_plain(pdf_bn_train_bwd_impl, dy, lddy, y, ldy, relu, x, ldx, save_mean, save_rstd, gamma, scale, shift, C, R, dx, lddx, dres,
                          lddr, dgamma, dbeta, accumulate, ws, stream);
}

// ---- backward with FROZEN statistics (forward: pdf_bn_eval_fwd).  The statistics do not depend on x, so no mean term reaches dx:
//   g = dy * mask;  dx = g * scale;  dres = g;  dbeta = sum g;  dgamma = sum g * xhat,  xhat = (x - running_mean) * rsqrt(running_var + eps)
// ONE streaming pass (dy, x -> dx; y / dres with a residual) where the training backward makes two over (dy, x); the per-chunk sums
// it leaves in `part` are finished by bn_eval_bwd_finalize_kernel.  xhat comes from the running statistics, never from
// (y - beta) / gamma: a channel with gamma == 0 still has a dgamma.  SUMS == false (neither parameter wants a gradient): purely
// element-wise -- no partials, no LDS, no second launch, and x is read only to recompute the mask (relu == 2).
template <int V, bool SUMS>
__global__ __launch_bounds__(256) void bn_eval_bwd_kernel(const float* __restrict__ dy, int lddy, const float* __restrict__ y, int ldy, int relu,
                                                          const float* __restrict__ x, int ldx, const float* __restrict__ rmean,
                                                          const float* __restrict__ rvar, float eps, const float* __restrict__ scale,
                                                          const float* __restrict__ shift, int C, long R, long rows_per_chunk,
                                                          float* __restrict__ dx, int lddx, float* __restrict__ dres, int lddr,
                                                          float* __restrict__ part) {
    const int tx = threadIdx.x & (BN_TX(V) - 1), ty = threadIdx.x / BN_TX(V);
    const int c0 = blockIdx.x * BN_CT + tx * V;
    const long r0 = blockIdx.y * rows_per_chunk, r1 = min(R, r0 + rows_per_chunk);
    vf<V> a = {}, b = {};
    if (c0 < C) {
        vf<V> m = {}, rs = {}, sc = {}, sh = {};
        if (SUMS) { m = vld<V>(rmean + c0); rs = vrsqrt_eps<V>(vld<V>(rvar + c0), eps); }
        if (dx != nullptr || relu == 2) sc = vld<V>(scale + c0);
        if (relu == 2) sh = vld<V>(shift + c0);
        const bool need_x = SUMS || relu == 2;
#pragma unroll 4
        for (long r = r0 + ty; r < r1; r += BN_TY(V)) {
            vf<V> g = vld<V>(dy + r * lddy + c0), xv = {};
            if (need_x) xv = vld<V>(x + r * ldx + c0);
            g = bn_masked_grad<V>(g, relu, y + r * ldy + c0, xv, sc, sh);
            if (dres != nullptr) vst<V>(dres + r * lddr + c0, g);
            if (dx != nullptr) vst<V>(dx + r * lddx + c0, g * sc);
            if (SUMS) { a += g; b = bn_acc<V>(b, g * (xv - m), rs); }
        }
    }
    if constexpr (SUMS) {
        __shared__ vf<V> sa[BN_TY(V)][BN_TX(V)], sb[BN_TY(V)][BN_TX(V)];
        bn_block_reduce<V>(a, b, sa, sb, part, C, c0, true);
    }
}

// the chunk partials (sum g, sum g * xhat) in a fixed order, in double -> dbeta, dgamma (either may be NULL)
__global__ __launch_bounds__(FIN_TX * FIN_TY) void bn_eval_bwd_finalize_kernel(const float* __restrict__ part, int chunks, int C,
                                                                               float* __restrict__ dgamma, float* __restrict__ dbeta, int accumulate) {
    __shared__ double s1[FIN_TY][FIN_TX], s2[FIN_TY][FIN_TX];
    const int c = blockIdx.x * FIN_TX + threadIdx.x;
    double a, b;
    reduce_chunks(part, chunks, C, c, threadIdx.y, s1, s2, a, b);
    if (c >= C || threadIdx.y != 0) return;
    if (dbeta != nullptr) { if (accumulate) dbeta[c] += (float)a; else dbeta[c] = (float)a; }
    if (dgamma != nullptr) { if (accumulate) dgamma[c] += (float)b; else dgamma[c] = (float)b; }
}

PDF_API int pdf_bn_eval_bwd(const float* dy, int lddy, const float* y, int ldy, int relu, const float* x, int ldx,
                            const float* running_mean, const float* running_var, float eps, const float* scale, const float* shift,
                            int C, long R, float* dx, int lddx, float* dres, int lddr,
                            float* dgamma, float* dbeta, int accumulate, float* ws, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (R <= 0 || C <= 0) return 0;
    const bool sums = dgamma != nullptr || dbeta != nullptr;
    const bool need_x = sums || relu == 2;
    if (relu < 0 || relu > 2 || dy == nullptr) return PDF_E_BADARG;
    if ((relu == 1 && y == nullptr) || (relu == 2 && (scale == nullptr || shift == nullptr || dres != nullptr))) return PDF_E_BADARG;
    if ((need_x && x == nullptr) || (dx != nullptr && scale == nullptr)) return PDF_E_BADARG;
    if (sums && (running_mean == nullptr || running_var == nullptr || ws == nullptr)) return PDF_E_BADARG;
    if (!sums && dx == nullptr && dres == nullptr) return 0;
    const BnSplit sp = bn_split(C, R);
    const bool use_sc = dx != nullptr || relu == 2;
    const bool vec = v4_ok(C, {lddy, need_x ? ldx : 0, dx ? lddx : 0, relu == 1 ? ldy : 0, dres ? lddr : 0},
                           {dy, need_x ? x : nullptr, dx, dres, relu == 1 ? y : nullptr, sums ? running_mean : nullptr, sums ? running_var : nullptr,
                            use_sc ? scale : nullptr, relu == 2 ? shift : nullptr});
    const long rpc = sums ? sp.rpc : apply_rows_per_chunk(C, R);      // element-wise: the finer chunks of the streaming passes
    const dim3 grid(cdiv(C, BN_CT), (unsigned)((R + rpc - 1) / rpc));
#define EVAL_BWD(V, SUMS) hipLaunchKernelGGL((bn_eval_bwd_kernel<V, SUMS>), grid, dim3(256), 0, s, dy, lddy, y, ldy, relu, x, ldx, running_mean, running_var, \
                                             eps, scale, shift, C, R, rpc, dx, lddx, dres, lddr, sums ? ws : nullptr)
    if (vec) { if (sums) EVAL_BWD(4, true); else EVAL_BWD(4, false); }
    else { if (sums) EVAL_BWD(1, true); else EVAL_BWD(1, false); }
#undef EVAL_BWD
    PDF_LAUNCH_CHECK();
    if (sums) {
        hipLaunchKernelGGL(bn_eval_bwd_finalize_kernel, dim3(cdiv(C, FIN_TX)), dim3(FIN_TX, FIN_TY), 0, s, ws, (int)sp.chunks, C, dgamma, dbeta, accumulate);
        PDF_LAUNCH_CHECK();
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------
// Set-abstraction tail (intaghand_encoder.py:59-62,79-82,97-100: BatchNorm2d -> ReLU -> MaxPool2d over the K neighbours) in
// one pass over the convolution output y [R][K][C]: out[r][c] = max_k relu(fma(y, scale, shift)), arg = first k attaining it.
// The normalised tensor (537 MB per hand at level 1) is never written; the backward rebuilds the gradient of y from
// (dout, arg, y): its two BatchNorm sums only involve the R*C selected elements.
__global__ __launch_bounds__(256) void bn_relu_maxk_fwd_kernel(const float* __restrict__ y, int ldy, const float* __restrict__ scale,
                                                               const float* __restrict__ shift, int C, int K, float* __restrict__ out, int ldo,
                                                               int* __restrict__ arg, long total /* R * C/4 */) {
    const int cq = C / 4;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long r = i / cq;
        const int c0 = (int)(i - r * cq) * 4;
        const float4 sc = *reinterpret_cast<const float4*>(scale + c0), sh = *reinterpret_cast<const float4*>(shift + c0);
        const float* p = y + r * K * ldy + c0;
        float4 best = make_float4(-1.f, -1.f, -1.f, -1.f);            // relu output is >= 0: the first k always wins against -1
        int4 bi = make_int4(0, 0, 0, 0);
#pragma unroll 4
        for (int k = 0; k < K; ++k) {
            const float4 v = *reinterpret_cast<const float4*>(p + (long)k * ldy);
            const float zx = fmaxf(fmaf(v.x, sc.x, sh.x), 0.f), zy = fmaxf(fmaf(v.y, sc.y, sh.y), 0.f);
            const float zz = fmaxf(fmaf(v.z, sc.z, sh.z), 0.f), zw = fmaxf(fmaf(v.w, sc.w, sh.w), 0.f);
            if (zx > best.x) { best.x = zx; bi.x = k; }
            if (zy > best.y) { best.y = zy; bi.y = k; }
            if (zz > best.z) { best.z = zz; bi.z = k; }
            if (zw > best.w) { best.w = zw; bi.w = k; }
        }
        *reinterpret_cast<float4*>(out + r * ldo + c0) = best;
        *reinterpret_cast<int4*>(arg + r * C + c0) = bi;
    }
}
// partial sums over the rows r of g = dout * [z > 0] and g * xhat at the selected neighbour (same [chunks][C][2] layout as
// bn_bwd_partial_kernel, so bn_bwd_finalize_kernel finishes them)
__global__ __launch_bounds__(256) void bn_maxk_bwd_partial_kernel(const float* __restrict__ dm, int lddm, const int* __restrict__ arg,
                                                                  const float* __restrict__ y, int ldy, const float* __restrict__ mean,
                                                                  const float* __restrict__ rstd, const float* __restrict__ scale,
                                                                  const float* __restrict__ shift, int C, int K, long R, long rows_per_chunk,
                                                                  float* __restrict__ part) {
    __shared__ vf<4> sa[BN_TY(4)][BN_TX(4)], sb[BN_TY(4)][BN_TX(4)];
    const int tx = threadIdx.x & (BN_TX(4) - 1), ty = threadIdx.x / BN_TX(4);
    const int c0 = blockIdx.x * BN_CT + tx * 4;
    const long r0 = blockIdx.y * rows_per_chunk, r1 = min(R, r0 + rows_per_chunk);
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
    if (c0 < C) {
        const float4 m = *reinterpret_cast<const float4*>(mean + c0), rs = *reinterpret_cast<const float4*>(rstd + c0);
        const float4 sc = *reinterpret_cast<const float4*>(scale + c0), sh = *reinterpret_cast<const float4*>(shift + c0);
        for (long r = r0 + ty; r < r1; r += BN_TY(4)) {
            const float4 g4 = *reinterpret_cast<const float4*>(dm + r * lddm + c0);
            const int4 k4 = *reinterpret_cast<const int4*>(arg + r * C + c0);
            const float* base = y + r * K * ldy + c0;
            const float vx = base[(long)k4.x * ldy], vy = base[(long)k4.y * ldy + 1], vz = base[(long)k4.z * ldy + 2], vw = base[(long)k4.w * ldy + 3];
            const float gx = fmaf(vx, sc.x, sh.x) > 0.f ? g4.x : 0.f, gy = fmaf(vy, sc.y, sh.y) > 0.f ? g4.y : 0.f;
            const float gz = fmaf(vz, sc.z, sh.z) > 0.f ? g4.z : 0.f, gw = fmaf(vw, sc.w, sh.w) > 0.f ? g4.w : 0.f;
            a.x += gx; a.y += gy; a.z += gz; a.w += gw;
            b.x += gx * (vx - m.x) * rs.x; b.y += gy * (vy - m.y) * rs.y; b.z += gz * (vz - m.z) * rs.z; b.w += gw * (vw - m.w) * rs.w;
        }
    }
    bn_block_reduce<4>(as_vf(a), as_vf(b), sa, sb, part, C, c0, true);
}
// dy[r][k][c] = a * (g - c1 - xhat * c2), g = dout[r][c] where k == arg[r][c] and the ReLU was active, else 0
__global__ __launch_bounds__(256) void bn_maxk_bwd_apply_kernel(const float* __restrict__ dm, int lddm, const int* __restrict__ arg,
                                                                const float* __restrict__ y, int ldy, const float* __restrict__ mean,
                                                                const float* __restrict__ rstd, const float* __restrict__ coef,
                                                                const float* __restrict__ scale, const float* __restrict__ shift, int C, int K,
                                                                float* __restrict__ dy, int lddy, long total /* R * C/4 */) {
    const int cq = C / 4;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long r = i / cq;
        const int c0 = (int)(i - r * cq) * 4;
        const float4 m = *reinterpret_cast<const float4*>(mean + c0), rs = *reinterpret_cast<const float4*>(rstd + c0);
        const float4 ka = *reinterpret_cast<const float4*>(coef + c0), k1 = *reinterpret_cast<const float4*>(coef + C + c0),
                     k2 = *reinterpret_cast<const float4*>(coef + 2 * C + c0);
        const float4 sc = *reinterpret_cast<const float4*>(scale + c0), sh = *reinterpret_cast<const float4*>(shift + c0);
        const float4 g4 = *reinterpret_cast<const float4*>(dm + r * lddm + c0);
        const int4 k4 = *reinterpret_cast<const int4*>(arg + r * C + c0);
        const float* p = y + r * K * ldy + c0;
        float* q = dy + r * K * lddy + c0;
#pragma unroll 4
        for (int k = 0; k < K; ++k) {
            const float4 v = *reinterpret_cast<const float4*>(p + (long)k * ldy);
            const float gx = (k == k4.x && fmaf(v.x, sc.x, sh.x) > 0.f) ? g4.x : 0.f, gy = (k == k4.y && fmaf(v.y, sc.y, sh.y) > 0.f) ? g4.y : 0.f;
            const float gz = (k == k4.z && fmaf(v.z, sc.z, sh.z) > 0.f) ? g4.z : 0.f, gw = (k == k4.w && fmaf(v.w, sc.w, sh.w) > 0.f) ? g4.w : 0.f;
            float4 o;
            o.x = ka.x * (gx - k1.x - (v.x - m.x) * rs.x * k2.x);
            o.y = ka.y * (gy - k1.y - (v.y - m.y) * rs.y * k2.y);
            o.z = ka.z * (gz - k1.z - (v.z - m.z) * rs.z * k2.z);
            o.w = ka.w * (gw - k1.w - (v.w - m.w) * rs.w * k2.w);
            *reinterpret_cast<float4*>(q + (long)k * lddy) = o;
        }
    }
}
// training != 0: batch statistics over all R*K rows (running statistics updated with `momentum`); else running statistics.
// C % 4 == 0, 16-byte aligned rows.  ws: pdf_bn_workspace_floats(C, R*K) floats.
static int pdf_bn_relu_maxk_fwd_impl(const float* y, int ldy, int C, long R, int K, const float* gamma, const float* beta,
                                 float* running_mean, float* running_var, float momentum, float eps, int training,
                                 float* out, int ldo, int* arg, float* save_mean, float* save_rstd, float* scale, float* shift,
                                 float* ws, void* stream, PdfCallOpts& co) {
    hipStream_t s = (hipStream_t)stream;
    if (R <= 0 || C <= 0 || K <= 0) return 0;
    if (!v4_ok(C, {ldy, ldo}, {y, out, arg, scale, shift})) return PDF_E_BADARG;
    const long rows = R * K;
    const TileStats ts = {co.tile_stats, co.tile_n, co.tile_rows};
    const BnFin fin = {gamma, beta, running_mean, running_var, momentum, eps, save_mean, save_rstd, scale, shift};
    if (training && ts.part != nullptr) {
        if (ts.tiles * ts.rows < rows || (ts.tiles - 1) * ts.rows >= rows) return PDF_E_BADARG;
        hipLaunchKernelGGL(bn_finalize_tiles_kernel, dim3(cdiv(C, FT_C)), dim3(FT_C * FT_L), 0, s, ts.part, (int)ts.tiles, ts.rows, C, rows, fin);
    } else if (training) {
        const BnSplit sp = bn_split(C, rows);
        hipLaunchKernelGGL((bn_partial_kernel<4, false>), dim3(cdiv(C, BN_CT), (unsigned)sp.chunks), dim3(256), 0, s, y, ldy, C, rows, sp.rpc, ws, (float*)nullptr);
        hipLaunchKernelGGL(bn_finalize_kernel, dim3(cdiv(C, FIN_TX)), dim3(FIN_TX, FIN_TY), 0, s, ws, (int)sp.chunks, y, C, rows, fin);
    } else {
        hipLaunchKernelGGL(bn_eval_coeff_kernel, dim3(cdiv(C, 128)), dim3(128), 0, s, C, gamma, beta, running_mean, running_var, eps, scale, shift);
    }
    PDF_LAUNCH_CHECK();
    const long total = R * (C / 4);
    hipLaunchKernelGGL(bn_relu_maxk_fwd_kernel, dim3(grid_for(total)), dim3(256), 0, s, y, ldy, scale, shift, C, K, out, ldo, arg, total);
    PDF_LAUNCH_CHECK();
    return 0;
}
PDF_API int pdf_bn_relu_maxk_fwd_x(const float* y, int ldy, int C, long R, int K, const float* gamma, const float* beta,
                                 float* running_mean, float* running_var, float momentum, float eps, int training,
                                 float* out, int ldo, int* arg, float* save_mean, float* save_rstd, float* scale, float* shift,
                                 float* ws, void* stream, PdfCallOpts* opts) {
    return pdf_call_x(opts, pdf_bn_relu_maxk_fwd_impl, y, ldy, C, R, K, gamma, beta, running_mean, running_var, momentum, eps, training, out, ldo,
                      arg, save_mean, save_rstd, scale, shift, ws, stream);
}
PDF_API int pdf_bn_relu_maxk_fwd(const float* y, int ldy, int C, long R, int K, const float* gamma, const float* beta,
                                 float* running_mean, float* running_var, float momentum, float eps, int training,
                                 float* out, int ldo, int* arg, float* save_mean, float* save_rstd, float* scale, float* shift,
                                 float* ws, void* stream) {
    return pdf_call_plain(pdf_bn_relu_maxk_fwd_impl, y, ldy, C, R, K, gamma, beta, running_mean, running_var, momentum, eps, training, out, ldo, arg,
                          save_mean, save_rstd, scale, shift, ws, stream);
}

// ws: pdf_bn_workspace_floats(C, R) + 3*C floats
PDF_API int pdf_bn_relu_maxk_bwd(const float* dout, int lddo, const int* arg, const float* y, int ldy, const float* save_mean, const float* save_rstd,
                                 const float* gamma, const float* scale, const float* shift, int C, long R, int K,
                                 float* dy, int lddy, float* dgamma, float* dbeta, int accumulate, float* ws, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (R <= 0 || C <= 0 || K <= 0) return 0;
    if (!v4_ok(C, {ldy, lddo, lddy}, {y, dout, dy, arg, save_mean, save_rstd, scale, shift, ws})) return PDF_E_BADARG;
    const BnSplit sp = bn_split(C, R);
    float* coef = ws + pdf_bn_workspace_floats(C, R);
    hipLaunchKernelGGL(bn_maxk_bwd_partial_kernel, dim3(cdiv(C, BN_CT), (unsigned)sp.chunks), dim3(256), 0, s, dout, lddo, arg, y, ldy, save_mean, save_rstd,
                       scale, shift, C, K, R, sp.rpc, ws);
    // the statistics were taken over R*K rows: the means of the backward are over R*K as well
    hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(cdiv(C, FIN_TX)), dim3(FIN_TX, FIN_TY), 0, s, ws, (int)sp.chunks, C, R * K, gamma, save_rstd, dgamma, dbeta, accumulate, coef);
    const long total = R * (C / 4);
    hipLaunchKernelGGL(bn_maxk_bwd_apply_kernel, dim3(grid_for(total)), dim3(256), 0, s, dout, lddo, arg, y, ldy, save_mean, save_rstd, coef,
                       scale, shift, C, K, dy, lddy, total);
    PDF_LAUNCH_CHECK();
    return 0;
}

// ---- the same tail with FROZEN statistics (forward: training == 0).  No mean term reaches the rows that lost the max, so their
// gradient is an exact zero and y is needed only at the R*C selected elements.  Of the two possible shapes -- a zero fill of dy
// followed by a scatter of the selected elements, or the apply kernel's walk over k -- this is the walk: dy is written exactly
// once, in whole float4 rows (the scatter would write 4-byte pieces into rows the fill has just streamed out, behind a second
// launch), and y is still not streamed: each thread gathers its four selected elements before the loop.
__global__ __launch_bounds__(256) void bn_maxk_eval_bwd_partial_kernel(const float* __restrict__ dm, int lddm, const int* __restrict__ arg,
                                                                       const float* __restrict__ y, int ldy, const float* __restrict__ rmean,
                                                                       const float* __restrict__ rvar, float eps, const float* __restrict__ scale,
                                                                       const float* __restrict__ shift, int C, int K, long R, long rows_per_chunk,
                                                                       float* __restrict__ part) {
    __shared__ vf<4> sa[BN_TY(4)][BN_TX(4)], sb[BN_TY(4)][BN_TX(4)];
    const int tx = threadIdx.x & (BN_TX(4) - 1), ty = threadIdx.x / BN_TX(4);
    const int c0 = blockIdx.x * BN_CT + tx * 4;
    const long r0 = blockIdx.y * rows_per_chunk, r1 = min(R, r0 + rows_per_chunk);
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
    if (c0 < C) {
        const float4 m = *reinterpret_cast<const float4*>(rmean + c0), var = *reinterpret_cast<const float4*>(rvar + c0);
        const float4 rs = make_float4(1.f / sqrtf(var.x + eps), 1.f / sqrtf(var.y + eps), 1.f / sqrtf(var.z + eps), 1.f / sqrtf(var.w + eps));
        const float4 sc = *reinterpret_cast<const float4*>(scale + c0), sh = *reinterpret_cast<const float4*>(shift + c0);
        for (long r = r0 + ty; r < r1; r += BN_TY(4)) {
            const float4 g4 = *reinterpret_cast<const float4*>(dm + r * lddm + c0);
            const int4 k4 = *reinterpret_cast<const int4*>(arg + r * C + c0);
            const float* base = y + r * K * ldy + c0;
            const float vx = base[(long)k4.x * ldy], vy = base[(long)k4.y * ldy + 1], vz = base[(long)k4.z * ldy + 2], vw = base[(long)k4.w * ldy + 3];
            const float gx = fmaf(vx, sc.x, sh.x) > 0.f ? g4.x : 0.f, gy = fmaf(vy, sc.y, sh.y) > 0.f ? g4.y : 0.f;
            const float gz = fmaf(vz, sc.z, sh.z) > 0.f ? g4.z : 0.f, gw = fmaf(vw, sc.w, sh.w) > 0.f ? g4.w : 0.f;
            a.x += gx; a.y += gy; a.z += gz; a.w += gw;
            b.x += gx * (vx - m.x) * rs.x; b.y += gy * (vy - m.y) * rs.y; b.z += gz * (vz - m.z) * rs.z; b.w += gw * (vw - m.w) * rs.w;
        }
    }
    bn_block_reduce<4>(as_vf(a), as_vf(b), sa, sb, part, C, c0, true);
}
// dy[r][k][c] = dout[r][c] * scale[c] where k == arg[r][c] and the ReLU was active, else 0
__global__ __launch_bounds__(256) void bn_maxk_eval_bwd_apply_kernel(const float* __restrict__ dm, int lddm, const int* __restrict__ arg,
                                                                     const float* __restrict__ y, int ldy, const float* __restrict__ scale,
                                                                     const float* __restrict__ shift, int C, int K,
                                                                     float* __restrict__ dy, int lddy, long total /* R * C/4 */) {
    const int cq = C / 4;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long r = i / cq;
        const int c0 = (int)(i - r * cq) * 4;
        const float4 sc = *reinterpret_cast<const float4*>(scale + c0), sh = *reinterpret_cast<const float4*>(shift + c0);
        const float4 g4 = *reinterpret_cast<const float4*>(dm + r * lddm + c0);
        const int4 k4 = *reinterpret_cast<const int4*>(arg + r * C + c0);
        const float* p = y + r * K * ldy + c0;
        const float ox = fmaf(p[(long)k4.x * ldy], sc.x, sh.x) > 0.f ? g4.x * sc.x : 0.f, oy = fmaf(p[(long)k4.y * ldy + 1], sc.y, sh.y) > 0.f ? g4.y * sc.y : 0.f;
        const float oz = fmaf(p[(long)k4.z * ldy + 2], sc.z, sh.z) > 0.f ? g4.z * sc.z : 0.f, ow = fmaf(p[(long)k4.w * ldy + 3], sc.w, sh.w) > 0.f ? g4.w * sc.w : 0.f;
        float* q = dy + r * K * lddy + c0;
#pragma unroll 4
        for (int k = 0; k < K; ++k)
            *reinterpret_cast<float4*>(q + (long)k * lddy) = make_float4(k == k4.x ? ox : 0.f, k == k4.y ? oy : 0.f, k == k4.z ? oz : 0.f, k == k4.w ? ow : 0.f);
    }
}
// ws: pdf_bn_workspace_floats(C, R) floats when sums are asked for.  dgamma == dbeta == NULL: the apply launch alone.  dy == NULL: sums only.
// arg must hold indices in [0, K) (what the forward wrote).
PDF_API int pdf_bn_relu_maxk_eval_bwd(const float* dout, int lddo, const int* arg, const float* y, int ldy,
                                      const float* running_mean, const float* running_var, float eps, const float* scale, const float* shift,
                                      int C, long R, int K, float* dy, int lddy, float* dgamma, float* dbeta, int accumulate, float* ws, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (R <= 0 || C <= 0 || K <= 0) return 0;
    const bool sums = dgamma != nullptr || dbeta != nullptr;
    if (dout == nullptr || arg == nullptr || y == nullptr || scale == nullptr || shift == nullptr) return PDF_E_BADARG;
    if (sums && (running_mean == nullptr || running_var == nullptr || ws == nullptr)) return PDF_E_BADARG;
    if (!v4_ok(C, {ldy, lddo, dy ? lddy : 0}, {y, dout, dy, arg, scale, shift, sums ? running_mean : nullptr, sums ? running_var : nullptr})) return PDF_E_BADARG;
    if (sums) {
        const BnSplit sp = bn_split(C, R);
        hipLaunchKernelGGL(bn_maxk_eval_bwd_partial_kernel, dim3(cdiv(C, BN_CT), (unsigned)sp.chunks), dim3(256), 0, s, dout, lddo, arg, y, ldy,
                           running_mean, running_var, eps, scale, shift, C, K, R, sp.rpc, ws);
        PDF_LAUNCH_CHECK();
        hipLaunchKernelGGL(bn_eval_bwd_finalize_kernel, dim3(cdiv(C, FIN_TX)), dim3(FIN_TX, FIN_TY), 0, s, ws, (int)sp.chunks, C, dgamma, dbeta, accumulate);
        PDF_LAUNCH_CHECK();
    }
    if (dy != nullptr) {
        const long total = R * (C / 4);
        hipLaunchKernelGGL(bn_maxk_eval_bwd_apply_kernel, dim3(grid_for(total)), dim3(256), 0, s, dout, lddo, arg, y, ldy, scale, shift, C, K, dy, lddy, total);
        PDF_LAUNCH_CHECK();
    }
    return 0;
}

// column sums: out[c] (+)= sum_r g[r][c]   (conv / linear bias gradients), optional relu mask by y
__global__ __launch_bounds__(FIN_TX * FIN_TY) void colsum_finalize_kernel(const float* __restrict__ part, int chunks, int C, float* __restrict__ out,
                                                                          float* __restrict__ out1, int accumulate) {
    __shared__ double s1[FIN_TY][FIN_TX], s2[FIN_TY][FIN_TX];
    if (blockIdx.y) { part += (long)chunks * C * 2; out = out1; }
    const int c = blockIdx.x * FIN_TX + threadIdx.x;
    double a, b;
    reduce_chunks(part, chunks, C, c, threadIdx.y, s1, s2, a, b);
    if (c >= C || threadIdx.y != 0) return;
    out[c] = (accumulate ? out[c] : 0.f) + (float)a;
}

// (blockIdx.z == 1 is group 1 of a paired call -- rows [R, 2R), partials after group 0's)
template <int V>
__global__ __launch_bounds__(256) void colsum_partial_kernel(const float* __restrict__ g, int ldg, int C, long R, long rows_per_chunk, float* __restrict__ part) {
    __shared__ vf<V> sa[BN_TY(V)][BN_TX(V)], sb[BN_TY(V)][BN_TX(V)];
    if (blockIdx.z) { g += R * ldg; part += (long)gridDim.y * C * 2; }
    const int tx = threadIdx.x & (BN_TX(V) - 1), ty = threadIdx.x / BN_TX(V);
    const int c0 = blockIdx.x * BN_CT + tx * V;
    const long r0 = blockIdx.y * rows_per_chunk, r1 = min(R, r0 + rows_per_chunk);
    vf<V> a = {};
    if (c0 < C) {
#pragma unroll 4
        for (long r = r0 + ty; r < r1; r += BN_TY(V)) a += vld<V>(g + r * ldg + c0);
    }
    bn_block_reduce<V>(a, a, sa, sb, part, C, c0, false);
}

static int colsum_launch(const float* g, int ldg, int C, long R, float* out, float* out1, int accumulate, float* ws, hipStream_t s) {
    if (R <= 0 || C <= 0) return 0;
    const unsigned groups = out1 ? 2 : 1;
    const BnSplit sp = bn_split(C, R);
    const dim3 grid(cdiv(C, BN_CT), (unsigned)sp.chunks, groups);
    if (v4_ok(C, {ldg, (int)((R * ldg) % 4)}, {g}))
        hipLaunchKernelGGL(colsum_partial_kernel<4>, grid, dim3(256), 0, s, g, ldg, C, R, sp.rpc, ws);
    else
        hipLaunchKernelGGL(colsum_partial_kernel<1>, grid, dim3(256), 0, s, g, ldg, C, R, sp.rpc, ws);
    PDF_LAUNCH_CHECK();
    hipLaunchKernelGGL(colsum_finalize_kernel, dim3(cdiv(C, FIN_TX), groups), dim3(FIN_TX, FIN_TY), 0, s, ws, (int)sp.chunks, C, out, out1, accumulate);
    PDF_LAUNCH_CHECK();
    return 0;
}
int pdf_internal_colsum(const float* g, int ldg, int C, long R, float* out, int accumulate, float* ws, hipStream_t s) {
    return colsum_launch(g, ldg, C, R, out, nullptr, accumulate, ws, s);
}
long pdf_internal_colsum_ws(int C, long R) { return pdf_bn_workspace_floats(C, R); }
PDF_API int pdf_colsum(const float* g, int ldg, int C, long R, float* out, int accumulate, float* ws, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    return colsum_launch(g, ldg, C, R, out, nullptr, accumulate, ws, s);
}
// paired bias gradients: rows [0, R) -> out0, rows [R, 2R) -> out1; ws >= 2 * pdf_bn_workspace_floats(C, R)
PDF_API int pdf_colsum_pair(const float* g, int ldg, int C, long R, float* out0, float* out1, int accumulate, float* ws, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    return colsum_launch(g, ldg, C, R, out0, out1, accumulate, ws, s);
}

// ---------------------------------------------------------------------------------------------
// LayerNorm over the last axis (F <= 1024), one wave per row (nn.LayerNorm(eps=1e-6) in model_attn/*).
#define LN_MAXV 16
// One kernel family serves the plain op and the decoder's fused forms (gcn.py:100-110, self_attn.py:24-33,78-84):
//   z = x + dropout(add)      (optional; z is written out because it is also the residual the next block adds)
//   y = act( LayerNorm(z) * gamma_g + beta_g ),  g = 0 for rows < R_split, 1 otherwise (left / right hand parameters)
// blockIdx.y = group, so a block's dgamma / dbeta partial sums belong to one parameter set.
__global__ __launch_bounds__(256) void layernorm_fwd_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ add, int ldadd,
                                                            float p, unsigned long long seed, const unsigned long long* __restrict__ step,
                                                            int F, long R, long R_split, const float* __restrict__ gamma0, const float* __restrict__ beta0,
                                                            const float* __restrict__ gamma1, const float* __restrict__ beta1, float eps, int act,
                                                            float* __restrict__ z, int ldz, float* __restrict__ y, int ldy,
                                                            float* __restrict__ mean, float* __restrict__ rstd) {
    const int lane = threadIdx.x & 63;
    const long rb = blockIdx.y ? R_split : 0, re = blockIdx.y ? R : min(R, R_split);
    const float* __restrict__ gamma = blockIdx.y ? gamma1 : gamma0;
    const float* __restrict__ beta = blockIdx.y ? beta1 : beta0;
    const long w0 = (blockIdx.x * (long)blockDim.x + threadIdx.x) >> 6;
    const long nw = ((long)gridDim.x * blockDim.x) >> 6;
    const float sc = 1.f / (1.f - p);
    if (add != nullptr && p > 0.f && step != nullptr) seed += step[0] * 0x9E3779B97F4A7C15ull;
    for (long r = rb + w0; r < re; r += nw) {
        float v[LN_MAXV];
        float sum = 0.f;
#pragma unroll
        for (int i = 0; i < LN_MAXV; ++i) {
            int c = lane + 64 * i;
            float t = 0.f;
            if (c < F) {
                t = x[r * ldx + c];
                if (add != nullptr) {
                    float a = add[r * ldadd + c];
                    if (p > 0.f) a = pdf_uniform(seed, (unsigned long long)(r * F + c)) >= p ? a * sc : 0.f;
                    t += a;
                    z[r * ldz + c] = t;
                }
            }
            v[i] = t;
            sum += t;
        }
        const float mu = wave_sum(sum) / (float)F;
        float sq = 0.f;
#pragma unroll
        for (int i = 0; i < LN_MAXV; ++i) {
            int c = lane + 64 * i;
            float d = c < F ? v[i] - mu : 0.f;
            sq += d * d;
        }
        const float rs = 1.0f / sqrtf(wave_sum(sq) / (float)F + eps);
#pragma unroll
        for (int i = 0; i < LN_MAXV; ++i) {
            int c = lane + 64 * i;
            if (c < F) {
                float o = (v[i] - mu) * rs * gamma[c] + beta[c];
                if (act == 1) o = fmaxf(o, 0.f);
                y[r * ldy + c] = o;
            }
        }
        if (lane == 0) { mean[r] = mu; rstd[r] = rs; }
    }
}

static int ln_fwd_launch(const float* x, int ldx, const float* add, int ldadd, float p, unsigned long long seed, const unsigned long long* step,
                         int F, long R, long R_split, const float* g0, const float* b0, const float* g1, const float* b1, float eps, int act,
                         float* z, int ldz, float* y, int ldy, float* mean, float* rstd, hipStream_t s) {
    if (F > 64 * LN_MAXV || (add != nullptr && z == nullptr)) return PDF_E_BADARG;
    if (R <= 0) return 0;
    const unsigned groups = R_split < R ? 2 : 1;
    const long rows = groups == 2 ? max(R_split, R - R_split) : R;
    hipLaunchKernelGGL(layernorm_fwd_kernel, dim3(grid_for(rows * 64), groups), dim3(256), 0, s, x, ldx, add, ldadd, p, seed, step, F, R, R_split,
                       g0, b0, g1, b1, eps, act, z, ldz, y, ldy, mean, rstd);
    PDF_LAUNCH_CHECK();
    return 0;
}
PDF_API int pdf_layernorm_fwd(const float* x, int ldx, int F, long R, const float* gamma, const float* beta, float eps,
                              float* y, int ldy, float* mean, float* rstd, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    return ln_fwd_launch(x, ldx, nullptr, 0, 0.f, 0, nullptr, F, R, R, gamma, beta, gamma, beta, eps, 0, nullptr, 0, y, ldy, mean, rstd, s);
}
// fused / paired form, see the kernel comment.  add == NULL: plain LayerNorm input (z unused).  R_split >= R: one parameter set.
PDF_API int pdf_layernorm_fused_fwd(const float* x, int ldx, const float* add, int ldadd, float p, unsigned long long seed,
                                    const unsigned long long* step, int F, long R, long R_split,
                                    const float* gamma0, const float* beta0, const float* gamma1, const float* beta1, float eps, int act,
                                    float* z, int ldz, float* y, int ldy, float* mean, float* rstd, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    return ln_fwd_launch(x, ldx, add, ldadd, p, seed, step, F, R, R_split, gamma0, beta0, gamma1, beta1, eps, act, z, ldz, y, ldy, mean, rstd, s);
}

// dz = rstd * (g - mean(g) - xhat * mean(g*xhat)) [+ dz_in], g = dy * act'(y) * gamma; dgamma += sum dy' * xhat; dbeta += sum dy'
// dadd = dropout-mask(dz) (the gradient of the dropped operand); dz itself is the gradient of x (the residual operand).
// (dgamma/dbeta accumulated with one atomic per channel per block; caller zero-fills or accumulates)
// DZ: write dz / dadd (the data gradient, on the dependent chain); PARAMS: accumulate dgamma / dbeta.  The two halves can be
// launched separately: the parameter half then runs on the weight-gradient side stream, and the chain's half has no atomics
// (512 blocks adding into the same 2 F addresses were most of the one-shot kernel's 28 us).
template <bool DZ, bool PARAMS>
__global__ __launch_bounds__(256) void layernorm_bwd_kernel(const float* __restrict__ dy, int lddy, const float* __restrict__ y, int ldy, int act,
                                                            const float* __restrict__ zin, int ldz, int F, long R, long R_split,
                                                            const float* __restrict__ gamma0, const float* __restrict__ gamma1,
                                                            const float* __restrict__ mean, const float* __restrict__ rstd,
                                                            const float* __restrict__ dz_in, int lddzin, float* __restrict__ dz, int lddz,
                                                            float* __restrict__ dadd, int lddadd, float p, unsigned long long seed,
                                                            const unsigned long long* __restrict__ step,
                                                            float* __restrict__ dgamma0, float* __restrict__ dbeta0,
                                                            float* __restrict__ dgamma1, float* __restrict__ dbeta1) {
    __shared__ float sg[PARAMS ? 64 * LN_MAXV : 1], sb[PARAMS ? 64 * LN_MAXV : 1];
    if constexpr (PARAMS) {
        for (int i = threadIdx.x; i < F; i += 256) { sg[i] = 0.f; sb[i] = 0.f; }
        __syncthreads();
    }
    const int lane = threadIdx.x & 63;
    const long rb = blockIdx.y ? R_split : 0, re = blockIdx.y ? R : min(R, R_split);
    const float* __restrict__ gamma = blockIdx.y ? gamma1 : gamma0;
    float* __restrict__ dgamma = blockIdx.y ? dgamma1 : dgamma0;
    float* __restrict__ dbeta = blockIdx.y ? dbeta1 : dbeta0;
    const long w0 = (blockIdx.x * (long)blockDim.x + threadIdx.x) >> 6;
    const long nw = ((long)gridDim.x * blockDim.x) >> 6;
    const float sc = 1.f / (1.f - p);
    if (dadd != nullptr && p > 0.f && step != nullptr) seed += step[0] * 0x9E3779B97F4A7C15ull;
    float ag[LN_MAXV], ab[LN_MAXV];
#pragma unroll
    for (int i = 0; i < LN_MAXV; ++i) { ag[i] = 0.f; ab[i] = 0.f; }
    for (long r = rb + w0; r < re; r += nw) {
        const float mu = mean[r], rs = rstd[r];
        float g[LN_MAXV], xh[LN_MAXV];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < LN_MAXV; ++i) {
            int c = lane + 64 * i;
            float d = 0.f, h = 0.f;
            if (c < F) {
                d = dy[r * lddy + c];
                if (act == 1 && !(y[r * ldy + c] > 0.f)) d = 0.f;
                h = (zin[r * ldz + c] - mu) * rs;
                if constexpr (PARAMS) { ag[i] += d * h; ab[i] += d; }
                d *= gamma[c];
            }
            g[i] = d; xh[i] = h;
            s1 += d; s2 += d * h;
        }
        if constexpr (!DZ) continue;
        s1 = wave_sum(s1) / (float)F;
        s2 = wave_sum(s2) / (float)F;
#pragma unroll
        for (int i = 0; i < LN_MAXV; ++i) {
            int c = lane + 64 * i;
            if (c < F) {
                float o = rs * (g[i] - s1 - xh[i] * s2);
                if (dz_in != nullptr) o += dz_in[r * lddzin + c];
                dz[r * lddz + c] = o;
                if (dadd != nullptr) {
                    if (p > 0.f) o = pdf_uniform(seed, (unsigned long long)(r * F + c)) >= p ? o * sc : 0.f;
                    dadd[r * lddadd + c] = o;
                }
            }
        }
    }
    if constexpr (PARAMS) {
#pragma unroll
        for (int i = 0; i < LN_MAXV; ++i) {
            int c = lane + 64 * i;
            if (c < F) { atomicAdd(&sg[c], ag[i]); atomicAdd(&sb[c], ab[i]); }
        }
        __syncthreads();
        for (int i = threadIdx.x; i < F; i += 256) {
            if (dgamma != nullptr) atomicAdd(&dgamma[i], sg[i]);
            if (dbeta != nullptr) atomicAdd(&dbeta[i], sb[i]);
        }
    }
}

static int ln_bwd_launch(const float* dy, int lddy, const float* y, int ldy, int act, const float* z, int ldz, int F, long R, long R_split,
                         const float* g0, const float* g1, const float* mean, const float* rstd, const float* dz_in, int lddzin,
                         float* dz, int lddz, float* dadd, int lddadd, float p, unsigned long long seed, const unsigned long long* step,
                         float* dg0, float* db0, float* dg1, float* db1, hipStream_t s) {
    if (F > 64 * LN_MAXV || (act == 1 && y == nullptr)) return PDF_E_BADARG;
    if (R <= 0) return 0;
    const unsigned groups = R_split < R ? 2 : 1;
    const long rows = groups == 2 ? max(R_split, R - R_split) : R;
    const bool params = dg0 != nullptr || db0 != nullptr || dg1 != nullptr || db1 != nullptr;
    if (dz == nullptr && !params) return 0;
    if (dz == nullptr && (dadd != nullptr || dz_in != nullptr)) return PDF_E_BADARG;
    // one-shot / parameter half: few blocks (every block ends with 2 F same-address atomics); data half: one row per wave
    const int grid = grid_for(rows * 64, 256, dz == nullptr ? 128 : params ? 512 : 4096);
#define LN_BWD(DZ_, PA_) hipLaunchKernelGGL((layernorm_bwd_kernel<DZ_, PA_>), dim3(grid, groups), dim3(256), 0, s, dy, lddy, y, ldy, act, z, ldz, F, R, \
                       R_split, g0, g1, mean, rstd, dz_in, lddzin, dz, lddz, dadd, lddadd, p, seed, step, dg0, db0, dg1, db1)
    if (dz == nullptr) LN_BWD(false, true); else if (params) LN_BWD(true, true); else LN_BWD(true, false);
#undef LN_BWD
    PDF_LAUNCH_CHECK();
    return 0;
}
PDF_API int pdf_layernorm_bwd(const float* dy, int lddy, const float* x, int ldx, int F, long R, const float* gamma,
                              const float* mean, const float* rstd, float* dx, int lddx, float* dgamma, float* dbeta, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    return ln_bwd_launch(dy, lddy, nullptr, 0, 0, x, ldx, F, R, R, gamma, gamma, mean, rstd, nullptr, 0, dx, lddx, nullptr, 0, 0.f, 0, nullptr,
                         dgamma, dbeta, dgamma, dbeta, s);
}
PDF_API int pdf_layernorm_fused_bwd(const float* dy, int lddy, const float* y, int ldy, int act, const float* z, int ldz, int F, long R, long R_split,
                                    const float* gamma0, const float* gamma1, const float* mean, const float* rstd,
                                    const float* dz_in, int lddzin, float* dz, int lddz, float* dadd, int lddadd,
                                    float p, unsigned long long seed, const unsigned long long* step,
                                    float* dgamma0, float* dbeta0, float* dgamma1, float* dbeta1, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    return ln_bwd_launch(dy, lddy, y, ldy, act, z, ldz, F, R, R_split, gamma0, gamma1, mean, rstd, dz_in, lddzin, dz, lddz, dadd, lddadd, p, seed, step,
                         dgamma0, dbeta0, dgamma1, dbeta1, s);
}

// ---------------------------------------------------------------------------------------------
// L2Norm (intaghand_encoder.py:318-334): y = w[c] * x / (sqrt(sum_c x^2) + 1e-10), one wave per pixel.
__global__ __launch_bounds__(256) void l2norm_fwd_kernel(const float* __restrict__ x, int ldx, int C, long R, const float* __restrict__ w,
                                                         float eps, float* __restrict__ y, int ldy, float* __restrict__ norm) {
    const int lane = threadIdx.x & 63;
    const long w0 = (blockIdx.x * (long)blockDim.x + threadIdx.x) >> 6;
    const long nw = ((long)gridDim.x * blockDim.x) >> 6;
    for (long r = w0; r < R; r += nw) {
        float sq = 0.f;
        for (int c = lane; c < C; c += 64) { float v = x[r * ldx + c]; sq += v * v; }
        const float n = sqrtf(wave_sum(sq)) + eps;
        for (int c = lane; c < C; c += 64) y[r * ldy + c] = w[c] * (x[r * ldx + c] / n);
        if (lane == 0) norm[r] = n;
    }
}

PDF_API int pdf_l2norm_fwd(const float* x, int ldx, int C, long R, const float* w, float eps, float* y, int ldy, float* norm, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (R <= 0) return 0;
    hipLaunchKernelGGL(l2norm_fwd_kernel, dim3(grid_for(R * 64)), dim3(256), 0, s, x, ldx, C, R, w, eps, y, ldy, norm);
    PDF_LAUNCH_CHECK();
    return 0;
}

// dx_j = w_j g_j / n - x_j * (sum_c w_c g_c x_c) / (n^2 * (n - eps));  dw_c += sum_r g_c x_c / n
#define L2_MAXV 8     // channels per lane: C <= 512
__global__ __launch_bounds__(256) void l2norm_bwd_kernel(const float* __restrict__ dy, int lddy, const float* __restrict__ x, int ldx, int C, long R,
                                                         const float* __restrict__ w, float eps, const float* __restrict__ norm,
                                                         float* __restrict__ dx, int lddx, float* __restrict__ dw) {
    extern __shared__ float sw[];
    for (int i = threadIdx.x; i < C; i += 256) sw[i] = 0.f;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const long w0 = (blockIdx.x * (long)blockDim.x + threadIdx.x) >> 6;
    const long nw = ((long)gridDim.x * blockDim.x) >> 6;
    float acc[L2_MAXV], wv[L2_MAXV];
#pragma unroll
    for (int i = 0; i < L2_MAXV; ++i) { acc[i] = 0.f; int c = lane + 64 * i; wv[i] = c < C ? w[c] : 0.f; }
    for (long r = w0; r < R; r += nw) {
        const float n = norm[r];
        float g[L2_MAXV], xv[L2_MAXV];
        float dot = 0.f;
#pragma unroll
        for (int i = 0; i < L2_MAXV; ++i) {
            int c = lane + 64 * i;
            g[i] = c < C ? dy[r * lddy + c] : 0.f;
            xv[i] = c < C ? x[r * ldx + c] : 0.f;
            dot += wv[i] * g[i] * xv[i];
        }
        dot = wave_sum(dot);
        const float nn = n - eps;
        const float k = nn > 0.f ? dot / (n * n * nn) : 0.f;
        const float in = 1.f / n;
#pragma unroll
        for (int i = 0; i < L2_MAXV; ++i) {
            int c = lane + 64 * i;
            if (c < C) dx[r * lddx + c] = wv[i] * g[i] * in - xv[i] * k;
            acc[i] += g[i] * xv[i] * in;                     // dw partial stays in registers across this wave's rows
        }
    }
#pragma unroll
    for (int i = 0; i < L2_MAXV; ++i) { int c = lane + 64 * i; if (c < C) atomicAdd(&sw[c], acc[i]); }
    __syncthreads();
    for (int i = threadIdx.x; i < C; i += 256) atomicAdd(&dw[i], sw[i]);
}

PDF_API int pdf_l2norm_bwd(const float* dy, int lddy, const float* x, int ldx, int C, long R, const float* w, float eps,
                           const float* norm, float* dx, int lddx, float* dw, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (R <= 0) return 0;
    if (C > 64 * L2_MAXV) return PDF_E_BADARG;
    int grid = grid_for(R * 64, 256, 1024);
    hipLaunchKernelGGL(l2norm_bwd_kernel, dim3(grid), dim3(256), C * sizeof(float), s, dy, lddy, x, ldx, C, R, w, eps, norm, dx, lddx, dw);
    PDF_LAUNCH_CHECK();
    return 0;
}

// ---- the pyramid form (intaghand_encoder.py:724-739): up to 4 maps L2-normalised into / out of ONE concatenated NHWC buffer
// in ONE launch (blockIdx.y = part).  One launch per part reads a 1 KB slice of every 4 KB row of the concatenated gradient,
// i.e. a quarter of the HBM channels at a time: measured 529 us per part against 87 us on contiguous rows.
#define L2_MAXPARTS 4
struct L2Parts {
    const float* x[L2_MAXPARTS]; const float* w[L2_MAXPARTS]; float* norm[L2_MAXPARTS]; float* dx[L2_MAXPARTS]; float* dw[L2_MAXPARTS];
    unsigned short* dx16[L2_MAXPARTS];                   // optional bf16 shadows of dx (bf16 mode)
    int C[L2_MAXPARTS], off[L2_MAXPARTS];
};
__global__ __launch_bounds__(256) void l2norm_cat_fwd_kernel(const L2Parts p, long R, float eps, float* __restrict__ y, int ldy,
                                                             unsigned short* __restrict__ y16) {
    const int part = blockIdx.y, C = p.C[part], lane = threadIdx.x & 63;
    const float* __restrict__ x = p.x[part]; const float* __restrict__ w = p.w[part];
    float* __restrict__ yo = y + p.off[part];
    const long w0 = (blockIdx.x * (long)blockDim.x + threadIdx.x) >> 6;
    const long nw = ((long)gridDim.x * blockDim.x) >> 6;
    for (long r = w0; r < R; r += nw) {
        float sq = 0.f;
        for (int c = lane; c < C; c += 64) { float v = x[r * C + c]; sq += v * v; }
        const float n = sqrtf(wave_sum(sq)) + eps;
        for (int c = lane; c < C; c += 64) {
            const float v = w[c] * (x[r * C + c] / n);
            yo[r * ldy + c] = v;
            if (y16 != nullptr) {                            // bf16 shadow: lanes pair up so that 4-byte words are written
                const float vn = __shfl_down(v, 1, 64);
                if ((lane & 1) == 0) *reinterpret_cast<unsigned int*>(y16 + p.off[part] + r * ldy + c) = pdf_pk_bf16(v, vn);
            }
        }
        if (lane == 0) p.norm[part][r] = n;
    }
}
// 256-channel parts (the pyramid): a lane owns 4 consecutive channels -- one 16-byte load per row, the row stays in registers for
// the second pass, two rows per wave in flight (the generic form above re-reads the row with 4-byte accesses: 2.8 TB/s by counters)
__global__ __launch_bounds__(256) void l2norm_cat_fwd_c256_kernel(const L2Parts p, long R, float eps, float* __restrict__ y, int ldy,
                                                                  unsigned short* __restrict__ y16) {
    typedef float v4f __attribute__((ext_vector_type(4)));
    typedef unsigned int v2u __attribute__((ext_vector_type(2)));
    const int part = blockIdx.y, lane = threadIdx.x & 63;
    const float* __restrict__ x = p.x[part];
    float* __restrict__ yo = y + p.off[part];
    const v4f wv = reinterpret_cast<const v4f*>(p.w[part])[lane];
    const long w0 = (blockIdx.x * (long)blockDim.x + threadIdx.x) >> 6;
    const long nw = ((long)gridDim.x * blockDim.x) >> 6;
    for (long r = w0; r < R; r += 2 * nw) {
        const long r1 = r + nw;
        const bool two = r1 < R;
        const v4f a = reinterpret_cast<const v4f*>(x + r * 256)[lane];
        v4f b = {0.f, 0.f, 0.f, 0.f};
        if (two) b = reinterpret_cast<const v4f*>(x + r1 * 256)[lane];
        const float na = sqrtf(wave_sum(a.x * a.x + a.y * a.y + a.z * a.z + a.w * a.w)) + eps;
        const float nb = sqrtf(wave_sum(b.x * b.x + b.y * b.y + b.z * b.z + b.w * b.w)) + eps;
        const v4f oa = {wv.x * (a.x / na), wv.y * (a.y / na), wv.z * (a.z / na), wv.w * (a.w / na)};
        *reinterpret_cast<v4f*>(yo + r * ldy + 4 * lane) = oa;
        if (y16 != nullptr) *reinterpret_cast<v2u*>(y16 + p.off[part] + r * ldy + 4 * lane) = v2u{pdf_pk_bf16(oa.x, oa.y), pdf_pk_bf16(oa.z, oa.w)};
        if (lane == 0) p.norm[part][r] = na;
        if (two) {
            const v4f ob = {wv.x * (b.x / nb), wv.y * (b.y / nb), wv.z * (b.z / nb), wv.w * (b.w / nb)};
            *reinterpret_cast<v4f*>(yo + r1 * ldy + 4 * lane) = ob;
            if (y16 != nullptr) *reinterpret_cast<v2u*>(y16 + p.off[part] + r1 * ldy + 4 * lane) = v2u{pdf_pk_bf16(ob.x, ob.y), pdf_pk_bf16(ob.z, ob.w)};
            if (lane == 0) p.norm[part][r1] = nb;
        }
    }
}
template <int MAXV>
__global__ __launch_bounds__(256) void l2norm_cat_bwd_kernel(const L2Parts p, long R, float eps, const float* __restrict__ dy, int lddy) {
    // blockIdx.y = part, one wave per pixel.  Kept light on registers (MAXV = channels per lane: 4 for the 256-channel pyramid):
    // this kernel runs beside the `feat` weight gradient, whose three resident blocks per CU leave ~80 VGPRs per SIMD lane free -- a
    // walk over all four parts per wave (96 VGPRs) could not co-reside at all and took 4.9 ms there (0.3 ms alone); this form 2.5.
    // (The same trimming of the BatchNorm backward kernels -- 100 -> 54-80 VGPRs via unroll 2-3 -- was measured and is neutral in fp32,
    // -2 % in bf16 where they run alone more often.)
    __shared__ float sw[64 * MAXV];
    const int q = blockIdx.y, C = p.C[q], lane = threadIdx.x & 63;
    const float* __restrict__ x = p.x[q]; const float* __restrict__ w = p.w[q]; const float* __restrict__ norm = p.norm[q];
    const float* __restrict__ g0 = dy + p.off[q];
    float* __restrict__ dx = p.dx[q];
    unsigned short* __restrict__ dx16 = p.dx16[q];
    for (int i = threadIdx.x; i < C; i += 256) sw[i] = 0.f;
    __syncthreads();
    const long w0 = (blockIdx.x * (long)blockDim.x + threadIdx.x) >> 6;
    const long nw = ((long)gridDim.x * blockDim.x) >> 6;
    float acc[MAXV], wv[MAXV];
#pragma unroll
    for (int i = 0; i < MAXV; ++i) { acc[i] = 0.f; const int c = lane + 64 * i; wv[i] = c < C ? w[c] : 0.f; }
    for (long r = w0; r < R; r += nw) {
        const float n = norm[r];
        float g[MAXV], xv[MAXV];
        float dot = 0.f;
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            const int c = lane + 64 * i;
            g[i] = c < C ? g0[r * lddy + c] : 0.f;
            xv[i] = c < C ? x[r * C + c] : 0.f;
            dot += wv[i] * g[i] * xv[i];
        }
        dot = wave_sum(dot);
        const float nn = n - eps;
        const float k = nn > 0.f ? dot / (n * n * nn) : 0.f;
        const float in = 1.f / n;
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            const int c = lane + 64 * i;
            const float o = wv[i] * g[i] * in - xv[i] * k;
            if (c < C) dx[r * C + c] = o;
            if (dx16 != nullptr) {                            // (C % 64 == 0 then: whole waves, lanes pair up for 4-byte words)
                const float on = __shfl_down(o, 1, 64);
                if (c < C && (lane & 1) == 0) *reinterpret_cast<unsigned int*>(dx16 + r * C + c) = pdf_pk_bf16(o, on);
            }
            acc[i] += g[i] * xv[i] * in;
        }
    }
#pragma unroll
    for (int i = 0; i < MAXV; ++i) { const int c = lane + 64 * i; if (c < C) atomicAdd(&sw[c], acc[i]); }
    __syncthreads();
    for (int i = threadIdx.x; i < C; i += 256) atomicAdd(&p.dw[q][i], sw[i]);
}
static int l2_parts(L2Parts& p, int nparts, const float* const* x, const float* const* w, float* const* norm, float* const* dx, float* const* dw,
                    const int* C) {
    if (nparts < 1 || nparts > L2_MAXPARTS) return PDF_E_BADARG;
    int off = 0;
    for (int i = 0; i < nparts; ++i) {
        if (C[i] <= 0 || C[i] > 64 * L2_MAXV) return PDF_E_BADARG;
        p.x[i] = x[i]; p.w[i] = w[i]; p.norm[i] = norm[i]; p.dx[i] = dx ? dx[i] : nullptr; p.dw[i] = dw ? dw[i] : nullptr;
        p.C[i] = C[i]; p.off[i] = off;
        off += C[i];
    }
    return 0;
}
// x[i]: [R][C[i]] contiguous rows; y: [R][ldy] with part i at channel offset C[0] + ... + C[i-1]; norm[i]: [R]
static int pdf_l2norm_cat_fwd_impl(int nparts, const float* const* x, const int* C, const float* const* w, float eps, long R,
                               float* y, int ldy, float* const* norm, void* stream, PdfCallOpts& co) {
    hipStream_t s = (hipStream_t)stream;
    void* y16 = co.out_bf16;                                 // bf16 shadow of y (needs even channel counts)
    if (R <= 0) return 0;
    L2Parts p = {};
    if (int rc = l2_parts(p, nparts, x, w, norm, nullptr, nullptr, C)) return rc;
    for (int i = 0; y16 != nullptr && i < nparts; ++i) if (C[i] % 64) return PDF_E_BADARG;
    bool c256 = ldy % 4 == 0 && (reinterpret_cast<uintptr_t>(y) & 15) == 0 && (y16 == nullptr || (reinterpret_cast<uintptr_t>(y16) & 7) == 0);
    for (int i = 0; i < nparts; ++i)
        c256 = c256 && C[i] == 256 && p.off[i] % 4 == 0 && (reinterpret_cast<uintptr_t>(x[i]) & 15) == 0 && (reinterpret_cast<uintptr_t>(w[i]) & 15) == 0;
    if (c256) hipLaunchKernelGGL(l2norm_cat_fwd_c256_kernel, dim3(grid_for(R * 32, 256, 4096), nparts), dim3(256), 0, s, p, R, eps, y, ldy,
                                 reinterpret_cast<unsigned short*>(y16));
    else hipLaunchKernelGGL(l2norm_cat_fwd_kernel, dim3(grid_for(R * 64, 256, 2048), nparts), dim3(256), 0, s, p, R, eps, y, ldy,
                            reinterpret_cast<unsigned short*>(y16));
    PDF_LAUNCH_CHECK();
    return 0;
}
PDF_API int pdf_l2norm_cat_fwd_x(int nparts, const float* const* x, const int* C, const float* const* w, float eps, long R,
                               float* y, int ldy, float* const* norm, void* stream, PdfCallOpts* opts) {
    return pdf_call_x(opts, pdf_l2norm_cat_fwd_impl, nparts, x, C, w, eps, R, y, ldy, norm, stream);
}
PDF_API int pdf_l2norm_cat_fwd(int nparts, const float* const* x, const int* C, const float* const* w, float eps, long R,
                               float* y, int ldy, float* const* norm, void* stream) {
    return pdf_call_plain(pdf_l2norm_cat_fwd_impl, nparts, x, C, w, eps, R, y, ldy, norm, stream);
}

// dw[i] must be zero-filled (atomically accumulated)
PDF_API int pdf_l2norm_cat_bwd(int nparts, const float* dy, int lddy, const float* const* x, const int* C, const float* const* w, float eps, long R,
                               float* const* norm, float* const* dx, float* const* dw, void* const* dx16, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (R <= 0) return 0;
    L2Parts p = {};
    if (int rc = l2_parts(p, nparts, x, w, norm, dx, dw, C)) return rc;
    for (int i = 0; dx16 != nullptr && i < nparts; ++i) {
        if (dx16[i] != nullptr && C[i] % 64) return PDF_E_BADARG;
        p.dx16[i] = reinterpret_cast<unsigned short*>(dx16[i]);
    }
    int cmax = 0;
    for (int i = 0; i < nparts; ++i) cmax = max(cmax, C[i]);
    const dim3 grid(grid_for(R * 64, 256, 1024), nparts);
    if (cmax <= 256) hipLaunchKernelGGL(l2norm_cat_bwd_kernel<4>, grid, dim3(256), 0, s, p, R, eps, dy, lddy);
    else hipLaunchKernelGGL(l2norm_cat_bwd_kernel<L2_MAXV>, grid, dim3(256), 0, s, p, R, eps, dy, lddy);
    PDF_LAUNCH_CHECK();
    return 0;
}
