// Shared helpers for the gfx950 kernels of libpdfnet_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "pdfnet_hip.h"      // the public contract: every PDF_API definition below is compiled against its prototype, the argument blocks are its structs

// Every entry point returns 0 on success or a negative PDF_E_* / positive hipError_t code (pdfnet_hip.h).
#define PDF_API extern "C" __attribute__((visibility("default")))

#define PDF_LAUNCH_CHECK()                                  \
    do {                                                    \
        hipError_t e__ = hipGetLastError();                 \
        if (e__ != hipSuccess) return (int)e__;             \
    } while (0)

static inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// memory-bound launches: cap the grid and grid-stride the rest (guide: Guideline 11)
static inline int grid_for(long n, int block = 256, int cap = 256 * 8) {
    long g = (n + block - 1) / block;
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return (int)g;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// stateless counter RNG for dropout masks (same mask regenerated in backward from seed+index)
__device__ __forceinline__ uint32_t pdf_hash32(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
    return x;
}
__device__ __forceinline__ float pdf_uniform(uint64_t seed, uint64_t idx) {
    uint32_t h = pdf_hash32((uint32_t)idx ^ pdf_hash32((uint32_t)(idx >> 32) + (uint32_t)seed) ^ (uint32_t)(seed >> 32) * 0x9E3779B9U);
    return (float)(h >> 8) * (1.0f / 16777216.0f);
}

// Scratch for the split-K partial sums of the small-M GEMMs (entry points without a workspace argument): a 256 MiB ring
// allocated once (pdf_init), handed out in launch order.  One use takes at most 16 MiB and a train step a few tens of MiB, so
// a region comes round again only several steps later -- far beyond what the launch queue can hold in flight.
#define PDF_SCRATCH_RING (1L << 26)
#define PDF_SCRATCH_MAX (1L << 22)
float* pdf_scratch(long floats);
// Column sums of a [R][C] matrix through the BatchNorm partial-sum kernels (norm.hip); ws: pdf_internal_colsum_ws(C, R) floats
int pdf_internal_colsum(const float* g, int ldg, int C, long R, float* out, int accumulate, float* ws, hipStream_t s);
long pdf_internal_colsum_ws(int C, long R);
// bf16 packing: the shadows (PdfCallOpts below) and the x3 components are written with these
typedef __bf16 pdf_bf16x2 __attribute__((ext_vector_type(2)));
typedef float pdf_f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned int pdf_pk_bf16(float a, float b) {      // two floats -> packed bf16 pair, round-to-nearest-even
    pdf_f32x2 f = {a, b};
    pdf_bf16x2 v = __builtin_convertvector(f, pdf_bf16x2);
    return *reinterpret_cast<unsigned int*>(&v);
}
// x3 arithmetic (gemm_x3.hip): a fp32 pair -> its three bf16 components, packed pairs h / m / l with a = h + m + l exactly
__device__ __forceinline__ void pdf_x3_split2(float a, float b, unsigned& h, unsigned& m, unsigned& l) {
    h = pdf_pk_bf16(a, b);
    float ra = a - __uint_as_float(h << 16), rb = b - __uint_as_float(h & 0xffff0000u);
    m = pdf_pk_bf16(ra, rb);
    ra -= __uint_as_float(m << 16); rb -= __uint_as_float(m & 0xffff0000u);
    l = pdf_pk_bf16(ra, rb);
}
// ... stored at element offsets o, o + cs, o + 2 cs of a bf16 tensor (o even)
__device__ __forceinline__ void pdf_x3_store2(unsigned short* base, long o, long cs, float a, float b) {
    unsigned h, m, l;
    pdf_x3_split2(a, b, h, m, l);
    *reinterpret_cast<unsigned*>(base + o) = h;
    *reinterpret_cast<unsigned*>(base + o + cs) = m;
    *reinterpret_cast<unsigned*>(base + o + 2 * cs) = l;
}
// PdfCallOpts (pdfnet_hip.h): everything a call may take beyond its positional arguments.  An entry point that takes options has ONE body,
// `int name_impl(positional arguments..., void* stream, PdfCallOpts& co)`, and two exported one-line forms that forward to it through the two
// helpers below -- the only places that know the calling conventions.
// `_x` form: opts == NULL means an all-zero block; stats_tiles / stats_rows are zeroed before the body looks at an argument; the thread's
// hand-over slots are not touched.
template <class F, class... A> static inline int pdf_call_x(PdfCallOpts* opts, F impl, A... a) {
    PdfCallOpts none = {};
    PdfCallOpts& co = opts != nullptr ? *opts : none;
    co.stats_tiles = co.stats_rows = 0;
    return impl(a..., co);
}
// plain form: take AND CLEAR every slot the pdf_set_* functions armed on this thread first thing (constructor), so no return path of the body
// leaves one armed; afterwards publish stats_tiles / stats_rows for pdf_stats_result_* (destructor).  The slots themselves are private to
// elementwise.hip, which defines both.
struct PdfPlainCall { PdfCallOpts co; PdfPlainCall(); ~PdfPlainCall(); };
template <class F, class... A> static inline int pdf_call_plain(F impl, A... a) {
    PdfPlainCall call;
    return impl(a..., call.co);
}
