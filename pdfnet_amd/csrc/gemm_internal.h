// Host functions that gemm.hip, winograd.hip and gemm_x3.hip call in each other: declared once here, and every defining file includes
// this header, so a changed signature is a compile error instead of a silent mismatch at link time.
#pragma once
#include "common.h"

// ---- gemm.hip: batched launches of the fp32 MFMA kernels
int pdf_internal_batched_gemm(const float* A, const float* B, float* C, int batch, long gsA, long gsB, long gsC, int M, int N, int K, hipStream_t s);
int pdf_internal_batched_wgemm(const float* P, const float* Q, float* slab, int batch, long gsP, long gsQ, int M, int NI, int NJ, int splits, hipStream_t s);

// ---- workspace plans.  A launch that works in a caller's workspace is planned ONCE, by one function of its shape: whether the layer takes
// the path at all, which form, and where every buffer lies.  The size queries of the header return plan.total, the call sites of gemm.hip
// check it against the workspace they were handed, and the launchers take the plan: none of them works out a size, an offset or a format.
struct WsRegion { long off, len; };                          // floats from the start of the workspace

// winograd.hip: forward (flip = 0: x -> y, Ck = Cin, Cn = Cout) or backward-data (flip = 1: dy -> dx, Ck = Cout, Cn = Cin) of a stride-1 3x3 convolution
struct WinoPlan {
    int ok;                                                  // the layer takes the Winograd path (else total = 0 and nothing else is set)
    int N, H, W, Ck, Cn, flip;
    int m;                                                   // output tile edge: 4 = F(4x4, 3x3), 2 = F(2x2, 3x3)
    long T, P;                                               // tiles, planes ((m + 2)^2)
    int x3;                                                  // U and V are x3 planes (6 bytes per element) and the products run in gemm_x3.hip
    int shared_v_x3;                                         // format of a V handed in from another forward's workspace (PdfCallOpts::wino_v): used only when == x3; -1: none can exist
    WsRegion U, V, M;
    long total;
    long v_offset;                                           // forward: V.off when the weight gradient of the same layer may read V from there, else -1
};
WinoPlan wino_plan(int N, int H, int W, int Ck, int Cn, int KH, int KW, int stride, int pad, int flip);
int pdf_internal_conv3x3_winograd(const WinoPlan& p, const float* x, int ldx, const float* w, const float* bias, float* y, int ldy, float* ws,
                                  int act, int accum, const float* v_shared, hipStream_t s);
// winograd.hip: the F(4x4) weight gradient
struct WinoWgradPlan {
    int ok;
    int N, H, W, Cin, Cout;
    long T;
    int x3;                                                  // V and Yh are x3 planes
    int shared_v_x3;                                         // format of the V the forward of this layer leaves at its v_offset; -1: that forward is not F(4x4)
    int splits;
    WsRegion V, Yh, slab, colsum;
    long total;
};
WinoWgradPlan wino_wgrad_plan(int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad);
int pdf_internal_conv3x3_winograd_wgrad(const WinoWgradPlan& p, const float* x, int ldx, const float* dy, int lddy, float* dw, float* db, float* ws,
                                        int accumulate, const float* v_cached, hipStream_t s);

// ---- gemm_x3.hip: fp32 products on the bf16 matrix pipe
int pdf_internal_x3_mode();                                  // bit 0 = the Winograd transform-domain products, bit 1 = the transposed convolutions, bit 2 = the mesh decoder (PDF_X3*, pdf_set_x3_mode)
int pdf_internal_x3_batched_gemm(const void* A3, long csA, const void* B3, long csB, float* C, int batch, long gsA, long gsB, long gsC,
                                 int M, int N, int K, int variant, int nprod, hipStream_t s);
int pdf_internal_x3_batched_wgemm(const void* P3, long csP, const void* Q3, long csQ, float* slab, int batch, long gsP, long gsQ,
                                  int M, int NI, int NJ, int splits, int variant, int nprod, hipStream_t s);
// a pre-split operand: three component planes of bf16, `cs` elements apart, rows of `ld` elements (the gathering forms keep one zero row behind
// the data rows of every plane: at cs - ld)
struct X3Operand { long off, len, ld, cs; };                // off, len: floats of workspace; ld, cs: bf16 elements
// a transposed convolution (pass 0: forward, 1: backward-data, 2: weight gradient) as x3 GEMMs
struct X3DeconvPlan {
    int ok;
    int pass, general;                                       // general = 0: kernel == stride, pad 0 (one plain GEMM + pixel shuffle); 1: kernel a multiple of the stride (implicit GEMMs over the taps)
    int N, H, W, Cin, Cout, K, stride, pad, OH, OW;
    X3Operand w, a;                                          // first and second operand in the workspace -- forward / backward-data: the weights, then the activations (x / dy);
                                                             // weight gradient: x, then dy
    int splits;                                              // weight gradient, general form: slabs of the split reduction
    WsRegion slab;
    long total;
};
X3DeconvPlan x3_deconv_plan(int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int pass);
int pdf_internal_x3_deconv_fwd(const X3DeconvPlan& p, const float* x, const float* w, const float* bias, float* y, float* ws, int ldy, hipStream_t s);
int pdf_internal_x3_deconv_bwd_data(const X3DeconvPlan& p, const float* dy, const float* w, float* dx, float* ws, int lddx, int lddy, hipStream_t s);
int pdf_internal_x3_deconv_bwd_weight(const X3DeconvPlan& p, const float* x, const float* dy, float* dw, float* ws, int lddy, int accumulate, hipStream_t s);
