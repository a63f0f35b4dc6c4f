// Host functions that gemm.hip, winograd.hip and gemm_x3.hip call in each other: declared once here, and every defining file includes
// this header, so a changed signature is a compile error instead of a silent mismatch at link time.
#pragma once
#include "common.h"

// ---- gemm.hip: batched launches of the fp32 MFMA kernels
int pdf_internal_batched_gemm(const float* A, const float* B, float* C, int batch, long gsA, long gsB, long gsC, int M, int N, int K, hipStream_t s);
int pdf_internal_batched_wgemm(const float* P, const float* Q, float* slab, int batch, long gsP, long gsQ, int M, int NI, int NJ, int splits, hipStream_t s);

// ---- winograd.hip: the Winograd path of the stride-1 3x3 convolutions
long pdf_internal_wino_workspace(int N, int H, int W, int Ck, int Cn, int flip);
int pdf_internal_wino_eligible(int N, int H, int W, int Ck, int Cn, int KH, int KW, int stride, int pad, int flip);
int pdf_internal_conv3x3_winograd(const float* x, int ldx, const float* w, const float* bias, float* y, int ldy, float* ws,
                                  int N, int H, int W, int Ck, int Cn, int act, int accum, int flip, const float* v_shared, hipStream_t s);
int pdf_internal_wino_wgrad_eligible(int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad);
long pdf_internal_wino_wgrad_workspace(int N, int H, int W, int Cin, int Cout);
long pdf_internal_wino_v_offset(int N, int H, int W, int Ck, int Cn);
int pdf_internal_conv3x3_winograd_wgrad(const float* x, int ldx, const float* dy, int lddy, float* dw, float* db, float* ws,
                                        int N, int H, int W, int Cin, int Cout, int accumulate, const float* v_cached, hipStream_t s);

// ---- gemm_x3.hip: fp32 products on the bf16 matrix pipe
int pdf_internal_x3_mode();                                  // bit 0 = the Winograd transform-domain products, bit 1 = the transposed convolutions, bit 2 = the mesh decoder (PDF_X3*, pdf_set_x3_mode)
int pdf_internal_x3_batched_gemm(const void* A3, long csA, const void* B3, long csB, float* C, int batch, long gsA, long gsB, long gsC,
                                 int M, int N, int K, int variant, int nprod, hipStream_t s);
int pdf_internal_x3_batched_wgemm(const void* P3, long csP, const void* Q3, long csQ, float* slab, int batch, long gsP, long gsQ,
                                  int M, int NI, int NJ, int splits, int variant, int nprod, hipStream_t s);
long pdf_internal_x3_deconv_workspace(int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int backward);
int pdf_internal_x3_deconv_fwd(const float* x, const float* w, const float* bias, float* y, float* ws, int N, int H, int W, int Cin, int Cout,
                               int KH, int KW, int stride, int OH, int OW, int ldy, hipStream_t s);
int pdf_internal_x3_deconv_bwd_data(const float* dy, const float* w, float* dx, float* ws, int N, int H, int W, int Cin, int lddx, int Cout,
                                    int KH, int KW, int stride, int OH, int OW, int lddy, hipStream_t s);
int pdf_internal_x3_deconv_general_fwd(const float* x, const float* w, const float* bias, float* y, float* ws, int N, int H, int W, int Cin, int Cout,
                                       int K, int stride, int pad, int OH, int OW, int ldy, hipStream_t s);
int pdf_internal_x3_deconv_general_bwd_data(const float* dy, const float* w, float* dx, float* ws, int N, int H, int W, int Cin, int lddx, int Cout,
                                            int K, int stride, int pad, int OH, int OW, int lddy, hipStream_t s);
int pdf_internal_x3_deconv_general_bwd_weight(const float* x, const float* dy, float* dw, float* ws, int N, int H, int W, int Cin, int Cout,
                                              int K, int stride, int pad, int OH, int OW, int lddy, int accumulate, hipStream_t s);
int pdf_internal_x3_deconv_bwd_weight(const float* x, const float* dy, float* dw, float* ws, int N, int H, int W, int Cin, int Cout,
                                      int KH, int KW, int stride, int OH, int OW, int lddy, int accumulate, hipStream_t s);
