// Host-only check of pdf_parity_taps (csrc/gemm_common.h) against the three loops it replaced, which live on only here:
// the input-parity classes of the strided convolution's backward-data, the output-parity classes of the transposed convolution's
// forward (both gemm.hip) and the per-class tap table of the general x3 transposed convolution (gemm_x3.hip).
// Same taps, same order, same offsets over k in {1, 2, 3, 4, 7, 8}, stride in {1, 2, 4, 8}, pad in 0 .. k - 1 and every class.
// Built with the address and undefined-behaviour sanitizers (tests/test_ws_plan_cpu.py); needs no device.
#include "gemm_common.h"
#include <cstdio>

// gemm.hip, pdf_conv2d_bwd_data_impl and pdf_deconv2d_fwd_impl (the two copies differed in comments only)
static int old_igemm_taps(int KH, int KW, int stride, int pad, int py, int px, int* gdy, int* gdx, int* gwt) {
    int T = 0;
    for (int ky = 0; ky < KH; ++ky) {
        if ((py + pad - ky) % stride != 0) continue;
        for (int kx = 0; kx < KW; ++kx) {
            if ((px + pad - kx) % stride != 0) continue;
            int ny = py + pad - ky, nx = px + pad - kx;
            gdy[T] = (int)(ny >= 0 ? ny / stride : -((-ny) / stride));
            gdx[T] = (int)(nx >= 0 ? nx / stride : -((-nx) / stride));
            gwt[T] = (int)(ky * KW + kx);
            ++T;
        }
    }
    return T;
}
// gemm_x3.hip, pdf_internal_x3_deconv_general_fwd: (ky, kx) per class, the offsets derived from them at the launch
static int old_x3_taps(int K, int stride, int pad, int py, int px, int* tdy, int* tdx, int* wt) {
    int n = 0;
    for (int ky = 0; ky < K; ++ky) {
        if (((py + pad - ky) % stride + stride) % stride != 0) continue;
        for (int kx = 0; kx < K; ++kx) {
            if (((px + pad - kx) % stride + stride) % stride != 0) continue;
            tdy[n] = (py + pad - ky) / stride; tdx[n] = (px + pad - kx) / stride; wt[n] = ky * K + kx;
            ++n;
        }
    }
    return n;
}

int main() {
    const int ks[] = {1, 2, 3, 4, 7, 8}, strides[] = {1, 2, 4, 8};
    long cases = 0, taps = 0;
    for (int K : ks)
        for (int stride : strides)
            for (int pad = 0; pad < K; ++pad)
                for (int py = 0; py < stride; ++py)
                    for (int px = 0; px < stride; ++px) {
                        // exactly K * K entries each: the sanitizer sees a write past the documented capacity
                        int* a = new int[3 * K * K]; int* b = new int[3 * K * K]; int* c = new int[3 * K * K];
                        const int Ta = pdf_parity_taps(K, K, stride, pad, py, px, a, a + K * K, a + 2 * K * K);
                        const int Tb = old_igemm_taps(K, K, stride, pad, py, px, b, b + K * K, b + 2 * K * K);
                        const int Tc = old_x3_taps(K, stride, pad, py, px, c, c + K * K, c + 2 * K * K);
                        bool ok = Ta == Tb && Ta == Tc;
                        for (int t = 0; ok && t < Ta; ++t)
                            for (int f = 0; f < 3; ++f) ok = ok && a[f * K * K + t] == b[f * K * K + t] && a[f * K * K + t] == c[f * K * K + t];
                        if (!ok) { std::printf("MISMATCH k=%d stride=%d pad=%d class (%d, %d): %d / %d / %d taps\n", K, stride, pad, py, px, Ta, Tb, Tc); return 1; }
                        ++cases; taps += Ta;
                        delete[] a; delete[] b; delete[] c;
                    }
    // a non-square kernel (the implicit-GEMM loops take KH and KW)
    for (int stride : strides)
        for (int p = 0; p < stride * stride; ++p) {
            int a[3][12], b[3][12];
            const int Ta = pdf_parity_taps(3, 4, stride, 1, p / stride, p % stride, a[0], a[1], a[2]);
            if (Ta != old_igemm_taps(3, 4, stride, 1, p / stride, p % stride, b[0], b[1], b[2])) return 1;
            for (int t = 0; t < Ta; ++t)
                if (a[0][t] != b[0][t] || a[1][t] != b[1][t] || a[2][t] != b[2][t]) return 1;
            ++cases;
        }
    std::printf("parity taps ok: %ld classes, %ld taps\n", cases, taps);
    return 0;
}
