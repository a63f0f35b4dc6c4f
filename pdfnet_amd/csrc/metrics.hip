// Aligned evaluation metrics (lib/utils/eval.py:96-119 align_w_scale, :54-73 calculate_fscore; the reference keeps its only call site,
// lib/trains/base_trainer.py:396-398, under `if False`): Procrustes-aligned point errors and the nearest-neighbour distances behind the mesh
// F-scores.  Like point_dist_sum_kernel (loss.hip): one block of 256 threads per row = (sample, hand), the points of the row staged in LDS as
// x / y / z planes.  No atomics, every reduction in a fixed order: two runs on the same input are bit-identical.
#include "common.h"

#define MET_T 256
#define MET_MAXN 1024

// row [n][3] (global) -> planes x, y, z [n] (LDS); consecutive lanes read consecutive floats
__device__ __forceinline__ void met_stage(const float* __restrict__ row, int n, float* x, float* y, float* z) {
    for (int e = threadIdx.x; e < 3 * n; e += MET_T) {
        const int i = e / 3, k = e - 3 * i;
        (k == 0 ? x : k == 1 ? y : z)[i] = row[e];
    }
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// v[0..K) summed over the block, every thread gets the result; sm [4 * K].  Wave partials by the xor butterfly, then (w0 + w1) + (w2 + w3).
template <int K>
__device__ __forceinline__ void block_sum_d(double* v, double* sm) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = wave_sum_d(v[k]);
    __syncthreads();
    if (lane == 0)
        for (int k = 0; k < K; ++k) sm[wave * K + k] = v[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = (sm[k] + sm[K + k]) + (sm[2 * K + k] + sm[3 * K + k]);
}

// Orthogonal Procrustes of a 3x3 matrix in one lane: M = U S V^T by one-sided Jacobi (Hestenes) rotations of the columns of G = M V, which
// converge to U S with V the accumulated rotations.  Returns tr S and R = U V^T, WITHOUT a determinant correction (scipy's
// orthogonal_procrustes: a mirrored prediction aligns exactly).  A singular direction whose sigma is below 1e-12 of the largest gets its left
// vector from the orthogonal complement of the others instead of from rounding noise, so R stays orthogonal for any rank; rank 0: R = I.
__device__ double met_procrustes_3x3(const double M[3][3], double R[3][3]) {
    double g[3][3], v[3][3];                                   // g[c] / v[c]: COLUMN c of G / V
    for (int c = 0; c < 3; ++c)
        for (int r = 0; r < 3; ++r) { g[c][r] = M[r][c]; v[c][r] = r == c ? 1.0 : 0.0; }
    for (int sweep = 0; sweep < 30; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                const double a = g[p][0] * g[p][0] + g[p][1] * g[p][1] + g[p][2] * g[p][2];
                const double b = g[q][0] * g[q][0] + g[q][1] * g[q][1] + g[q][2] * g[q][2];
                const double c = g[p][0] * g[q][0] + g[p][1] * g[q][1] + g[p][2] * g[q][2];
                if (!(c * c > 1e-30 * a * b)) continue;        // columns orthogonal to 1e-15 (also: a zero column, an underflowed product)
                rotated = true;
                const double zeta = (b - a) / (2.0 * c);
                const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
                for (int r = 0; r < 3; ++r) {
                    const double gp = g[p][r], gq = g[q][r], vp = v[p][r], vq = v[q][r];
                    g[p][r] = cs * gp - sn * gq; g[q][r] = sn * gp + cs * gq;
                    v[p][r] = cs * vp - sn * vq; v[q][r] = sn * vp + cs * vq;
                }
            }
        if (!rotated) break;
    }
    double sg[3];
    for (int c = 0; c < 3; ++c) sg[c] = sqrt(g[c][0] * g[c][0] + g[c][1] * g[c][1] + g[c][2] * g[c][2]);
    for (int i = 0; i < 2; ++i)                                // sigma descending (columns of G and V move together)
        for (int j = 0; j < 2 - i; ++j)
            if (sg[j] < sg[j + 1]) {
                double t = sg[j]; sg[j] = sg[j + 1]; sg[j + 1] = t;
                for (int r = 0; r < 3; ++r) {
                    t = g[j][r]; g[j][r] = g[j + 1][r]; g[j + 1][r] = t;
                    t = v[j][r]; v[j][r] = v[j + 1][r]; v[j + 1][r] = t;
                }
            }
    const double trace = sg[0] + sg[1] + sg[2];
    if (!(sg[0] > 0.0)) {                                      // M = 0 (also a NaN input: finite R, the NaN shows in `aligned`)
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) R[r][c] = r == c ? 1.0 : 0.0;
        return trace;
    }
    const double tiny = 1e-12 * sg[0];
    double u[3][3];
    for (int r = 0; r < 3; ++r) u[0][r] = g[0][r] / sg[0];
    if (sg[1] > tiny) {
        for (int r = 0; r < 3; ++r) u[1][r] = g[1][r] / sg[1];
    } else {                                                   // any unit vector orthogonal to u0: u0 x (the axis u0 leans on least)
        const double ax = fabs(u[0][0]), ay = fabs(u[0][1]), az = fabs(u[0][2]);
        const int k = ax <= ay && ax <= az ? 0 : (ay <= az ? 1 : 2);
        const double e[3] = {k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0};
        double w[3] = {u[0][1] * e[2] - u[0][2] * e[1], u[0][2] * e[0] - u[0][0] * e[2], u[0][0] * e[1] - u[0][1] * e[0]};
        const double nw = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
        for (int r = 0; r < 3; ++r) u[1][r] = w[r] / nw;
    }
    if (sg[2] > tiny) {
        for (int r = 0; r < 3; ++r) u[2][r] = g[2][r] / sg[2];
    } else {
        u[2][0] = u[0][1] * u[1][2] - u[0][2] * u[1][1];
        u[2][1] = u[0][2] * u[1][0] - u[0][0] * u[1][2];
        u[2][2] = u[0][0] * u[1][1] - u[0][1] * u[1][0];
    }
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) R[r][c] = u[0][r] * v[0][c] + u[1][r] * v[1][c] + u[2][r] * v[2][c];
    return trace;
}

// align_w_scale(gt, pred) per row, then the point distances.  fp32 in and out, the arithmetic between in double: the distances are differences
// of aligned coordinates ~100x their size, and the double rate is not what bounds 1,000 points per block.
__global__ __launch_bounds__(MET_T) void procrustes_dist_kernel(const float* __restrict__ pred, const float* __restrict__ gt, int n,
                                                                float* __restrict__ sum, float* __restrict__ dist, float* __restrict__ aligned) {
    __shared__ float gx[MET_MAXN], gy[MET_MAXN], gz[MET_MAXN], px[MET_MAXN], py[MET_MAXN], pz[MET_MAXN];
    __shared__ double red[4 * 11];
    __shared__ double trafo[12];                               // s * s1 / s2 * R (row-major), then t1
    const long row = blockIdx.x;
    met_stage(gt + row * n * 3, n, gx, gy, gz);
    met_stage(pred + row * n * 3, n, px, py, pz);
    __syncthreads();
    // pass 1: the means t1 (gt), t2 (pred)
    double m[6] = {0, 0, 0, 0, 0, 0};
    for (int i = threadIdx.x; i < n; i += MET_T) {
        m[0] += gx[i]; m[1] += gy[i]; m[2] += gz[i];
        m[3] += px[i]; m[4] += py[i]; m[5] += pz[i];
    }
    block_sum_d<6>(m, red);
    for (int k = 0; k < 6; ++k) m[k] /= (double)n;
    // pass 2: squared Frobenius norms of the centred sets and their nine cross sums  C[r][c] = sum_i gt_c[i][r] * pred_c[i][c]
    double a[11] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = threadIdx.x; i < n; i += MET_T) {
        const double g[3] = {gx[i] - m[0], gy[i] - m[1], gz[i] - m[2]};
        const double p[3] = {px[i] - m[3], py[i] - m[4], pz[i] - m[5]};
        a[0] += g[0] * g[0] + g[1] * g[1] + g[2] * g[2];
        a[1] += p[0] * p[0] + p[1] * p[1] + p[2] * p[2];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) a[2 + 3 * r + c] += g[r] * p[c];
    }
    block_sum_d<11>(a, red);
    if (threadIdx.x == 0) {
        const double s1 = sqrt(a[0]) + 1e-8, s2 = sqrt(a[1]) + 1e-8;
        double M[3][3], R[3][3];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) M[r][c] = a[2 + 3 * r + c] / (s1 * s2);
        const double s = met_procrustes_3x3(M, R);
        const double k = s * s1 / s2;                          // aligned = (pred_c / s2) R^T * s * s1 + t1
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) trafo[3 * r + c] = k * R[r][c];
        trafo[9] = m[0]; trafo[10] = m[1]; trafo[11] = m[2];
    }
    __syncthreads();
    // pass 3: apply, distances; the aligned points replace the prediction in LDS for a coalesced store
    double acc[1] = {0};
    for (int i = threadIdx.x; i < n; i += MET_T) {
        const double p[3] = {px[i] - m[3], py[i] - m[4], pz[i] - m[5]};
        const double ax = trafo[0] * p[0] + trafo[1] * p[1] + trafo[2] * p[2] + trafo[9];
        const double ay = trafo[3] * p[0] + trafo[4] * p[1] + trafo[5] * p[2] + trafo[10];
        const double az = trafo[6] * p[0] + trafo[7] * p[1] + trafo[8] * p[2] + trafo[11];
        const double dx = ax - gx[i], dy = ay - gy[i], dz = az - gz[i];
        const double d = sqrt(dx * dx + dy * dy + dz * dz);
        acc[0] += d;
        if (dist != nullptr) dist[row * n + i] = (float)d;
        px[i] = (float)ax; py[i] = (float)ay; pz[i] = (float)az;
    }
    block_sum_d<1>(acc, red);                                  // (its barriers also publish the aligned points)
    if (threadIdx.x == 0) sum[row] = (float)acc[0];
    if (aligned != nullptr) {
        float* o = aligned + row * n * 3;
        for (int e = threadIdx.x; e < 3 * n; e += MET_T) {
            const int i = e / 3, k = e - 3 * i;
            o[e] = (k == 0 ? px : k == 1 ? py : pz)[i];
        }
    }
}
PDF_API int pdf_procrustes_dist(const float* pred, const float* gt, int rows, int n, float* sum, float* dist, float* aligned, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (rows <= 0 || n <= 0) return 0;
    if (n > MET_MAXN) return PDF_E_BADARG;
    hipLaunchKernelGGL(procrustes_dist_kernel, dim3(rows), dim3(MET_T), 0, s, pred, gt, n, sum, dist, aligned);
    PDF_LAUNCH_CHECK();
    return 0;
}

// Nearest-neighbour distances between the two point sets of a row (calculate_fscore's compute_point_cloud_distance, both directions) and the
// number of points closer than each threshold.  Each thread owns points i, i + 256, ... of one set and scans the other set, which every lane
// reads at the same address (LDS broadcast), four points per read; the planes are padded to a multiple of four with far-away points.
#define MET_MAXT 4
#define MET_FAR 1e18f                                          // (its square is finite in fp32 and beyond any distance of real points)
struct MetThr { float t[MET_MAXT]; };

__device__ __forceinline__ void met_nn_scan(const float* sx, const float* sy, const float* sz, const float* ox, const float* oy, const float* oz,
                                            int n, int n4, const MetThr& thr, int T, float* __restrict__ d_out, int* cnt /*[MET_MAXT]*/) {
    for (int i = threadIdx.x; i < n; i += MET_T) {
        const float x = sx[i], y = sy[i], z = sz[i];
        float best = 3.0e38f;
        for (int j = 0; j < n4; j += 4) {
            const float4 X = *reinterpret_cast<const float4*>(ox + j), Y = *reinterpret_cast<const float4*>(oy + j),
                         Z = *reinterpret_cast<const float4*>(oz + j);
            const float d0 = (x - X.x) * (x - X.x) + (y - Y.x) * (y - Y.x) + (z - Z.x) * (z - Z.x);
            const float d1 = (x - X.y) * (x - X.y) + (y - Y.y) * (y - Y.y) + (z - Z.y) * (z - Z.y);
            const float d2 = (x - X.z) * (x - X.z) + (y - Y.z) * (y - Y.z) + (z - Z.z) * (z - Z.z);
            const float d3 = (x - X.w) * (x - X.w) + (y - Y.w) * (y - Y.w) + (z - Z.w) * (z - Z.w);
            best = fminf(best, fminf(fminf(d0, d1), fminf(d2, d3)));
        }
        const float d = sqrtf(best);
        if (d_out != nullptr) d_out[i] = d;
#pragma unroll
        for (int t = 0; t < MET_MAXT; ++t) cnt[t] += t < T && d < thr.t[t] ? 1 : 0;      // strict <, as calculate_fscore
    }
}

__global__ __launch_bounds__(MET_T) void mesh_nn_counts_kernel(const float* __restrict__ pred, const float* __restrict__ gt, int n, MetThr thr, int T,
                                                               int* __restrict__ counts, float* __restrict__ d_gt, float* __restrict__ d_pred) {
    __shared__ float4 planes[6][MET_MAXN / 4];                 // (float4: the scan reads four points per 16-byte access)
    __shared__ int red[4][2 * MET_MAXT];
    float *gx = reinterpret_cast<float*>(planes[0]), *gy = reinterpret_cast<float*>(planes[1]), *gz = reinterpret_cast<float*>(planes[2]);
    float *px = reinterpret_cast<float*>(planes[3]), *py = reinterpret_cast<float*>(planes[4]), *pz = reinterpret_cast<float*>(planes[5]);
    const long row = blockIdx.x;
    const int n4 = (n + 3) & ~3;                               // <= MET_MAXN, which is a multiple of four
    met_stage(gt + row * n * 3, n, gx, gy, gz);
    met_stage(pred + row * n * 3, n, px, py, pz);
    if (threadIdx.x < n4 - n) {
        const int i = n + threadIdx.x;
        gx[i] = gy[i] = gz[i] = px[i] = py[i] = pz[i] = MET_FAR;
    }
    __syncthreads();
    int cnt[2 * MET_MAXT] = {0, 0, 0, 0, 0, 0, 0, 0};          // [0, 4): gt points near the prediction, [4, 8): predicted points near gt
    met_nn_scan(gx, gy, gz, px, py, pz, n, n4, thr, T, d_gt != nullptr ? d_gt + row * n : nullptr, cnt);
    met_nn_scan(px, py, pz, gx, gy, gz, n, n4, thr, T, d_pred != nullptr ? d_pred + row * n : nullptr, cnt + MET_MAXT);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 2 * MET_MAXT; ++k) {
        const int w = wave_sum_i(cnt[k]);
        if (lane == 0) red[wave][k] = w;
    }
    __syncthreads();
    if (threadIdx.x < 2 * T) {
        const int t = threadIdx.x >> 1, k = (threadIdx.x & 1) * MET_MAXT + t;
        counts[(row * T + t) * 2 + (threadIdx.x & 1)] = red[0][k] + red[1][k] + red[2][k] + red[3][k];
    }
}
PDF_API int pdf_mesh_nn_counts(const float* pred, const float* gt, int rows, int n, const float* thr, int T, int* counts, float* d_gt, float* d_pred,
                               void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (rows <= 0 || n <= 0) return 0;
    if (n > MET_MAXN || T < 1 || T > MET_MAXT || thr == nullptr) return PDF_E_BADARG;
    MetThr th = {{0.f, 0.f, 0.f, 0.f}};
    for (int t = 0; t < T; ++t) th.t[t] = thr[t];              // host array: travels in the kernel arguments
    hipLaunchKernelGGL(mesh_nn_counts_kernel, dim3(rows), dim3(MET_T), 0, s, pred, gt, n, th, T, counts, d_gt, d_pred);
    PDF_LAUNCH_CHECK();
    return 0;
}
