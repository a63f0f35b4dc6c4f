// Aligned evaluation metrics (lib/utils/eval.py:96-119 align_w_scale, :54-73 calculate_fscore; the reference keeps its only call site,
// lib/trains/base_trainer.py:396-398, under `if False`): Procrustes-aligned point errors and the nearest-neighbour distances behind the mesh
// F-scores.  Like point_dist_sum_kernel (loss.hip): one block of 256 threads per row = (sample, hand), the points of the row staged in LDS as
// x / y / z planes.  No atomics, every reduction in a fixed order: two runs on the same input are bit-identical.
#include "common.h"
#include "svd3.h"                                             // met_procrustes_3x3
#include "mesh_geom.h"                                        // HAND_MAXN, HAND_MAXF, geo_stage_planes, geo_stage_faces, geo_solid_angle

#define MET_T 256

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

// align_w_scale(gt, pred) per row, then the point distances.  fp32 in and out, the arithmetic between in double: the distances are differences
// of aligned coordinates ~100x their size, and the double rate is not what bounds 1,000 points per block.
__global__ __launch_bounds__(MET_T) void procrustes_dist_kernel(const float* __restrict__ pred, const float* __restrict__ gt, int n,
                                                                float* __restrict__ sum, float* __restrict__ dist, float* __restrict__ aligned) {
    __shared__ float gx[HAND_MAXN], gy[HAND_MAXN], gz[HAND_MAXN], px[HAND_MAXN], py[HAND_MAXN], pz[HAND_MAXN];
    __shared__ double red[4 * 11];
    __shared__ double trafo[12];                               // s * s1 / s2 * R (row-major), then t1
    const long row = blockIdx.x;
    geo_stage_planes(gt + row * n * 3, n, gx, gy, gz);
    geo_stage_planes(pred + row * n * 3, n, px, py, pz);
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
    if (n > HAND_MAXN) return PDF_E_BADARG;
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
    __shared__ float4 planes[6][HAND_MAXN / 4];                // (float4: the scan reads four points per 16-byte access)
    __shared__ int red[4][2 * MET_MAXT];
    float *gx = reinterpret_cast<float*>(planes[0]), *gy = reinterpret_cast<float*>(planes[1]), *gz = reinterpret_cast<float*>(planes[2]);
    float *px = reinterpret_cast<float*>(planes[3]), *py = reinterpret_cast<float*>(planes[4]), *pz = reinterpret_cast<float*>(planes[5]);
    const long row = blockIdx.x;
    const int n4 = (n + 3) & ~3;                               // <= HAND_MAXN, which is a multiple of four
    geo_stage_planes(gt + row * n * 3, n, gx, gy, gz);
    geo_stage_planes(pred + row * n * 3, n, px, py, pz);
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
    if (n > HAND_MAXN || T < 1 || T > MET_MAXT || thr == nullptr) return PDF_E_BADARG;
    MetThr th = {{0.f, 0.f, 0.f, 0.f}};
    for (int t = 0; t < T; ++t) th.t[t] = thr[t];              // host array: travels in the kernel arguments
    hipLaunchKernelGGL(mesh_nn_counts_kernel, dim3(rows), dim3(MET_T), 0, s, pred, gt, n, th, T, counts, d_gt, d_pred);
    PDF_LAUNCH_CHECK();
    return 0;
}

// Inter-hand penetration: every vertex of one hand against the triangle mesh of the other hand of the same sample.  One block per row
// = (sample, hand); the OTHER hand's vertex planes (12 KB) and its face indices as 16-bit triples (16 KB) are staged in LDS, one lane owns one
// query vertex and all lanes walk the triangles together, so every LDS read of the loop is a broadcast.  1,024 lanes: the 778 vertices of a
// hand take one round of 13 waves, 3-4 per SIMD, which hide each other's LDS and atan2f latency (profiles/NOTES.md has the 256-lane form's time).
// Per triangle, with a, b, c the corners relative to the query:
//   solid angle  2 atan2(a.(b x c), |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|)   (Van Oosterom-Strackee), summed in double, / 4 pi = wind;
//   distance^2 = the smallest of the three segment distances (parameter clamped to [0, 1]: the vertex and edge regions) and, where the
//   projection of the query falls inside the triangle (the face region), of the plane distance (a.n)^2 / n.n with n = (b - a) x (c - a).
// A triangle collapsed to a point has a.(b x c) = 0 and n = 0 exactly: it adds atan2(0, den >= +0) = 0 and the distance to that point.
// Nothing is divided by a length that can be zero, so finite coordinates (|x| < 1e6: the cubes stay finite) give finite output.
#define PEN_T 1024
#define PEN_TINY 1e-37f

__device__ __forceinline__ float pen_seg_d2(float px, float py, float pz, float ex, float ey, float ez) {
    // squared distance from the origin to the segment p + t e, t in [0, 1]
    const float ee = ex * ex + ey * ey + ez * ez, pe = px * ex + py * ey + pz * ez;
    const float t = fminf(fmaxf(-pe * __frcp_rn(fmaxf(ee, PEN_TINY)), 0.f), 1.f);
    const float qx = px + t * ex, qy = py + t * ey, qz = pz + t * ez;
    return qx * qx + qy * qy + qz * qz;
}

__global__ __launch_bounds__(PEN_T) void mesh_penetration_kernel(const float* __restrict__ verts, const long long* __restrict__ faces, int n, int Fc,
                                                                 float* __restrict__ wind, float* __restrict__ dist, int* __restrict__ count,
                                                                 float* __restrict__ depth, float* __restrict__ gap) {
    __shared__ float ox[HAND_MAXN], oy[HAND_MAXN], oz[HAND_MAXN];
    __shared__ ushort4 tri[HAND_MAXF];
    __shared__ int red_c[PEN_T / 64];
    __shared__ float red_d[PEN_T / 64], red_g[PEN_T / 64];
    const long row = blockIdx.x;
    const int h = (int)(row & 1);
    const float* other = verts + (row ^ 1) * n * 3;            // rows 2b, 2b + 1 are the two hands of sample b
    geo_stage_planes(other, n, ox, oy, oz);
    geo_stage_faces(faces + (long)(1 - h) * Fc * 3, Fc, n, tri);
    __syncthreads();
    int cnt = 0;
    float dep = 0.f, gp = 3.0e38f;
    for (int i = threadIdx.x; i < n; i += PEN_T) {
        const float* p = verts + (row * n + i) * 3;
        const float x = p[0], y = p[1], z = p[2];
        double omega = 0.0;
        float best = 3.0e38f;
        for (int t = 0; t < Fc; ++t) {
            const ushort4 f = tri[t];
            const float ax = ox[f.x] - x, ay = oy[f.x] - y, az = oz[f.x] - z;
            const float bx = ox[f.y] - x, by = oy[f.y] - y, bz = oz[f.y] - z;
            const float cx = ox[f.z] - x, cy = oy[f.z] - y, cz = oz[f.z] - z;
            float det, den;
            geo_solid_angle(ax, ay, az, bx, by, bz, cx, cy, cz, det, den);      // (shared with penetration_loss_kernel: its `inside` is this wind > 0.5)
            omega += (double)atan2f(det, den);
            // edges e1 = b - a, e2 = c - a; d1 .. d6 of the region test: e1.(-a), e2.(-a), e1.(-b), e2.(-b), e1.(-c), e2.(-c)
            const float e1x = bx - ax, e1y = by - ay, e1z = bz - az, e2x = cx - ax, e2y = cy - ay, e2z = cz - az;
            float d2 = fminf(fminf(pen_seg_d2(ax, ay, az, e1x, e1y, e1z), pen_seg_d2(ax, ay, az, e2x, e2y, e2z)),
                             pen_seg_d2(bx, by, bz, cx - bx, cy - by, cz - bz));
            const float d1 = -(e1x * ax + e1y * ay + e1z * az), d2a = -(e2x * ax + e2y * ay + e2z * az);
            const float d3 = -(e1x * bx + e1y * by + e1z * bz), d4 = -(e2x * bx + e2y * by + e2z * bz);
            const float d5 = -(e1x * cx + e1y * cy + e1z * cz), d6 = -(e2x * cx + e2y * cy + e2z * cz);
            const float vc = d1 * d4 - d3 * d2a, vb = d5 * d2a - d1 * d6, va = d3 * d6 - d5 * d4;
            const float nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
            const float nn = nx * nx + ny * ny + nz * nz;
            // (a sliver whose corner angle is below 1e-5 rad has a normal made of rounding noise: its segments are the triangle)
            const float e11 = e1x * e1x + e1y * e1y + e1z * e1z, e22 = e2x * e2x + e2y * e2y + e2z * e2z;
            if (va >= 0.f && vb >= 0.f && vc >= 0.f && nn > fmaxf(1e-10f * e11 * e22, PEN_TINY)) {
                const float an = ax * nx + ay * ny + az * nz;
                d2 = fminf(d2, an * an * __frcp_rn(nn));
            }
            best = fminf(best, d2);
        }
        const float w = (float)(omega * (2.0 / (4.0 * 3.14159265358979323846))), d = sqrtf(best);
        if (wind != nullptr) wind[row * n + i] = w;
        if (dist != nullptr) dist[row * n + i] = d;
        gp = fminf(gp, d);
        if (w > 0.5f) { ++cnt; dep = fmaxf(dep, d); }
    }
    // count: an integer sum; depth / gap: a maximum / minimum.  None depends on the order, which is fixed anyway.
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    cnt = wave_sum_i(cnt);
    dep = wave_max(dep);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) gp = fminf(gp, __shfl_xor(gp, o, 64));
    if (lane == 0) { red_c[wave] = cnt; red_d[wave] = dep; red_g[wave] = gp; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < PEN_T / 64; ++k) { cnt += red_c[k]; dep = fmaxf(dep, red_d[k]); gp = fminf(gp, red_g[k]); }
        count[row] = cnt; depth[row] = dep; gap[row] = gp;
    }
}
PDF_API int pdf_mesh_penetration(const float* verts, const long long* faces, int B, int n, int Fc, float* wind, float* dist, int* count,
                                 float* depth, float* gap, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (B <= 0) return 0;
    if (n < 1 || n > HAND_MAXN || Fc < 1 || Fc > HAND_MAXF || verts == nullptr || faces == nullptr || count == nullptr || depth == nullptr || gap == nullptr)
        return PDF_E_BADARG;
    hipLaunchKernelGGL(mesh_penetration_kernel, dim3(2 * B), dim3(PEN_T), 0, s, verts, faces, n, Fc, wind, dist, count, depth, gap);
    PDF_LAUNCH_CHECK();
    return 0;
}
