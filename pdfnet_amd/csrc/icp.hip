// ICP refinement of a predicted hand mesh against that hand's sensor point cloud (contract: pdf_mesh_icp in pdfnet_hip.h).  Nothing in the
// reference does this: its pipeline never looks at the depth measurement again once the mesh is out.
//
// One launch for the whole loop, one workgroup of 1,024 lanes per row = (sample, hand), lane t owns cloud point t and vertex t.
//   LDS: the hand's CURRENT vertices as x / y / z planes (12 KB), its faces as 16-bit triples (16 KB), and the list of the camera-facing
//   triangles of the current mesh as their three corners, 48 B a triangle (96 KB), rebuilt before every association: lane t tests face
//   base + t, the survivors are compacted in face order by a 64-bit __ballot + popcount prefix per wave and the wave totals through LDS
//   (render_tile_kernel's idiom).  The walk reads the list front to back, every lane the same triangle: three broadcast 16-byte reads and no
//   index to chase.
//   Association: closest point by the seven regions (Ericson, Real-Time Collision Detection 5.1.5), tested in the order vertex A, vertex B,
//   edge AB, vertex C, edge AC, edge BC, face; fp32; a strictly smaller squared distance replaces the best, so the lowest face index wins a tie.
//   Every quotient has its denominator held at or above ICP_TINY.
//   Update: count, sum p, sum q, sum q p^T and sum |p - q|^2 over the inliers as doubles: xor butterfly per wave, the 16 wave partials through
//   LDS, added by lane 0 as a balanced tree.  Lane 0 solves (svd3.h) and composes the step into (R, t), kept in double in LDS; every lane then
//   rewrites its vertex of the LDS copy as fp32(R v0 + t) from the ORIGINAL vertex it holds in registers, so rounding does not pile up over
//   the iterations and out_verts is exactly the fp32 rounding of R v + t.
// No atomics, no global scratch: two runs are bit-identical and a row does not depend on the other rows of the batch.
// The same association feeds cloud_mesh_loss_kernel at the end of this file: the residual as a loss, with its gradient (pdf_cloud_mesh_loss).
#include "svd3.h"                                               // met_svd_3x3
#include "mesh_geom.h"

#define ICP_MAXIT 64

// the camera-facing triangles of the current LDS mesh -> s.ca / cb / cc in face order; returns their number (block-uniform)
__device__ __forceinline__ int icp_facing(IcpShared& s, int Fc) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    int total = 0;
    for (int base = 0; base < Fc; base += ICP_T) {
        const int g = base + t;
        bool keep = false;
        float ax = 0.f, ay = 0.f, az = 0.f, bx = 0.f, by = 0.f, bz = 0.f, cx = 0.f, cy = 0.f, cz = 0.f;
        if (g < Fc) {
            const ushort4 f = s.tri[g];
            ax = s.vx[f.x]; ay = s.vy[f.x]; az = s.vz[f.x];
            bx = s.vx[f.y]; by = s.vy[f.y]; bz = s.vz[f.y];
            cx = s.vx[f.z]; cy = s.vy[f.z]; cz = s.vz[f.z];
            keep = geo_faces_camera(ax, ay, az, bx, by, bz, cx, cy, cz);
        }
        const unsigned long long mask = __ballot(keep);
        if (lane == 0) s.wave_n[wave] = __popcll(mask);
        __syncthreads();
        int off = total + __popcll(mask & ((1ULL << lane) - 1ULL));
#pragma unroll
        for (int w = 0; w < ICP_W; ++w) {
            const int c = s.wave_n[w];
            if (w < wave) off += c;
            total += c;
        }
        if (keep) {                                            // off < total <= base + ICP_T, at most Fc <= HAND_MAXF
            s.ca[off] = make_float4(ax, ay, az, __int_as_float(g));
            s.cb[off] = make_float4(bx, by, bz, 0.f);
            s.cc[off] = make_float4(cx, cy, cz, 0.f);
        }
        __syncthreads();                                       // wave_n is rewritten by the next chunk; the list is read after the last one
    }
    return total;
}

// One step from the inlier sums a[]: composes it into xf (R row-major, t).  Returns false when the iteration stops.
__device__ __forceinline__ bool icp_step(const double* a, int rigid, double* xf, double (*ws)[3][3]) {
    const double N = a[0];
    if (N < (rigid ? 3.0 : 1.0)) return false;
    const double pm[3] = {a[1] / N, a[2] / N, a[3] / N}, qm[3] = {a[4] / N, a[5] / N, a[6] / N};
    double Rk[3][3];
    bool full = false;
    if (rigid) {
        double (*H)[3] = ws[0], (*u)[3] = ws[2], (*v)[3] = ws[3], sg[3];      // H = sum (q - qm)(p - pm)^T = U S V^T; R_k = V diag(1, 1, d) U^T
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) H[r][c] = a[7 + 3 * r + c] - N * qm[r] * pm[c];
        if (met_svd_3x3(H, ws[1], u, v, sg) && sg[1] >= 1e-6 * sg[0]) {
            full = true;
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 3; ++c) Rk[r][c] = v[0][r] * u[0][c] + v[1][r] * u[1][c] + v[2][r] * u[2][c];
            const double det = Rk[0][0] * (Rk[1][1] * Rk[2][2] - Rk[1][2] * Rk[2][1]) - Rk[0][1] * (Rk[1][0] * Rk[2][2] - Rk[1][2] * Rk[2][0]) +
                               Rk[0][2] * (Rk[1][0] * Rk[2][1] - Rk[1][1] * Rk[2][0]);
            if (det < 0.0)                                     // d = -1: the weakest direction changes sign
                for (int r = 0; r < 3; ++r)
                    for (int c = 0; c < 3; ++c) Rk[r][c] -= 2.0 * v[2][r] * u[2][c];
        }
    }
    if (!full)
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) Rk[r][c] = r == c ? 1.0 : 0.0;
    double tk[3], Rn[3][3], tn[3];
    for (int r = 0; r < 3; ++r) tk[r] = pm[r] - (Rk[r][0] * qm[0] + Rk[r][1] * qm[1] + Rk[r][2] * qm[2]);
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) Rn[r][c] = Rk[r][0] * xf[c] + Rk[r][1] * xf[3 + c] + Rk[r][2] * xf[6 + c];
        tn[r] = Rk[r][0] * xf[9] + Rk[r][1] * xf[10] + Rk[r][2] * xf[11] + tk[r];
    }
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) xf[3 * r + c] = Rn[r][c];
        xf[9 + r] = tn[r];
    }
    return true;
}

__global__ __launch_bounds__(ICP_T) void mesh_icp_kernel(const float* __restrict__ verts, const long long* __restrict__ faces,
                                                         const float* __restrict__ cloud, const float* __restrict__ valid, int n, int Fc, int P,
                                                         int iters, float trim, int rigid, float* __restrict__ out_verts, float* __restrict__ R,
                                                         float* __restrict__ tr, float* __restrict__ rms, int* __restrict__ inliers,
                                                         float* __restrict__ closest, int* __restrict__ tri) {
    __shared__ IcpShared s;
    const int t = threadIdx.x;
    const long row = blockIdx.x;
    const int h = (int)(row & 1);
    // The lane's point and its original vertex are read again where they are used (12 bytes each, from L2) instead of being held across the
    // one-lane solve, which needs the registers: the kernel must fit 128 VGPRs without scratch.
    const float* pp = cloud + (row * P + min(t, P - 1)) * 3;
    const float* vp = verts + (row * n + min(t, n - 1)) * 3;
    const bool live = t < P && pp[2] > 0.f;
    const bool row_ok = valid == nullptr || valid[row] != 0.f;
    if (!__syncthreads_or(live && row_ok)) {                   // block-uniform: the hand stays where it is
        if (t < n && out_verts != nullptr) { float* o = out_verts + (row * n + t) * 3; o[0] = vp[0]; o[1] = vp[1]; o[2] = vp[2]; }
        if (t < 9 && R != nullptr) R[row * 9 + t] = t % 4 == 0 ? 1.f : 0.f;
        if (t < 3 && tr != nullptr) tr[row * 3 + t] = 0.f;
        if (t == 0) { rms[row] = 0.f; inliers[row] = 0; }
        if (t < P) {
            if (closest != nullptr) { float* c = closest + (row * P + t) * 3; c[0] = c[1] = c[2] = 0.f; }
            if (tri != nullptr) tri[row * P + t] = -1;
        }
        return;
    }
    if (t < n) { s.vx[t] = vp[0]; s.vy[t] = vp[1]; s.vz[t] = vp[2]; }
    geo_stage_faces(faces + (long)h * Fc * 3, Fc, n, s.tri);
    if (t < 12) s.xf[t] = t < 9 && t % 4 == 0 ? 1.0 : 0.0;
    if (t == 0) s.stop = 0;
    __syncthreads();

    float best, qx, qy, qz, wa, wb, wc;                        // (the weights are not computed here)
    int face;
    for (int it = 0; ; ++it) {
        const int count = icp_facing(s, Fc);                   // (ends in a barrier)
        const float px = pp[0], py = pp[1], pz = pp[2];
        best = 3.0e38f; qx = qy = qz = 0.f; face = -1;
        if (__ballot(live) != 0ULL) icp_walk<false>(s, count, px, py, pz, best, qx, qy, qz, face, wa, wb, wc);      // wave-uniform; a dead lane's result is not used
        const bool in = live && face >= 0 && sqrtf(best) < trim;
        const double dpx = in ? px : 0.f, dpy = in ? py : 0.f, dpz = in ? pz : 0.f, dqx = in ? qx : 0.f, dqy = in ? qy : 0.f, dqz = in ? qz : 0.f;
        double a[ICP_K];
        a[0] = in ? 1.0 : 0.0; a[1] = dpx; a[2] = dpy; a[3] = dpz; a[4] = dqx; a[5] = dqy; a[6] = dqz;
        a[7] = dqx * dpx; a[8] = dqx * dpy; a[9] = dqx * dpz; a[10] = dqy * dpx; a[11] = dqy * dpy; a[12] = dqy * dpz;
        a[13] = dqz * dpx; a[14] = dqz * dpy; a[15] = dqz * dpz;
        a[16] = in ? (double)best : 0.0;
        icp_block_sum<ICP_K>(a, s.red, s.sum);
        if (it == iters) break;                                // the final association: s.sum feeds rms and inliers
        if (t == 0 && !icp_step(s.sum, rigid, s.xf, s.svd)) s.stop = 1;
        __syncthreads();
        if (s.stop) {                                          // block-uniform.  The mesh did not move: this association is the final one
            break;
        }
        if (t < n) {
            const double x = vp[0], y = vp[1], z = vp[2];
            s.vx[t] = (float)(s.xf[0] * x + s.xf[1] * y + s.xf[2] * z + s.xf[9]);
            s.vy[t] = (float)(s.xf[3] * x + s.xf[4] * y + s.xf[5] * z + s.xf[10]);
            s.vz[t] = (float)(s.xf[6] * x + s.xf[7] * y + s.xf[8] * z + s.xf[11]);
        }
        __syncthreads();
    }
    if (t < n && out_verts != nullptr) { float* o = out_verts + (row * n + t) * 3; o[0] = s.vx[t]; o[1] = s.vy[t]; o[2] = s.vz[t]; }
    if (t < 9 && R != nullptr) R[row * 9 + t] = (float)s.xf[t];
    if (t < 3 && tr != nullptr) tr[row * 3 + t] = (float)s.xf[9 + t];
    if (t == 0) {
        rms[row] = s.sum[0] > 0.0 ? (float)sqrt(s.sum[16] / s.sum[0]) : 0.f;
        inliers[row] = (int)s.sum[0];
    }
    if (t < P) {
        const bool hit = live && face >= 0;
        if (closest != nullptr) { float* c = closest + (row * P + t) * 3; c[0] = hit ? qx : 0.f; c[1] = hit ? qy : 0.f; c[2] = hit ? qz : 0.f; }
        if (tri != nullptr) tri[row * P + t] = hit ? face : -1;
    }
}

PDF_API int pdf_mesh_icp(const float* verts, const long long* faces, const float* cloud, const float* valid, int B, int n, int Fc, int P, int iters,
                         float trim, int rigid, float* out_verts, float* R, float* t, float* rms, int* inliers, float* closest, int* tri,
                         void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (B <= 0) return 0;
    if (n < 1 || n > HAND_MAXN || Fc < 1 || Fc > HAND_MAXF || P < 1 || P > HAND_MAXP || iters < 0 || iters > ICP_MAXIT || !(trim > 0.f) ||
        !(trim <= 3.0e38f) || verts == nullptr || faces == nullptr || cloud == nullptr || rms == nullptr || inliers == nullptr)
        return PDF_E_BADARG;
    hipLaunchKernelGGL(mesh_icp_kernel, dim3(2 * B), dim3(ICP_T), 0, s, verts, faces, cloud, valid, n, Fc, P, iters, trim, rigid, out_verts, R, t,
                       rms, inliers, closest, tri);
    PDF_LAUNCH_CHECK();
    return 0;
}

// ---- differentiable cloud-to-mesh loss (contract: pdf_cloud_mesh_loss in pdfnet_hip.h) ----------------------------------------------------
// The association of mesh_icp_kernel with iters = 0 -- icp_facing and icp_walk, shared -- then loss = mean |p - q|^2 over the inliers and its
// gradient with respect to the vertices: corner k of an inlier's triangle receives -(2/m) w_k (p - q) (the envelope theorem: q is the minimiser
// over the triangle, so only the explicit dependence of q = wa a + wb b + wc c on the corners counts).
// The gather is without atomics: geo_corner_gather over the P records of the row's points, each carrying -(2/m) (p - q), behind the block
// sum's barriers; lane t < n gets the sum for vertex t, added in double in ascending point order.
__global__ __launch_bounds__(ICP_T) void cloud_mesh_loss_kernel(const float* __restrict__ verts, const long long* __restrict__ faces,
                                                                const float* __restrict__ cloud, const float* __restrict__ valid, int n, int Fc,
                                                                int P, float trim, float* __restrict__ loss, int* __restrict__ inliers,
                                                                float* __restrict__ grad, int* __restrict__ tri, float* __restrict__ closest,
                                                                float* __restrict__ bary) {
    __shared__ IcpShared s;
    const int t = threadIdx.x;
    const long row = blockIdx.x;
    const int h = (int)(row & 1);
    const float* pp = cloud + (row * P + min(t, P - 1)) * 3;
    const float* vp = verts + (row * n + min(t, n - 1)) * 3;
    const bool live = t < P && pp[2] > 0.f;
    const bool row_ok = valid == nullptr || valid[row] != 0.f;
    if (!__syncthreads_or(live && row_ok)) {                   // block-uniform: nothing to compare the hand with
        if (t == 0) { loss[row] = 0.f; inliers[row] = 0; }
        if (t < n && grad != nullptr) { float* g = grad + (row * n + t) * 3; g[0] = g[1] = g[2] = 0.f; }
        if (t < P) {
            if (closest != nullptr) { float* c = closest + (row * P + t) * 3; c[0] = c[1] = c[2] = 0.f; }
            if (bary != nullptr) { float* w = bary + (row * P + t) * 3; w[0] = w[1] = w[2] = 0.f; }
            if (tri != nullptr) tri[row * P + t] = -1;
        }
        return;
    }
    if (t < n) { s.vx[t] = vp[0]; s.vy[t] = vp[1]; s.vz[t] = vp[2]; }
    geo_stage_faces(faces + (long)h * Fc * 3, Fc, n, s.tri);
    __syncthreads();

    const int count = icp_facing(s, Fc);                       // (ends in a barrier)
    const float px = pp[0], py = pp[1], pz = pp[2];
    float best = 3.0e38f, qx = 0.f, qy = 0.f, qz = 0.f, wa = 0.f, wb = 0.f, wc = 0.f;
    int face = -1;
    if (__ballot(live) != 0ULL) icp_walk<true>(s, count, px, py, pz, best, qx, qy, qz, face, wa, wb, wc);      // wave-uniform
    const bool hit = live && face >= 0, in = hit && sqrtf(best) < trim;
    double a[2] = {in ? 1.0 : 0.0, in ? (double)best : 0.0};
    icp_block_sum<2>(a, s.red, s.sum);                         // (its barriers: every lane has left the walk, the corner list is dead)
    const double m = s.sum[0];
    if (t == 0) {
        loss[row] = m > 0.0 ? (float)(s.sum[1] / m) : 0.f;
        inliers[row] = (int)m;
    }
    if (t < P) {
        if (closest != nullptr) { float* c = closest + (row * P + t) * 3; c[0] = hit ? qx : 0.f; c[1] = hit ? qy : 0.f; c[2] = hit ? qz : 0.f; }
        if (bary != nullptr) { float* w = bary + (row * P + t) * 3; w[0] = hit ? wa : 0.f; w[1] = hit ? wb : 0.f; w[2] = hit ? wc : 0.f; }
        if (tri != nullptr) tri[row * P + t] = hit ? face : -1;
    }
    if (grad == nullptr) return;                               // block-uniform
    const float sc = in ? (float)(-2.0 / m) : 0.f;
    const double3 gv = geo_corner_gather(s, wa, wb, wc, in ? sc * (px - qx) : 0.f, in ? sc * (py - qy) : 0.f, in ? sc * (pz - qz) : 0.f,
                                         in ? face : -1, P, n);
    if (t < n) {
        float* g = grad + (row * n + t) * 3;
        g[0] = (float)gv.x; g[1] = (float)gv.y; g[2] = (float)gv.z;
    }
}

PDF_API int pdf_cloud_mesh_loss(const float* verts, const long long* faces, const float* cloud, const float* valid, int B, int n, int Fc, int P,
                                float trim, float* loss, int* inliers, float* grad, int* tri, float* closest, float* bary, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (B <= 0) return 0;
    if (n < 1 || n > HAND_MAXN || Fc < 1 || Fc > HAND_MAXF || P < 1 || P > HAND_MAXP || !(trim > 0.f) || !(trim <= 3.0e38f) || verts == nullptr ||
        faces == nullptr || cloud == nullptr || loss == nullptr || inliers == nullptr)
        return PDF_E_BADARG;
    hipLaunchKernelGGL(cloud_mesh_loss_kernel, dim3(2 * B), dim3(ICP_T), 0, s, verts, faces, cloud, valid, n, Fc, P, trim, loss, inliers, grad, tri,
                       closest, bary);
    PDF_LAUNCH_CHECK();
    return 0;
}

// ---- per-vertex targets of a MANO fit against the cloud (contract: pdf_mano_cloud_targets in pdfnet_hip.h) ---------------------------------
// cloud_mesh_loss_kernel's association once more -- icp_facing and icp_walk<true>, shared -- for ONE hand per row (faces [Fc][3], no hand
// index).  An inlier's residual d = p - q goes to the three corners of its triangle with the weights w_k of q = wa a + wb b + wc c: vertex v
// collects W_v = sum w_k and S_v = sum w_k d (geo_corner_gather_w: in double, ascending point order, no atomics), and the weighted per-vertex
// energy sum_v W_v |M_v - (v + S_v / W_v)|^2 majorises the point-to-surface energy of the fixed association, with equality at M = verts.  The
// anchor adds anchor_weight |M_v - a_v|^2 per vertex; both merge into one target and one weight, which is what mano_fit_kernel takes.
__global__ __launch_bounds__(ICP_T) void mano_cloud_targets_kernel(const float* __restrict__ verts, const long long* __restrict__ faces,
                                                                   const float* __restrict__ cloud, const float* __restrict__ valid,
                                                                   const float* __restrict__ anchor, float alpha, int n, int Fc, int P, float trim,
                                                                   float* __restrict__ target, float* __restrict__ weight, float* __restrict__ rms,
                                                                   int* __restrict__ inliers, int* __restrict__ tri, float* __restrict__ closest,
                                                                   float* __restrict__ bary) {
    __shared__ IcpShared s;
    const int t = threadIdx.x;
    const long row = blockIdx.x;
    const float* pp = cloud + (row * P + min(t, P - 1)) * 3;
    const float* vp = verts + (row * n + min(t, n - 1)) * 3;
    const float* ap = anchor != nullptr ? anchor + (row * n + min(t, n - 1)) * 3 : nullptr;
    if (ap == nullptr) alpha = 0.f;
    const bool live = t < P && pp[2] > 0.f;
    const bool row_ok = valid == nullptr || valid[row] != 0.f;
    if (!__syncthreads_or(live && row_ok)) {                   // block-uniform: nothing to compare the hand with; the anchor alone
        if (t == 0) { rms[row] = 0.f; inliers[row] = 0; }
        if (t < n) {
            const float* src = alpha > 0.f ? ap : vp;
            float* o = target + (row * n + t) * 3;
            o[0] = src[0]; o[1] = src[1]; o[2] = src[2];
            weight[row * n + t] = alpha;
        }
        if (t < P) {
            if (closest != nullptr) { float* c = closest + (row * P + t) * 3; c[0] = c[1] = c[2] = 0.f; }
            if (bary != nullptr) { float* w = bary + (row * P + t) * 3; w[0] = w[1] = w[2] = 0.f; }
            if (tri != nullptr) tri[row * P + t] = -1;
        }
        return;
    }
    if (t < n) { s.vx[t] = vp[0]; s.vy[t] = vp[1]; s.vz[t] = vp[2]; }
    geo_stage_faces(faces, Fc, n, s.tri);
    __syncthreads();

    const int count = icp_facing(s, Fc);                       // (ends in a barrier)
    const float px = pp[0], py = pp[1], pz = pp[2];
    float best = 3.0e38f, qx = 0.f, qy = 0.f, qz = 0.f, wa = 0.f, wb = 0.f, wc = 0.f;
    int face = -1;
    if (__ballot(live) != 0ULL) icp_walk<true>(s, count, px, py, pz, best, qx, qy, qz, face, wa, wb, wc);      // wave-uniform
    const bool hit = live && face >= 0, in = hit && sqrtf(best) < trim;
    double a[2] = {in ? 1.0 : 0.0, in ? (double)best : 0.0};
    icp_block_sum<2>(a, s.red, s.sum);                         // (its barriers: every lane has left the walk, the corner list is dead)
    if (t == 0) {
        rms[row] = s.sum[0] > 0.0 ? (float)sqrt(s.sum[1] / s.sum[0]) : 0.f;
        inliers[row] = (int)s.sum[0];
    }
    if (t < P) {
        if (closest != nullptr) { float* c = closest + (row * P + t) * 3; c[0] = hit ? qx : 0.f; c[1] = hit ? qy : 0.f; c[2] = hit ? qz : 0.f; }
        if (bary != nullptr) { float* w = bary + (row * P + t) * 3; w[0] = hit ? wa : 0.f; w[1] = hit ? wb : 0.f; w[2] = hit ? wc : 0.f; }
        if (tri != nullptr) tri[row * P + t] = hit ? face : -1;
    }
    const double4 ws = geo_corner_gather_w(s, wa, wb, wc, in ? px - qx : 0.f, in ? py - qy : 0.f, in ? pz - qz : 0.f, in ? face : -1, P, n);
    if (t < n) {
        const double W = ws.w, den = W + (double)alpha;
        const float vx = s.vx[t], vy = s.vy[t], vz = s.vz[t];
        float* o = target + (row * n + t) * 3;
        if (W == 0.0) {                                         // no inlier names the vertex: the anchor, or the vertex itself
            const float* src = alpha > 0.f ? ap : vp;
            o[0] = src[0]; o[1] = src[1]; o[2] = src[2];
        } else {
            const double ax = alpha > 0.f ? (double)alpha * ap[0] : 0.0, ay = alpha > 0.f ? (double)alpha * ap[1] : 0.0,
                         az = alpha > 0.f ? (double)alpha * ap[2] : 0.0;
            o[0] = (float)((W * vx + ws.x + ax) / den);
            o[1] = (float)((W * vy + ws.y + ay) / den);
            o[2] = (float)((W * vz + ws.z + az) / den);
        }
        weight[row * n + t] = (float)den;
    }
}

PDF_API int pdf_mano_cloud_targets(const float* verts, const long long* faces, const float* cloud, const float* valid, const float* anchor,
                                   float anchor_weight, int B, int n, int Fc, int P, float trim, float* target, float* weight, float* rms,
                                   int* inliers, int* tri, float* closest, float* bary, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (B <= 0) return 0;
    if (n < 1 || n > HAND_MAXN || Fc < 1 || Fc > HAND_MAXF || P < 1 || P > HAND_MAXP || !(trim > 0.f) || !(trim <= 3.0e38f) ||
        !(anchor_weight >= 0.f) || !(anchor_weight <= 3.0e38f) || verts == nullptr || faces == nullptr || cloud == nullptr || target == nullptr ||
        weight == nullptr || rms == nullptr || inliers == nullptr)
        return PDF_E_BADARG;
    hipLaunchKernelGGL(mano_cloud_targets_kernel, dim3(B), dim3(ICP_T), 0, s, verts, faces, cloud, valid, anchor, anchor_weight, n, Fc, P, trim,
                       target, weight, rms, inliers, tri, closest, bary);
    PDF_LAUNCH_CHECK();
    return 0;
}
