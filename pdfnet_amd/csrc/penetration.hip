// Differentiable inter-hand penetration loss (contract: pdf_penetration_loss in pdfnet_hip.h).  Nothing in the reference does this: it neither
// measures nor penalises one hand's surface inside the other's.
//
// One launch, one workgroup of 1,024 lanes per row = (sample, hand); lane t owns vertex t of hand h, and the mesh is the OTHER hand's.
//   LDS (IcpShared, mesh_geom.h): the other hand's vertices as x / y / z planes (12 KB), its faces as 16-bit triples (16 KB), and ALL its
//   triangles as their three corners in face order, 48 B a triangle (96 KB): both loops read the list front to back, every lane the same
//   triangle, three broadcast 16-byte reads.
//   Inside: the generalized winding number of mesh_penetration_kernel (metrics.hip) -- the corners relative to the vertex, each triangle's
//   term by the function both kernels call (geo_solid_angle), atan2f, summed in double in ascending face order, the same scaling and the same
//   fp32 comparison with 0.5.  The corner list holds the very floats metrics.hip reads from its planes, so `inside` is its wind > 0.5
//   (tests/test_penetration_loss_gpu.py compares the two entry points bit for bit).
//   Closest point: icp_walk<true>, the device code behind pdf_mesh_icp and pdf_cloud_mesh_loss, over the whole list.  Only a wave that holds
//   an inside vertex walks (wave-uniform); separated hands walk nothing.
//   loss = (1/n) sum |v - q|^2 over the inside vertices, by the fixed-order block sum.  grad_self of an inside vertex is (2/n)(v - q).
//   grad_other, without atomics: geo_corner_gather over the n records of the row's vertices, each carrying -(2/n)(v - q); lane t < n gets the
//   sum for vertex t of the other hand.  A row writes only its own row of both gradient tensors, so nothing is accumulated across workgroups.
#include "mesh_geom.h"

__global__ __launch_bounds__(ICP_T) void penetration_loss_kernel(const float* __restrict__ verts, const long long* __restrict__ faces,
                                                                 const float* __restrict__ valid, int n, int Fc, float* __restrict__ loss,
                                                                 int* __restrict__ count, float* __restrict__ grad_self,
                                                                 float* __restrict__ grad_other, int* __restrict__ inside_out,
                                                                 int* __restrict__ tri, float* __restrict__ bary, float* __restrict__ closest) {
    __shared__ IcpShared s;
    const int t = threadIdx.x;
    const long row = blockIdx.x;
    const int h = (int)(row & 1);
    const long at = row * n + t;                               // (used by lanes t < n only)
    const bool row_ok = valid == nullptr || (valid[row] != 0.f && valid[row ^ 1] != 0.f);      // block-uniform: both hands of the sample
    if (!row_ok) {
        if (t == 0) { loss[row] = 0.f; count[row] = 0; }
        if (t < n) {
            if (grad_self != nullptr) { float* g = grad_self + at * 3; g[0] = g[1] = g[2] = 0.f; }
            if (grad_other != nullptr) { float* g = grad_other + at * 3; g[0] = g[1] = g[2] = 0.f; }
            if (inside_out != nullptr) inside_out[at] = 0;
            if (tri != nullptr) tri[at] = -1;
            if (bary != nullptr) { float* w = bary + at * 3; w[0] = w[1] = w[2] = 0.f; }
            if (closest != nullptr) { float* c = closest + at * 3; c[0] = c[1] = c[2] = 0.f; }
        }
        return;
    }
    const float* other = verts + (row ^ 1) * n * 3;            // rows 2b, 2b + 1 are the two hands of sample b
    geo_stage_planes(other, n, s.vx, s.vy, s.vz);
    geo_stage_faces(faces + (long)(1 - h) * Fc * 3, Fc, n, s.tri);
    __syncthreads();
    for (int g = t; g < Fc; g += ICP_T) {                      // every triangle is listed, in face order; ca.w carries the face index
        const ushort4 f = s.tri[g];
        s.ca[g] = make_float4(s.vx[f.x], s.vy[f.x], s.vz[f.x], __int_as_float(g));
        s.cb[g] = make_float4(s.vx[f.y], s.vy[f.y], s.vz[f.y], 0.f);
        s.cc[g] = make_float4(s.vx[f.z], s.vy[f.z], s.vz[f.z], 0.f);
    }
    __syncthreads();

    const float* p = verts + (row * n + min(t, n - 1)) * 3;
    const float x = p[0], y = p[1], z = p[2];
    bool in = false;
    if (t < n) {
        double omega = 0.0;
        for (int j = 0; j < Fc; ++j) {
            const float4 A = s.ca[j], B = s.cb[j], C = s.cc[j];
            const float ax = A.x - x, ay = A.y - y, az = A.z - z;
            const float bx = B.x - x, by = B.y - y, bz = B.z - z;
            const float cx = C.x - x, cy = C.y - y, cz = C.z - z;
            float det, den;
            geo_solid_angle(ax, ay, az, bx, by, bz, cx, cy, cz, det, den);
            omega += (double)atan2f(det, den);
        }
        const float w = (float)(omega * (2.0 / (4.0 * 3.14159265358979323846)));
        in = w > 0.5f;
    }
    float best = 3.0e38f, qx = 0.f, qy = 0.f, qz = 0.f, wa = 0.f, wb = 0.f, wc = 0.f;
    int face = -1;
    if (__ballot(in) != 0ULL) icp_walk<true>(s, Fc, x, y, z, best, qx, qy, qz, face, wa, wb, wc);      // wave-uniform; only an inside lane's result is used
    double a[2] = {in ? 1.0 : 0.0, in ? (double)best : 0.0};
    icp_block_sum<2>(a, s.red, s.sum);                         // (its barriers: every lane has left the walk, the corner list is dead)
    const int m = (int)s.sum[0];
    if (t == 0) {
        loss[row] = (float)(s.sum[1] / (double)n);
        count[row] = m;
    }
    const float k2 = (float)(2.0 / (double)n);
    const float gx = in ? k2 * (x - qx) : 0.f, gy = in ? k2 * (y - qy) : 0.f, gz = in ? k2 * (z - qz) : 0.f;
    if (t < n) {
        if (grad_self != nullptr) { float* g = grad_self + at * 3; g[0] = gx; g[1] = gy; g[2] = gz; }
        if (inside_out != nullptr) inside_out[at] = in ? 1 : 0;
        if (tri != nullptr) tri[at] = in ? face : -1;
        if (bary != nullptr) { float* w = bary + at * 3; w[0] = in ? wa : 0.f; w[1] = in ? wb : 0.f; w[2] = in ? wc : 0.f; }
        if (closest != nullptr) { float* c = closest + at * 3; c[0] = in ? qx : 0.f; c[1] = in ? qy : 0.f; c[2] = in ? qz : 0.f; }
    }
    if (grad_other == nullptr) return;                         // block-uniform
    if (m == 0) {                                              // block-uniform: no record names a vertex
        if (t < n) { float* g = grad_other + at * 3; g[0] = g[1] = g[2] = 0.f; }
        return;
    }
    // (an inside lane's walk found a face: Fc >= 1)
    const double3 go = geo_corner_gather(s, wa, wb, wc, -gx, -gy, -gz, in ? face : -1, n, n);
    if (t < n) {
        float* g = grad_other + at * 3;
        g[0] = (float)go.x; g[1] = (float)go.y; g[2] = (float)go.z;
    }
}

PDF_API int pdf_penetration_loss(const float* verts, const long long* faces, const float* valid, int B, int n, int Fc, float* loss, int* count,
                                 float* grad_self, float* grad_other, int* inside, int* tri, float* bary, float* closest, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (B <= 0) return 0;
    if (n < 1 || n > HAND_MAXN || Fc < 1 || Fc > HAND_MAXF || verts == nullptr || faces == nullptr || loss == nullptr || count == nullptr)
        return PDF_E_BADARG;
    hipLaunchKernelGGL(penetration_loss_kernel, dim3(2 * B), dim3(ICP_T), 0, s, verts, faces, valid, n, Fc, loss, count, grad_self, grad_other,
                       inside, tri, bary, closest);
    PDF_LAUNCH_CHECK();
    return 0;
}
