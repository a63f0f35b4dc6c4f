// Visibility-aware mesh-to-cloud loss: the other half of the Chamfer distance between a predicted hand mesh and that hand's sensor point cloud
// (contract: pdf_mesh_cloud_loss in pdfnet_hip.h).  pdf_cloud_mesh_loss (icp.hip) pulls the surface towards every sensor point; this one pulls
// every vertex THE CAMERA SEES towards its nearest sensor point, so surface predicted into free space draws a gradient too.  Nothing in the
// reference does this.
//
// One launch, one workgroup of 1,024 lanes per row = (sample, hand); lane t owns vertex t, which it holds in registers.
//   LDS (85 KB): the vertices of BOTH hands of the sample as x / y / z planes (24 KB), the hand's cloud as x / y / z planes (12 KB), and one
//   list of occluders, 48 B an entry: the three corners, and in the spare words the three vertex indices as 16-bit values (0xffff, which is
//   no vertex, for a triangle of the other hand).  The camera-facing triangles of both hands at the bounds are 2 x 2,048 x 48 B, which does
//   not fit, so the occluders are streamed in chunks of 1,024 faces: lane t tests face base + t of the own hand, then of the other hand, by
//   icp_facing's test (geo_faces_camera); the survivors are compacted in face order by a 64-bit __ballot + popcount prefix per wave and the wave totals
//   through LDS (render_tile_kernel's idiom); behind a barrier every lane walks the list front to back, every lane the same entry: three
//   broadcast 16-byte reads.  A wave none of whose lanes can still change its answer skips the walk of a chunk.
//   Occlusion: the ray from the vertex v to the camera at the origin against triangle (a, b, c), with the corners taken relative to the vertex
//   (a' = a - v, ...): s0 = v . (b' x c'), s1 = v . (c' x a'), s2 = v . (a' x b'), S = s0 + s1 + s2, det = a' . (b' x c').  The cross products
//   are made of separately rounded products (geo_det2) and the dot products are icp_dot, so each s_k is EXACTLY odd in the exchange of its
//   edge's two corners: evaluating it from the lower to the higher vertex index and negating as needed (render.hip's idiom) gives the bits
//   that the direct evaluation gives, and the two faces at an edge agree up to sign -- a ray through a shared edge or vertex hits both, a
//   closed surface has no gap.  Hit: s0, s1, s2 >= 0 and S > 0, or s0, s1, s2 <= 0 and S < 0.  With D = -det (S > 0) or det, A = |S|, the
//   occluder hides the vertex when D < A (the hit lies between camera and vertex) and D |v| > margin A (more than `margin` metres from the
//   vertex along the ray).  No division.  A triangle of the own hand that has the vertex as a corner never hides it, and makes it `front`.
//   Match: a visible vertex walks the cloud planes, four points per 16-byte broadcast read; squared distance by icp_dot; a strictly smaller
//   value replaces the best, so the lowest point index wins a tie; a point with Z <= 0 is passed over.
//   Sums: inliers, sum |v - p|^2 and visible vertices as doubles through icp_block_sum, the fixed-order reduction of icp.hip.
// No atomics, no global scratch: two runs are bit-identical and a row depends only on the two hands of its own sample.
#include "mesh_geom.h"

#define MC_CHUNK ICP_T                                         // faces set up per pass = the capacity of the occluder list
#define MC_NOVERT 0xffff

struct McShared {                                              // (the small members first: their addresses fit a DS instruction's 16-bit offset)
    double red[ICP_W * 3], sum[3];
    int wave_n[ICP_W];
    float vx[2][HAND_MAXN], vy[2][HAND_MAXN], vz[2][HAND_MAXN];      // [0]: this row's hand, [1]: the other hand of the sample
    alignas(16) float px[HAND_MAXP];
    alignas(16) float py[HAND_MAXP];
    alignas(16) float pz[HAND_MAXP];
    float4 ca[MC_CHUNK], cb[MC_CHUNK], cc[MC_CHUNK];           // corners; ca.w: indices of a and b as 16-bit halves, cb.w: index of c
};

// faces [base, base + MC_CHUNK) of `fo`, on the staged vertices of hand `which`: the camera-facing ones -> s.ca / cb / cc in face order; returns
// their number (block-uniform).  Ends in a barrier; the caller's walk must be over before the next call writes the list (that call's first
// barrier sees to it).
__device__ __forceinline__ int mc_occluders(McShared& s, const long long* __restrict__ fo, int base, int Fc, int n, int which) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int g = base + t;
    bool keep = false;
    int ia = 0, ib = 0, ic = 0;
    float ax = 0.f, ay = 0.f, az = 0.f, bx = 0.f, by = 0.f, bz = 0.f, cx = 0.f, cy = 0.f, cz = 0.f;
    if (g < Fc) {
        ia = geo_index(fo + 3 * g, n); ib = geo_index(fo + 3 * g + 1, n); ic = geo_index(fo + 3 * g + 2, n);
        ax = s.vx[which][ia]; ay = s.vy[which][ia]; az = s.vz[which][ia];
        bx = s.vx[which][ib]; by = s.vy[which][ib]; bz = s.vz[which][ib];
        cx = s.vx[which][ic]; cy = s.vy[which][ic]; cz = s.vz[which][ic];
        keep = geo_faces_camera(ax, ay, az, bx, by, bz, cx, cy, cz);
    }
    const unsigned long long mask = __ballot(keep);
    if (lane == 0) s.wave_n[wave] = __popcll(mask);
    __syncthreads();                                           // (every lane has also left the walk of the previous chunk)
    int off = __popcll(mask & ((1ULL << lane) - 1ULL)), total = 0;
#pragma unroll
    for (int w = 0; w < ICP_W; ++w) {
        const int c = s.wave_n[w];
        if (w < wave) off += c;
        total += c;
    }
    if (keep) {                                                // off < total <= MC_CHUNK
        if (which != 0) ia = ib = ic = MC_NOVERT;              // a triangle of the other hand names no vertex of this one
        s.ca[off] = make_float4(ax, ay, az, __int_as_float(ia | (ib << 16)));
        s.cb[off] = make_float4(bx, by, bz, __int_as_float(ic));
        s.cc[off] = make_float4(cx, cy, cz, 0.f);
    }
    __syncthreads();
    return total;
}

__global__ __launch_bounds__(ICP_T) void mesh_cloud_loss_kernel(const float* __restrict__ verts, const long long* __restrict__ faces,
                                                                const float* __restrict__ cloud, const float* __restrict__ valid, int n, int Fc,
                                                                int P, float trim, float margin, float* __restrict__ loss,
                                                                int* __restrict__ inliers, int* __restrict__ visible, float* __restrict__ grad,
                                                                int* __restrict__ vis, int* __restrict__ nn) {
    __shared__ McShared s;
    const int t = threadIdx.x;
    const long row = blockIdx.x;
    const int h = (int)(row & 1);
    if (valid != nullptr && valid[row] == 0.f) {               // block-uniform: the hand is not there
        if (t == 0) { loss[row] = 0.f; inliers[row] = 0; visible[row] = 0; }
        if (t < n) {
            if (grad != nullptr) { float* g = grad + (row * n + t) * 3; g[0] = g[1] = g[2] = 0.f; }
            if (vis != nullptr) vis[row * n + t] = 0;
            if (nn != nullptr) nn[row * n + t] = -1;
        }
        return;
    }
    const bool other_ok = valid == nullptr || valid[row ^ 1] != 0.f;
    const float* vp = verts + (row * n + min(t, n - 1)) * 3;
    const float vx = vp[0], vy = vp[1], vz = vp[2];
    if (t < n) {
        s.vx[0][t] = vx; s.vy[0][t] = vy; s.vz[0][t] = vz;
        const float* op = verts + ((row ^ 1) * n + t) * 3;
        s.vx[1][t] = op[0]; s.vy[1][t] = op[1]; s.vz[1][t] = op[2];
    }
    {                                                          // every slot of the planes: a slot past P holds Z = 0, which is no point
        const float* pp = cloud + (row * P + min(t, P - 1)) * 3;
        const bool there = t < P;
        s.px[t] = there ? pp[0] : 0.f; s.py[t] = there ? pp[1] : 0.f; s.pz[t] = there ? pp[2] : 0.f;
    }
    __syncthreads();
    const float vlen = sqrtf(icp_dot(vx, vy, vz, vx, vy, vz));
    bool hidden = t >= n, front = false;                       // hidden: nothing can make this lane's vertex visible any more
    for (int which = 0; which < (other_ok ? 2 : 1); ++which) {
        const long long* fo = faces + (long)(h ^ which) * Fc * 3;
        if (which == 1) hidden = hidden || !front;             // the own hand is through: front is final
        for (int base = 0; base < Fc; base += MC_CHUNK) {
            const int count = mc_occluders(s, fo, base, Fc, n, which);
            if (__ballot(!hidden) == 0ULL) continue;           // wave-uniform
            for (int j = 0; j < count; ++j) {
                const float4 a = s.ca[j], b = s.cb[j], c = s.cc[j];
                const int iab = __float_as_int(a.w), ic = __float_as_int(b.w);
                const bool mine = (iab & 0xffff) == t || ((iab >> 16) & 0xffff) == t || ic == t;
                front = front || mine;
                const float ax = a.x - vx, ay = a.y - vy, az = a.z - vz;
                const float bx = b.x - vx, by = b.y - vy, bz = b.z - vz;
                const float cx = c.x - vx, cy = c.y - vy, cz = c.z - vz;
                const float ux = geo_det2(by, cz, bz, cy), uy = geo_det2(bz, cx, bx, cz), uz = geo_det2(bx, cy, by, cx);      // b' x c'
                const float s0 = icp_dot(vx, vy, vz, ux, uy, uz);
                const float s1 = icp_dot(vx, vy, vz, geo_det2(cy, az, cz, ay), geo_det2(cz, ax, cx, az), geo_det2(cx, ay, cy, ax));
                const float s2 = icp_dot(vx, vy, vz, geo_det2(ay, bz, az, by), geo_det2(az, bx, ax, bz), geo_det2(ax, by, ay, bx));
                const float det = icp_dot(ax, ay, az, ux, uy, uz);
                const float S = s0 + s1 + s2;
                const bool hit = (s0 >= 0.f && s1 >= 0.f && s2 >= 0.f && S > 0.f) || (s0 <= 0.f && s1 <= 0.f && s2 <= 0.f && S < 0.f);
                const float D = S > 0.f ? -det : det, A = fabsf(S);
                hidden = hidden || (hit && !mine && D < A && D * vlen > margin * A);
            }
        }
    }
    const bool seen = !hidden && front;

    float best = 3.0e38f;
    int near = -1;
    if (__ballot(seen) != 0ULL) {                              // wave-uniform; the result of a lane that is not `seen` is not used
        for (int j = 0; j < P; j += 4) {                       // (the slots up to the next multiple of 4 hold Z = 0)
            const float4 X = *reinterpret_cast<const float4*>(&s.px[j]), Y = *reinterpret_cast<const float4*>(&s.py[j]),
                         Z = *reinterpret_cast<const float4*>(&s.pz[j]);
            const float xs[4] = {X.x, X.y, X.z, X.w}, ys[4] = {Y.x, Y.y, Y.z, Y.w}, zs[4] = {Z.x, Z.y, Z.z, Z.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float dx = vx - xs[k], dy = vy - ys[k], dz = vz - zs[k];
                const float dd = icp_dot(dx, dy, dz, dx, dy, dz);
                if (zs[k] > 0.f && dd < best) { best = dd; near = j + k; }
            }
        }
    }
    const bool matched = seen && near >= 0, in = matched && sqrtf(best) < trim;
    double a[3] = {in ? 1.0 : 0.0, in ? (double)best : 0.0, seen ? 1.0 : 0.0};
    icp_block_sum<3>(a, s.red, s.sum);
    const double m = s.sum[0];
    if (t == 0) {
        loss[row] = m > 0.0 ? (float)(s.sum[1] / m) : 0.f;
        inliers[row] = (int)m;
        visible[row] = (int)s.sum[2];
    }
    if (t < n) {
        if (grad != nullptr) {
            const int k = in ? near : 0;
            const float sc = in ? (float)(2.0 / m) : 0.f;
            float* g = grad + (row * n + t) * 3;
            g[0] = in ? sc * (vx - s.px[k]) : 0.f; g[1] = in ? sc * (vy - s.py[k]) : 0.f; g[2] = in ? sc * (vz - s.pz[k]) : 0.f;
        }
        if (vis != nullptr) vis[row * n + t] = seen ? 1 : 0;
        if (nn != nullptr) nn[row * n + t] = matched ? near : -1;
    }
}

PDF_API int pdf_mesh_cloud_loss(const float* verts, const long long* faces, const float* cloud, const float* valid, int B, int n, int Fc, int P,
                                float trim, float margin, float* loss, int* inliers, int* visible, float* grad, int* vis, int* nn, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (B <= 0) return 0;
    if (n < 1 || n > HAND_MAXN || Fc < 1 || Fc > HAND_MAXF || P < 1 || P > HAND_MAXP || !(trim > 0.f) || !(trim <= 3.0e38f) || !(margin >= 0.f) ||
        !(margin <= 3.0e38f) || verts == nullptr || faces == nullptr || cloud == nullptr || loss == nullptr || inliers == nullptr ||
        visible == nullptr)
        return PDF_E_BADARG;
    hipLaunchKernelGGL(mesh_cloud_loss_kernel, dim3(2 * B), dim3(ICP_T), 0, s, verts, faces, cloud, valid, n, Fc, P, trim, margin, loss, inliers,
                       visible, grad, vis, nn);
    PDF_LAUNCH_CHECK();
    return 0;
}
