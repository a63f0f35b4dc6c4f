// Differentiable soft-silhouette loss of the two hand meshes against per-hand masks (contract: pdf_silhouette_loss in pdfnet_hip.h).  The
// reference's legacy branch trained on pytorch3d's rendered masks (lib/trains/simplified.py); csrc/render.hip is the hard rasteriser behind
// the evaluation's silhouette IoU and has no gradient.  Here every triangle is a sigmoid of its signed squared screen distance and the
// triangles of a hand are aggregated as a product: no z-buffer, no coverage decision, smooth by construction.  The projection (geo_project,
// mesh_geom.h) and the pixel centres are render.hip's.  Deterministic, no atomics: two runs are bit-identical.
//
// DESIGN (five launches; the last two only when a gradient is asked for)
//   sil_vertex_kernel: one thread per (sample, hand, vertex) writes (x, y, 1/Z, Z) into the scratch.
//   sil_tile_kernel: grid (ceil(W/16), 2 ceil(H/16), B), 256 threads = one 16 x 16 tile of ONE hand, one pixel per thread (render_tile_kernel's
//   shape).  The hand's Fc faces are taken 256 at a time: thread t sets up face t (sil_face: the rejections, the bounding box grown by rho)
//   and tests the grown box against the tile's pixel centres; the survivors are compacted in face order (64-bit __ballot + popcount prefix per
//   wave, wave totals through LDS) into an LDS list of 48 B per face -- (x0, y0, x1, y1), (x2, y2, sign(A2), -), the grown box -- 12 KB.
//   After a barrier every pixel walks the list (each LDS read a 16-byte broadcast), tests ITS centre against the grown box (the inclusion rule:
//   the tiles only prune) and adds log(1 - sigmoid(x)) in ascending face order.  The epilogue writes T = exp(sum) and the tile's
//   (sum w S M, sum w (S + M - S M)) in double: a butterfly per wave, the four waves added in order by thread 0.
//   sil_finish_kernel: one block per (sample, hand) stages the tile partials through LDS 256 at a time and thread 0 adds them in ascending
//   tile order in double; it writes loss, (I, U) and the two coefficients of d loss / d S.
//   sil_face_grad_kernel: one wave per face walks the pixels of the face's grown box clipped to the image (the float bounds are clamped to
//   the image BEFORE they become integers, and only for a face that passed the finiteness check), applies the same inclusion test, recomputes
//   x, the nearest edge and t by the forward's own function (sil_eval), reads T, M and w, and accumulates d loss / d (screen corner) in six
//   floats per lane, reduced by a butterfly; lane 0 writes gface [B,2,Fc,3,2].  A skipped face writes zeros.
//   sil_vertex_grad_kernel: one thread per vertex gathers gface over the vertex -> face table in ascending face order, finds its corner(s) by
//   comparing clamped indices, applies the pinhole Jacobian and writes grad.  A vertex without a contribution gets exactly 0.
#include "mesh_geom.h"                                          // HAND_MAXN, HAND_MAXF, geo_det2, geo_index, geo_project

#define SIL_T 256
#define SIL_TILE 16
#define SIL_MAXM 32
#define SIL_MAXHW 2048
#define SIL_CUT 16.0f                                           // rho^2 = SIL_CUT sigma: sigmoid(-16) = 1.1e-7 at the inclusion border

struct SilFace {
    float x0, y0, x1, y1, x2, y2, s;                            // screen corners, sign(A2)
    float bx0, by0, bx1, by1;                                   // the bounding box grown by rho
};

// The corners of a face from the vertex pass's records and every rejection of the contract.  false: the face is skipped whole.
__device__ __forceinline__ bool sil_face(const float4 a, const float4 b, const float4 c, float z_near, float rho, SilFace& f) {
#pragma clang fp contract(off)
    const bool front = a.w >= z_near && b.w >= z_near && c.w >= z_near;                     // (false for a NaN depth)
    const bool finite = isfinite(a.x) && isfinite(a.y) && isfinite(b.x) && isfinite(b.y) && isfinite(c.x) && isfinite(c.y);
    const float a2 = geo_det2(b.x - a.x, c.y - a.y, c.x - a.x, b.y - a.y);                  // products rounded separately: a repeated corner gives exactly 0
    f.x0 = a.x; f.y0 = a.y; f.x1 = b.x; f.y1 = b.y; f.x2 = c.x; f.y2 = c.y;
    f.s = a2 > 0.f ? 1.f : -1.f;
    f.bx0 = fminf(fminf(a.x, b.x), c.x) - rho; f.bx1 = fmaxf(fmaxf(a.x, b.x), c.x) + rho;
    f.by0 = fminf(fminf(a.y, b.y), c.y) - rho; f.by1 = fmaxf(fmaxf(a.y, b.y), c.y) + rho;
    return front && finite && fabsf(a2) > 0.f;
}

__device__ __forceinline__ bool sil_included(const SilFace& f, float px, float py) {
    return px >= f.bx0 && px <= f.bx1 && py >= f.by0 && py <= f.by1;
}

// Squared distance from p to the segment a -> b, its parameter t in [0, 1] and r = p - q.
__device__ __forceinline__ float sil_edge(float px, float py, float ax, float ay, float bx, float by, float& t, float& rx, float& ry) {
    const float ex = bx - ax, ey = by - ay, dx = px - ax, dy = py - ay;
    const float len2 = ex * ex + ey * ey;
    t = len2 > 0.f ? fminf(fmaxf((dx * ex + dy * ey) / len2, 0.f), 1.f) : 0.f;
    rx = px - (ax + t * ex);
    ry = py - (ay + t * ey);
    return rx * rx + ry * ry;
}

// x = +- d^2 / sigma of face f at pixel centre p (+ inside), the nearest edge e (e: corner e -> corner (e + 1) % 3; the first of equals), its
// t and r = p - q.
__device__ __forceinline__ float sil_eval(const SilFace& f, float px, float py, float inv_sigma, int& e, float& t, float& rx, float& ry) {
    float t1, rx1, ry1, t2, rx2, ry2;
    float d2 = sil_edge(px, py, f.x0, f.y0, f.x1, f.y1, t, rx, ry);
    const float d21 = sil_edge(px, py, f.x1, f.y1, f.x2, f.y2, t1, rx1, ry1);
    const float d22 = sil_edge(px, py, f.x2, f.y2, f.x0, f.y0, t2, rx2, ry2);
    e = 0;
    if (d21 < d2) { d2 = d21; e = 1; t = t1; rx = rx1; ry = ry1; }
    if (d22 < d2) { d2 = d22; e = 2; t = t2; rx = rx2; ry = ry2; }
    const float e0 = f.s * ((f.x1 - f.x0) * (py - f.y0) - (f.y1 - f.y0) * (px - f.x0));
    const float e1 = f.s * ((f.x2 - f.x1) * (py - f.y1) - (f.y2 - f.y1) * (px - f.x1));
    const float e2 = f.s * ((f.x0 - f.x2) * (py - f.y2) - (f.y0 - f.y2) * (px - f.x2));
    const bool inside = e0 >= 0.f && e1 >= 0.f && e2 >= 0.f;
    const float x = d2 * inv_sigma;
    return inside ? x : -x;
}

// log(1 - sigmoid(x)) = -softplus(x), in the form that neither overflows nor cancels
__device__ __forceinline__ float sil_log_one_minus_sigmoid(float x) {
    return x >= 0.f ? -(x + log1pf(expf(-x))) : -log1pf(expf(x));
}
__device__ __forceinline__ float sil_sigmoid(float x) {
    if (x >= 0.f) return 1.f / (1.f + expf(-x));
    const float e = expf(x);
    return e / (1.f + e);
}

__global__ __launch_bounds__(SIL_T) void sil_vertex_kernel(const float* __restrict__ verts, const float* __restrict__ K, long total, int n,
                                                           float4* __restrict__ scr) {
    const long e = (long)blockIdx.x * SIL_T + threadIdx.x;       // (b, h, i)
    if (e >= total) return;
    const float* p = verts + e * 3;
    scr[e] = geo_project(K + (e / n >> 1) * 9, p[0], p[1], p[2]);
}

__global__ __launch_bounds__(SIL_T) void sil_tile_kernel(const long long* __restrict__ faces, const float* __restrict__ valid,
                                                         const float* __restrict__ mask, const float* __restrict__ weight,
                                                         const float4* __restrict__ scr, int n, int Fc, int H, int W, int tiles_y, float inv_sigma,
                                                         float rho, float z_near, float* __restrict__ trans, double2* __restrict__ partial) {
    __shared__ float4 list[SIL_T * 3];
    __shared__ int wave_n[SIL_T / 64];
    __shared__ double red[SIL_T / 64][2];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int h = blockIdx.y / tiles_y, ty = blockIdx.y - h * tiles_y;
    const long bh = (long)blockIdx.z * 2 + h;
    const int tx0 = blockIdx.x * SIL_TILE, ty0 = ty * SIL_TILE;
    const int col = tx0 + (t & (SIL_TILE - 1)), row = ty0 + (t >> 4);
    const float px = (float)col + 0.5f, py = (float)row + 0.5f;
    // pixel centres of this tile, clipped to the image
    const float cx0 = (float)tx0 + 0.5f, cx1 = (float)min(tx0 + SIL_TILE, W) - 0.5f, cy0 = (float)ty0 + 0.5f, cy1 = (float)min(ty0 + SIL_TILE, H) - 0.5f;
    const bool live = valid == nullptr || valid[bh] != 0.f;     // block-uniform
    const long long* hf = faces + (long)h * Fc * 3;
    const float4* sv = scr + bh * n;
    float sum = 0.f;
    for (int base = 0; live && base < Fc; base += SIL_T) {
        const int g = base + t;
        bool keep = false;
        SilFace f;
        if (g < Fc) {
            const long long* fi = hf + (long)g * 3;
            keep = sil_face(sv[geo_index(fi, n)], sv[geo_index(fi + 1, n)], sv[geo_index(fi + 2, n)], z_near, rho, f);
            keep = keep && !(f.bx1 < cx0 || f.bx0 > cx1 || f.by1 < cy0 || f.by0 > cy1);
        }
        const unsigned long long m = __ballot(keep);
        if (lane == 0) wave_n[wave] = __popcll(m);
        __syncthreads();
        int off = __popcll(m & ((1ULL << lane) - 1ULL)), count = 0;
#pragma unroll
        for (int w = 0; w < SIL_T / 64; ++w) {
            const int c = wave_n[w];
            if (w < wave) off += c;
            count += c;
        }
        if (keep) {                                                // off < count <= SIL_T
            list[off * 3 + 0] = make_float4(f.x0, f.y0, f.x1, f.y1);
            list[off * 3 + 1] = make_float4(f.x2, f.y2, f.s, 0.f);
            list[off * 3 + 2] = make_float4(f.bx0, f.by0, f.bx1, f.by1);
        }
        __syncthreads();
        for (int j = 0; j < count; ++j) {
            const float4 l0 = list[j * 3 + 0], l1 = list[j * 3 + 1], l2 = list[j * 3 + 2];
            SilFace q;
            q.x0 = l0.x; q.y0 = l0.y; q.x1 = l0.z; q.y1 = l0.w; q.x2 = l1.x; q.y2 = l1.y; q.s = l1.z;
            q.bx0 = l2.x; q.by0 = l2.y; q.bx1 = l2.z; q.by1 = l2.w;
            if (sil_included(q, px, py)) {
                int e;
                float tt, rx, ry;
                sum += sil_log_one_minus_sigmoid(sil_eval(q, px, py, inv_sigma, e, tt, rx, ry));
            }
        }
        __syncthreads();                                           // the list is rewritten by the next chunk
    }
    double a = 0.0, u = 0.0;
    if (col < W && row < H) {
        const long pix = (bh * H + row) * W + col;
        const float T = expf(sum);                                 // no face: expf(0) = 1 exactly
        trans[pix] = T;
        const double S = 1.0 - (double)T, M = (double)mask[pix], w = weight != nullptr ? (double)weight[pix] : 1.0;
        a = w * S * M;
        u = w * (S + M - S * M);
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) { a += __shfl_xor(a, s, 64); u += __shfl_xor(u, s, 64); }
    if (lane == 0) { red[wave][0] = a; red[wave][1] = u; }
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < SIL_T / 64; ++w) { a += red[w][0]; u += red[w][1]; }
        partial[(bh * tiles_y + ty) * gridDim.x + blockIdx.x] = make_double2(a, u);
    }
}

__global__ __launch_bounds__(SIL_T) void sil_finish_kernel(const double2* __restrict__ partial, const float* __restrict__ valid, int tiles,
                                                           float* __restrict__ loss, float* __restrict__ sums, float* __restrict__ coef) {
    __shared__ double2 stage[SIL_T];
    const long bh = blockIdx.x;
    const double2* p = partial + bh * tiles;
    double I = 0.0, U = 0.0;
    for (int base = 0; base < tiles; base += SIL_T) {
        if (base + (int)threadIdx.x < tiles) stage[threadIdx.x] = p[base + threadIdx.x];
        __syncthreads();
        if (threadIdx.x == 0) {
            const int m = min(SIL_T, tiles - base);
            for (int j = 0; j < m; ++j) { I += stage[j].x; U += stage[j].y; }
        }
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const bool live = valid == nullptr || valid[bh] != 0.f;
    const double d = U + 1e-6;
    loss[bh] = live ? (float)(1.0 - I / d) : 0.f;
    sums[bh * 2] = (float)I; sums[bh * 2 + 1] = (float)U;
    // d loss / d S_p = w_p (-M_p coef0 + (1 - M_p) coef1)
    coef[bh * 2] = live ? (float)(1.0 / d) : 0.f;
    coef[bh * 2 + 1] = live ? (float)(I / (d * d)) : 0.f;
}

__global__ __launch_bounds__(SIL_T) void sil_face_grad_kernel(const long long* __restrict__ faces, const float* __restrict__ valid,
                                                              const float* __restrict__ mask, const float* __restrict__ weight,
                                                              const float4* __restrict__ scr, const float* __restrict__ trans,
                                                              const float* __restrict__ coef, long total, int n, int Fc, int H, int W,
                                                              float inv_sigma, float rho, float z_near, float* __restrict__ gface) {
    const int lane = threadIdx.x & 63;
    const long e = (long)blockIdx.x * (SIL_T / 64) + (threadIdx.x >> 6);      // (b, h, face): wave-uniform
    if (e >= total) return;
    const long bh = e / Fc;
    const int g = (int)(e - bh * Fc), h = (int)(bh & 1);
    float* out = gface + e * 6;
    SilFace f;
    bool keep = valid == nullptr || valid[bh] != 0.f;
    if (keep) {
        const long long* fi = faces + ((long)h * Fc + g) * 3;
        const float4* sv = scr + bh * n;
        keep = sil_face(sv[geo_index(fi, n)], sv[geo_index(fi + 1, n)], sv[geo_index(fi + 2, n)], z_near, rho, f);
    }
    // a face whose grown box misses every pixel centre contributes nothing either (its clamped window would hold pixels it does not include)
    keep = keep && f.bx1 >= 0.5f && f.by1 >= 0.5f && f.bx0 <= (float)W - 0.5f && f.by0 <= (float)H - 0.5f;
    if (!keep) {                                                   // wave-uniform
        if (lane < 6) out[lane] = 0.f;
        return;
    }
    // finite bounds (sil_face), clamped to the image as floats before they become integers; one pixel of slack, the test below decides
    const int j0 = (int)fminf(fmaxf(f.bx0 - 1.f, 0.f), (float)(W - 1)), j1 = (int)fminf(fmaxf(f.bx1 + 1.f, 0.f), (float)(W - 1));
    const int i0 = (int)fminf(fmaxf(f.by0 - 1.f, 0.f), (float)(H - 1)), i1 = (int)fminf(fmaxf(f.by1 + 1.f, 0.f), (float)(H - 1));
    const int bw = j1 - j0 + 1, count = bw * (i1 - i0 + 1);       // <= 2048 * 2048
    const float c0 = coef[bh * 2], c1 = coef[bh * 2 + 1];
    float g0x = 0.f, g0y = 0.f, g1x = 0.f, g1y = 0.f, g2x = 0.f, g2y = 0.f;
    for (int k = lane; k < count; k += 64) {
        const int r = k / bw, row = i0 + r, col = j0 + (k - r * bw);
        const float px = (float)col + 0.5f, py = (float)row + 0.5f;
        if (!sil_included(f, px, py)) continue;
        int ed;
        float t, rx, ry;
        const float x = sil_eval(f, px, py, inv_sigma, ed, t, rx, ry);
        const long pix = (bh * H + row) * W + col;
        const float M = mask[pix], w = weight != nullptr ? weight[pix] : 1.f;
        const float dS = w * ((1.f - M) * c1 - M * c0);            // d loss / d S
        // d S / d x = T sigmoid(x); d x / d d^2 = +- 1 / sigma; d d^2 / d a = -2 (1 - t) r, d d^2 / d b = -2 t r
        const float k2 = -2.f * dS * trans[pix] * sil_sigmoid(x) * (x >= 0.f ? inv_sigma : -inv_sigma);
        const float ka = k2 * (1.f - t), kb = k2 * t;
        const float ax = ka * rx, ay = ka * ry, bx = kb * rx, by = kb * ry;
        if (ed == 0) { g0x += ax; g0y += ay; g1x += bx; g1y += by; }
        else if (ed == 1) { g1x += ax; g1y += ay; g2x += bx; g2y += by; }
        else { g2x += ax; g2y += ay; g0x += bx; g0y += by; }
    }
    g0x = wave_sum(g0x); g0y = wave_sum(g0y); g1x = wave_sum(g1x); g1y = wave_sum(g1y); g2x = wave_sum(g2x); g2y = wave_sum(g2y);
    if (lane == 0) { out[0] = g0x; out[1] = g0y; out[2] = g1x; out[3] = g1y; out[4] = g2x; out[5] = g2y; }
}

__global__ __launch_bounds__(SIL_T) void sil_vertex_grad_kernel(const float* __restrict__ verts, const long long* __restrict__ faces,
                                                                const float* __restrict__ K, const int* __restrict__ table,
                                                                const float* __restrict__ gface, long total, int n, int Fc, int M,
                                                                float* __restrict__ grad) {
    const long e = (long)blockIdx.x * SIL_T + threadIdx.x;       // (b, h, i)
    if (e >= total) return;
    const long bh = e / n;
    const int i = (int)(e - bh * n), h = (int)(bh & 1);
    const long long* hf = faces + (long)h * Fc * 3;
    const float* gf = gface + bh * Fc * 6;
    float gx = 0.f, gy = 0.f;
    for (int m = 0; m < M; ++m) {
        const int f = table[((long)h * n + i) * M + m];
        if (f < 0 || f >= Fc) continue;
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (geo_index(hf + 3 * f + k, n) == i) { gx += gf[f * 6 + 2 * k]; gy += gf[f * 6 + 2 * k + 1]; }
    }
    float* o = grad + e * 3;
    if (gx == 0.f && gy == 0.f) {                                  // in no face, or only in skipped ones (whatever its Z): exactly 0
        o[0] = o[1] = o[2] = 0.f;
        return;
    }
    const float* k = K + (bh >> 1) * 9;
    const float* p = verts + e * 3;
    const float iz = 1.f / p[2];
    // u = K00 X / Z + K02, v = K11 Y / Z + K12
    const float ux = gx * k[0] * iz, vy = gy * k[4] * iz;
    o[0] = ux;
    o[1] = vy;
    o[2] = -(ux * p[0] + vy * p[1]) * iz;
}

PDF_API int pdf_silhouette_loss(const float* verts, const long long* faces, const float* K, const float* mask, const float* weight,
                                const float* valid, const int* table, int B, int n, int Fc, int M, int H, int W, float sigma, float z_near,
                                float* scratch, float* loss, float* sums, float* trans, float* grad, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (B <= 0) return 0;
    if (n < 1 || n > HAND_MAXN || Fc < 1 || Fc > HAND_MAXF || H < 1 || H > SIL_MAXHW || W < 1 || W > SIL_MAXHW || M < 1 || M > SIL_MAXM || B > 65535)
        return PDF_E_BADARG;
    if (verts == nullptr || faces == nullptr || K == nullptr || mask == nullptr || scratch == nullptr || loss == nullptr || sums == nullptr ||
        trans == nullptr || !(sigma > 0.f) || !(z_near > 0.f) || !(sigma <= 3.0e38f))
        return PDF_E_BADARG;
    if (grad != nullptr && table == nullptr) return PDF_E_BADARG;
    const int tiles_x = cdiv(W, SIL_TILE), tiles_y = cdiv(H, SIL_TILE), tiles = tiles_x * tiles_y;
    const long total = (long)B * 2 * n, total_f = (long)B * 2 * Fc;
    // scratch: screen records | tile partials | coefficients | face gradients (every region a multiple of 16 bytes)
    float4* scr = reinterpret_cast<float4*>(scratch);
    double2* partial = reinterpret_cast<double2*>(scratch + total * 4);
    float* coef = scratch + total * 4 + (long)B * 2 * tiles * 4;
    float* gface = coef + (long)B * 4;
    const float inv_sigma = 1.f / sigma, rho = sqrtf(SIL_CUT * sigma);
    hipLaunchKernelGGL(sil_vertex_kernel, dim3(cdiv(total, SIL_T)), dim3(SIL_T), 0, s, verts, K, total, n, scr);
    PDF_LAUNCH_CHECK();
    hipLaunchKernelGGL(sil_tile_kernel, dim3(tiles_x, 2 * tiles_y, B), dim3(SIL_T), 0, s, faces, valid, mask, weight, scr, n, Fc, H, W, tiles_y,
                       inv_sigma, rho, z_near, trans, partial);
    PDF_LAUNCH_CHECK();
    hipLaunchKernelGGL(sil_finish_kernel, dim3(2 * B), dim3(SIL_T), 0, s, partial, valid, tiles, loss, sums, coef);
    PDF_LAUNCH_CHECK();
    if (grad == nullptr) return 0;
    hipLaunchKernelGGL(sil_face_grad_kernel, dim3(cdiv(total_f, SIL_T / 64)), dim3(SIL_T), 0, s, faces, valid, mask, weight, scr, trans, coef,
                       total_f, n, Fc, H, W, inv_sigma, rho, z_near, gface);
    PDF_LAUNCH_CHECK();
    hipLaunchKernelGGL(sil_vertex_grad_kernel, dim3(cdiv(total, SIL_T)), dim3(SIL_T), 0, s, verts, faces, K, table, gface, total, n, Fc, M, grad);
    PDF_LAUNCH_CHECK();
    return 0;
}
