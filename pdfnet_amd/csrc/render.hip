// Forward-only, z-buffered rasteriser of the two hand meshes of every sample under that sample's pinhole camera (pdf_render_hands), and the
// image-plane comparison of two renders and a sensor depth map (pdf_render_compare).  Counterpart of the reference's pytorch3d
// MeshRasterizer + HardPhongShader pair (lib/models/networks/mano_utils.py:44-156: blur_radius 0, one face per pixel, no back-face culling).
// Deterministic, no atomics: two runs are bit-identical.
//
// ARITHMETIC CONTRACT (fp32 throughout; tests/test_render_gpu.py restates it in float64)
//   Camera    at the origin, looking down +z: u = K00 X / Z + K02, v = K11 Y / Z + K12.  Pixel (i, j) = (row, column) is sampled at
//             (u, v) = (j + 0.5, i + 0.5): u = 0 is the left border of pixel 0 (the reference's build_camera: -c 2 / size + 1).
//   Faces     0 .. Fc-1 are the left hand's, Fc .. 2Fc-1 the right hand's (faces [2,Fc,3], indices into that hand's n vertices, clamped).
//   Skipped   whole: a face whose hand has valid == 0; a face with a vertex at Z < z_near (or not a number); a face whose screen area
//             A2 = (x1-x0)(y2-y0) - (x2-x0)(y1-y0) is exactly 0.  No back-face culling.
//   Coverage  the edge opposite vertex k runs between the other two vertices a, b; it is evaluated FROM the one with the lower vertex index
//             (o) TO the other (t):  E = (xt-xo)(py-yo) - (yt-yo)(px-xo), products rounded separately (no fma), negated when the face's
//             own direction a -> b is t -> o, and multiplied by sign(A2): w_k.  Two faces sharing an edge evaluate the same bits up to
//             sign, so a pixel exactly on the edge belongs to both and a pixel off it to exactly one: a closed mesh has no holes.
//             Covered: w0 >= 0, w1 >= 0, w2 >= 0 and w0 + w1 + w2 > 0.
//   Depth     1/Z is linear in screen space: with q = w0/Z0 + w1/Z1 + w2/Z2, depth = (w0 + w1 + w2) / q and the perspective-correct
//             barycentrics are bary_k = (w_k / Z_k) / q.  The smallest depth wins; on an exact tie the lower face index.
//   Outputs   face int32 [B,H,W] (-1 background), depth f32 [B,H,W] (0 background), bary f32 [B,H,W,3] (0), rgb f32 [B,H,W,3] (0).
//   Shading   pytorch3d's documented HardPhongShader defaults as Renderer.__init__ uses them: one point light at (0,0,-1), ambient 0.5,
//             diffuse 0.3, specular 0.2, material colours 1, shininess 64, viewer at the origin.  Vertex normal = sum over the incident
//             faces (in the order of the vertex -> face table) of (p1-p0) x (p2-p0), divided by max(|.|, 1e-6).  Per pixel, with bary:
//             p = position, n = normal / max(|normal|, 1e-6), c = colour; l = (light - p) / max(|.|, 1e-6), v = -p / max(|p|, 1e-6),
//             r = 2 (n.l) n - l;  rgb = (0.5 + 0.3 max(n.l, 0)) c + 0.2 max(r.v, 0)^64 [n.l > 0].  ambient_only: rgb = c (AmbientLights).
//
// DESIGN
//   render_vertex_kernel: one thread per (sample, hand, vertex) writes (x, y, 1/Z, Z) and, when rgb is asked for, the vertex normal, gathered
//   over the padded vertex -> face table [2][n][M] (-1 = none; the ELL idiom of graph.hip), into the caller's scratch (16 B n floats).
//   render_tile_kernel: grid (ceil(W/16), ceil(H/16), B), 256 threads = one 16 x 16 tile, one pixel per thread.  The 2 Fc faces are taken 256
//   at a time: thread t sets up face t (the rejections above, its bounding box against the tile's pixel centres); the survivors are compacted in
//   face order (64-bit __ballot + popcount prefix per wave, wave totals through LDS) into an LDS list of 64 B per face -- per edge
//   (xo, yo, +-(xt-xo), +-(yt-yo)), then (1/Z0, 1/Z1, 1/Z2, id) -- 16 KB.  After a barrier every pixel walks the list (each LDS read a 16-byte
//   broadcast) with its winner in registers; the epilogue writes face / depth / bary and shades.
//   render_compare_kernel: one block of 1,024 threads per sample, integer counts and a double sum per thread over a fixed pixel stride, reduced
//   by wave shuffles and a fixed-order finish in thread 0.
#include "mesh_geom.h"                                          // HAND_MAXN, HAND_MAXF, geo_det2, geo_index, geo_project

#define RND_T 256
#define RND_TILE 16
#define RND_MAXM 32
#define RND_MAXHW 2048
#define RND_CMP_T 1024

__global__ __launch_bounds__(RND_T) void render_vertex_kernel(const float* __restrict__ verts, const long long* __restrict__ faces,
                                                              const float* __restrict__ K, const int* __restrict__ table, long total, int n, int Fc,
                                                              int M, int normals, float4* __restrict__ scr, float4* __restrict__ nrm) {
    const long e = (long)blockIdx.x * RND_T + threadIdx.x;    // (b, h, i)
    if (e >= total) return;
    const long bh = e / n;
    const int i = (int)(e - bh * n), h = (int)(bh & 1);
    const float* p = verts + e * 3;
    scr[e] = geo_project(K + (bh >> 1) * 9, p[0], p[1], p[2]);
    if (!normals) return;
    const float* hv = verts + bh * n * 3;
    const long long* hf = faces + (long)h * Fc * 3;
    float nx = 0.f, ny = 0.f, nz = 0.f;
    for (int m = 0; m < M; ++m) {
        const int f = table[((long)h * n + i) * M + m];
        if (f < 0 || f >= Fc) continue;
        const float* a = hv + 3 * geo_index(hf + 3 * f, n);
        const float* b = hv + 3 * geo_index(hf + 3 * f + 1, n);
        const float* c = hv + 3 * geo_index(hf + 3 * f + 2, n);
        const float ux = b[0] - a[0], uy = b[1] - a[1], uz = b[2] - a[2], vx = c[0] - a[0], vy = c[1] - a[1], vz = c[2] - a[2];
        nx += uy * vz - uz * vy;
        ny += uz * vx - ux * vz;
        nz += ux * vy - uy * vx;
    }
    const float inv = 1.f / fmaxf(sqrtf(nx * nx + ny * ny + nz * nz), 1e-6f);
    nrm[e] = make_float4(nx * inv, ny * inv, nz * inv, 0.f);
}

__global__ __launch_bounds__(RND_T) void render_tile_kernel(const float* __restrict__ verts, const long long* __restrict__ faces,
                                                            const float* __restrict__ valid, const float* __restrict__ colour, long colour_stride,
                                                            const float4* __restrict__ scr, const float4* __restrict__ nrm, int n, int Fc, int H, int W,
                                                            float z_near, int ambient_only, int* __restrict__ face, float* __restrict__ depth,
                                                            float* __restrict__ bary, float* __restrict__ rgb) {
    __shared__ float4 list[RND_T * 4];
    __shared__ int wave_n[RND_T / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long b = blockIdx.z;
    const int tx0 = blockIdx.x * RND_TILE, ty0 = blockIdx.y * RND_TILE;
    const int col = tx0 + (t & (RND_TILE - 1)), row = ty0 + (t >> 4);
    const float px = (float)col + 0.5f, py = (float)row + 0.5f;
    // pixel centres of this tile, clipped to the image
    const float cx0 = (float)tx0 + 0.5f, cx1 = (float)min(tx0 + RND_TILE, W) - 0.5f, cy0 = (float)ty0 + 0.5f, cy1 = (float)min(ty0 + RND_TILE, H) - 0.5f;
    const bool ok_left = valid == nullptr || valid[b * 2] != 0.f, ok_right = valid == nullptr || valid[b * 2 + 1] != 0.f;
    float best = 3.0e38f, bq = 1.f, c0 = 0.f, c1 = 0.f, c2 = 0.f;
    int bid = -1;
    for (int base = 0; base < 2 * Fc; base += RND_T) {
        const int g = base + t;
        bool keep = false;
        float4 e0, e1, e2, zz;
        if (g < 2 * Fc) {
            const int h = g >= Fc;
            if (h ? ok_right : ok_left) {
                const long long* f = faces + (long)g * 3;          // [2][Fc][3]: row g
                const int idx[3] = {geo_index(f, n), geo_index(f + 1, n), geo_index(f + 2, n)};
                const float4* sv = scr + (b * 2 + h) * n;
                const float4 v[3] = {sv[idx[0]], sv[idx[1]], sv[idx[2]]};
                const float a2 = geo_det2(v[1].x - v[0].x, v[2].y - v[0].y, v[2].x - v[0].x, v[1].y - v[0].y);
                const bool front = v[0].w >= z_near && v[1].w >= z_near && v[2].w >= z_near;
                const float lox = fminf(fminf(v[0].x, v[1].x), v[2].x), hix = fmaxf(fmaxf(v[0].x, v[1].x), v[2].x);
                const float loy = fminf(fminf(v[0].y, v[1].y), v[2].y), hiy = fmaxf(fmaxf(v[0].y, v[1].y), v[2].y);
                keep = front && fabsf(a2) > 0.f && !(hix < cx0 || lox > cx1 || hiy < cy0 || loy > cy1);
                const float s = a2 > 0.f ? 1.f : -1.f;
                float4 e[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) {                      // the edge opposite vertex k: a -> b
                    const int a = (k + 1) % 3, bb = (k + 2) % 3;
                    const bool fwd = idx[a] < idx[bb];
                    const float4 o = fwd ? v[a] : v[bb], to = fwd ? v[bb] : v[a];
                    const float sg = fwd ? s : -s;
                    e[k] = make_float4(o.x, o.y, sg * (to.x - o.x), sg * (to.y - o.y));
                }
                e0 = e[0]; e1 = e[1]; e2 = e[2];
                zz = make_float4(v[0].z, v[1].z, v[2].z, __int_as_float(g));
            }
        }
        const unsigned long long mask = __ballot(keep);
        if (lane == 0) wave_n[wave] = __popcll(mask);
        __syncthreads();
        int off = __popcll(mask & ((1ULL << lane) - 1ULL)), count = 0;
#pragma unroll
        for (int w = 0; w < RND_T / 64; ++w) {
            const int c = wave_n[w];
            if (w < wave) off += c;
            count += c;
        }
        if (keep) {                                                // off < count <= RND_T
            list[off * 4 + 0] = e0; list[off * 4 + 1] = e1; list[off * 4 + 2] = e2; list[off * 4 + 3] = zz;
        }
        __syncthreads();
        for (int j = 0; j < count; ++j) {
            const float4 f0 = list[j * 4 + 0], f1 = list[j * 4 + 1], f2 = list[j * 4 + 2], fz = list[j * 4 + 3];
            const float w0 = geo_det2(f0.z, py - f0.y, f0.w, px - f0.x);
            const float w1 = geo_det2(f1.z, py - f1.y, f1.w, px - f1.x);
            const float w2 = geo_det2(f2.z, py - f2.y, f2.w, px - f2.x);
            const float ws = w0 + w1 + w2;
            if (w0 >= 0.f && w1 >= 0.f && w2 >= 0.f && ws > 0.f) {
                const float q0 = w0 * fz.x, q1 = w1 * fz.y, q2 = w2 * fz.z, q = q0 + q1 + q2;
                const float d = ws / q;
                if (d < best) { best = d; bq = q; c0 = q0; c1 = q1; c2 = q2; bid = __float_as_int(fz.w); }
            }
        }
        __syncthreads();                                           // the list is rewritten by the next chunk
    }
    if (col >= W || row >= H) return;
    const long pix = (b * H + row) * W + col;
    const bool hit = bid >= 0;
    const float b0 = hit ? c0 / bq : 0.f, b1 = hit ? c1 / bq : 0.f, b2 = hit ? c2 / bq : 0.f;
    face[pix] = bid;
    depth[pix] = hit ? best : 0.f;
    if (bary != nullptr) { bary[pix * 3] = b0; bary[pix * 3 + 1] = b1; bary[pix * 3 + 2] = b2; }
    if (rgb == nullptr) return;
    float r = 0.f, gr = 0.f, bl = 0.f;
    if (hit) {
        const int h = bid >= Fc;
        const long long* f = faces + (long)bid * 3;
        const int i0 = geo_index(f, n), i1 = geo_index(f + 1, n), i2 = geo_index(f + 2, n);
        const long vb = (b * 2 + h) * n;
        const float* cl = colour + b * colour_stride + (long)h * n * 3;
        r = b0 * cl[3 * i0] + b1 * cl[3 * i1] + b2 * cl[3 * i2];
        gr = b0 * cl[3 * i0 + 1] + b1 * cl[3 * i1 + 1] + b2 * cl[3 * i2 + 1];
        bl = b0 * cl[3 * i0 + 2] + b1 * cl[3 * i1 + 2] + b2 * cl[3 * i2 + 2];
        if (!ambient_only) {
            const float* p0 = verts + (vb + i0) * 3;
            const float* p1 = verts + (vb + i1) * 3;
            const float* p2 = verts + (vb + i2) * 3;
            const float4 n0 = nrm[vb + i0], n1 = nrm[vb + i1], n2 = nrm[vb + i2];
            const float X = b0 * p0[0] + b1 * p1[0] + b2 * p2[0], Y = b0 * p0[1] + b1 * p1[1] + b2 * p2[1], Z = b0 * p0[2] + b1 * p1[2] + b2 * p2[2];
            float nx = b0 * n0.x + b1 * n1.x + b2 * n2.x, ny = b0 * n0.y + b1 * n1.y + b2 * n2.y, nz = b0 * n0.z + b1 * n1.z + b2 * n2.z;
            const float ni = 1.f / fmaxf(sqrtf(nx * nx + ny * ny + nz * nz), 1e-6f);
            nx *= ni; ny *= ni; nz *= ni;
            float lx = -X, ly = -Y, lz = -1.f - Z;                 // to the light at (0, 0, -1)
            const float li = 1.f / fmaxf(sqrtf(lx * lx + ly * ly + lz * lz), 1e-6f);
            lx *= li; ly *= li; lz *= li;
            const float vi = 1.f / fmaxf(sqrtf(X * X + Y * Y + Z * Z), 1e-6f);      // to the viewer at the origin: -p / |p|
            const float ndl = nx * lx + ny * ly + nz * lz;
            const float rx = 2.f * ndl * nx - lx, ry = 2.f * ndl * ny - ly, rz = 2.f * ndl * nz - lz;
            float sp = fmaxf(-(rx * X + ry * Y + rz * Z) * vi, 0.f);
#pragma unroll
            for (int k = 0; k < 6; ++k) sp *= sp;                  // ^64
            const float shade = 0.5f + 0.3f * fmaxf(ndl, 0.f), spec = ndl > 0.f ? 0.2f * sp : 0.f;
            r = shade * r + spec; gr = shade * gr + spec; bl = shade * bl + spec;
        }
    }
    rgb[pix * 3] = r; rgb[pix * 3 + 1] = gr; rgb[pix * 3 + 2] = bl;
}

PDF_API int pdf_render_hands(const float* verts, const long long* faces, const float* K, const float* valid, const float* colour, int colour_per_sample,
                             const int* table, int B, int n, int Fc, int M, int H, int W, float z_near, int ambient_only, float* scratch,
                             int* face, float* depth, float* bary, float* rgb, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (B <= 0) return 0;
    if (n < 1 || n > HAND_MAXN || Fc < 1 || Fc > HAND_MAXF || H < 1 || H > RND_MAXHW || W < 1 || W > RND_MAXHW || M < 1 || M > RND_MAXM || B > 65535)
        return PDF_E_BADARG;
    if (verts == nullptr || faces == nullptr || K == nullptr || scratch == nullptr || face == nullptr || depth == nullptr || !(z_near > 0.f))
        return PDF_E_BADARG;
    if (rgb != nullptr && (colour == nullptr || (table == nullptr && !ambient_only))) return PDF_E_BADARG;
    const long total = (long)B * 2 * n;
    float4* scr = reinterpret_cast<float4*>(scratch);
    const int normals = rgb != nullptr && !ambient_only;
    hipLaunchKernelGGL(render_vertex_kernel, dim3(cdiv(total, RND_T)), dim3(RND_T), 0, s, verts, faces, K, table, total, n, Fc, M, normals, scr, scr + total);
    PDF_LAUNCH_CHECK();
    hipLaunchKernelGGL(render_tile_kernel, dim3(cdiv(W, RND_TILE), cdiv(H, RND_TILE), B), dim3(RND_T), 0, s, verts, faces, valid, colour,
                       colour_per_sample ? (long)2 * n * 3 : 0L, scr, scr + total, n, Fc, H, W, z_near, ambient_only, face, depth, bary, rgb);
    PDF_LAUNCH_CHECK();
    return 0;
}

// Two face maps (prediction, ground truth), the prediction's depth map and a sensor depth map -> per sample and hand (intersection, union) of
// the pixels where that hand is the visible surface, and (sum |rendered Z - sensor Z|, count) over the pixels with a predicted surface and
// sensor depth > 0.
__global__ __launch_bounds__(RND_CMP_T) void render_compare_kernel(const int* __restrict__ fp, const int* __restrict__ fg, const float* __restrict__ dp,
                                                                   const float* __restrict__ sensor, int HW, int Fc, int* __restrict__ iou,
                                                                   float* __restrict__ res) {
    __shared__ int red_i[RND_CMP_T / 64][5];
    __shared__ double red_d[RND_CMP_T / 64];
    const long o = (long)blockIdx.x * HW;
    int c[5] = {0, 0, 0, 0, 0};                                    // inter L, union L, inter R, union R, residual pixels
    double sum = 0.0;
    for (int i = threadIdx.x; i < HW; i += RND_CMP_T) {
        const int p = fp[o + i], g = fg[o + i];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const bool inp = p >= h * Fc && p < (h + 1) * Fc, ing = g >= h * Fc && g < (h + 1) * Fc;
            c[2 * h] += inp && ing;
            c[2 * h + 1] += inp || ing;
        }
        if (sensor != nullptr && p >= 0) {
            const float sd = sensor[o + i];
            if (sd > 0.f) { sum += (double)fabsf(dp[o + i] - sd); ++c[4]; }
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 5; ++k) c[k] = wave_sum_i(c[k]);
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) sum += __shfl_xor(sum, s, 64);
    if (lane == 0) {
        for (int k = 0; k < 5; ++k) red_i[wave][k] = c[k];
        red_d[wave] = sum;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < RND_CMP_T / 64; ++w) {
            for (int k = 0; k < 5; ++k) c[k] += red_i[w][k];
            sum += red_d[w];
        }
        for (int k = 0; k < 4; ++k) iou[blockIdx.x * 4 + k] = c[k];
        if (res != nullptr) { res[blockIdx.x * 2] = (float)sum; res[blockIdx.x * 2 + 1] = (float)c[4]; }
    }
}
PDF_API int pdf_render_compare(const int* face_pred, const int* face_gt, const float* depth_pred, const float* sensor, int B, int H, int W, int Fc,
                               int* iou, float* res, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (B <= 0) return 0;
    if (Fc < 1 || Fc > HAND_MAXF || H < 1 || H > RND_MAXHW || W < 1 || W > RND_MAXHW) return PDF_E_BADARG;
    if (face_pred == nullptr || face_gt == nullptr || iou == nullptr || (sensor != nullptr && (depth_pred == nullptr || res == nullptr))) return PDF_E_BADARG;
    hipLaunchKernelGGL(render_compare_kernel, dim3(B), dim3(RND_CMP_T), 0, s, face_pred, face_gt, depth_pred, sensor, H * W, Fc, iou, res);
    PDF_LAUNCH_CHECK();
    return 0;
}
