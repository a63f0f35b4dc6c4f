// MANO fit: Levenberg-Marquardt over p = [root 3 | pose 45 | shape 10 | trans 3] against a target mesh -- the contract is pdf_mano_fit's in
// pdfnet_hip.h.  One workgroup per sample stays resident for the whole loop: the model is mano_lbs_kernel's (center_idx = -1, trans given),
// the Jacobian is formed by forward-mode tangents and never leaves the CU.
//
// Phases of one iteration (512 threads, 8 waves):
//   forward   Rodrigues (16 threads) -> shaped vertices -> joints (wave reductions) and pose blend shapes -> the chain, level by level (root,
//             then the five fingers' first, second, third joints: 60 threads a level) -> skinning, residual, cost (double, fixed order).
//   tangents  dR_j / da_k (48 threads); d G_j / dq for the 48 rotation and 10 shape parameters, one thread per (q, row of G): a row of
//             G_j = G_parent o [R_j | (I - R_j) j_j] depends on the same row of the parent alone, so a thread walks its sub-tree in registers.
//             Stored sparsely: the root's parameters move all 16 transforms, a finger joint's only the (at most 3) joints from it to the tip,
//             a shape coefficient only the translations.
//   J tiles   16 vertices at a time: [48 rows][61 columns + the residual as column 61], scaled by sqrt(w_v), into LDS (it aliases A, which is
//             only written once the last tile is consumed); one (vertex, column) item per thread, 2 rounds.
//   products  A = J^T W J, g = J^T W r as the upper 4x4 register tiles of the 64 x 64 product of the tile with itself (136 tiles x 3 row slices
//             = 408 threads, two float4 LDS reads per 16 FMAs); fp32 inside a tile, double across tiles.
//   solve     (A + lambda diag(max(A_ii, 1e-12))) delta = -g: right-looking Cholesky in double of the system bordered by -g (which does the forward
//             substitution on the way), every entry in a register of the thread that owns it; the back substitution on one wave, a row per
//             lane, x_k passed on by a shuffle.
//   trial     forward at p + delta (it overwrites the posed vertices and the residual: after a rejection nothing reads them before the next
//             accepted trial has rewritten them, and A, g of the unchanged p are kept, so a rejection costs a solve and a forward only).
// LDS: A 16 KiB, posed vertices and residual 9.1 KiB each, max(tangents 13.8 KiB, Cholesky factor 15.3 KiB), 6 KiB of small tables: 56 KiB.
// No atomics: every sum has a fixed order, so two runs are bit-identical and a row does not depend on the rest of the batch.
#include "common.h"

namespace {

constexpr int NV = 778, NR = NV * 3, NP = 61, NT = 512, NW = NT / 64;
constexpr int TV = 16, TR = TV * 3, JLD = 68, NTILE = (NV + TV - 1) / TV;    // a J tile: 16 vertices, rows of 68 floats (16-byte aligned, few bank conflicts)
constexpr int UT = 136, KS = 3, KROWS = TR / KS;                               // upper 4x4 tiles of the 64 x 64 product; row slices of a tile
constexpr int NLB = NP * (NP + 1) / 2 + NP;                                  // lower triangle of the system bordered by its right-hand side
constexpr float LAMBDA0 = 1e-3f;

__device__ __constant__ int c_fit_parent[16] = {-1, 0, 1, 2, 0, 4, 5, 0, 7, 8, 0, 10, 11, 0, 13, 14};
__device__ __constant__ int c_fit_order[21] = {0, 13, 14, 15, 16, 1, 2, 3, 17, 4, 5, 6, 18, 10, 11, 12, 19, 7, 8, 9, 20};

struct FitConsts { const float *vt, *sd, *pd, *jr, *wt; };

struct FitTangents {
    float dR[48 * 9];             // d R_j / d a_k at [j * 3 + k]
    float dGroot[3 * 16 * 12];    // d G_j / d root_k
    float dGfing[45 * 3 * 12];    // d G_{i + s} / d a_k of finger joint i (1..15) at [(i - 1) * 3 + k][s], s = 0 .. joints to the tip
    float dts[10 * 16 * 3];       // d t_j / d shape_k (the rotations do not depend on the shape)
    float Tt[TV * 9], Wt[TV * 16], sw[TV];     // per vertex of the current tile: rotation part of its blended transform, skinning weights, sqrt(w_v)
};

struct FitLds {
    float A[64 * 64];             // normal equations, row 61 / column 61 = J^T W r; while they are summed: the J tile [TR][JLD]
    float vp[NR];                 // posed vertices before skinning
    float r[NR];                  // shaped vertices during a forward pass, then the residual
    union { double L[NLB]; FitTangents t; } u;
    float Rm[16 * 9], pf[135], loc[16 * 12], G[16 * 12], jt[48], JS[480];      // JS[j][c][k] = d j_j[c] / d shape_k (constant)
    float p[64], pt[64], gv[64], jun[63];
    double sd[64], red[NW], E, piv;                             // sd: reciprocals of the factor's diagonal
};

__device__ __forceinline__ int tri(int i) { return i * (i + 1) / 2; }

// R = I + sin(t) L + (1 - cos(t)) L^2, t = |a| + 1e-8, L = skew(a / t); 1 - cos(t) as 2 sin^2(t / 2), which keeps its relative accuracy at small angles
__device__ void fit_rodrigues(const float* a, float* R) {
    float x = a[0], y = a[1], z = a[2];
    const float th = sqrtf(x * x + y * y + z * z) + 1e-8f;
    x /= th; y /= th; z /= th;
    const float sn = sinf(th), h = sinf(0.5f * th), oc = 2.f * h * h;
    const float L[9] = {0.f, -z, y, z, 0.f, -x, -y, x, 0.f};
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            const float l2 = L[r * 3] * L[c] + L[r * 3 + 1] * L[3 + c] + L[r * 3 + 2] * L[6 + c];
            R[r * 3 + c] = (r == c ? 1.f : 0.f) + sn * L[r * 3 + c] + oc * l2;
        }
}

// d R / d a_k; the derivative of |a| at a = 0 is taken as 0 (mano_lbs_bwd_kernel's rule), which leaves dR = skew(e_k) there
__device__ void fit_rodrigues_d(const float* a, int k, float* dR) {
    const float nrm = sqrtf(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]), th = nrm + 1e-8f;
    const float n[3] = {a[0] / th, a[1] / th, a[2] / th};
    const float dth = nrm > 0.f ? a[k] / nrm : 0.f;
    float dn[3];
    for (int m = 0; m < 3; ++m) dn[m] = ((m == k ? 1.f : 0.f) - n[m] * dth) / th;
    const float sn = sinf(th), cs = cosf(th), h = sinf(0.5f * th), oc = 2.f * h * h;
    const float L[9] = {0.f, -n[2], n[1], n[2], 0.f, -n[0], -n[1], n[0], 0.f};
    const float D[9] = {0.f, -dn[2], dn[1], dn[2], 0.f, -dn[0], -dn[1], dn[0], 0.f};
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            float l2 = 0.f, m2 = 0.f;
            for (int m = 0; m < 3; ++m) { l2 += L[r * 3 + m] * L[m * 3 + c]; m2 += D[r * 3 + m] * L[m * 3 + c] + L[r * 3 + m] * D[m * 3 + c]; }
            dR[r * 3 + c] = cs * dth * L[r * 3 + c] + sn * D[r * 3 + c] + sn * dth * l2 + oc * m2;
        }
}

// The model at pv (an LDS vector of 61): leaves the posed vertices in s.vp, the residual M(pv) - target in s.r and
// E(pv) = sum_v w_v |r_v|^2 + prior_pose |pose|^2 + prior_shape |shape|^2 in s.E; with vout / jout also the mesh and its 21 joints.
__device__ void fit_forward(FitLds& s, const float* pv, const FitConsts& c, const float* __restrict__ tg, const float* __restrict__ wv,
                            float prior_pose, float prior_shape, int left_side, float* __restrict__ vout, float* __restrict__ jout) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < 16) fit_rodrigues(pv + tid * 3, s.Rm + tid * 9);
    for (int i = tid; i < NR; i += NT) {
        float a = c.vt[i];
        for (int k = 0; k < 10; ++k) a += c.sd[i * 10 + k] * pv[48 + k];
        s.r[i] = a;
    }
    __syncthreads();
    if (tid < 135) s.pf[tid] = s.Rm[9 + tid] - ((tid % 9) % 4 == 0 ? 1.f : 0.f);
    for (int o = wave; o < 48; o += NW) {                       // j_tpose = J_regressor @ v_shaped
        const int j = o / 3, cc = o % 3;
        float a = 0.f;
        for (int v = lane; v < NV; v += 64) a += c.jr[j * NV + v] * s.r[v * 3 + cc];
        a = wave_sum(a);
        if (lane == 0) s.jt[o] = a;
    }
    __syncthreads();
    if (tid < 192) {                                            // loc_j = [R_j | (I - R_j) j_j]
        const int j = tid / 12, e = tid % 12, r = e / 4, cc = e % 4;
        float a;
        if (cc < 3) a = s.Rm[j * 9 + r * 3 + cc];
        else {
            a = 0.f;
            for (int m = 0; m < 3; ++m) a += ((r == m ? 1.f : 0.f) - s.Rm[j * 9 + r * 3 + m]) * s.jt[j * 3 + m];
        }
        s.loc[tid] = a;
    }
    for (int i0 = wave * 8; i0 < NR; i0 += NW * 8) {            // pose blend shapes: 8 lanes share a row of posedirs, so a load touches 8 short runs
        const int i = i0 + (lane >> 3), sub = lane & 7;
        float a = 0.f;
        if (i < NR) {
            const float* pd = c.pd + (long)i * 135;
            for (int k = sub; k < 135; k += 8) a += pd[k] * s.pf[k];
        }
        a += __shfl_xor(a, 1, 64); a += __shfl_xor(a, 2, 64); a += __shfl_xor(a, 4, 64);
        if (sub == 0 && i < NR) s.vp[i] = s.r[i] + a;
    }
    __syncthreads();
    if (tid < 12) s.G[tid] = s.loc[tid];
    for (int lev = 1; lev <= 3; ++lev) {                        // the five fingers' joints of one depth at a time
        __syncthreads();
        if (tid < 60) {
            const int j = 1 + 3 * (tid / 12) + (lev - 1), e = tid % 12, r = e / 4, cc = e % 4, p = lev == 1 ? 0 : j - 1;
            float a = s.G[p * 12 + r * 4] * s.loc[j * 12 + cc] + s.G[p * 12 + r * 4 + 1] * s.loc[j * 12 + 4 + cc] + s.G[p * 12 + r * 4 + 2] * s.loc[j * 12 + 8 + cc];
            if (cc == 3) a += s.G[p * 12 + r * 4 + 3];
            s.G[j * 12 + e] = a;
        }
    }
    __syncthreads();
    const float t0 = pv[58], t1 = pv[59], t2 = pv[60];
    if (jout != nullptr && tid < 16) {
        const int p = c_fit_parent[tid];
        for (int r = 0; r < 3; ++r) {
            float a;
            if (p < 0) a = s.jt[r];
            else a = s.G[p * 12 + r * 4] * s.jt[tid * 3] + s.G[p * 12 + r * 4 + 1] * s.jt[tid * 3 + 1] + s.G[p * 12 + r * 4 + 2] * s.jt[tid * 3 + 2] + s.G[p * 12 + r * 4 + 3];
            s.jun[tid * 3 + r] = a + pv[58 + r];
        }
    }
    double e = 0.0;
    for (int v = tid; v < NV; v += NT) {
        float T[12];
        for (int k = 0; k < 12; ++k) T[k] = 0.f;
        for (int j = 0; j < 16; ++j) {
            const float w = c.wt[v * 16 + j];
            if (w != 0.f) for (int k = 0; k < 12; ++k) T[k] += w * s.G[j * 12 + k];
        }
        const float x = s.vp[v * 3], y = s.vp[v * 3 + 1], z = s.vp[v * 3 + 2];
        const float ox = T[0] * x + T[1] * y + T[2] * z + T[3] + t0;
        const float oy = T[4] * x + T[5] * y + T[6] * z + T[7] + t1;
        const float oz = T[8] * x + T[9] * y + T[10] * z + T[11] + t2;
        const float rx = ox - tg[v * 3], ry = oy - tg[v * 3 + 1], rz = oz - tg[v * 3 + 2];
        s.r[v * 3] = rx; s.r[v * 3 + 1] = ry; s.r[v * 3 + 2] = rz;
        const double w = wv != nullptr ? (double)fmaxf(wv[v], 0.f) : 1.0;
        e += w * ((double)rx * rx + (double)ry * ry + (double)rz * rz);
        if (vout != nullptr) { vout[v * 3] = ox; vout[v * 3 + 1] = oy; vout[v * 3 + 2] = oz; }
        if (jout != nullptr) {
            int tip = -1;
            if (v == 745) tip = 0; else if (v == 317) tip = 1; else if (v == (left_side ? 445 : 444)) tip = 2;
            else if (v == 556) tip = 3; else if (v == 673) tip = 4;
            if (tip >= 0) { s.jun[(16 + tip) * 3] = ox; s.jun[(16 + tip) * 3 + 1] = oy; s.jun[(16 + tip) * 3 + 2] = oz; }
        }
    }
    e = wave_sum_d(e);
    if (lane == 0) s.red[wave] = e;
    __syncthreads();
    if (tid == 0) {
        double a = 0.0, pp = 0.0, ps = 0.0;
        for (int w = 0; w < NW; ++w) a += s.red[w];
        for (int k = 3; k < 48; ++k) pp += (double)pv[k] * pv[k];
        for (int k = 48; k < 58; ++k) ps += (double)pv[k] * pv[k];
        s.E = a + (double)prior_pose * pp + (double)prior_shape * ps;
    }
    if (jout != nullptr && tid < 63) jout[tid] = s.jun[c_fit_order[tid / 3] * 3 + tid % 3];
    __syncthreads();
}

// A = J^T W J + diag(prior) into s.A (61 x 61 of the 64 x 64, both triangles), g = J^T W r + prior o p into s.gv, from s.vp, s.r and the
// transforms the forward pass at s.p left behind.  Overwrites the tangent tables (the union with the Cholesky factor).
__device__ void fit_build(FitLds& s, const FitConsts& c, const float* __restrict__ wv, float prior_pose, float prior_shape, int ti, int tj, int ks) {
    const int tid = threadIdx.x;
    FitTangents& t = s.u.t;
    if (tid < 48) fit_rodrigues_d(s.p + (tid / 3) * 3, tid % 3, t.dR + tid * 9);
    __syncthreads();
    if (tid < 144) {                                            // rotation parameter q = joint * 3 + axis, row r of the transforms below it
        const int q = tid / 3, r = tid % 3, i = q / 3;
        const float* dR = t.dR + q * 9;
        float dloc[12];                                         // d loc_i = [dR | -dR j_i]
        for (int m = 0; m < 3; ++m) {
            for (int cc = 0; cc < 3; ++cc) dloc[m * 4 + cc] = dR[m * 3 + cc];
            dloc[m * 4 + 3] = -(dR[m * 3] * s.jt[i * 3] + dR[m * 3 + 1] * s.jt[i * 3 + 1] + dR[m * 3 + 2] * s.jt[i * 3 + 2]);
        }
        float row0[4], row[4];
        if (i == 0) {
            for (int cc = 0; cc < 3; ++cc) row0[cc] = dR[r * 3 + cc];
            row0[3] = -(dR[r * 3] * s.jt[0] + dR[r * 3 + 1] * s.jt[1] + dR[r * 3 + 2] * s.jt[2]);
            for (int cc = 0; cc < 4; ++cc) { row[cc] = row0[cc]; t.dGroot[(q * 16) * 12 + r * 4 + cc] = row0[cc]; }
            for (int j = 1; j < 16; ++j) {
                const float* lj = s.loc + j * 12;
                const bool top = c_fit_parent[j] == 0;
                const float p0 = top ? row0[0] : row[0], p1 = top ? row0[1] : row[1], p2 = top ? row0[2] : row[2], p3 = top ? row0[3] : row[3];
                for (int cc = 0; cc < 4; ++cc) row[cc] = p0 * lj[cc] + p1 * lj[4 + cc] + p2 * lj[8 + cc];
                row[3] += p3;
                for (int cc = 0; cc < 4; ++cc) t.dGroot[(q * 16 + j) * 12 + r * 4 + cc] = row[cc];
            }
        } else {
            const int p = c_fit_parent[i], last = ((i - 1) / 3) * 3 + 3;
            for (int cc = 0; cc < 4; ++cc) {
                row[cc] = s.G[p * 12 + r * 4] * dloc[cc] + s.G[p * 12 + r * 4 + 1] * dloc[4 + cc] + s.G[p * 12 + r * 4 + 2] * dloc[8 + cc];
                t.dGfing[((q - 3) * 3) * 12 + r * 4 + cc] = row[cc];
            }
            for (int j = i + 1; j <= last; ++j) {
                const float* lj = s.loc + j * 12;
                float nw[4];
                for (int cc = 0; cc < 4; ++cc) nw[cc] = row[0] * lj[cc] + row[1] * lj[4 + cc] + row[2] * lj[8 + cc];
                nw[3] += row[3];
                for (int cc = 0; cc < 4; ++cc) { row[cc] = nw[cc]; t.dGfing[((q - 3) * 3 + (j - i)) * 12 + r * 4 + cc] = nw[cc]; }
            }
        }
    } else if (tid < 174) {                                     // shape coefficient k, row r: d t_j = A_parent (I - R_j) d j_j + d t_parent
        const int k = (tid - 144) / 3, r = (tid - 144) % 3;
        float d0 = 0.f, dprev = 0.f;
        for (int j = 0; j < 16; ++j) {
            float dc[3];
            for (int m = 0; m < 3; ++m) {
                float a = 0.f;
                for (int n = 0; n < 3; ++n) a += ((m == n ? 1.f : 0.f) - s.Rm[j * 9 + m * 3 + n]) * s.JS[(j * 3 + n) * 10 + k];
                dc[m] = a;
            }
            float d;
            if (j == 0) d = d0 = dc[r];
            else {
                const int p = c_fit_parent[j];
                d = s.G[p * 12 + r * 4] * dc[0] + s.G[p * 12 + r * 4 + 1] * dc[1] + s.G[p * 12 + r * 4 + 2] * dc[2] + (p == 0 ? d0 : dprev);
            }
            dprev = d;
            t.dts[(k * 16 + j) * 3 + r] = d;
        }
    }
    double tot[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) tot[e] = 0.0;
    float* Js = s.A;
    for (int tile = 0; tile < NTILE; ++tile) {
        const int v0 = tile * TV;
        if (tid < 256) { const int v = v0 + tid / 16; t.Wt[tid] = v < NV ? c.wt[v * 16 + tid % 16] : 0.f; }
        else if (tid < 256 + 144) {
            const int vl = (tid - 256) / 9, e = (tid - 256) % 9, v = v0 + vl, ge = (e / 3) * 4 + e % 3;
            float a = 0.f;
            if (v < NV) for (int j = 0; j < 16; ++j) { const float w = c.wt[v * 16 + j]; if (w != 0.f) a += w * s.G[j * 12 + ge]; }
            t.Tt[vl * 9 + e] = a;
        } else if (tid < 256 + 144 + TV) {
            const int v = v0 + tid - 400;
            t.sw[tid - 400] = v < NV ? (wv != nullptr ? sqrtf(fmaxf(wv[v], 0.f)) : 1.f) : 0.f;
        }
        __syncthreads();                                        // also: the previous tile's products are done with Js
        for (int rnd = 0; rnd < 2; ++rnd) {
            const int id = tid + rnd * NT, vl = id & 15, q = id >> 4, v = v0 + vl;      // 4 columns x 16 vertices a wave: a wave of one vertex and 64 columns runs every column kind's branch in turn and measured 1.5x slower
            float d0 = 0.f, d1 = 0.f, d2 = 0.f;
            if (v < NV) {
                const float x = s.vp[v * 3], y = s.vp[v * 3 + 1], z = s.vp[v * 3 + 2];
                const float* W = t.Wt + vl * 16;
                const float* T = t.Tt + vl * 9;
                float dv0 = 0.f, dv1 = 0.f, dv2 = 0.f;         // d (posed vertex) / dq, still to be rotated by the vertex's transform
                if (q < 48) {
                    const int i = q / 3;
                    const int j0 = i == 0 ? 0 : i, j1 = i == 0 ? 15 : ((i - 1) / 3) * 3 + 3;
                    const float* base = i == 0 ? t.dGroot + (q * 16) * 12 : t.dGfing + ((q - 3) * 3) * 12;
                    for (int j = j0; j <= j1; ++j) {
                        const float w = W[j];
                        if (w != 0.f) {
                            const float* D = base + (j - j0) * 12;
                            d0 += w * (D[0] * x + D[1] * y + D[2] * z + D[3]);
                            d1 += w * (D[4] * x + D[5] * y + D[6] * z + D[7]);
                            d2 += w * (D[8] * x + D[9] * y + D[10] * z + D[11]);
                        }
                    }
                    if (i > 0) {                                // pose blend shapes: the 9 columns of joint i
                        const float* dR = t.dR + q * 9;
                        const float* pd = c.pd + (long)(v * 3) * 135 + (i - 1) * 9;
                        for (int e = 0; e < 9; ++e) { dv0 += pd[e] * dR[e]; dv1 += pd[135 + e] * dR[e]; dv2 += pd[270 + e] * dR[e]; }
                    }
                } else if (q < 58) {
                    const int k = q - 48;
                    for (int j = 0; j < 16; ++j) {
                        const float w = W[j];
                        if (w != 0.f) { d0 += w * t.dts[(k * 16 + j) * 3]; d1 += w * t.dts[(k * 16 + j) * 3 + 1]; d2 += w * t.dts[(k * 16 + j) * 3 + 2]; }
                    }
                    dv0 = c.sd[(v * 3) * 10 + k]; dv1 = c.sd[(v * 3 + 1) * 10 + k]; dv2 = c.sd[(v * 3 + 2) * 10 + k];
                } else if (q < 61) {
                    d0 = q == 58 ? 1.f : 0.f; d1 = q == 59 ? 1.f : 0.f; d2 = q == 60 ? 1.f : 0.f;
                } else if (q == 61) {
                    d0 = s.r[v * 3]; d1 = s.r[v * 3 + 1]; d2 = s.r[v * 3 + 2];
                }
                if (q < 58) {
                    d0 += T[0] * dv0 + T[1] * dv1 + T[2] * dv2;
                    d1 += T[3] * dv0 + T[4] * dv1 + T[5] * dv2;
                    d2 += T[6] * dv0 + T[7] * dv1 + T[8] * dv2;
                }
                const float sw = t.sw[vl];
                d0 *= sw; d1 *= sw; d2 *= sw;
            }
            Js[(vl * 3) * JLD + q] = d0; Js[(vl * 3 + 1) * JLD + q] = d1; Js[(vl * 3 + 2) * JLD + q] = d2;
        }
        __syncthreads();
        if (tid < UT * KS) {
            float acc[16];
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[e] = 0.f;
            const float* row = Js + (ks * KROWS) * JLD;
#pragma unroll 4
            for (int kk = 0; kk < KROWS; ++kk, row += JLD) {
                const float4 a = *reinterpret_cast<const float4*>(row + 4 * ti);
                const float4 b = *reinterpret_cast<const float4*>(row + 4 * tj);
                acc[0] += a.x * b.x; acc[1] += a.x * b.y; acc[2] += a.x * b.z; acc[3] += a.x * b.w;
                acc[4] += a.y * b.x; acc[5] += a.y * b.y; acc[6] += a.y * b.z; acc[7] += a.y * b.w;
                acc[8] += a.z * b.x; acc[9] += a.z * b.y; acc[10] += a.z * b.z; acc[11] += a.z * b.w;
                acc[12] += a.w * b.x; acc[13] += a.w * b.y; acc[14] += a.w * b.z; acc[15] += a.w * b.w;
            }
#pragma unroll
            for (int e = 0; e < 16; ++e) tot[e] += (double)acc[e];
        }
    }
    for (int sl = 0; sl < KS; ++sl) {                           // the three row slices, added in a fixed order
        __syncthreads();
        if (tid < UT * KS && ks == sl) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int i = 4 * ti + e / 4, j = 4 * tj + e % 4;
                const float val = (float)tot[e];
                if (sl == 0) { s.A[i * 64 + j] = val; if (ti != tj) s.A[j * 64 + i] = val; }
                else { s.A[i * 64 + j] += val; if (ti != tj) s.A[j * 64 + i] += val; }
            }
        }
    }
    __syncthreads();
    if (tid < NP) {
        const float pr = tid >= 3 && tid < 48 ? prior_pose : (tid >= 48 && tid < 58 ? prior_shape : 0.f);
        s.A[tid * 65] += pr;
        s.gv[tid] = s.A[tid * 64 + 61] + pr * s.p[tid];
    }
    __syncthreads();
}

// (A + lambda diag(max(A_ii, 1e-12))) delta = -g; s.pt = s.p + delta.  Returns 0 when a pivot is not positive.
// Right-looking Cholesky of the system bordered by the right-hand side (row 61 = -g, so that row of the factor is y with L y = -g): every thread
// owns up to 4 fixed entries of the 1952 and keeps them in registers for all 61 steps; a step publishes the pivot, then the finished column
// (which is also where the factor is kept for the back substitution), then every entry right of it takes its rank-one update: two barriers and
// a handful of LDS reads per step.  L^T x = y runs on one wave, row i on lane i, x_k passed on by a shuffle, the pivots' reciprocals kept.
__device__ int fit_solve(FitLds& s, float lambda) {
    const int tid = threadIdx.x, lane = tid & 63;
    double* L = s.u.L;
    int ei[4], ej[4];
    double a[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        const int e = tid + n * NT;
        int i = (int)((sqrtf(8.f * e + 1.f) - 1.f) * 0.5f);
        while (tri(i + 1) <= e) ++i;
        while (tri(i) > e) --i;
        const int j = e - tri(i);
        ei[n] = e < NLB ? i : -1; ej[n] = j;
        a[n] = 0.0;
        if (e < NLB) {
            if (i == NP) a[n] = -(double)s.gv[j];
            else if (i == j) a[n] = (double)s.A[i * 65] + (double)lambda * (double)fmaxf(s.A[i * 65], 1e-12f);
            else a[n] = (double)s.A[i * 64 + j];
        }
    }
    int ok = 1;
    for (int k = 0; k < NP; ++k) {
#pragma unroll
        for (int n = 0; n < 4; ++n) if (ei[n] == k && ej[n] == k) s.piv = a[n];
        __syncthreads();
        const double d = s.piv;                                 // every thread reads the same pivot: the branch is uniform
        if (!(d > 0.0)) { ok = 0; break; }
        const double sq = sqrt(d), rinv = 1.0 / sq;
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            if (ej[n] == k && ei[n] > k) { a[n] *= rinv; L[tri(ei[n]) + k] = a[n]; }
            else if (ej[n] == k && ei[n] == k) { L[tri(k) + k] = sq; s.sd[k] = rinv; }
        }
        __syncthreads();
#pragma unroll
        for (int n = 0; n < 4; ++n) if (ei[n] >= 0 && ej[n] > k) a[n] -= L[tri(ei[n]) + k] * L[tri(ej[n]) + k];
    }
    __syncthreads();
    if (ok && tid < 64) {                                       // L^T x = y: lane i owns row i
        double b = lane < NP ? L[tri(NP) + lane] : 0.0;
        for (int k = NP - 1; k >= 0; --k) {
            if (lane == k) b *= s.sd[k];
            const double xk = __shfl(b, k, 64);
            if (lane < k) b -= L[tri(k) + lane] * xk;
        }
        s.pt[lane] = lane < NP ? s.p[lane] + (float)b : 0.f;
    }
    __syncthreads();
    return ok;
}

__global__ __launch_bounds__(NT) void mano_fit_kernel(
    const float* __restrict__ target, const float* __restrict__ valid, const float* __restrict__ weight, const float* __restrict__ init,
    FitConsts c, int left_side, int iters, float prior_pose, float prior_shape,
    float* __restrict__ params, float* __restrict__ verts, float* __restrict__ joints, float* __restrict__ cost, int* __restrict__ info,
    float* __restrict__ lambda_out, float* __restrict__ Aout, float* __restrict__ gout) {
    __shared__ __attribute__((aligned(16))) FitLds s;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* tg = target + (long)b * NR;
    const float* wv = weight != nullptr ? weight + (long)b * NV : nullptr;
    float* vout = verts + (long)b * NR;
    float* jout = joints + (long)b * 63;
    if (tid < 64) s.p[tid] = init != nullptr && tid < NP ? init[b * NP + tid] : 0.f;
    __syncthreads();
    if (init == nullptr && wave < 3) {                          // trans = mean(target) - mean(v_template)
        double a = 0.0;
        for (int v = lane; v < NV; v += 64) a += (double)tg[v * 3 + wave] - (double)c.vt[v * 3 + wave];
        a = wave_sum_d(a);
        if (lane == 0) s.p[58 + wave] = (float)(a / NV);
    }
    __syncthreads();
    if (valid != nullptr && valid[b] == 0.f) {                  // no step: the start point and its mesh, zero costs
        fit_forward(s, s.p, c, tg, wv, prior_pose, prior_shape, left_side, vout, jout);
        if (tid < NP) params[b * NP + tid] = s.p[tid];
        if (tid < 2) { cost[b * 2 + tid] = 0.f; info[b * 2 + tid] = 0; }
        if (tid == 0) lambda_out[b] = LAMBDA0;
        if (Aout != nullptr) for (int i = tid; i < NP * NP; i += NT) Aout[(long)b * NP * NP + i] = 0.f;
        if (gout != nullptr && tid < NP) gout[b * NP + tid] = 0.f;
        return;
    }
    for (int o = wave; o < 480; o += NW) {                      // d j_tpose / d shape = J_regressor @ shapedirs
        const int j = o / 30, cc = (o / 10) % 3, k = o % 10;
        float a = 0.f;
        for (int v = lane; v < NV; v += 64) a += c.jr[j * NV + v] * c.sd[(v * 3 + cc) * 10 + k];
        a = wave_sum(a);
        if (lane == 0) s.JS[o] = a;
    }
    int ti = 0, tj = 0, ks = 0;                                 // this thread's tile of the upper triangle and its row slice
    if (tid < UT * KS) {
        ks = tid / UT;
        int rest = tid % UT;
        while (rest >= 16 - ti) { rest -= 16 - ti; ++ti; }
        tj = ti + rest;
    }
    fit_forward(s, s.p, c, tg, wv, prior_pose, prior_shape, left_side, nullptr, nullptr);
    const double E0 = s.E;
    double E = E0;
    float lambda = LAMBDA0;
    int accepted = 0, rejected = 0, build = 1;
    for (int it = 0; it < iters; ++it) {
        if (build) fit_build(s, c, wv, prior_pose, prior_shape, ti, tj, ks);
        build = 0;
        int ok = fit_solve(s, lambda);
        if (ok) {
            fit_forward(s, s.pt, c, tg, wv, prior_pose, prior_shape, left_side, nullptr, nullptr);
            ok = s.E < E;
        }
        if (ok) {
            E = s.E;
            if (tid < 64) s.p[tid] = s.pt[tid];
            lambda = fmaxf(lambda * 0.25f, 1e-7f);
            ++accepted; build = 1;
        } else {
            lambda = fminf(lambda * 8.f, 1e6f);
            ++rejected;
        }
        __syncthreads();
    }
    if (iters == 0 && (Aout != nullptr || gout != nullptr)) fit_build(s, c, wv, prior_pose, prior_shape, ti, tj, ks);
    if (Aout != nullptr) for (int i = tid; i < NP * NP; i += NT) Aout[(long)b * NP * NP + i] = s.A[(i / NP) * 64 + i % NP];
    if (gout != nullptr && tid < NP) gout[b * NP + tid] = s.gv[tid];
    fit_forward(s, s.p, c, tg, wv, prior_pose, prior_shape, left_side, vout, jout);
    if (tid < NP) params[b * NP + tid] = s.p[tid];
    if (tid == 0) {
        cost[b * 2] = (float)E0; cost[b * 2 + 1] = (float)E;
        info[b * 2] = accepted; info[b * 2 + 1] = rejected;
        lambda_out[b] = lambda;
    }
}

}  // namespace

PDF_API long pdf_mano_fit_workspace_floats(int B) {
    (void)B;
    return 0;                                                   // J is streamed through LDS in tiles; nothing is spilled
}

PDF_API int pdf_mano_fit(const float* target, const float* valid, const float* weight, const float* init,
                         const float* v_template, const float* shapedirs, const float* posedirs, const float* J_reg, const float* weights,
                         int B, int left_side, int iters, float prior_pose, float prior_shape,
                         float* params, float* verts, float* joints, float* cost, int* info, float* lambda, float* A, float* g,
                         float* workspace, void* stream) {
    (void)workspace;
    if (B <= 0) return 0;
    if (target == nullptr || v_template == nullptr || shapedirs == nullptr || posedirs == nullptr || J_reg == nullptr || weights == nullptr ||
        params == nullptr || verts == nullptr || joints == nullptr || cost == nullptr || info == nullptr || lambda == nullptr)
        return PDF_E_BADARG;
    if (iters < 0 || iters > 1000 || !(prior_pose >= 0.f && prior_pose <= 3.0e38f) || !(prior_shape >= 0.f && prior_shape <= 3.0e38f)) return PDF_E_BADARG;
    const FitConsts c = {v_template, shapedirs, posedirs, J_reg, weights};
    hipLaunchKernelGGL(mano_fit_kernel, dim3(B), dim3(NT), 0, (hipStream_t)stream, target, valid, weight, init, c, left_side, iters,
                       prior_pose, prior_shape, params, verts, joints, cost, info, lambda, A, g);
    PDF_LAUNCH_CHECK();
    return 0;
}

// ---- MANO fit against the sensor cloud (contract: pdf_mano_fit_cloud in pdfnet_hip.h) -----------------------------------------------------
// The loop is host code: mano_cloud_targets_kernel (icp.hip) turns the association at the current mesh into per-vertex targets and weights,
// mano_fit_kernel -- launched as pdf_mano_fit launches it -- takes `inner` steps against them.  The parameters alternate between `params` and
// the workspace, started on the side that makes the last launch write `params`; every per-iteration output is a contiguous slice.
namespace {
constexpr long FC_TARGET = NR, FC_WEIGHT = NV, FC_PARAMS = NP, FC_SMALL = 5;      // per row: lambda, the start launch's cost [2] and info [2]
}

PDF_API long pdf_mano_fit_cloud_workspace_floats(int B, int outer) {
    (void)outer;
    return B > 0 ? (long)B * (FC_TARGET + FC_WEIGHT + FC_PARAMS + FC_SMALL) : 0;
}

PDF_API int pdf_mano_fit_cloud(const float* cloud, const long long* faces, const float* valid, const float* init, const float* anchor,
                               float anchor_weight, float trim, int outer, int inner, float prior_pose, float prior_shape,
                               const float* v_template, const float* shapedirs, const float* posedirs, const float* J_reg, const float* weights,
                               int B, int Fc, int P, int left_side,
                               float* params, float* verts, float* joints, float* rms, int* inliers, float* cost, int* info,
                               float* workspace, void* stream) {
    if (B <= 0) return 0;
    if (cloud == nullptr || faces == nullptr || init == nullptr || v_template == nullptr || shapedirs == nullptr || posedirs == nullptr ||
        J_reg == nullptr || weights == nullptr || params == nullptr || verts == nullptr || joints == nullptr || rms == nullptr ||
        inliers == nullptr || workspace == nullptr || (outer > 0 && (cost == nullptr || info == nullptr)))
        return PDF_E_BADARG;
    if (outer < 0 || outer > 64 || inner < 1 || inner > 1000 || Fc < 1 || Fc > 2048 || P < 1 || P > 1024 || !(trim > 0.f) || !(trim <= 3.0e38f) ||
        !(anchor_weight >= 0.f && anchor_weight <= 3.0e38f) || !(prior_pose >= 0.f && prior_pose <= 3.0e38f) ||
        !(prior_shape >= 0.f && prior_shape <= 3.0e38f))
        return PDF_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    float* target = workspace;
    float* weight = target + (long)B * FC_TARGET;
    float* other = weight + (long)B * FC_WEIGHT;
    float* lambda = other + (long)B * FC_PARAMS;
    float* cost0 = lambda + B;
    int* info0 = reinterpret_cast<int*>(cost0 + 2L * B);
    float* pp[2] = {params, other};
    int cur = outer & 1;                                        // after `outer` swaps the parameters are in `params`
    { hipError_t e = hipMemsetAsync(target, 0, sizeof(float) * (size_t)B * FC_TARGET, s); if (e != hipSuccess) return (int)e; }
    int rc = pdf_mano_fit(target, valid, nullptr, init, v_template, shapedirs, posedirs, J_reg, weights, B, left_side, 0, prior_pose, prior_shape,
                          pp[cur], verts, joints, cost0, info0, lambda, nullptr, nullptr, nullptr, stream);
    for (int o = 0; o <= outer && rc == 0; ++o) {
        rc = pdf_mano_cloud_targets(verts, faces, cloud, valid, anchor, anchor_weight, B, NV, Fc, P, trim, target, weight, rms + (long)o * B,
                                    inliers + (long)o * B, nullptr, nullptr, nullptr, stream);
        if (rc != 0 || o == outer) break;
        rc = pdf_mano_fit(target, valid, weight, pp[cur], v_template, shapedirs, posedirs, J_reg, weights, B, left_side, inner, prior_pose,
                          prior_shape, pp[cur ^ 1], verts, joints, cost + (long)o * B * 2, info + (long)o * B * 2, lambda, nullptr, nullptr,
                          nullptr, stream);
        cur ^= 1;
    }
    return rc;
}
