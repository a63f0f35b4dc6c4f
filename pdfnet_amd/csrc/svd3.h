// 3x3 singular value decomposition in one lane, shared by the aligned metrics (metrics.hip) and the ICP refinement (icp.hip).
#pragma once
#include "common.h"

// M = U S V^T by one-sided Jacobi (Hestenes) rotations of the columns of G = M V, which converge to U S with V the accumulated rotations.
// u[c] / v[c]: COLUMN c of U / V, sg descending.  A singular direction whose sigma is below 1e-12 of the largest gets its left vector from the
// orthogonal complement of the others instead of from rounding noise, so U stays orthogonal for any rank.  Returns false, with sg alone
// written, when no sigma is positive (M = 0, also a NaN input).  g: workspace.  A caller short of registers hands in LDS arrays.
__device__ __forceinline__ bool met_svd_3x3(const double M[3][3], double g[3][3] /* g[c]: COLUMN c of G */, double u[3][3], double v[3][3],
                                            double sg[3]) {
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
    if (!(sg[0] > 0.0)) return false;
    const double tiny = 1e-12 * sg[0];
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
    return true;
}

// Orthogonal Procrustes of a 3x3 matrix: returns tr S and R = U V^T, WITHOUT a determinant correction (scipy's orthogonal_procrustes: a
// mirrored prediction aligns exactly).  R is orthogonal for any rank; rank 0: R = I.
__device__ inline double met_procrustes_3x3(const double M[3][3], double R[3][3]) {
    double g[3][3], u[3][3], v[3][3], sg[3];
    const bool ok = met_svd_3x3(M, g, u, v, sg);
    const double trace = sg[0] + sg[1] + sg[2];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) R[r][c] = ok ? u[0][r] * v[0][c] + u[1][r] * v[1][c] + u[2][r] * v[2][c] : (r == c ? 1.0 : 0.0);
    return trace;
}
