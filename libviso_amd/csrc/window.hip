// window.hip — the opt-in sliding-window bundle adjustment over feature tracks (include/viso_hip.h, "window refinement";
// DESIGN.md 5.10).  Not in the reference.  Two kernels:
//   - window_links_kernel, one workgroup per frame: L' (the usable inliers, in the list's order) and the frame's two uniqueness
//     tables (the row by cur-left, the row by prev-left; -1 none, -2 more than one), cleared by the workgroup itself and filled
//     with integer compare-and-swap (the outcome does not depend on the order of the writers);
//   - window_refine_kernel, one workgroup per frame t: the anchor, the window's tracks in a fixed order (s ascending, then L'_{s+1}'s
//     order; an ordered compaction), and the whole Levenberg-Marquardt loop.  The camera block (6 (len - 1) <= 24 square) is
//     assembled chunk by chunk: CH threads each write one track's rows into an LDS slot (the camera Jacobian rows J~c, W~ = l^-1 Hcp'
//     and the track's share of s), then the threads sum 3 x 3 tiles of S (with diag Hcc) and of s over the chunk in track order,
//     each tile in a fixed number of interleaved partials (wn_pass_a); the damped S is factored in LDS column by column.
// The order of every sum depends on the window's inputs only: the batch at any chunking and the direct call give byte-identical
// records.  fp64 throughout; no scratch memory (-Rpass-analysis=kernel-resource-usage, tests/test_window_cpu.py).  The motions'
// rotations (RotLite: w_0 = (1, 0, 0), w_1 = (0, cx, sx), w_2 = (sy, w21, w22)), the LM schedule (LM_*) and the covariance write-out
// (write_cov6) are solver_dev.h's, shared with refine.hip.
#include "solver_dev.h"

#include <math.h>
#include <string.h>
#include <vector>

#define WN_THREADS 256
#define WN_WAVES (WN_THREADS / 64)
#define WN_KMAX 5
#define WN_NCMAX (6 * (WN_KMAX - 1))
#define WN_SLOTS 5632            // doubles of LDS for the chunk's track slots (44 KiB)
#define WN_CHMAX 64
#define WN_EMAX (WN_NCMAX * (WN_NCMAX + 1) / 2 + 2 * WN_NCMAX)   // S upper | s | diag Hcc
#define WN_SS 24                 // row stride of the LDS camera matrix

struct WinArgs {
    WinData d;
    WinWork w;
    SolverParamsDev sp;
    int K, mode, t0, n_items;
    double sigma2;
    viso_window_record* out;   // [n_items]
};

__device__ __forceinline__ int wn_slot_size(int len) { return (3 * (len - 1) + 4) * (6 * (len - 1)) + 30; }
__device__ __forceinline__ int wn_chunk(int len) { const int c = WN_SLOTS / wn_slot_size(len); return c < WN_CHMAX ? c : WN_CHMAX; }
__device__ __forceinline__ int wn_tri(int j) { return j * (j + 1) / 2; }   // A[j][i] at wn_tri(j) + i, 9 doubles each

// ---- links ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void wn_insert(int* T, int tab, int p, int r) {
    if (p < 0 || p >= tab) return;   // a key outside the table cannot link
    const int old = atomicCAS(T + p, -1, r);
    if (old != -1) atomicExch(T + p, -2);
}

__global__ __launch_bounds__(WN_THREADS) void window_links_kernel(WinData d, WinWork w, int j0, int n) {
    __shared__ int wcnt[WN_WAVES];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if ((int)blockIdx.x >= n) return;
    const int j = j0 + (int)blockIdx.x;
    const int ld = d.ld;
    int m = d.m[j];
    m = m < 0 ? 0 : m > ld ? ld : m;
    int n_inl = d.n_inl[j];
    n_inl = n_inl < 0 ? 0 : n_inl > m ? m : n_inl;
    const double* X = d.X + (size_t)j * 3 * ld;
    const int* inl = d.inl + (size_t)j * ld;
    int* Lp = w.Lp + (size_t)j * ld;
    int nl = 0;
    for (int i0 = 0; i0 < n_inl; i0 += WN_THREADS) {
        const int i = i0 + tid;
        bool good = false;
        int k = 0;
        if (i < n_inl) {
            k = inl[i];
            if (k >= 0 && k < m) {
                const double x = X[k], y = X[ld + k], z = X[2 * ld + k];
                good = isfinite(x) && isfinite(y) && isfinite(z) && z > 0.0;
            }
        }
        const unsigned long long bal = __ballot(good);
        if (lane == 0) wcnt[wave] = __popcll(bal);
        __syncthreads();
        int off = nl, all = 0;
#pragma unroll
        for (int v = 0; v < WN_WAVES; ++v) { off += v < wave ? wcnt[v] : 0; all += wcnt[v]; }
        if (good) Lp[off + __popcll(bal & ((1ull << lane) - 1ull))] = k;
        nl += all;
        __syncthreads();
    }
    if (tid == 0) w.nLp[j] = nl;
    int* T = w.tabs + (size_t)j * 2 * d.tab;
    for (int i = tid; i < 2 * d.tab; i += WN_THREADS) T[i] = -1;
    __threadfence();
    __syncthreads();
    const int* left = d.left + (size_t)j * d.left_fs;
    for (int i = tid; i < nl; i += WN_THREADS) {
        const int r = Lp[i];
        wn_insert(T, d.tab, left[(size_t)r * d.lstride], r);
        wn_insert(T + d.tab, d.tab, left[(size_t)r * d.lstride + d.lprev], r);
    }
}

// The row of L'_{j-1} that row r of L'_j links to, or -1 (tables of frames j - 1 and j).
__device__ __forceinline__ int wn_back(const WinData& d, const WinWork& w, int j, int r) {
    const int p = d.left[(size_t)j * d.left_fs + (size_t)r * d.lstride + d.lprev];
    if (p < 0 || p >= d.tab) return -1;
    if (w.tabs[((size_t)j * 2 + 1) * d.tab + p] != r) return -1;
    const int q = w.tabs[((size_t)(j - 1) * 2) * d.tab + p];
    return q >= 0 ? q : -1;
}
// The row of L'_{j+1} that links to row r of L'_j, or -1.
__device__ __forceinline__ int wn_fwd(const WinData& d, const WinWork& w, int j, int r) {
    const int p = d.left[(size_t)j * d.left_fs + (size_t)r * d.lstride];
    if (p < 0 || p >= d.tab) return -1;
    if (w.tabs[((size_t)j * 2) * d.tab + p] != r) return -1;
    const int q = w.tabs[((size_t)(j + 1) * 2 + 1) * d.tab + p];
    return q >= 0 ? q : -1;
}

// ---- one track -----------------------------------------------------------------------------------------------------------------
// z0 of a track: pi_0 of Xp_c[F][:, r] (triangulate_rectified inverted), as the motion refinement's rf_obs.
__device__ __forceinline__ void wn_z0(const WinData& d, const SolverParamsDev& sp, int F, int r, double (&z0)[3]) {
    const double* X = d.X + (size_t)F * 3 * d.ld;
    const double x = X[r], y = X[d.ld + r], z = X[2 * d.ld + r];
    const double g = sp.f / z;
    z0[0] = g * x + sp.cu;
    z0[1] = g * y + sp.cv;
    z0[2] = g * (x - sp.base) + sp.cu;
}

// The track's share of the cost with the motions rl[0 .. len-2] (frame offset i + 1) and the point (px, py, pz).
// trk: the item's track table [5][T] (s | e << 4, then the rows r_{s+1} .. r_e).
__device__ __forceinline__ double wn_cost(const WinArgs& a, const int* trk, size_t T, const RotLite* rl, int anc, int k, double px, double py, double pz) {
    const SolverParamsDev& sp = a.sp;
    const int se = trk[k];
    const int so = se & 15, eo = se >> 4;
    const int ld = a.d.ld;
    double Y0 = px, Y1 = py, Y2 = pz, c = 0.0;
    for (int j = 0; j <= eo; ++j) {
        if (j > 0) {
            const RotLite& R = rl[j - 1];
            const double q0 = R.r00 * Y0 + R.r01 * Y1 + R.r02 * Y2, q1 = R.r10 * Y0 + R.r11 * Y1 + R.r12 * Y2;
            const double q2 = R.r20 * Y0 + R.r21 * Y1 + R.r22 * Y2;
            Y0 = q0 + R.tx; Y1 = q1 + R.ty; Y2 = q2 + R.tz;
        }
        if (j == so) {
            double z0[3];
            wn_z0(a.d, sp, anc + so + 1, trk[T + k], z0);
            const double g = sp.f / Y2;
            const double r0 = z0[0] - (g * Y0 + sp.cu), r1 = z0[1] - (g * Y1 + sp.cv), r2 = z0[2] - (g * (Y0 - sp.base) + sp.cu);
            c += r0 * r0 + r1 * r1 + r2 * r2;
        } else if (j > so) {
            const int r = trk[(size_t)(j - so) * T + k];
            const double* ob = a.d.obs + (size_t)(anc + j) * 4 * ld;
            const double fz = sp.f / Y2;
            const double u = ob[r] - (fz * Y0 + sp.cu), v = ob[ld + r] - (fz * Y1 + sp.cv);
            const double rr = ob[2 * ld + r] - (fz * (Y0 - sp.base) + sp.cu), ww = ob[3 * ld + r] - (fz * Y1 + sp.cv);
            c += u * u + v * v + rr * rr + ww * ww;
        }
    }
    return c;
}

// One group of a track's rows at frame offset j: Pj the 3 x 3 projection Jacobian w.r.t. Y_j (rows uL, vL or sqrt 2 vL, uR), r the
// three (merged) residuals.  Jx = Pj A[j][0] enters Hpp, gp (and hx when the rows depend on the cameras); the camera rows
// Pj A[j][i] D_i (i <= j; D_i = [w_k x q_i | I]) go to U's rows `row`.., and Hcp' and the track's share of s are accumulated in Wt, g.
__device__ __forceinline__ void wn_group(const double (&Pj)[3][3], const double (&r)[3], int j, bool camdep, int nc, const double* Am,
                                         const RotLite* rl, const double* Qv, double* U, double* Wt, double* g, int& row,
                                         double (&h)[6], double (&gp)[3], double (&hx)[6]) {
    const double* A0 = Am + 9 * wn_tri(j);
    double Jx[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int c = 0; c < 3; ++c) Jx[a][c] = Pj[a][0] * A0[c] + Pj[a][1] * A0[3 + c] + Pj[a][2] * A0[6 + c];
    double hh[6];
    hh[0] = Jx[0][0] * Jx[0][0] + Jx[1][0] * Jx[1][0] + Jx[2][0] * Jx[2][0];
    hh[1] = Jx[0][0] * Jx[0][1] + Jx[1][0] * Jx[1][1] + Jx[2][0] * Jx[2][1];
    hh[2] = Jx[0][0] * Jx[0][2] + Jx[1][0] * Jx[1][2] + Jx[2][0] * Jx[2][2];
    hh[3] = Jx[0][1] * Jx[0][1] + Jx[1][1] * Jx[1][1] + Jx[2][1] * Jx[2][1];
    hh[4] = Jx[0][1] * Jx[0][2] + Jx[1][1] * Jx[1][2] + Jx[2][1] * Jx[2][2];
    hh[5] = Jx[0][2] * Jx[0][2] + Jx[1][2] * Jx[1][2] + Jx[2][2] * Jx[2][2];
#pragma unroll
    for (int e = 0; e < 6; ++e) { h[e] += hh[e]; hx[e] += camdep ? hh[e] : 0.0; }   // no branch: a select of the
                                                                                    // destination would put h, hx in scratch
#pragma unroll
    for (int c = 0; c < 3; ++c) gp[c] += Jx[0][c] * r[0] + Jx[1][c] * r[1] + Jx[2][c] * r[2];
    if (!camdep) return;
    const int ncam = nc / 6;
    for (int i = 1; i <= ncam; ++i) {
        double J[3][6];
        if (i <= j) {
            const double* Ai = Am + 9 * (wn_tri(j) + i);
            double M3[3][3];
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int c = 0; c < 3; ++c) M3[a][c] = Pj[a][0] * Ai[c] + Pj[a][1] * Ai[3 + c] + Pj[a][2] * Ai[6 + c];
            const RotLite& R = rl[i - 1];
            const double q0 = Qv[3 * i], q1 = Qv[3 * i + 1], q2 = Qv[3 * i + 2];
            // w_k x q: w_0 = (1, 0, 0), w_1 = (0, cx, sx), w_2 = (sy, w21, w22)
            const double d0[3] = {0.0, -q2, q1};
            const double d1[3] = {R.cx * q2 - R.sx * q1, R.sx * q0, -R.cx * q0};
            const double d2[3] = {R.w21 * q2 - R.w22 * q1, R.w22 * q0 - R.sy * q2, R.sy * q1 - R.w21 * q0};
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                J[a][0] = M3[a][0] * d0[0] + M3[a][1] * d0[1] + M3[a][2] * d0[2];
                J[a][1] = M3[a][0] * d1[0] + M3[a][1] * d1[1] + M3[a][2] * d1[2];
                J[a][2] = M3[a][0] * d2[0] + M3[a][1] * d2[1] + M3[a][2] * d2[2];
                J[a][3] = M3[a][0]; J[a][4] = M3[a][1]; J[a][5] = M3[a][2];
            }
        } else {
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int c = 0; c < 6; ++c) J[a][c] = 0.0;
        }
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            const int col = 6 * (i - 1) + c;
            U[(row + 0) * nc + col] = J[0][c];
            U[(row + 1) * nc + col] = J[1][c];
            U[(row + 2) * nc + col] = J[2][c];
#pragma unroll
            for (int e = 0; e < 3; ++e) Wt[e * nc + col] += J[0][c] * Jx[0][e] + J[1][c] * Jx[1][e] + J[2][c] * Jx[2][e];
            g[col] += J[0][c] * r[0] + J[1][c] * r[1] + J[2][c] * r[2];
        }
    }
    row += 3;
}

// Track k at the current state (rl[0], Am) with damping lam: fills the slot (U rows, Wt = W~ = l^-1 Hcp', g = the track's share
// of s) and *nU; STEP: also dX = l^-T (y - W~ dtr).  Returns false when a pivot of Hpp_d or (s = a) of I - M'M fails the test.
template <bool STEP>
__device__ __forceinline__ bool wn_point(const WinArgs& a, const int* trk, size_t T, int anc, int nc, int k, double px, double py, double pz,
                         const RotLite* rl, const double* Am, double lam, double* slot, int* nU, const double* dtr, double (&dX)[3]) {
    const SolverParamsDev& sp = a.sp;
    const double f = sp.f, b = sp.base, RT2 = 1.4142135623730951;
    const int ld = a.d.ld;
    const int se = trk[k];
    const int so = se & 15, eo = se >> 4;
    const int nUmax = 3 * (nc / 6);
    double* U = slot;
    double* Wt = slot + nUmax * nc;
    double* g = Wt + 3 * nc;
    double* Yv = g + nc;        // Y_j [5][3]
    double* Qv = Yv + 15;       // q_j = R_j Y_{j-1} [5][3]
    for (int c = 0; c < 4 * nc; ++c) Wt[c] = 0.0;   // Wt and g
    Yv[0] = px; Yv[1] = py; Yv[2] = pz;
    for (int j = 1; j <= eo; ++j) {
        const RotLite& R = rl[j - 1];
        const double y0 = Yv[3 * j - 3], y1 = Yv[3 * j - 2], y2 = Yv[3 * j - 1];
        const double q0 = R.r00 * y0 + R.r01 * y1 + R.r02 * y2, q1 = R.r10 * y0 + R.r11 * y1 + R.r12 * y2;
        const double q2 = R.r20 * y0 + R.r21 * y1 + R.r22 * y2;
        Qv[3 * j] = q0; Qv[3 * j + 1] = q1; Qv[3 * j + 2] = q2;
        Yv[3 * j] = q0 + R.tx; Yv[3 * j + 1] = q1 + R.ty; Yv[3 * j + 2] = q2 + R.tz;
    }
    double h[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, hx[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, gp[3] = {0.0, 0.0, 0.0};
    int row = 0;
    {   // frame s: pi_0(Y_s) against z0
        double z0[3];
        wn_z0(a.d, sp, anc + so + 1, trk[T + k], z0);
        const double X = Yv[3 * so], Y = Yv[3 * so + 1], Z = Yv[3 * so + 2];
        const double iz = 1.0 / Z, gz = f * iz, gz2 = gz * iz;
        const double Pj[3][3] = {{gz, 0.0, -gz2 * X}, {0.0, gz, -gz2 * Y}, {gz, 0.0, -gz2 * (X - b)}};
        const double r[3] = {z0[0] - (gz * X + sp.cu), z0[1] - (gz * Y + sp.cv), z0[2] - (gz * (X - b) + sp.cu)};
        wn_group(Pj, r, so, so > 0, nc, Am, rl, Qv, U, Wt, g, row, h, gp, hx);
    }
    for (int j = so + 1; j <= eo; ++j) {   // frames s+1 .. e: compute_J's prediction, the v rows merged
        const int rr = trk[(size_t)(j - so) * T + k];
        const double* ob = a.d.obs + (size_t)(anc + j) * 4 * ld;
        const double X = Yv[3 * j], Y = Yv[3 * j + 1], Z = Yv[3 * j + 2];
        const double iz = 1.0 / Z, fz = f * iz, fz2 = fz * iz;
        const double r1u = ob[rr] - (fz * X + sp.cu), r1v = ob[ld + rr] - (fz * Y + sp.cv);
        const double r1r = ob[2 * ld + rr] - (fz * (X - b) + sp.cu), r1w = ob[3 * ld + rr] - (fz * Y + sp.cv);
        const double Pj[3][3] = {{fz, 0.0, -fz2 * X}, {0.0, RT2 * fz, RT2 * (-fz2 * Y)}, {fz, 0.0, -fz2 * (X - b)}};
        const double r[3] = {r1u, (r1v + r1w) * (1.0 / RT2), r1r};
        wn_group(Pj, r, j, true, nc, Am, rl, Qv, U, Wt, g, row, h, gp, hx);
    }
    *nU = row;
    h[0] *= 1.0 + lam; h[3] *= 1.0 + lam; h[5] *= 1.0 + lam;
    // l = chol(Hpp_d), packed l00, l10, l11, l20, l21, l22
    bool good = h[0] > 1e-12 * h[0];
    const double l0 = sqrt(h[0]), il0 = 1.0 / l0;
    const double l1 = h[1] * il0, l3 = h[2] * il0;
    const double s11 = h[3] - l1 * l1;
    good = good && s11 > 1e-12 * h[3];
    const double l2 = sqrt(s11), il1 = 1.0 / l2;
    const double l4 = (h[4] - l3 * l1) * il1;
    const double s22 = h[5] - l3 * l3 - l4 * l4;
    good = good && s22 > 1e-12 * h[5];
    const double l5 = sqrt(s22), il2 = 1.0 / l5;
    auto fwd3 = [&](double a0, double a1, double a2, double (&o)[3]) {
        o[0] = a0 * il0;
        o[1] = (a1 - l1 * o[0]) * il1;
        o[2] = (a2 - l3 * o[0] - l4 * o[1]) * il2;
    };
    if (so == 0) {   // I - M'M, M'M = l^-1 hx l^-T
        double B0[3], B1[3], B2[3], C0[3], C1[3], C2[3];
        fwd3(hx[0], hx[1], hx[2], B0);   // l^-1 hx (columns)
        fwd3(hx[1], hx[3], hx[4], B1);
        fwd3(hx[2], hx[4], hx[5], B2);
        fwd3(B0[0], B1[0], B2[0], C0);   // l^-1 (l^-1 hx)' (columns): M'M
        fwd3(B0[1], B1[1], B2[1], C1);
        fwd3(B0[2], B1[2], B2[2], C2);
        const double Q00 = 1.0 - C0[0], Q10 = -C0[1], Q20 = -C0[2], Q11 = 1.0 - C1[1], Q21 = -C1[2], Q22 = 1.0 - C2[2];
        good = good && Q00 > 1e-12 * Q00;
        const double G0 = sqrt(Q00), iG0 = 1.0 / G0;
        const double G1 = Q10 * iG0, G3 = Q20 * iG0;
        const double t11 = Q11 - G1 * G1;
        good = good && t11 > 1e-12 * Q11;
        const double G2 = sqrt(t11), iG2 = 1.0 / G2;
        const double G4 = (Q21 - G3 * G1) * iG2;
        const double t22 = Q22 - G3 * G3 - G4 * G4;
        good = good && t22 > 1e-12 * Q22;
    }
    double y[3];
    fwd3(gp[0], gp[1], gp[2], y);
    double v0 = y[0], v1 = y[1], v2 = y[2];
    for (int p = 0; p < nc; ++p) {
        double w[3];
        fwd3(Wt[p], Wt[nc + p], Wt[2 * nc + p], w);
        Wt[p] = w[0]; Wt[nc + p] = w[1]; Wt[2 * nc + p] = w[2];
        g[p] -= w[0] * y[0] + w[1] * y[1] + w[2] * y[2];
        if (STEP) { v0 -= w[0] * dtr[p]; v1 -= w[1] * dtr[p]; v2 -= w[2] * dtr[p]; }
    }
    if (STEP) {   // l' dX = v
        dX[2] = v2 * il2;
        dX[1] = (v1 - l4 * dX[2]) * il1;
        dX[0] = (v0 - l1 * dX[1] - l3 * dX[2]) * il0;
    }
    return good;
}

// ---- the block -----------------------------------------------------------------------------------------------------------------
// Workgroup sum of one value per thread (DPP rows, then the waves in a fixed order); every thread returns the total.
__device__ __forceinline__ double wn_reduce(double v, double* red) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    v = wave_sum_to_lane63(v);
    __syncthreads();
    if (lane == 63) red[wave] = v;
    __syncthreads();
    double s = red[0];
#pragma unroll
    for (int w = 1; w < WN_WAVES; ++w) s += red[w];
    return s;
}

// Motions and chain products of a state: rl[i] for the cameras 1..len-1 (thread i - 1) and A[j][i] = R_j ... R_{i+1} (thread 0).
__device__ __forceinline__ void wn_state(const double* trv, int len, RotLite* rl, double* Am) {
    const int tid = threadIdx.x;
    __syncthreads();
    if (tid < len - 1) rot_lite(trv + 6 * tid, rl[tid]);
    __syncthreads();
    if (Am && tid == 0) {
        for (int j = 0; j < len; ++j) {
            double* Ajj = Am + 9 * (wn_tri(j) + j);
#pragma unroll
            for (int e = 0; e < 9; ++e) Ajj[e] = (e % 4 == 0) ? 1.0 : 0.0;
            for (int i = j - 1; i >= 0; --i) {   // A[j][i] = A[j][i+1] R_{i+1}
                const double* P = Am + 9 * (wn_tri(j) + i + 1);
                const RotLite& R = rl[i];
                const double Rm[9] = {R.r00, R.r01, R.r02, R.r10, R.r11, R.r12, R.r20, R.r21, R.r22};
                double* O = Am + 9 * (wn_tri(j) + i);
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int c = 0; c < 3; ++c) O[3 * r + c] = P[3 * r] * Rm[c] + P[3 * r + 1] * Rm[3 + c] + P[3 * r + 2] * Rm[6 + c];
            }
        }
    }
    __syncthreads();
}

__device__ __forceinline__ void wn_zero(viso_window_record* o, const double* tr_t, const double* trw, int nw, int status, int len, int np, int nrows) {
    static_assert(sizeof(viso_window_record) == 584, "viso_window_record layout");
    double* dd = reinterpret_cast<double*>(o);   // tr | cov | tr_win | sigma2 | cost0 | cost | gap: 70 contiguous doubles
    for (int i = threadIdx.x; i < 70; i += WN_THREADS)
        dd[i] = i < 6 ? tr_t[i] : (i >= 42 && i < 42 + nw) ? trw[i - 42] : 0.0;
    if (threadIdx.x == 0) { o->iters = 0; o->status = status; o->len = len; o->n_points = np; o->n_rows = nrows; o->_pad = 0; }
}

// Pass A: the reduced camera system at the current state with damping lam into ent[] (S upper | s | diag Hcc); returns false when
// a track failed a pivot test.  Uniform.  The sums are tiled: with nb = nc / 3, a tile is a 3 x 3 block (bp <= bq) of S (plus the
// U-only diagonal on the diagonal blocks) or a 3-vector of s; each tile's sum over the chunk's tracks is split into PP interleaved
// partials (track kk of the chunk to partial kk % PP), one thread each, and the partials are added in order at the end.  Nine or
// three independent accumulators per thread and one load of six U words per row: the chains are short and overlap.
__device__ __forceinline__ bool wn_pass_a(const WinArgs& a, const int* trk, size_t T, const double* P, int anc, int len, int np, const RotLite* rl,
                          const double* Am, double lam, double* slots, int* nUr, double* ent, int* bad) {
    const int tid = threadIdx.x;
    const int nc = 6 * (len - 1), nS = nc * (nc + 1) / 2, nb = nc / 3;
    const int nSt = nb * (nb + 1) / 2, nT = nSt + nb;   // S tiles | s tiles
    const int PP = WN_THREADS / nT;                     // >= 5 (nT <= 44 at nc = 24)
    const int SL = wn_slot_size(len), CH = wn_chunk(len);
    const int UW = 3 * (nc / 6) * nc;                   // doubles of U rows in a slot: W~ follows
    const bool act = tid < nT * PP;
    const int tile = act ? tid / PP : 0, part = act ? tid % PP : 0;
    int bp = 0, bq = 0;
    if (tile < nSt) {
        int q = tile;
        while (q >= nb - bp) { q -= nb - bp; ++bp; }
        bq = q + bp;
    } else {
        bp = tile - nSt;
    }
    const int p0 = 3 * bp, q0 = 3 * bq;
    double acc[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, hd[3] = {0.0, 0.0, 0.0};
    if (tid == 0) *bad = 0;
    const double zero[1] = {0.0};
    for (int j0 = 0; j0 < np; j0 += CH) {
        __syncthreads();   // the slots are free
        const int k = j0 + tid;
        if (tid < CH && k < np) {
            double dX[3];
            if (!wn_point<false>(a, trk, T, anc, nc, k, P[k], P[T + k], P[2 * T + k], rl, Am, lam, slots + (size_t)tid * SL, nUr + tid,
                                 zero, dX))
                *bad = 1;
        }
        __syncthreads();
        const int nk = np - j0 < CH ? np - j0 : CH;
        if (!act) continue;
        for (int kk = part; kk < nk; kk += PP) {
            const double* U = slots + (size_t)kk * SL;
            const double* Wt = U + UW;
            if (tile < nSt) {
                const int nu = nUr[kk];
                for (int r = 0; r < nu; ++r) {
                    const double u0 = U[r * nc + p0], u1 = U[r * nc + p0 + 1], u2 = U[r * nc + p0 + 2];
                    const double v0 = U[r * nc + q0], v1 = U[r * nc + q0 + 1], v2 = U[r * nc + q0 + 2];
                    acc[0] += u0 * v0; acc[1] += u0 * v1; acc[2] += u0 * v2;
                    acc[3] += u1 * v0; acc[4] += u1 * v1; acc[5] += u1 * v2;
                    acc[6] += u2 * v0; acc[7] += u2 * v1; acc[8] += u2 * v2;
                    hd[0] += u0 * u0; hd[1] += u1 * u1; hd[2] += u2 * u2;
                }
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const double u0 = Wt[c * nc + p0], u1 = Wt[c * nc + p0 + 1], u2 = Wt[c * nc + p0 + 2];
                    const double v0 = Wt[c * nc + q0], v1 = Wt[c * nc + q0 + 1], v2 = Wt[c * nc + q0 + 2];
                    acc[0] -= u0 * v0; acc[1] -= u0 * v1; acc[2] -= u0 * v2;
                    acc[3] -= u1 * v0; acc[4] -= u1 * v1; acc[5] -= u1 * v2;
                    acc[6] -= u2 * v0; acc[7] -= u2 * v1; acc[8] -= u2 * v2;
                }
            } else {
                const double* g = Wt + 3 * nc;
                acc[0] += g[p0]; acc[1] += g[p0 + 1]; acc[2] += g[p0 + 2];
            }
        }
    }
    __syncthreads();   // the slots hold the partials from here: [tile][part][12]
    if (act) {
        double* o = slots + ((size_t)tile * PP + part) * 12;
#pragma unroll
        for (int e = 0; e < 9; ++e) o[e] = acc[e];
#pragma unroll
        for (int e = 0; e < 3; ++e) o[9 + e] = hd[e];
    }
    __syncthreads();
    for (int x = tid; x < nT * 12; x += WN_THREADS) {
        const int tl = x / 12, e = x % 12;
        int tp = 0, tq = 0;
        if (tl < nSt) {
            int q = tl;
            while (q >= nb - tp) { q -= nb - tp; ++tp; }
            tq = q + tp;
        } else {
            tp = tl - nSt;
        }
        int dst = -1;
        if (tl < nSt && e < 9) {
            const int p = 3 * tp + e / 3, q = 3 * tq + e % 3;
            if (p <= q) dst = p * nc - p * (p - 1) / 2 + (q - p);
        } else if (tl < nSt) {
            if (tp == tq) dst = nS + nc + 3 * tp + (e - 9);
        } else if (e < 3) {
            dst = nS + 3 * tp + e;
        }
        if (dst < 0) continue;
        const double* src = slots + (size_t)tl * PP * 12 + e;
        double v = src[0];
        for (int pp = 1; pp < PP; ++pp) v += src[pp * 12];
        ent[dst] = v;
    }
    __syncthreads();
    return *bad == 0;
}

// Cholesky of the damped camera block (Sm, row stride WN_SS, the full symmetric matrix) in place: the lower triangle becomes L, id
// the reciprocals of its diagonal.  False when a pivot is not > 1e-12 x its diagonal entry.  Uniform.
__device__ __forceinline__ bool wn_chol(double* Sm, double* id, const double* dgd, int nc) {
    const int tid = threadIdx.x;
    bool good = true;
    for (int j = 0; j < nc; ++j) {
        __syncthreads();
        const double s = Sm[j * WN_SS + j];
        good = good && s > 1e-12 * dgd[j];
        if (!good) break;
        const double l = sqrt(s), il = 1.0 / l;
        __syncthreads();
        if (tid > j && tid < nc) Sm[tid * WN_SS + j] *= il;
        if (tid == 0) { Sm[j * WN_SS + j] = l; id[j] = il; }
        __syncthreads();
        const int nn = nc - j - 1;
        for (int e = tid; e < nn * nn; e += WN_THREADS) {
            const int i = j + 1 + e / nn, k = j + 1 + e % nn;
            if (k <= i) Sm[i * WN_SS + k] -= Sm[i * WN_SS + j] * Sm[k * WN_SS + j];
        }
    }
    __syncthreads();
    return good;
}

// ent -> the damped S (full) in Sm and its damped diagonal in dgd; false when a sum is not finite.  Uniform.
__device__ __forceinline__ bool wn_build(const double* ent, int nc, double lam, double* Sm, double* dgd) {
    const int tid = threadIdx.x, nS = nc * (nc + 1) / 2;
    bool fin = true;
    for (int e = 0; e < nS + 2 * nc; ++e) fin = fin && isfinite(ent[e]);
    __syncthreads();
    for (int e = tid; e < nS; e += WN_THREADS) {
        int p = 0, q = e;
        while (q >= nc - p) { q -= nc - p; ++p; }
        q += p;
        const double v = p == q ? ent[e] + lam * ent[nS + nc + p] : ent[e];
        Sm[p * WN_SS + q] = v;
        Sm[q * WN_SS + p] = v;
        if (p == q) dgd[p] = v;
    }
    __syncthreads();
    return fin;
}

__global__ __launch_bounds__(WN_THREADS) void window_refine_kernel(WinArgs a) {
    __shared__ double slots[WN_SLOTS];
    __shared__ int nUr[WN_CHMAX];
    __shared__ double ent[WN_EMAX];
    __shared__ double Sm[WN_NCMAX * WN_SS];
    __shared__ double dgd[WN_NCMAX], Lid[WN_NCMAX], dtr[WN_NCMAX], trc[WN_NCMAX], trn[WN_NCMAX], trin[WN_NCMAX], tv[WN_NCMAX];
    __shared__ double Am[9 * 15];
    __shared__ RotLite rl[2][WN_KMAX - 1];
    __shared__ double red[WN_WAVES];
    __shared__ double Li[36];
    __shared__ int wcnt[WN_WAVES];
    __shared__ int bad, nrow_s;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if ((int)blockIdx.x >= a.n_items) return;
    const int t = a.t0 + (int)blockIdx.x;
    const WinData& d = a.d;
    const WinWork& w = a.w;
    viso_window_record* o = a.out + blockIdx.x;
    const size_t T = w.maxT;
    int* trk = w.trk + (size_t)blockIdx.x * 5 * T;
    double* P0 = w.pts + (size_t)blockIdx.x * 6 * T;   // [2][3][T]
    const double* tr_t = d.tr + (size_t)t * 6;
    if (t == 0 || !d.ok[t]) { wn_zero(o, tr_t, tr_t, 0, 0, 0, 0, 0); return; }
    if (w.nLp[t] < 6) { wn_zero(o, tr_t, tr_t, 0, -1, 0, 0, 0); return; }
    int anc = t - a.K + 1 > 0 ? t - a.K + 1 : 0;
    for (int j = anc > 1 ? anc : 1; j < t; ++j)
        if (!d.ok[j] || w.nLp[j] < 6) anc = j;
    const int len = t - anc + 1, nc = 6 * (len - 1);
    if (tid < nc) { trin[tid] = d.tr[(size_t)(anc + 1) * 6 + tid]; trc[tid] = trin[tid]; }
    if (tid == 0) nrow_s = 0;
    __syncthreads();
    // the tracks, in order: s ascending, then L'_{s+1}'s order
    int np = 0, nrow = 0;
    for (int so = 0; so < len - 1; ++so) {
        const int j = anc + so + 1, nl = w.nLp[j];
        const int* Lp = w.Lp + (size_t)j * d.ld;
        for (int i0 = 0; i0 < nl; i0 += WN_THREADS) {
            const int i = i0 + tid;
            bool start = false;
            int r = 0;
            if (i < nl) {
                r = Lp[i];
                start = so == 0 || wn_back(d, w, j, r) < 0;
            }
            const unsigned long long bal = __ballot(start);
            if (lane == 0) wcnt[wave] = __popcll(bal);
            __syncthreads();
            int off = np, all = 0;
#pragma unroll
            for (int v = 0; v < WN_WAVES; ++v) { off += v < wave ? wcnt[v] : 0; all += wcnt[v]; }
            if (start) {
                const int pos = off + __popcll(bal & ((1ull << lane) - 1ull));
                int e = so + 1, cur = r;
                trk[T + pos] = r;
                while (anc + e < t) {
                    const int q = wn_fwd(d, w, anc + e, cur);
                    if (q < 0) break;
                    ++e;
                    trk[(size_t)(e - so) * T + pos] = q;
                    cur = q;
                }
                trk[pos] = so | (e << 4);
                nrow += 3 + 4 * (e - so);
            }
            np += all;
            __syncthreads();
        }
    }
    atomicAdd(&nrow_s, nrow);   // integers: the order does not matter
    __threadfence_block();
    __syncthreads();
    nrow = nrow_s;
    const int denom = nrow - 3 * np - nc;
    if (denom <= 0) { wn_zero(o, tr_t, trin, nc, -1, len, np, nrow); return; }
    // the starting points: T_s^-1 Xp_c[s+1][:, r_{s+1}]
    wn_state(trc, len, rl[0], Am);
    for (int k = tid; k < np; k += WN_THREADS) {
        const int so = trk[k] & 15, r = trk[T + k];
        const double* X = d.X + (size_t)(anc + so + 1) * 3 * d.ld;
        double y0 = X[r], y1 = X[d.ld + r], y2 = X[2 * d.ld + r];
        for (int i = so; i >= 1; --i) {
            const RotLite& R = rl[0][i - 1];
            const double e0 = y0 - R.tx, e1 = y1 - R.ty, e2 = y2 - R.tz;
            y0 = R.r00 * e0 + R.r10 * e1 + R.r20 * e2;
            y1 = R.r01 * e0 + R.r11 * e1 + R.r21 * e2;
            y2 = R.r02 * e0 + R.r12 * e1 + R.r22 * e2;
        }
        P0[k] = y0; P0[T + k] = y1; P0[2 * T + k] = y2;
    }
    __threadfence_block();
    __syncthreads();
    int cur = 0, acc_steps = 0, rej = 0, status = 1;
    double lam = LM_LAMBDA0, C, C0;
    {
        double c = 0.0;
        for (int k = tid; k < np; k += WN_THREADS) c += wn_cost(a, trk, T, rl[0], anc, k, P0[k], P0[T + k], P0[2 * T + k]);
        C = C0 = wn_reduce(c, red);
    }
    if (!isfinite(C)) status = -3;
    while (status == 1 && C != 0.0) {
        const double* Pc = P0 + (size_t)cur * 3 * T;
        if (!wn_pass_a(a, trk, T, Pc, anc, len, np, rl[0], Am, lam, slots, nUr, ent, &bad)) { status = -2; break; }
        if (!wn_build(ent, nc, lam, Sm, dgd)) { status = -3; break; }
        if (!wn_chol(Sm, Lid, dgd, nc)) { status = -2; break; }
        if (tid == 0) {   // S dtr = s
            for (int i = 0; i < nc; ++i) {
                double x = ent[nc * (nc + 1) / 2 + i];
                for (int k = 0; k < i; ++k) x -= Sm[i * WN_SS + k] * tv[k];
                tv[i] = x * Lid[i];
            }
            for (int i = nc - 1; i >= 0; --i) {
                double x = tv[i];
                for (int k = i + 1; k < nc; ++k) x -= Sm[k * WN_SS + i] * dtr[k];
                dtr[i] = x * Lid[i];
            }
            for (int i = 0; i < nc; ++i) trn[i] = trc[i] + dtr[i];
        }
        __syncthreads();
        // pass B: the candidate points (dX = l^-T (y - W~ dtr)) into the other half, then the candidate's cost
        double* Pn = P0 + (size_t)(1 - cur) * 3 * T;
        {
            const int SL = wn_slot_size(len), CH = wn_chunk(len);
            for (int j0 = 0; j0 < np; j0 += CH) {
                const int k = j0 + tid;
                if (tid < CH && k < np) {
                    double dX[3];
                    const double px = Pc[k], py = Pc[T + k], pz = Pc[2 * T + k];
                    wn_point<true>(a, trk, T, anc, nc, k, px, py, pz, rl[0], Am, lam, slots + (size_t)tid * SL, nUr + tid, dtr, dX);
                    Pn[k] = px + dX[0]; Pn[T + k] = py + dX[1]; Pn[2 * T + k] = pz + dX[2];
                }
            }
        }
        wn_state(trn, len, rl[1], nullptr);
        __threadfence_block();
        __syncthreads();
        double Cn;
        {
            double c = 0.0;
            for (int k = tid; k < np; k += WN_THREADS) c += wn_cost(a, trk, T, rl[1], anc, k, Pn[k], Pn[T + k], Pn[2 * T + k]);
            Cn = wn_reduce(c, red);
        }
        if (Cn < C) {
            ++acc_steps;
            rej = 0;
            lam = fmax(lam / 10.0, LM_LAMBDA_MIN);
            const bool stop = C - Cn <= LM_REL_TOL * C || Cn == 0.0 || acc_steps == LM_MAX_ACCEPT;
            __syncthreads();
            if (tid < nc) trc[tid] = trn[tid];
            cur = 1 - cur;
            C = Cn;
            wn_state(trc, len, rl[0], Am);
            if (stop) break;
        } else {
            lam *= 10.0;
            if (++rej == LM_MAX_REJECT) break;
        }
    }
    if (status == 1) {   // the final state without damping
        const double* Pc = P0 + (size_t)cur * 3 * T;
        if (!wn_pass_a(a, trk, T, Pc, anc, len, np, rl[0], Am, 0.0, slots, nUr, ent, &bad)) status = -2;
        else if (!wn_build(ent, nc, 0.0, Sm, dgd)) status = -3;
        else if (!wn_chol(Sm, Lid, dgd, nc)) status = -2;
        if (status == 1) {
            const double sigma2 = a.mode == 2 ? a.sigma2 : C / (double)denom;
            double ss = 0.0;
            for (int i = 0; i < nc; ++i) {   // every thread: t = L^-1 s, gap = |t|^2 / sigma^2
                double x = ent[nc * (nc + 1) / 2 + i];
                for (int k = 0; k < i; ++k) x -= Sm[i * WN_SS + k] * tv[k];
                x *= Lid[i];
                __syncthreads();
                if (tid == 0) tv[i] = x;
                __syncthreads();
                ss += x * x;
            }
            const double gap = sigma2 > 0.0 ? ss / sigma2 : 0.0;
            // the tr_t block of S^-1 = L_tt^-T L_tt^-1 (L_tt the trailing 6 x 6 block of L): lanes 0..5 the columns of L_tt^-1
            const int o6 = nc - 6;
            if (tid < 6) {
                double x[6];
#pragma unroll
                for (int i = 0; i < 6; ++i) {
                    double v = i == tid ? 1.0 : 0.0;
#pragma unroll
                    for (int k = 0; k < i; ++k) v -= Sm[(o6 + i) * WN_SS + o6 + k] * x[k];
                    x[i] = v * Lid[o6 + i];
                }
#pragma unroll
                for (int i = 0; i < 6; ++i) Li[i * 6 + tid] = x[i];
            }
            __syncthreads();
            bool fin = isfinite(gap) && isfinite(sigma2);
            for (int p = 0; p < nc; ++p) fin = fin && isfinite(trc[p]);
            for (int e = 0; e < 36; ++e) fin = fin && isfinite(Li[e]);
            if (!fin) status = -3;
            if (status == 1) {
                write_cov6(Li, sigma2, o->cov);
                if (tid < 6) o->tr[tid] = trc[o6 + tid];
                if (tid < 24) o->tr_win[tid / 6][tid % 6] = tid < nc ? trc[tid] : 0.0;
                if (tid == 0) {
                    o->sigma2 = sigma2; o->cost0 = C0; o->cost = C; o->gap = gap;
                    o->iters = acc_steps; o->status = 1; o->len = len; o->n_points = np; o->n_rows = nrow; o->_pad = 0;
                }
                return;
            }
        }
    }
    __syncthreads();
    wn_zero(o, tr_t, trin, nc, status, len, np, nrow);
}

bool window_refine_args_ok(int K, int mode, double sigma_px) {
    return K >= 2 && K <= WN_KMAX && motion_args_ok(mode, sigma_px);
}

int launch_window_links(hipStream_t s, const WinData& d, const WinWork& w, int j0, int n) {
    if (n <= 0) return VISO_OK;
    hipLaunchKernelGGL(window_links_kernel, dim3((unsigned)n), dim3(WN_THREADS), 0, s, d, w, j0, n);
    HIP_TRY(hipGetLastError());
    return VISO_OK;
}

int launch_window_refine(hipStream_t s, const WinData& d, const WinWork& w, const SolverParamsDev& sp, int K, int mode, double sigma,
                         int t0, int n, viso_window_record* out) {
    if (n <= 0) return VISO_OK;
    WinArgs a;
    a.d = d; a.w = w; a.sp = sp; a.K = K; a.mode = mode; a.t0 = t0; a.n_items = n;
    a.sigma2 = mode == 2 ? sigma * sigma : 0.0; a.out = out;
    hipLaunchKernelGGL(window_refine_kernel, dim3((unsigned)n), dim3(WN_THREADS), 0, s, a);
    HIP_TRY(hipGetLastError());
    return VISO_OK;
}

// ---- the direct call: host pointers, default context ----------------------------------------------------------------------

extern "C" int viso_window_refine(int len, const int* m, const double* X, const double* obs, const int32_t* left, const double* tr,
                                  const int32_t* inl, const int* n_inl, const viso_param* param, int mode, double sigma_px,
                                  viso_window_record* out) {
    bool ok = len >= 2 && len <= WN_KMAX && m && tr && n_inl && param && out && motion_args_ok(mode, sigma_px);
    size_t rows = 0, ninl = 0;
    int ld = 1, tab = 1;
    for (int j = 0; ok && j < len - 1; ++j) {
        ok = m[j] >= 0 && n_inl[j] >= 0 && n_inl[j] <= m[j];
        rows += ok ? (size_t)m[j] : 0;
        ninl += ok ? (size_t)n_inl[j] : 0;
        if (ok && m[j] > ld) ld = m[j];
    }
    ok = ok && (rows == 0 || (X && obs && left)) && (ninl == 0 || inl);
    for (size_t i = 0; ok && i < 2 * rows; ++i) {
        ok = left[i] >= 0 && left[i] < (1 << 20);
        if (ok && left[i] + 1 > tab) tab = left[i] + 1;
    }
    {
        size_t off = 0;
        for (int j = 0; ok && j < len - 1; ++j) {
            for (int i = 0; ok && i < n_inl[j]; ++i) ok = inl[off + (size_t)i] >= 0 && inl[off + (size_t)i] < m[j];
            off += ok ? (size_t)n_inl[j] : 0;
        }
    }
    if (!ok) {
        viso_set_error("viso_window_refine: bad argument (len in 2..5, m >= 0, 0 <= n_inl <= m, indices in [0, m), left in [0, 2^20), "
                       "mode 1 or mode 2 with a finite sigma_px > 0)");
        return VISO_ERR_ARG;
    }
    const size_t nf = (size_t)len, L = (size_t)ld, maxT = (size_t)(len - 1) * L;
    // one block: X [nf][3][ld] | obs [nf][4][ld] | left [nf][ld][2] | inl [nf][ld] | tr [nf][6] | ok, n_inl, m [nf] each | L' [nf][ld]
    // | nL' [nf] | tables [nf][2][tab] | tracks [5][maxT] | points [2][3][maxT] | the record
    const size_t oX = 0, oO = al256(oX + sizeof(double) * 3 * nf * L), oLe = al256(oO + sizeof(double) * 4 * nf * L),
                 oI = al256(oLe + sizeof(int) * 2 * nf * L), oT = al256(oI + sizeof(int) * nf * L), oW = al256(oT + sizeof(double) * 6 * nf),
                 oLp = al256(oW + sizeof(int) * 3 * nf), oN = al256(oLp + sizeof(int) * nf * L), oTb = al256(oN + sizeof(int) * nf),
                 oK = al256(oTb + sizeof(int) * 2 * nf * (size_t)tab), oP = al256(oK + sizeof(int) * 5 * maxT),
                 oR = al256(oP + sizeof(double) * 6 * maxT), bytes = al256(oR + sizeof(viso_window_record));
    // the host image of the inputs: frame 0 is empty (m = 0), frames 1..len-1 the caller's (built in front of the call: it outlives it)
    std::vector<double> hX(3 * nf * L, 0.0), hO(4 * nf * L, 0.0), hT(6 * nf, 0.0);
    std::vector<int> hL(2 * nf * L, 0), hI(nf * L, 0), hW(3 * nf, 0);
    {
        size_t ro = 0, io = 0;
        for (int j = 1; j < len; ++j) {
            const size_t mj = (size_t)m[j - 1];
            for (int row = 0; row < 3; ++row)
                for (size_t i = 0; i < mj; ++i) hX[((size_t)j * 3 + row) * L + i] = X[3 * ro + row * mj + i];
            for (int row = 0; row < 4; ++row)
                for (size_t i = 0; i < mj; ++i) hO[((size_t)j * 4 + row) * L + i] = obs[4 * ro + row * mj + i];
            for (size_t i = 0; i < 2 * mj; ++i) hL[(size_t)j * 2 * L + i] = left[2 * ro + i];
            for (int i = 0; i < n_inl[j - 1]; ++i) hI[(size_t)j * L + i] = inl[io + (size_t)i];
            for (int p = 0; p < 6; ++p) hT[(size_t)j * 6 + p] = tr[(size_t)(j - 1) * 6 + p];
            hW[j] = 1; hW[nf + j] = n_inl[j - 1]; hW[2 * nf + j] = m[j - 1];
            ro += mj;
            io += (size_t)n_inl[j - 1];
        }
        hW[0] = 1;
    }
    DirectCall dc;
    VISO_TRY(dc.begin());
    char* dv;
    VISO_TRY(dc.scratch(SLOT_GEN0, bytes, &dv));
    VISO_TRY(dc.up(dv + oX, hX.data(), hX.size()));
    VISO_TRY(dc.up(dv + oO, hO.data(), hO.size()));
    VISO_TRY(dc.up(dv + oLe, hL.data(), hL.size()));
    VISO_TRY(dc.up(dv + oI, hI.data(), hI.size()));
    VISO_TRY(dc.up(dv + oT, hT.data(), hT.size()));
    VISO_TRY(dc.up(dv + oW, hW.data(), hW.size()));
    WinData d;
    d.X = reinterpret_cast<const double*>(dv + oX); d.obs = reinterpret_cast<const double*>(dv + oO);
    d.left = reinterpret_cast<const int*>(dv + oLe); d.left_fs = 2 * L; d.lstride = 2; d.lprev = 1;
    d.tr = reinterpret_cast<const double*>(dv + oT);
    const int* words = reinterpret_cast<const int*>(dv + oW);
    d.ok = words; d.n_inl = words + nf; d.m = words + 2 * nf;
    d.inl = reinterpret_cast<const int*>(dv + oI);
    d.ld = ld; d.tab = tab;
    WinWork w;
    w.Lp = reinterpret_cast<int*>(dv + oLp); w.nLp = reinterpret_cast<int*>(dv + oN); w.tabs = reinterpret_cast<int*>(dv + oTb);
    w.trk = reinterpret_cast<int*>(dv + oK); w.pts = reinterpret_cast<double*>(dv + oP); w.maxT = maxT;
    SolverParamsDev sp;
    fill_solver_params(&sp, param);
    VISO_TRY(launch_window_links(dc.s, d, w, 1, len - 1));
    VISO_TRY(launch_window_refine(dc.s, d, w, sp, len, mode, sigma_px, len - 1, 1, reinterpret_cast<viso_window_record*>(dv + oR)));
    VISO_TRY(dc.down(out, dv + oR, 1));
    return dc.wait();
}
