// covariance.hip — the opt-in per-frame motion covariance (include/viso_hip.h, "motion covariance").  Not in the
// reference.  One workgroup per frame: every lane strides over the final inlier list and keeps the 21 + 21 + 6 + 2 sums
// (A = sum w^2 J'J, B = sum w^4 J'(I + M M')J, g = sum w^2 J'r, sum |r|^2, sum |M|_F^2) in fp64 registers; the sums go through the
// workgroup sum of solver_dev.h (block_sum: DPP rows, then the waves in a fixed order in LDS), and one lane does the 6 x 6 Cholesky work
// (A^-1 B A^-1, delta = A^-1 g, g'B^-1 g).  The summation tree depends on n only: the batch at any chunking and the direct call
// give byte-identical records for the same inputs.  No scratch memory (check with -Rpass-analysis=kernel-resource-usage).  The
// direct call's staging (pose_call_stage) and the estimators' argument rule (motion_args_ok) are here; viso_pose_refine uses both.
#include "solver_dev.h"

#include <math.h>
#include <string.h>

#define COV_THREADS 256
#define COV_WAVES (COV_THREADS / 64)
#define COV_NS 50   // sums per lane: A upper triangle [0, 21) | B upper triangle [21, 42) | g [42, 48) | sum |r|^2 | sum |M|_F^2

struct CovArgs {
    const SolverItem* items;
    int n_items;
    int mode;          // 1: sigma^2 estimated, 2: sigma2 given
    double sigma2;     // mode 2
    SolverParamsDev sp;
    viso_motion_cov* out;   // [n_items]
};

// One inlier's contribution: j its position in the list (the weight's column, Q6), k the point.
__device__ __forceinline__ void cov_point(const RotDev& R, const SolverParamsDev& sp, const double* X, const double* obs, int ld,
                                          int k, int j, double (&S)[COV_NS]) {
    const double Xp = X[0 * ld + k], Yp = X[1 * ld + k], Zp = X[2 * ld + k];
    double pred[4], Xc, Yc, Zc, X2c;
    predict_point(R, sp, Xp, Yp, Zp, pred, Xc, Yc, Zc, X2c);
    const double w = 1.0 / (fabs(obs[0 * ld + j] - sp.cu) / fabs(sp.cu) + 0.05);
    const double w2 = w * w, w4 = w2 * w2;
    const double r0 = obs[0 * ld + k] - pred[0], r1 = obs[1 * ld + k] - pred[1];
    const double r2 = obs[2 * ld + k] - pred[2], r3 = obs[3 * ld + k] - pred[3];
    // J: rows uL, vL (= vR), uR of d pred / d tr, compute_J without the weight (src/viso.cpp:1478-1481)
    const double Xd[6] = {0.0, R.rdry00 * Xp + R.rdry01 * Yp + R.rdry02 * Zp, R.rdrz00 * Xp + R.rdrz01 * Yp, 1.0, 0.0, 0.0};
    const double Yd[6] = {R.rdrx10 * Xp + R.rdrx11 * Yp + R.rdrx12 * Zp, R.rdry10 * Xp + R.rdry11 * Yp + R.rdry12 * Zp,
                          R.rdrz10 * Xp + R.rdrz11 * Yp, 0.0, 1.0, 0.0};
    const double Zd[6] = {R.rdrx20 * Xp + R.rdrx21 * Yp + R.rdrx22 * Zp, R.rdry20 * Xp + R.rdry21 * Yp + R.rdry22 * Zp,
                          R.rdrz20 * Xp + R.rdrz21 * Yp, 0.0, 0.0, 1.0};
    const double iz = 1.0 / Zc, fz = sp.f * iz, fz2 = fz * iz;
    double Ju[6], Jv[6], Jr[6];
#pragma unroll
    for (int p = 0; p < 6; ++p) {
        Ju[p] = (Xd[p] * Zc - Xc * Zd[p]) * fz2;
        Jv[p] = (Yd[p] * Zc - Yc * Zd[p]) * fz2;
        Jr[p] = (Xd[p] * Zc - X2c * Zd[p]) * fz2;
    }
    // M = Pc R T: Pc rows uL (fz, 0, -fz Xc/Zc), vL (0, fz, -fz Yc/Zc), uR (fz, 0, -fz X2c/Zc); T = dX/d(uL, vL, uR) of the
    // previous frame's triangulation at d = f b / Zp
    const double pu2 = -fz * Xc * iz, pv2 = -fz * Yc * iz, pr2 = -fz * X2c * iz;
    double Mu[3], Mv[3], Mr[3];
    {
        const double id = Zp / (sp.f * sp.base);   // 1 / d
        const double T[3][3] = {{sp.base * id - Xp * id, 0.0, Xp * id},
                                {-Yp * id, sp.base * id, Yp * id},
                                {-Zp * id, 0.0, Zp * id}};
        const double Rm[3][3] = {{R.r00, R.r01, R.r02}, {R.r10, R.r11, R.r12}, {R.r20, R.r21, R.r22}};
        double xu[3], xv[3], xr[3];   // rows of Jx = Pc R
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            xu[c] = fz * Rm[0][c] + pu2 * Rm[2][c];
            xv[c] = fz * Rm[1][c] + pv2 * Rm[2][c];
            xr[c] = fz * Rm[0][c] + pr2 * Rm[2][c];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            Mu[c] = xu[0] * T[0][c] + xu[1] * T[1][c] + xu[2] * T[2][c];
            Mv[c] = xv[0] * T[0][c] + xv[1] * T[1][c] + xv[2] * T[2][c];
            Mr[c] = xr[0] * T[0][c] + xr[1] * T[1][c] + xr[2] * T[2][c];
        }
    }
    // K = M'J (3 x 6) over the four rows (vR repeats vL)
    double K[3][6];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int p = 0; p < 6; ++p) K[c][p] = Mu[c] * Ju[p] + Mr[c] * Jr[p] + 2.0 * (Mv[c] * Jv[p]);
    int s = 0;
#pragma unroll
    for (int p = 0; p < 6; ++p) {
#pragma unroll
        for (int q = p; q < 6; ++q) {
            const double jj = Ju[p] * Ju[q] + Jr[p] * Jr[q] + 2.0 * (Jv[p] * Jv[q]);
            const double kk = K[0][p] * K[0][q] + K[1][p] * K[1][q] + K[2][p] * K[2][q];
            S[s] = fma(w2, jj, S[s]);
            S[21 + s] = fma(w4, jj + kk, S[21 + s]);
            ++s;
        }
        S[42 + p] = fma(w2, Ju[p] * r0 + Jv[p] * (r1 + r3) + Jr[p] * r2, S[42 + p]);
    }
    S[48] += r0 * r0 + r1 * r1 + r2 * r2 + r3 * r3;
    S[49] += Mu[0] * Mu[0] + Mu[1] * Mu[1] + Mu[2] * Mu[2] + Mr[0] * Mr[0] + Mr[1] * Mr[1] + Mr[2] * Mr[2] +
             2.0 * (Mv[0] * Mv[0] + Mv[1] * Mv[1] + Mv[2] * Mv[2]);
}

// In-place Cholesky of a symmetric 6 x 6 (lower triangle of the result in L); false when a pivot is not > 1e-12 x the original
// diagonal entry (NaN included).  Every index is static: the matrix stays in registers.
__device__ __forceinline__ bool chol6(double (&L)[6][6]) {
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double s = L[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) s -= L[j][k] * L[j][k];
        if (!(s > 1e-12 * L[j][j])) return false;
        L[j][j] = sqrt(s);
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double t = L[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) t -= L[i][k] * L[j][k];
            L[i][j] = t / L[j][j];
        }
    }
    return true;
}

// y = L^-1 b (forward substitution)
__device__ __forceinline__ void fwd6(const double (&L)[6][6], const double (&b)[6], double (&y)[6]) {
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double t = b[i];
#pragma unroll
        for (int k = 0; k < i; ++k) t -= L[i][k] * y[k];
        y[i] = t / L[i][i];
    }
}

// Lane 0 of the workgroup: the record from the 50 reduced sums.
__device__ __forceinline__ void cov_finish(const double* tot, int n, int mode, double sigma2_in, viso_motion_cov* o) {
    double LA[6][6], B[6][6];
#pragma unroll
    for (int p = 0; p < 6; ++p)
#pragma unroll
        for (int q = p; q < 6; ++q) {
            LA[p][q] = LA[q][p] = tot[up6(p, q)];
            B[p][q] = B[q][p] = tot[21 + up6(p, q)];
        }
    double g[6];
#pragma unroll
    for (int p = 0; p < 6; ++p) g[p] = tot[42 + p];
    const double sigma2 = mode == 2 ? sigma2_in : tot[48] / (4.0 * n + tot[49] - 6.0);
    bool good = chol6(LA);
    // A^-1 = L^-T L^-1: the columns of L^-1 by forward substitution of the unit vectors
    double Ai[6][6];
    if (good) {
        double Li[6][6];
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            double e[6], y[6];
#pragma unroll
            for (int i = 0; i < 6; ++i) e[i] = i == c ? 1.0 : 0.0;
            fwd6(LA, e, y);
#pragma unroll
            for (int i = 0; i < 6; ++i) Li[i][c] = y[i];
        }
#pragma unroll
        for (int p = 0; p < 6; ++p)
#pragma unroll
            for (int q = p; q < 6; ++q) {
                double s = 0.0;
#pragma unroll
                for (int k = q; k < 6; ++k) s += Li[k][p] * Li[k][q];   // L^-1 is lower: rows k >= max(p, q)
                Ai[p][q] = Ai[q][p] = s;
            }
    }
    double C[6][6], cov[6][6], delta[6], gap = 0.0;
    if (good) {
#pragma unroll
        for (int p = 0; p < 6; ++p)
#pragma unroll
            for (int q = 0; q < 6; ++q) {
                double s = 0.0;
#pragma unroll
                for (int k = 0; k < 6; ++k) s += Ai[p][k] * B[k][q];
                C[p][q] = s;
            }
#pragma unroll
        for (int p = 0; p < 6; ++p) {
#pragma unroll
            for (int q = p; q < 6; ++q) {
                double s = 0.0;
#pragma unroll
                for (int k = 0; k < 6; ++k) s += C[p][k] * Ai[k][q];
                cov[p][q] = cov[q][p] = sigma2 * s;
            }
            double d = 0.0;
#pragma unroll
            for (int k = 0; k < 6; ++k) d += Ai[p][k] * g[k];
            delta[p] = d;
        }
        good = chol6(B);
        if (good) {
            double y[6];
            fwd6(B, g, y);
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < 6; ++k) s += y[k] * y[k];
            gap = sigma2 > 0.0 ? s / sigma2 : 0.0;
        }
    }
#pragma unroll
    for (int p = 0; p < 6; ++p) {
#pragma unroll
        for (int q = 0; q < 6; ++q) o->cov[p * 6 + q] = good ? cov[p][q] : 0.0;
        o->delta[p] = good ? delta[p] : 0.0;
    }
    o->sigma2 = good ? sigma2 : 0.0;
    o->gap = good ? gap : 0.0;
    o->status = good ? 1 : -2;
    o->n = n;
}

__device__ __forceinline__ void cov_zero(viso_motion_cov* o, int status, int n) {
    double* d = reinterpret_cast<double*>(o);   // cov | delta | sigma2 | gap: 44 contiguous doubles at the start of the record
    static_assert(offsetof(viso_motion_cov, status) == 44 * sizeof(double), "viso_motion_cov layout");
    for (int i = threadIdx.x; i < 44; i += COV_THREADS) d[i] = 0.0;
    if (threadIdx.x == 0) { o->status = status; o->n = n; }
}

__global__ __launch_bounds__(COV_THREADS) void motion_cov_kernel(CovArgs a) {
    __shared__ double red[COV_WAVES * COV_NS];
    __shared__ double tot[COV_NS];
    const int item = blockIdx.x;
    if (item >= a.n_items) return;
    const SolverItem S = a.items[item];
    viso_motion_cov* o = a.out + item;
    const int m = min(*S.m_ptr, S.ld);
    int n = *S.n_inl;
    n = n < 0 ? 0 : n > m ? m : n;   // the refit's list: n <= m indices below m
    if (!*S.ok) { cov_zero(o, 0, n); return; }   // uniform: every lane read the same words
    if (n < 6) { cov_zero(o, -1, n); return; }
    double tr[6];
#pragma unroll
    for (int p = 0; p < 6; ++p) tr[p] = S.tr[p];
    RotDev R;
    make_rot(tr, R);
    double acc[COV_NS];
#pragma unroll
    for (int k = 0; k < COV_NS; ++k) acc[k] = 0.0;
    for (int j = threadIdx.x; j < n; j += COV_THREADS) cov_point(R, a.sp, S.X, S.obs, S.ld, S.inl[j], j, acc);
    block_sum<COV_NS, COV_WAVES>(acc, red, tot);
    if (threadIdx.x == 0) cov_finish(tot, n, a.mode, a.sigma2, o);
}

int launch_motion_cov(hipStream_t s, const SolverItem* items_dev, int n_items, const SolverParamsDev& sp, int mode, double sigma,
                      viso_motion_cov* out) {
    if (n_items <= 0) return VISO_OK;
    CovArgs a;
    a.items = items_dev; a.n_items = n_items; a.mode = mode; a.sigma2 = mode == 2 ? sigma * sigma : 0.0; a.sp = sp; a.out = out;
    hipLaunchKernelGGL(motion_cov_kernel, dim3((unsigned)n_items), dim3(COV_THREADS), 0, s, a);
    HIP_TRY(hipGetLastError());
    return VISO_OK;
}

bool motion_args_ok(int mode, double sigma_px) {
    return mode == 1 || (mode == 2 && isfinite(sigma_px) && sigma_px > 0.0);
}

// ---- the direct calls: host pointers, default context ---------------------------------------------------------------------
int pose_call_stage(const char* where, const double* X, const double* obs, int m, const double* tr, const int32_t* inl, int n_inl,
                    const viso_param* param, int mode, double sigma_px, const void* out, size_t rec_bytes, size_t extra_bytes,
                    PoseCall* pc) {
    bool ok = m >= 0 && n_inl >= 0 && n_inl <= m && tr && param && out && (m == 0 || (X && obs)) && (n_inl == 0 || inl) &&
              motion_args_ok(mode, sigma_px);
    for (int j = 0; ok && j < n_inl; ++j) ok = inl[j] >= 0 && inl[j] < m;
    if (!ok) {
        viso_set_error("%s: bad argument (m >= 0, 0 <= n_inl <= m, indices in [0, m), mode 1 or mode 2 with a finite sigma_px > 0)",
                       where);
        return VISO_ERR_ARG;
    }
    DirectCall& dc = pc->dc;
    VISO_TRY(dc.begin());
    const size_t ld = (size_t)(m > 0 ? m : 1);
    // one block: X [3][ld] | obs [4][ld] | inl [ld] | tr [6] | ok, n_inl, m | the item | the record | the caller's extra
    const size_t oX = 0, oO = al256(oX + sizeof(double) * 3 * ld), oI = al256(oO + sizeof(double) * 4 * ld),
                 oT = al256(oI + sizeof(int) * ld), oW = al256(oT + sizeof(double) * 6), oS = al256(oW + sizeof(int) * 4),
                 oR = al256(oS + sizeof(SolverItem)), oE = al256(oR + rec_bytes), bytes = al256(oE + extra_bytes);
    char* d;
    VISO_TRY(dc.scratch(SLOT_GEN0, bytes, &d));
    SolverItem it;
    memset(&it, 0, sizeof(it));
    it.X = reinterpret_cast<double*>(d + oX); it.obs = reinterpret_cast<double*>(d + oO); it.ld = (int)ld;
    it.inl = reinterpret_cast<int*>(d + oI); it.tr = reinterpret_cast<double*>(d + oT);
    int* words = reinterpret_cast<int*>(d + oW);
    it.ok = words; it.n_inl = words + 1; it.m_ptr = words + 2;
    const int hw[4] = {1, n_inl, m, 0};
    VISO_TRY(dc.up(d + oX, X, 3 * (size_t)m));
    VISO_TRY(dc.up(d + oO, obs, 4 * (size_t)m));
    VISO_TRY(dc.up(d + oI, inl, (size_t)n_inl));
    VISO_TRY(dc.up(d + oT, tr, 6));
    VISO_TRY(dc.up(words, hw, 4));
    VISO_TRY(dc.up(d + oS, &it, 1));
    fill_solver_params(&pc->sp, param);
    pc->ld = ld;
    pc->item = reinterpret_cast<const SolverItem*>(d + oS);
    pc->rec = d + oR;
    pc->extra = d + oE;
    return VISO_OK;
}

extern "C" int viso_pose_covariance(const double* X, const double* obs, int m, const double tr[6], const int32_t* inl, int n_inl,
                                    const viso_param* param, int mode, double sigma_px, viso_motion_cov* out) {
    PoseCall pc;
    VISO_TRY(pose_call_stage("viso_pose_covariance", X, obs, m, tr, inl, n_inl, param, mode, sigma_px, out, sizeof(viso_motion_cov), 0, &pc));
    VISO_TRY(launch_motion_cov(pc.dc.s, pc.item, 1, pc.sp, mode, sigma_px, reinterpret_cast<viso_motion_cov*>(pc.rec)));
    VISO_TRY(pc.dc.down(out, pc.rec, 1));
    return pc.dc.wait();
}
