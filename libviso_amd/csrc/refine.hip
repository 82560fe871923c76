// refine.hip — the opt-in two-frame bundle adjustment of motion and structure (include/viso_hip.h, "motion refinement";
// DESIGN.md 5.9).  Not in the reference.  One workgroup per frame runs the whole Levenberg-Marquardt loop:
//   - the used points L' (finite inputs with Z > 0, in the inlier list's order) are compacted once into the per-frame point
//     buffer [2][3][ld] (current | candidate) and index list [ld];
//   - pass A strides over L' and keeps the 35 sums of the reduced system in fp64 registers -- S = Hcc - sum Hcp Hpp^-1 Hcp'
//     (21) and s (6) -- and an LDS flag for a failed 3 x 3 pivot (the diagonal of Hcc, for the damping, is summed once per state
//     with the cost, into LDS); the point's
//     share of S as V'V (rf_point: one 3 x 6 block alive);
//   - every lane factors the damped 6 x 6 S itself (the same instructions on the same LDS words: no broadcast, no divergence,
//     ~60 live registers, where motion_cov_kernel's serial lane-0 work held 256);
//   - pass B recomputes the point blocks, forms dX and writes it into the other half, and sums the candidate's cost.
// The summation tree (block_sum of solver_dev.h: DPP rows, then the waves in a fixed order in LDS) depends on n only: the batch at any
// chunking and the direct call give byte-identical records.  No scratch memory (-Rpass-analysis=kernel-resource-usage).  The
// rotation (RotLite), the LM schedule (LM_*) and the covariance write-out (write_cov6) are solver_dev.h's, shared with window.hip.
#include "solver_dev.h"

#include <math.h>
#include <string.h>

#define RF_THREADS 256
#define RF_WAVES (RF_THREADS / 64)
#define RF_NS 27   // S upper triangle [0, 21) | s [21, 27)

struct RefineArgs {
    const SolverItem* items;
    int n_items;
    int mode;          // 1: sigma^2 estimated, 2: sigma2 given
    double sigma2;     // mode 2
    SolverParamsDev sp;
    double* pts;       // [n_items][2][3][ld of the item]: current and candidate points, L' order
    int* idx;          // [n_items][ld]: L'
    size_t stride;     // elements per item of pts / 6 and of idx (>= every item's ld)
    viso_motion_refine* out;   // [n_items]
};

// One point at the state (R, P) with damping lam.  The four current-frame rows enter as three, the shared v row scaled by sqrt 2
// (J~, Jx~; r~_v = (r_vL + r_vR) / sqrt 2), so that J'J = J~'J~, Hcp = J~'Jx~ and J'r1 = J~'r~.  With l the Cholesky factor of
// Hpp_d and M = Jx~ l^-T (3 x 3), y = l^-1 gp:
//   Hcp Hpp_d^-1 Hcp' = J~'M M'J~, so the point's share of S is J~'(I - M M')J~ = V'V with V = G'J~, G G' = I - M M' (positive
//   definite: the eigenvalues of M M' are those of l^-1 Jx~'Jx~ l^-T < 1), and its share of s is J~'(r~ - M y);
//   dX = Hpp_d^-1 (gp - Hcp' dtr) = l^-T (y - M'(J~ dtr)).
// STEP false: the shares of S and s are added to acc (V is the only 3 x 6 block alive:
// registers).  STEP true: dX for the step dtr.  Returns false when a pivot of Hpp_d or of I - M M'
// fails the 1e-12 test.
template <bool STEP>
__device__ __forceinline__ bool rf_point(const RotLite& R, const SolverParamsDev& sp, const double (&z0)[3], const double (&z1)[4],
                                         double Px, double Py, double Pz, double lam, double (&acc)[RF_NS], const double (&dtr)[6],
                                         double (&dX)[3]) {
    const double f = sp.f, b = sp.base;
    const double RT2 = 1.4142135623730951;
    const double qx = R.r00 * Px + R.r01 * Py + R.r02 * Pz, qy = R.r10 * Px + R.r11 * Py + R.r12 * Pz;
    const double qz = R.r20 * Px + R.r21 * Py + R.r22 * Pz;
    const double Xc = qx + R.tx, Yc = qy + R.ty, Zc = qz + R.tz;
    const double X2c = Xc - b;
    const double iz = 1.0 / Zc, fz = f * iz, fz2 = fz * iz;
    const double r1u = z1[0] - (fz * Xc + sp.cu), r1v = z1[1] - (fz * Yc + sp.cv);
    const double r1r = z1[2] - (fz * X2c + sp.cu), r1w = z1[3] - (fz * Yc + sp.cv);
    // previous frame: pi_0(P) and its Jacobian rows (f/Z, 0, -f X/Z^2), (0, f/Z, -f Y/Z^2), (f/Z, 0, -f (X - b)/Z^2)
    const double ip = 1.0 / Pz, gz = f * ip, gz2 = gz * ip;
    const double r0u = z0[0] - (gz * Px + sp.cu), r0v = z0[1] - (gz * Py + sp.cv), r0r = z0[2] - (gz * (Px - b) + sp.cu);
    const double q0 = -gz2 * Px, q1 = -gz2 * Py, q2 = -gz2 * (Px - b);
    // Jx = Pc R: rows uL, vL (= vR), uR
    const double pu = -fz2 * Xc, pv = -fz2 * Yc, pr = -fz2 * X2c;
    const double xu[3] = {fz * R.r00 + pu * R.r20, fz * R.r01 + pu * R.r21, fz * R.r02 + pu * R.r22};
    const double xv[3] = {fz * R.r10 + pv * R.r20, fz * R.r11 + pv * R.r21, fz * R.r12 + pv * R.r22};
    const double xr[3] = {fz * R.r00 + pr * R.r20, fz * R.r01 + pr * R.r21, fz * R.r02 + pr * R.r22};
    // Hpp = Jx'Jx + P0'P0 (P0 columns: (gz, 0, gz), (0, gz, 0), (q0, q1, q2)), gp = Jx'r1 + P0'r0
    const double rv = r1v + r1w;
    double h00 = xu[0] * xu[0] + xr[0] * xr[0] + 2.0 * (xv[0] * xv[0]) + 2.0 * (gz * gz);
    const double h01 = xu[0] * xu[1] + xr[0] * xr[1] + 2.0 * (xv[0] * xv[1]);
    const double h02 = xu[0] * xu[2] + xr[0] * xr[2] + 2.0 * (xv[0] * xv[2]) + gz * (q0 + q2);
    double h11 = xu[1] * xu[1] + xr[1] * xr[1] + 2.0 * (xv[1] * xv[1]) + gz * gz;
    const double h12 = xu[1] * xu[2] + xr[1] * xr[2] + 2.0 * (xv[1] * xv[2]) + gz * q1;
    double h22 = xu[2] * xu[2] + xr[2] * xr[2] + 2.0 * (xv[2] * xv[2]) + (q0 * q0 + q1 * q1 + q2 * q2);
    const double g0 = xu[0] * r1u + xv[0] * rv + xr[0] * r1r + gz * (r0u + r0r);
    const double g1 = xu[1] * r1u + xv[1] * rv + xr[1] * r1r + gz * r0v;
    const double g2 = xu[2] * r1u + xv[2] * rv + xr[2] * r1r + (q0 * r0u + q1 * r0v + q2 * r0r);
    h00 = h00 * (1.0 + lam); h11 = h11 * (1.0 + lam); h22 = h22 * (1.0 + lam);
    // l = chol(Hpp_d), packed l00, l10, l11, l20, l21, l22
    bool good = h00 > 1e-12 * h00;   // NaN and h00 <= 0 fail it
    const double l0 = sqrt(h00), il0 = 1.0 / l0;
    const double l1 = h01 * il0, l3 = h02 * il0;
    const double s11 = h11 - l1 * l1;
    good = good && s11 > 1e-12 * h11;
    const double l2 = sqrt(s11), il1 = 1.0 / l2;
    const double l4 = (h12 - l3 * l1) * il1;
    const double s22 = h22 - l3 * l3 - l4 * l4;
    good = good && s22 > 1e-12 * h22;
    const double l5 = sqrt(s22), il2 = 1.0 / l5;
    auto fwd3 = [&](double a0, double a1, double a2, double (&o)[3]) {
        o[0] = a0 * il0;
        o[1] = (a1 - l1 * o[0]) * il1;
        o[2] = (a2 - l3 * o[0] - l4 * o[1]) * il2;
    };
    double y[3], mu[3], mv[3], mr[3];   // y = l^-1 gp; the rows of M
    fwd3(g0, g1, g2, y);
    fwd3(xu[0], xu[1], xu[2], mu);
    fwd3(RT2 * xv[0], RT2 * xv[1], RT2 * xv[2], mv);
    fwd3(xr[0], xr[1], xr[2], mr);
    // d Xc / d tr: w_i x q for the rotation, the unit vectors for the translation; J~ column p = (ju, jv, jr)
    const double Xd[6] = {0.0, R.cx * qz - R.sx * qy, R.w21 * qz - R.w22 * qy, 1.0, 0.0, 0.0};
    const double Yd[6] = {-qz, R.sx * qx, R.w22 * qx - R.sy * qz, 0.0, 1.0, 0.0};
    const double Zd[6] = {qy, -R.cx * qx, R.sy * qy - R.w21 * qx, 0.0, 0.0, 1.0};
    if (STEP) {
        double t0 = 0.0, t1 = 0.0, t2 = 0.0;   // J~ dtr
#pragma unroll
        for (int p = 0; p < 6; ++p) {
            t0 += (Xd[p] * Zc - Xc * Zd[p]) * fz2 * dtr[p];
            t1 += RT2 * ((Yd[p] * Zc - Yc * Zd[p]) * fz2) * dtr[p];
            t2 += (Xd[p] * Zc - X2c * Zd[p]) * fz2 * dtr[p];
        }
        double v[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = y[c] - (mu[c] * t0 + mv[c] * t1 + mr[c] * t2);
        // l' dX = v
        dX[2] = v[2] * il2;
        dX[1] = (v[1] - l4 * dX[2]) * il1;
        dX[0] = (v[0] - l1 * dX[1] - l3 * dX[2]) * il0;
        return good;
    }
    // G = chol(I - M M'), packed like l; V = G' J~
    const double Q00 = 1.0 - (mu[0] * mu[0] + mu[1] * mu[1] + mu[2] * mu[2]);
    const double Q10 = -(mv[0] * mu[0] + mv[1] * mu[1] + mv[2] * mu[2]);
    const double Q11 = 1.0 - (mv[0] * mv[0] + mv[1] * mv[1] + mv[2] * mv[2]);
    const double Q20 = -(mr[0] * mu[0] + mr[1] * mu[1] + mr[2] * mu[2]);
    const double Q21 = -(mr[0] * mv[0] + mr[1] * mv[1] + mr[2] * mv[2]);
    const double Q22 = 1.0 - (mr[0] * mr[0] + mr[1] * mr[1] + mr[2] * mr[2]);
    // positive definite in exact arithmetic; a pivot that fails the test of Hpp_d counts as a failed pivot (status -2)
    good = good && Q00 > 1e-12 * Q00;
    const double G0 = sqrt(Q00), iG0 = 1.0 / G0;
    const double G1 = Q10 * iG0, G3 = Q20 * iG0;
    const double t11 = Q11 - G1 * G1;
    good = good && t11 > 1e-12 * Q11;
    const double G2 = sqrt(t11), iG2 = 1.0 / G2;
    const double G4 = (Q21 - G3 * G1) * iG2;
    const double t22 = Q22 - G3 * G3 - G4 * G4;
    good = good && t22 > 1e-12 * Q22;
    const double G5 = sqrt(t22);
    // u = r~ - M y
    const double u0 = r1u - (mu[0] * y[0] + mu[1] * y[1] + mu[2] * y[2]);
    const double u1 = rv * (1.0 / RT2) - (mv[0] * y[0] + mv[1] * y[1] + mv[2] * y[2]);
    const double u2 = r1r - (mr[0] * y[0] + mr[1] * y[1] + mr[2] * y[2]);
    double V[3][6];
#pragma unroll
    for (int p = 0; p < 6; ++p) {
        const double ju = (Xd[p] * Zc - Xc * Zd[p]) * fz2;
        const double jv = RT2 * ((Yd[p] * Zc - Yc * Zd[p]) * fz2);
        const double jr = (Xd[p] * Zc - X2c * Zd[p]) * fz2;
        V[0][p] = G0 * ju + G1 * jv + G3 * jr;
        V[1][p] = G2 * jv + G4 * jr;
        V[2][p] = G5 * jr;
        acc[21 + p] += ju * u0 + jv * u1 + jr * u2;
    }
    int c = 0;
#pragma unroll
    for (int p = 0; p < 6; ++p)
#pragma unroll
        for (int q = p; q < 6; ++q) { acc[c] += V[0][p] * V[0][q] + V[1][p] * V[1][q] + V[2][p] * V[2][q]; ++c; }
    return good;
}

// The point's share of the cost at (R, P).
__device__ __forceinline__ double rf_cost(const RotLite& R, const SolverParamsDev& sp, const double (&z0)[3], const double (&z1)[4],
                                          double Px, double Py, double Pz) {
    const double f = sp.f, b = sp.base;
    const double Xc = R.r00 * Px + R.r01 * Py + R.r02 * Pz + R.tx;
    const double Yc = R.r10 * Px + R.r11 * Py + R.r12 * Pz + R.ty;
    const double Zc = R.r20 * Px + R.r21 * Py + R.r22 * Pz + R.tz;
    const double fz = f / Zc, gz = f / Pz;
    const double r1u = z1[0] - (fz * Xc + sp.cu), r1v = z1[1] - (fz * Yc + sp.cv);
    const double r1r = z1[2] - (fz * (Xc - b) + sp.cu), r1w = z1[3] - (fz * Yc + sp.cv);
    const double r0u = z0[0] - (gz * Px + sp.cu), r0v = z0[1] - (gz * Py + sp.cv), r0r = z0[2] - (gz * (Px - b) + sp.cu);
    return (r1u * r1u + r1v * r1v + r1r * r1r + r1w * r1w) + (r0u * r0u + r0v * r0v + r0r * r0r);
}

// The point's share of the cost and of the diagonal of Hcc = sum J'J at (R, P): acc[0] += C_k, acc[1 + p] += (J'J)_pp.  The
// diagonal depends on the state only, not on lambda, so it is summed once per state here (the starting state, every candidate)
// and kept in LDS, not in pass A's registers.
__device__ __forceinline__ void rf_cost_diag(const RotLite& R, const SolverParamsDev& sp, const double (&z0)[3], const double (&z1)[4],
                                             double Px, double Py, double Pz, double (&acc)[7]) {
    acc[0] += rf_cost(R, sp, z0, z1, Px, Py, Pz);
    const double qx = R.r00 * Px + R.r01 * Py + R.r02 * Pz, qy = R.r10 * Px + R.r11 * Py + R.r12 * Pz;
    const double qz = R.r20 * Px + R.r21 * Py + R.r22 * Pz;
    const double Xc = qx + R.tx, Yc = qy + R.ty, Zc = qz + R.tz, X2c = Xc - sp.base;
    const double iz = 1.0 / Zc, fz2 = sp.f * iz * iz;
    const double Xd[6] = {0.0, R.cx * qz - R.sx * qy, R.w21 * qz - R.w22 * qy, 1.0, 0.0, 0.0};
    const double Yd[6] = {-qz, R.sx * qx, R.w22 * qx - R.sy * qz, 0.0, 1.0, 0.0};
    const double Zd[6] = {qy, -R.cx * qx, R.sy * qy - R.w21 * qx, 0.0, 0.0, 1.0};
#pragma unroll
    for (int p = 0; p < 6; ++p) {
        const double ju = (Xd[p] * Zc - Xc * Zd[p]) * fz2;
        const double jv = (Yd[p] * Zc - Yc * Zd[p]) * fz2;
        const double jr = (Xd[p] * Zc - X2c * Zd[p]) * fz2;
        acc[1 + p] += ju * ju + 2.0 * (jv * jv) + jr * jr;
    }
}

// The observations of point k: z0 from the input point (triangulate_rectified inverted), z1 = obs[:, k].
__device__ __forceinline__ void rf_obs(const SolverItem& S, const SolverParamsDev& sp, int k, double (&z0)[3], double (&z1)[4]) {
    const int ld = S.ld;
    const double X = S.X[0 * ld + k], Y = S.X[1 * ld + k], Z = S.X[2 * ld + k];
    const double g = sp.f / Z;
    z0[0] = g * X + sp.cu;
    z0[1] = g * Y + sp.cv;
    z0[2] = g * (X - sp.base) + sp.cu;
#pragma unroll
    for (int r = 0; r < 4; ++r) z1[r] = S.obs[r * ld + k];
}

// Cholesky of the symmetric 6 x 6 whose upper triangle is u[21] (plus lam x dg on the diagonal) into the packed lower factor
// L[21] (row i at i (i + 1) / 2) and the reciprocals of its diagonal; false when a pivot is not > 1e-12 x its diagonal entry.
__device__ __forceinline__ bool rf_chol6(const double* u, const double* dg, double lam, double (&L)[21], double (&id)[6]) {
    bool good = true;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const double a = u[up6(j, j)] + lam * dg[j];
        double s = a;
#pragma unroll
        for (int k = 0; k < j; ++k) s -= L[j * (j + 1) / 2 + k] * L[j * (j + 1) / 2 + k];
        good = good && s > 1e-12 * a;
        L[j * (j + 1) / 2 + j] = sqrt(s);
        id[j] = 1.0 / L[j * (j + 1) / 2 + j];
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double t = u[up6(j, i)];
#pragma unroll
            for (int k = 0; k < j; ++k) t -= L[i * (i + 1) / 2 + k] * L[j * (j + 1) / 2 + k];
            L[i * (i + 1) / 2 + j] = t * id[j];
        }
    }
    return good;
}

__device__ __forceinline__ void rf_fwd6(const double (&L)[21], const double (&id)[6], const double (&b)[6], double (&x)[6]) {
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double t = b[i];
#pragma unroll
        for (int k = 0; k < i; ++k) t -= L[i * (i + 1) / 2 + k] * x[k];
        x[i] = t * id[i];
    }
}

__device__ __forceinline__ void rf_bwd6(const double (&L)[21], const double (&id)[6], double (&x)[6]) {
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        double t = x[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k) t -= L[k * (k + 1) / 2 + i] * x[k];
        x[i] = t * id[i];
    }
}

__device__ __forceinline__ void rf_zero(viso_motion_refine* o, const double* tr_in, int status, int n) {
    static_assert(sizeof(viso_motion_refine) == 384, "viso_motion_refine layout");
    double* d = reinterpret_cast<double*>(o);   // tr | cov | sigma2 | cost0 | cost | gap: 46 contiguous doubles
    for (int i = threadIdx.x; i < 46; i += RF_THREADS) d[i] = i < 6 ? tr_in[i] : 0.0;
    if (threadIdx.x == 0) { o->iters = 0; o->status = status; o->n = n; o->_pad = 0; }
}


// 255 VGPRs, occupancy 2, no scratch.  Pinning the budget with amdgpu_waves_per_eu(2) makes this compiler spill 54 VGPRs, so
// the budget is checked instead: tests/test_refine_cpu.py compiles this file and fails below occupancy 2 or on any scratch.
__global__ __launch_bounds__(RF_THREADS) void motion_refine_kernel(RefineArgs a) {
    __shared__ double red[RF_WAVES * RF_NS];
    __shared__ double tot[RF_NS];
    __shared__ double Li[36];
    __shared__ int wcnt[RF_WAVES];
    __shared__ double dg[6];   // the diagonal of Hcc at the current state
    __shared__ int bad;   // a point of the pass failed a pivot test (every writer stores 1: no order to depend on)
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int item = blockIdx.x;
    if (item >= a.n_items) return;
    const SolverItem S = a.items[item];
    const SolverParamsDev sp = a.sp;
    const double zero6[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    viso_motion_refine* o = a.out + item;
    const int ld = S.ld;
    const int m = min(*S.m_ptr, ld);
    int n_inl = *S.n_inl;
    n_inl = n_inl < 0 ? 0 : n_inl > m ? m : n_inl;   // the refit's list: n_inl <= m indices below m
    double tr_in[6];
#pragma unroll
    for (int p = 0; p < 6; ++p) tr_in[p] = S.tr[p];
    double* P0 = a.pts + (size_t)item * 6 * a.stride;   // [2][3][stride]
    int* idx = a.idx + (size_t)item * a.stride;
    // L': compaction of the usable inliers, in the list's order
    int n = 0;
    for (int j0 = 0; j0 < n_inl; j0 += RF_THREADS) {
        const int j = j0 + tid;
        bool good = false;
        int k = 0;
        double x = 0.0, yv = 0.0, z = 0.0;
        if (j < n_inl) {
            k = S.inl[j];
            if (k >= 0 && k < m) {
                x = S.X[0 * ld + k]; yv = S.X[1 * ld + k]; z = S.X[2 * ld + k];
                good = isfinite(x) && isfinite(yv) && isfinite(z) && z > 0.0;
            }
        }
        const unsigned long long bal = __ballot(good);
        if (lane == 0) wcnt[wave] = __popcll(bal);
        __syncthreads();
        int off = n, all = 0;
#pragma unroll
        for (int w = 0; w < RF_WAVES; ++w) {
            off += w < wave ? wcnt[w] : 0;
            all += wcnt[w];
        }
        if (good) {
            const int pos = off + __popcll(bal & ((1ull << lane) - 1ull));
            idx[pos] = k;
            P0[0 * a.stride + pos] = x; P0[1 * a.stride + pos] = yv; P0[2 * a.stride + pos] = z;
        }
        n += all;
        __syncthreads();
    }
    if (!*S.ok) { rf_zero(o, tr_in, 0, n); return; }   // uniform: every lane read the same words
    if (n < 6) { rf_zero(o, tr_in, -1, n); return; }
    __threadfence_block();   // the compacted points are read by other lanes below (global memory, same workgroup)
    __syncthreads();

    double tr[6];
#pragma unroll
    for (int p = 0; p < 6; ++p) tr[p] = tr_in[p];
    int cur = 0, acc_steps = 0, rej = 0, status = 1;
    double lam = LM_LAMBDA0, C = 0.0, C0 = 0.0;
    {   // the starting cost
        RotLite R;
        rot_lite(tr, R);
        double accC[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int j = tid; j < n; j += RF_THREADS) {
            double z0[3], z1[4];
            rf_obs(S, sp, idx[j], z0, z1);
            rf_cost_diag(R, sp, z0, z1, P0[j], P0[a.stride + j], P0[2 * a.stride + j], accC);
        }
        block_sum<7, RF_WAVES>(accC, red, tot);
        C = C0 = tot[0];
        if (tid < 6) dg[tid] = tot[1 + tid];
    }
    if (!isfinite(C)) status = -3;
    while (status == 1 && C != 0.0) {
        __syncthreads();   // tot and bad are rewritten by the next pass
        // pass A: the reduced system at the current state with damping lam
        {
            RotLite R;
            rot_lite(tr, R);
            const double* Pc = P0 + (size_t)cur * 3 * a.stride;
            double acc[RF_NS];
#pragma unroll
            for (int k = 0; k < RF_NS; ++k) acc[k] = 0.0;
            if (tid == 0) bad = 0;
            __syncthreads();
            for (int j = tid; j < n; j += RF_THREADS) {
                double z0[3], z1[4], dX[3];
                rf_obs(S, sp, idx[j], z0, z1);
                if (!rf_point<false>(R, sp, z0, z1, Pc[j], Pc[a.stride + j], Pc[2 * a.stride + j], lam, acc, zero6, dX)) bad = 1;
            }
            block_sum<RF_NS, RF_WAVES>(acc, red, tot);
        }
        if (bad) { status = -2; break; }
        bool fin = true;
#pragma unroll
        for (int k = 0; k < RF_NS; ++k) fin = fin && isfinite(tot[k]);
#pragma unroll
        for (int k = 0; k < 6; ++k) fin = fin && isfinite(dg[k]);
        if (!fin) { status = -3; break; }
        double L[21], id[6], dtr[6];
        if (!rf_chol6(tot, dg, lam, L, id)) { status = -2; break; }
        {
            double s[6], t[6];
#pragma unroll
            for (int p = 0; p < 6; ++p) s[p] = tot[21 + p];
            rf_fwd6(L, id, s, t);
            rf_bwd6(L, id, t);
#pragma unroll
            for (int p = 0; p < 6; ++p) dtr[p] = t[p];
        }
        // pass B: dX = Hpp_d^-1 (gp - Hcp' dtr) into the other half, and the candidate's cost
        double trn[6];
#pragma unroll
        for (int p = 0; p < 6; ++p) trn[p] = tr[p] + dtr[p];
        {
            RotLite R, Rn;
            rot_lite(tr, R);
            rot_lite(trn, Rn);
            const double* Pc = P0 + (size_t)cur * 3 * a.stride;
            double* Pn = P0 + (size_t)(1 - cur) * 3 * a.stride;
            double accC[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, dummy[RF_NS];
            for (int j = tid; j < n; j += RF_THREADS) {
                double z0[3], z1[4], d[3];
                rf_obs(S, sp, idx[j], z0, z1);
                const double px = Pc[j], py = Pc[a.stride + j], pz = Pc[2 * a.stride + j];
                rf_point<true>(R, sp, z0, z1, px, py, pz, lam, dummy, dtr, d);
                const double d0 = d[0], d1 = d[1], d2 = d[2];
                const double nx = px + d0, ny = py + d1, nz = pz + d2;
                Pn[j] = nx; Pn[a.stride + j] = ny; Pn[2 * a.stride + j] = nz;
                rf_cost_diag(Rn, sp, z0, z1, nx, ny, nz, accC);
            }
            block_sum<7, RF_WAVES>(accC, red, tot);
        }
        const double Cn = tot[0];
        if (Cn < C) {
            ++acc_steps;
            rej = 0;
            lam = fmax(lam / 10.0, LM_LAMBDA_MIN);
            const bool stop = C - Cn <= LM_REL_TOL * C || Cn == 0.0 || acc_steps == LM_MAX_ACCEPT;
#pragma unroll
            for (int p = 0; p < 6; ++p) tr[p] = trn[p];
            cur = 1 - cur;
            C = Cn;
            if (tid < 6) dg[tid] = tot[1 + tid];   // read behind the next barrier
            __threadfence_block();   // the candidate points written above are the current ones from here on
            if (stop) break;
        } else {
            lam *= 10.0;
            if (++rej == LM_MAX_REJECT) break;
        }
    }
    if (status == 1) {
        // the final state without damping: S, s
        __syncthreads();
        {
            RotLite R;
            rot_lite(tr, R);
            const double* Pc = P0 + (size_t)cur * 3 * a.stride;
            double acc[RF_NS];
#pragma unroll
            for (int k = 0; k < RF_NS; ++k) acc[k] = 0.0;
            if (tid == 0) bad = 0;
            __syncthreads();
            for (int j = tid; j < n; j += RF_THREADS) {
                double z0[3], z1[4], dX[3];
                rf_obs(S, sp, idx[j], z0, z1);
                if (!rf_point<false>(R, sp, z0, z1, Pc[j], Pc[a.stride + j], Pc[2 * a.stride + j], 0.0, acc, zero6, dX)) bad = 1;
            }
            block_sum<RF_NS, RF_WAVES>(acc, red, tot);
        }
        bool fin = true;
#pragma unroll
        for (int k = 0; k < RF_NS; ++k) fin = fin && isfinite(tot[k]);
#pragma unroll
        for (int k = 0; k < 6; ++k) fin = fin && isfinite(dg[k]);
        double L[21], id[6];
        if (bad) status = -2;
        else if (!fin) status = -3;
        else if (!rf_chol6(tot, dg, 0.0, L, id)) status = -2;
        if (status == 1) {
            const double sigma2 = a.mode == 2 ? a.sigma2 : C / (4.0 * n - 6.0);
            double s[6], t[6];
#pragma unroll
            for (int p = 0; p < 6; ++p) s[p] = tot[21 + p];
            rf_fwd6(L, id, s, t);
            double ss = 0.0;
#pragma unroll
            for (int p = 0; p < 6; ++p) ss += t[p] * t[p];
            const double gap = sigma2 > 0.0 ? ss / sigma2 : 0.0;
            // S^-1 = L^-T L^-1: lanes 0..5 write the columns of L^-1, lanes 0..20 one entry of the upper triangle each
            if (tid < 6) {
                double e[6], x[6];
#pragma unroll
                for (int i = 0; i < 6; ++i) e[i] = i == tid ? 1.0 : 0.0;
                rf_fwd6(L, id, e, x);
#pragma unroll
                for (int i = 0; i < 6; ++i) Li[i * 6 + tid] = x[i];
            }
            __syncthreads();
            bool fin2 = isfinite(gap) && isfinite(sigma2);
#pragma unroll
            for (int p = 0; p < 6; ++p) fin2 = fin2 && isfinite(tr[p]);
            for (int e = 0; e < 36; ++e) fin2 = fin2 && isfinite(Li[e]);
            if (!fin2) status = -3;
            if (status == 1) {
                write_cov6(Li, sigma2, o->cov);
                if (tid < 6) o->tr[tid] = tr[tid];
                if (tid == 0) {
                    o->sigma2 = sigma2; o->cost0 = C0; o->cost = C; o->gap = gap;
                    o->iters = acc_steps; o->status = 1; o->n = n; o->_pad = 0;
                }
                // the refined points in half 0 (viso_batch_get_refined_points)
                if (cur == 1) {
                    __syncthreads();
                    for (int j = tid; j < n; j += RF_THREADS)
#pragma unroll
                        for (int c = 0; c < 3; ++c) P0[c * a.stride + j] = P0[(3 + c) * a.stride + j];
                }
                return;
            }
        }
    }
    rf_zero(o, tr_in, status, n);
}

int launch_motion_refine(hipStream_t s, const SolverItem* items_dev, int n_items, const SolverParamsDev& sp, int mode, double sigma,
                         double* pts, int* idx, size_t stride, viso_motion_refine* out) {
    if (n_items <= 0) return VISO_OK;
    RefineArgs a;
    a.items = items_dev; a.n_items = n_items; a.mode = mode; a.sigma2 = mode == 2 ? sigma * sigma : 0.0; a.sp = sp;
    a.pts = pts; a.idx = idx; a.stride = stride; a.out = out;
    hipLaunchKernelGGL(motion_refine_kernel, dim3((unsigned)n_items), dim3(RF_THREADS), 0, s, a);
    HIP_TRY(hipGetLastError());
    return VISO_OK;
}

// ---- the direct call: host pointers, default context (pose_call_stage, covariance.hip) --------------------------------------
extern "C" int viso_pose_refine(const double* X, const double* obs, int m, const double tr[6], const int32_t* inl, int n_inl,
                                const viso_param* param, int mode, double sigma_px, viso_motion_refine* out, double* Xout) {
    PoseCall pc;
    // extra: points [2][3][ld] | L' [ld]
    const size_t ld = (size_t)(m > 0 ? m : 1), oL = al256(sizeof(double) * 6 * ld);
    VISO_TRY(pose_call_stage("viso_pose_refine", X, obs, m, tr, inl, n_inl, param, mode, sigma_px, out, sizeof(viso_motion_refine),
                             oL + sizeof(int) * ld, &pc));
    VISO_TRY(launch_motion_refine(pc.dc.s, pc.item, 1, pc.sp, mode, sigma_px, reinterpret_cast<double*>(pc.extra),
                                  reinterpret_cast<int*>(pc.extra + oL), ld, reinterpret_cast<viso_motion_refine*>(pc.rec)));
    VISO_TRY(pc.dc.down(out, pc.rec, 1));
    VISO_TRY(pc.dc.wait());
    if (Xout) {   // the refined points, L' order: rows of n_inl doubles, the first out->n columns set when status is 1
        if (out->status == 1 && out->n > 0)
            for (int row = 0; row < 3; ++row)
                HIP_TRY(hipMemcpy(Xout + (size_t)row * (size_t)n_inl, pc.extra + sizeof(double) * (size_t)row * ld,
                                  sizeof(double) * (size_t)out->n, hipMemcpyDeviceToHost));
    }
    return VISO_OK;
}
