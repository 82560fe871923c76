// hostmath.cpp — once-per-call host arithmetic of the boundary: parameter
// constructors, tr2mat, the pose chain step, F_from_P and the RANSAC sample
// stream.  A handful of flops each; nothing here is worth a kernel launch.
#include "solver_dev.h"
#include "alignmath.h"

#include <float.h>
#include <math.h>
#include <string.h>

extern "C" void viso_match_params_stereo(viso_match_params* mp, const double F[9]) {
    memset(mp, 0, sizeof(*mp));       // MatchParams(Mat F), reference src/viso.cpp:62-71
    mp->enforce_epipolar = 1;
    mp->sampson_thresh = 1;
    mp->enforce_2nd_best = 0;
    mp->ratio_2nd_best = .8;
    mp->max_neighbors = 200;
    mp->radius = 80;
    if (F) memcpy(mp->F, F, 9 * sizeof(double));
}

extern "C" void viso_match_params_temporal(viso_match_params* mp) {
    memset(mp, 0, sizeof(*mp));       // MatchParams(), reference src/viso.cpp:72-74
    mp->enforce_epipolar = 0;
    mp->enforce_2nd_best = 1;
    mp->ratio_2nd_best = .9;
    mp->max_neighbors = 250;
    mp->radius = 80;
}

extern "C" void viso_param_default(viso_param* p) {
    memset(p, 0, sizeof(*p));         // param(), reference src/viso.h:60
    p->ransac_iter = 50;
    p->inlier_threshold = 2;
    p->save_debug = 1;
    p->thresh = 1e-4;
}

// tr2mat, reference src/viso.cpp:109-133
extern "C" void viso_tr2mat(const double tr[6], double T[16]) {
    const double rx = tr[0], ry = tr[1], rz = tr[2], tx = tr[3], ty = tr[4], tz = tr[5];
    const double sx = sin(rx), cx = cos(rx), sy = sin(ry), cy = cos(ry), sz = sin(rz), cz = cos(rz);
    T[0] = +cy * cz;                 T[1] = -cy * sz;                 T[2] = +sy;       T[3] = tx;
    T[4] = +sx * sy * cz + cx * sz;  T[5] = -sx * sy * sz + cx * cz;  T[6] = -sx * cy;  T[7] = ty;
    T[8] = -cx * sy * cz + sx * sz;  T[9] = +cx * sy * sz + sx * cz;  T[10] = +cx * cy; T[11] = tz;
    T[12] = 0; T[13] = 0; T[14] = 0; T[15] = 1;
}

// pose * inv(tr2mat(tr)), reference src/viso.cpp:1316-1319.  tr2mat is rigid, so
// the inverse is [R' | -R' t] (cv::Mat::inv's LU result agrees to round-off).
extern "C" void viso_pose_update(const double pose[16], const double tr[6], double out[16]) {
    double T[16], Ti[16], r[16];
    viso_tr2mat(tr, T);
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) Ti[4 * i + j] = T[4 * j + i];
        Ti[4 * i + 3] = -(T[0 * 4 + i] * T[3] + T[1 * 4 + i] * T[7] + T[2 * 4 + i] * T[11]);
    }
    Ti[12] = Ti[13] = Ti[14] = 0; Ti[15] = 1;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double s = 0;
            for (int k = 0; k < 4; ++k) s += pose[4 * i + k] * Ti[4 * k + j];
            r[4 * i + j] = s;
        }
    memcpy(out, r, sizeof(r));
}

static double det3(const double a[3], const double b[3], const double c[3]) {
    return a[0] * (b[1] * c[2] - b[2] * c[1]) - a[1] * (b[0] * c[2] - b[2] * c[0]) +
           a[2] * (b[0] * c[1] - b[1] * c[0]);
}

// 4x4 determinant by cofactor expansion along the first row
static double det4rows(const double* r0, const double* r1, const double* r2, const double* r3) {
    double d = 0;
    for (int c = 0; c < 4; ++c) {
        double a[3], b[3], e[3];
        int k = 0;
        for (int j = 0; j < 4; ++j) {
            if (j == c) continue;
            a[k] = r1[j]; b[k] = r2[j]; e[k] = r3[j];
            ++k;
        }
        const double minor = det3(a, b, e);
        d += ((c & 1) ? -1.0 : 1.0) * r0[c] * minor;
    }
    return d;
}

// F_from_P<double>, reference src/mvg.h:41-66, then src/viso.cpp:1177-1180.
extern "C" void viso_F_from_P(const double P1[12], const double P2[12], double F[9]) {
    static const int pick[3][2] = {{1, 2}, {2, 0}, {0, 1}};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            F[3 * i + j] = det4rows(P1 + 4 * pick[j][0], P1 + 4 * pick[j][1],
                                    P2 + 4 * pick[i][0], P2 + 4 * pick[i][1]);
    if (F[8] > DBL_MIN) {
        const double s = F[8];
        for (int k = 0; k < 9; ++k) F[k] /= s;
    }
}

// randomsample(3, m, .) with a reproducible stream, reference src/viso.cpp:87-107
extern "C" void viso_ransac_samples(uint64_t seed, uint64_t frame, int iters, int m, int32_t* out) {
    for (int h = 0; h < iters; ++h) {
        int s3[3];
        viso_sample3(seed, frame, h, m, s3);
        out[3 * h] = s3[0]; out[3 * h + 1] = s3[1]; out[3 * h + 2] = s3[2];
    }
}

// Propagation of the per-frame motion covariances along hostmath.chain_poses' list (include/viso_hip.h, "motion covariance";
// DESIGN.md 5.8).  Right perturbation P = P^ Exp(xi), xi = (phi, rho): P_k = P_{k-1} inv(T_k) gives
// S_k = Ad(T_k) S_{k-1} Ad(T_k)' + G_k cov_k G_k'.  G_k = d Log(T_k inv(T(tr))) / d tr at tr_k: with dR = [w]x R (w_rx = e_x,
// w_ry = Rx e_y, w_rz = Rx Ry e_z, the columns of W), T_k inv(T(tr)) = [I - [w]x | -dt - [t]x w] to first order, so
// G = [[-W, 0], [-[t]x W, -I]].
static void mat6_mul(const double* a, const double* b, double* out, bool bt) {   // out = a b (bt: a b')
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) {
            double s = 0;
            for (int k = 0; k < 6; ++k) s += a[6 * i + k] * (bt ? b[6 * j + k] : b[6 * k + j]);
            out[6 * i + j] = s;
        }
}

// Ad(T) and G of one motion tr (the comment above): shared by the chain and by viso_motion_edge.  T (or null): tr2mat(tr).
static void motion_ad_g(const double* tr, double* Ad, double* G, double* T_out = nullptr) {
    double T[16];
    viso_tr2mat(tr, T);
    if (T_out) memcpy(T_out, T, sizeof(T));
    const double R[3][3] = {{T[0], T[1], T[2]}, {T[4], T[5], T[6]}, {T[8], T[9], T[10]}};
    const double tv[3] = {T[3], T[7], T[11]};
    const double tx[3][3] = {{0, -tv[2], tv[1]}, {tv[2], 0, -tv[0]}, {-tv[1], tv[0], 0}};
    const double sx = sin(tr[0]), cx = cos(tr[0]), sy = sin(tr[1]), cy = cos(tr[1]);
    const double W[3][3] = {{1, 0, sy}, {0, cx, -sx * cy}, {0, sx, cx * cy}};   // columns w_rx, w_ry, w_rz
    memset(Ad, 0, 36 * sizeof(double));
    memset(G, 0, 36 * sizeof(double));
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double tR = 0, tW = 0;
            for (int l = 0; l < 3; ++l) { tR += tx[i][l] * R[l][j]; tW += tx[i][l] * W[l][j]; }
            Ad[6 * i + j] = R[i][j];
            Ad[6 * (i + 3) + j + 3] = R[i][j];
            Ad[6 * (i + 3) + j] = tR;
            G[6 * i + j] = -W[i][j];
            G[6 * (i + 3) + j] = -tW;
            G[6 * (i + 3) + j + 3] = i == j ? -1.0 : 0.0;
        }
}

extern "C" int viso_chain_covariances(const double* tr, const int32_t* ok, const viso_motion_cov* cov, int n, double* pose_cov36,
                                      int32_t* valid, int* n_out) {
    if (n < 0 || !pose_cov36 || !valid || !n_out || (n > 0 && (!tr || !ok || !cov))) {
        viso_set_error("viso_chain_covariances: bad argument");
        return VISO_ERR_ARG;
    }
    double S[36] = {0}, Ad[36], G[36], tmp[36], a[36], c[36];
    memset(pose_cov36, 0, sizeof(double) * 36);
    valid[0] = 1;
    bool live = true;
    int k = 0;
    for (int t = 0; t < n; ++t) {
        if (!ok[t]) continue;
        ++k;
        live = live && cov[t].status == 1;
        double* out = pose_cov36 + 36 * (size_t)k;
        valid[k] = live ? 1 : 0;
        if (!live) { memset(out, 0, sizeof(double) * 36); continue; }
        motion_ad_g(tr + 6 * (size_t)t, Ad, G);
        mat6_mul(Ad, S, tmp, false);
        mat6_mul(tmp, Ad, a, true);
        mat6_mul(G, cov[t].cov, tmp, false);
        mat6_mul(tmp, G, c, true);
        for (int i = 0; i < 36; ++i) S[i] = a[i] + c[i];
        for (int i = 0; i < 6; ++i)   // exactly symmetric
            for (int j = 0; j < i; ++j) S[6 * i + j] = S[6 * j + i] = 0.5 * (S[6 * i + j] + S[6 * j + i]);
        memcpy(out, S, sizeof(S));
    }
    *n_out = k + 1;
    return VISO_OK;
}

// The pose-graph edge of one solved frame (include/viso_hip.h, "pose graph"): chain_poses steps P_k = P_{k-1} inv(T), so the edge
// between the two measures Z = inv(T), and its error in the tangent of the right perturbation has the covariance G cov G'.
extern "C" int viso_motion_edge(const double tr[6], const double cov36[36], double Z[16], double info[36]) {
    bool ok = tr && cov36 && Z && info;
    for (int i = 0; ok && i < 6; ++i) ok = isfinite(tr[i]);
    for (int i = 0; ok && i < 36; ++i) ok = isfinite(cov36[i]);
    if (!ok) { viso_set_error("viso_motion_edge: bad argument (non-null pointers, finite tr and cov)"); return VISO_ERR_ARG; }
    double T[16], Ad[36], G[36], tmp[36], S[36], L[36], Li[36];
    motion_ad_g(tr, Ad, G, T);
    mat6_mul(G, cov36, tmp, false);
    mat6_mul(tmp, G, S, true);
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < i; ++j) S[6 * i + j] = S[6 * j + i] = 0.5 * (S[6 * i + j] + S[6 * j + i]);
    if (!align_cholesky(S, L)) {
        viso_set_error("viso_motion_edge: G cov G' is not positive definite (a pivot of its Cholesky factor is not > 1e-12 x its diagonal entry)");
        return VISO_ERR_ARG;
    }
    memset(Li, 0, sizeof(Li));   // L^-1, column by column; info = L^-T L^-1
    for (int c = 0; c < 6; ++c)
        for (int r = c; r < 6; ++r) {
            double x = r == c ? 1.0 : 0.0;
            for (int m = c; m < r; ++m) x -= L[6 * r + m] * Li[6 * m + c];
            Li[6 * r + c] = x / L[6 * r + r];
        }
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) {
            double v = 0;
            for (int k = (i > j ? i : j); k < 6; ++k) v += Li[6 * k + i] * Li[6 * k + j];
            info[6 * i + j] = v;
        }
    for (int i = 0; i < 3; ++i) {   // inv(T) = [R' | -R' t]
        for (int j = 0; j < 3; ++j) Z[4 * i + j] = T[4 * j + i];
        Z[4 * i + 3] = -(T[0 * 4 + i] * T[3] + T[1 * 4 + i] * T[7] + T[2 * 4 + i] * T[11]);
    }
    Z[12] = Z[13] = Z[14] = 0; Z[15] = 1;
    return VISO_OK;
}
