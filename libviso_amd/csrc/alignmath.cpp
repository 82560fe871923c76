// alignmath.cpp — the host arithmetic of the frame-to-model alignment (include/viso_hip.h, "TSDF align", steps a..f): on the 28
// integers of a linearise, a 6 x 6 Cholesky solve, the increment of the pose and the loop's bookkeeping.  A few hundred flops an
// iteration; the kernel is tsdf_align.hip's.  Every operand order here is the header's, so that tests/align_ref.py follows a
// device trace step by step.  The photometric alignment ("TSDF photometric align") runs the same machine on the combined sums.
#include "alignmath.h"

#include <math.h>
#include <string.h>

#include <vector>

bool align_cholesky(const double H[36], double L[36]) {
    memset(L, 0, 36 * sizeof(double));
    for (int j = 0; j < 6; ++j) {
        double d = H[6 * j + j];
        for (int k = 0; k < j; ++k) d -= L[6 * j + k] * L[6 * j + k];
        if (!(d > 1e-12 * H[6 * j + j])) return false;   // false for a NaN
        L[6 * j + j] = sqrt(d);
        for (int i = j + 1; i < 6; ++i) {
            double v = H[6 * i + j];
            for (int k = 0; k < j; ++k) v -= L[6 * i + k] * L[6 * j + k];
            L[6 * i + j] = v / L[6 * j + j];
        }
    }
    return true;
}

void align_solve(const double L[36], const double r[6], double x[6]) {
    double y[6];
    for (int i = 0; i < 6; ++i) {
        double v = r[i];
        for (int k = 0; k < i; ++k) v -= L[6 * i + k] * y[k];
        y[i] = v / L[6 * i + i];
    }
    for (int i = 5; i >= 0; --i) {
        double v = y[i];
        for (int k = i + 1; k < 6; ++k) v -= L[6 * k + i] * x[k];
        x[i] = v / L[6 * i + i];
    }
}

void align_increment(double T[16], const double xi[6]) {
    const double* v = xi;
    const double* w = xi + 3;
    const double theta2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2], theta = sqrt(theta2);
    double A, B;
    if (theta < 1e-8) { A = 1.0 - theta2 / 6.0; B = 0.5 - theta2 / 24.0; }
    else { A = sin(theta) / theta; B = (1.0 - cos(theta)) / theta2; }
    const double K[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
    double D[12];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) D[4 * i + j] = ((i == j ? 1.0 : 0.0) + A * K[3 * i + j]) + B * (w[i] * w[j] - (i == j ? theta2 : 0.0));
        D[4 * i + 3] = v[i];
    }
    for (int i = 0; i < 3; ++i) {
        const double t0 = T[4 * i], t1 = T[4 * i + 1], t2 = T[4 * i + 2], t3 = T[4 * i + 3];
        for (int j = 0; j < 4; ++j) {
            const double r = (t0 * D[j] + t1 * D[4 + j]) + t2 * D[8 + j];
            T[4 * i + j] = j == 3 ? r + t3 : r;
        }
    }
}

namespace {
// steps a..c on a linearise: H (both triangles), b, C, and the factor L.  0, or the status -1 / -2
int align_system(const viso_tsdf_align_params& p, const viso_tsdf_normal& nm, double H[36], double b[6], double* C, double L[36]) {
    int at = 0;
    for (int i = 0; i < 7; ++i) {
        for (int j = i; j < 7; ++j, ++at) {
            const double v = (double)nm.n[at] / 65536.0;
            if (j < 6) { H[6 * i + j] = v; H[6 * j + i] = v; }
            else if (i < 6) b[i] = v;
            else *C = v;
        }
    }
    if (nm.n_used < (uint64_t)p.min_pixels) return -1;
    return align_cholesky(H, L) ? 0 : -2;
}

struct AlignFrame {
    double T[16];
    int iters, status;    // status 0: iterating
    bool final_pending, done;
};

template <class K>
void align_fail(typename K::Record* rec, const double guess[16], int status) {
    memset(rec, 0, sizeof(*rec));
    memcpy(K::base(*rec).pose, guess, 16 * sizeof(double));
    K::base(*rec).status = status;
}

}   // namespace

// Steps a..f and the final linearise for n frames, on the sums of whichever kind (the gray kind's N holds both rows' products).
template <class K>
int align_run(const typename K::Params& params, int n, const double* guesses, const AlignLinearize<K>& linearize, typename K::Record* records,
              typename K::Step* trace, int trace_cap) {
    const viso_tsdf_align_params& p = K::geo(params);
    const double lambda = K::lambda(params);
    static const double eye[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    std::vector<AlignFrame> fr((size_t)n);
    std::vector<double> poses((size_t)n * 16), guess((size_t)n * 16);
    std::vector<unsigned long long> active((size_t)n);
    std::vector<typename K::Normal> normals((size_t)n);
    for (int f = 0; f < n; ++f) {
        memcpy(&guess[(size_t)f * 16], guesses ? guesses + (size_t)f * 16 : eye, 16 * sizeof(double));
        memcpy(fr[f].T, &guess[(size_t)f * 16], 12 * sizeof(double));
        memcpy(fr[f].T + 12, eye + 12, 4 * sizeof(double));
        fr[f].iters = 0; fr[f].status = 0; fr[f].final_pending = false; fr[f].done = false;
    }
    int n_trace = 0;
    for (;;) {
        int left = 0;
        for (int f = 0; f < n; ++f) {
            active[f] = fr[f].done ? 0ull : 1ull;
            left += fr[f].done ? 0 : 1;
            memcpy(&poses[(size_t)f * 16], fr[f].T, 16 * sizeof(double));
        }
        if (!left) break;
        VISO_TRY(linearize(poses.data(), active.data(), normals.data()));
        for (int f = 0; f < n; ++f) {
            AlignFrame& a = fr[f];
            if (a.done) continue;
            const viso_tsdf_normal& nm = K::geo(normals[f]);
            if (f == 0 && trace && n_trace < trace_cap) {
                memcpy(trace[n_trace].pose, a.T, 16 * sizeof(double));
                trace[n_trace].normal = normals[f];
                ++n_trace;
            }
            double H[36], b[6], C = 0.0, L[36];
            const int bad = align_system(p, nm, H, b, &C, L);
            if (bad) { align_fail<K>(&records[f], &guess[(size_t)f * 16], bad); a.done = true; continue; }
            if (a.final_pending) {
                memset(&records[f], 0, sizeof(records[f]));
                viso_tsdf_alignment& rec = K::base(records[f]);
                memcpy(rec.pose, a.T, 16 * sizeof(double));
                const double n_used = (double)nm.n_used;
                const uint64_t rows = nm.n_used + K::photo_rows(normals[f]);
                const double dof = rows > 7 ? (double)(rows - 6) : 1.0;
                rec.cost = sqrt(C / n_used);
                const double sigma2 = C / dof;
                for (int j = 0; j < 6; ++j) {
                    double unit[6] = {0, 0, 0, 0, 0, 0}, col[6];
                    unit[j] = 1.0;
                    align_solve(L, unit, col);
                    for (int i = 0; i < 6; ++i) rec.cov[6 * i + j] = sigma2 * col[i];
                }
                rec.n_used = nm.n_used; rec.iters = a.iters; rec.status = a.status;
                K::finish(records[f], normals[f], C, lambda);
                a.done = true;
                continue;
            }
            double x[6], xi[6];
            align_solve(L, b, x);
            bool finite = true;
            for (int i = 0; i < 6; ++i) { xi[i] = -x[i]; finite = finite && isfinite(xi[i]); }
            if (!finite) { align_fail<K>(&records[f], &guess[(size_t)f * 16], -3); a.done = true; continue; }
            align_increment(a.T, xi);
            a.iters += 1;
            const double nv = sqrt((xi[0] * xi[0] + xi[1] * xi[1]) + xi[2] * xi[2]), nw = sqrt((xi[3] * xi[3] + xi[4] * xi[4]) + xi[5] * xi[5]);
            if (nw <= p.eps_rot && nv <= p.eps_trans) { a.status = 1; a.final_pending = true; }
            else if (a.iters >= p.max_iters) { a.status = 2; a.final_pending = true; }
        }
    }
    return VISO_OK;
}

template int align_run<AlignPlain>(const viso_tsdf_align_params&, int, const double*, const AlignLinearize<AlignPlain>&, viso_tsdf_alignment*,
                                   viso_tsdf_align_step*, int);
template int align_run<AlignGray>(const viso_tsdf_align_gray_params&, int, const double*, const AlignLinearize<AlignGray>&, viso_tsdf_alignment_gray*,
                                  viso_tsdf_align_gray_step*, int);
