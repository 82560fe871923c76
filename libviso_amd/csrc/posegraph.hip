// posegraph.hip — the opt-in pose-graph optimisation (include/viso_hip.h, "pose graph"): Levenberg-Marquardt over
// SE(3) poses joined by relative-pose edges and priors, fp64 throughout.  The graphs of this library are one odometry chain, priors
// and a few long edges, and the solver is direct on that shape: the chain edges and the damping are a block-tridiagonal matrix T,
// the L long edges a term U U' of rank 6 L, so (T + U U') delta = -g is one block-tridiagonal Cholesky, sweeps with 6 L + 1
// right-hand sides and one dense Cholesky of order 6 L (Woodbury).  Every sum has a fixed order (edges at a node in edge-index
// order, reductions as fixed trees) and nothing is accumulated by a float atomic: the same arrays give the same bytes.
//
// What lies where on the device (one block a call; doubles unless said otherwise):
//   poses [2][n][12]            the current poses and the trial, first three rows
//   pieces [2][E] of PG_PIECE   per edge: B_i = J_i' C and B_j = J_j' C (6 x 6 each, Omega = C C'), w = C' r, and w'w / 2.  With them
//                               g_a = B_a w, H_ab = B_a B_b', and an edge's block of U at node a is B_a itself.
//   D, E [n][36], g, dH [n][6]  per node: the chain edges' diagonal block, the block (k + 1, k), the gradient, diag H of all edges
//   Li, F [n][36]               the factor: the inverse of the diagonal block's Cholesky factor, and the block (k + 1, k) of L
//   W [n][6][ncol]              the sweeps' right-hand sides and results: U's 6 L columns, then -g (ncol = 6 L + 1)
//   S [6L][6L + 1], d0, z [6L]  the capacitance matrix I + U' W with U' y as its last column, its diagonal as it was, the solution
//   delta [n][6], scal [8]      the step; the words the host reads (PG_S_*)
#include "solver_dev.h"
#include "alignmath.h"

#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#define PG_MAX_POSES 65536
#define PG_MAX_EDGES (1 << 20)
#define PG_MAX_LONG 256
#define PG_MAX_DOUBLES ((size_t)1 << 28)
#define PG_PIECE 79            // B_i | B_j | w | cost
#define PG_SERIES_THETA2 1e-2  // below it the coefficients are their series, five terms each
#define PG_PIVOT 1e-12
#define PG_NB 32               // the dense factor's block
#define PG_KC 32               // and the chunk of earlier columns it stages: c0 is a multiple of it, so every chunk is whole
static_assert(PG_NB % PG_KC == 0, "the dense factor's chunks are whole");
#define PG_S_COST 0
#define PG_S_COST_BAD 1
#define PG_S_STEP 2
#define PG_S_STEP_BAD 3
#define PG_S_CHAIN_FAIL 4
#define PG_S_DENSE_FAIL 5

struct PgGraph {
    int n, ne, nl, ncol, n_runs;
    const int* fixed;      // [n]
    const int* ij;         // [ne][2]
    const double* Z;       // [ne][12]
    const double* C;       // [ne][36] the lower Cholesky factor of Omega, zeros above the diagonal
    const int* node_ptr;   // [n + 1] a node's entries in node_ent, in edge-index order
    const int* node_ent;   // edge * 2 + side (0: the node is the edge's i, 1: its j)
    const int* long_edge;  // [nl] the long edges
    const int* long_ij;    // [nl][2] their end nodes, -1 where the end has no column (fixed)
    const int* runs;       // [n_runs][2] first node and one past the last of every run of T
};

struct PgCoef { double a, b, c1, c2, c3, cp; };

// a = sin t / t, b = (1 - cos t) / t^2, c1 = (t - sin t) / t^3, c2 = (t^2 + 2 cos t - 2) / (2 t^4), c3 = (2 t - 3 sin t + t cos t) / (2 t^5),
// cp = (1 - a / (2 b)) / t^2 at t^2 = th2 (the header's "Exp and Log")
__device__ __forceinline__ PgCoef pg_coef(double th2) {
    PgCoef k;
    if (th2 < PG_SERIES_THETA2) {
        const double x = th2;
        k.a = 1.0 - x * (1.0 / 6 - x * (1.0 / 120 - x * (1.0 / 5040 - x / 362880)));
        k.b = 1.0 / 2 - x * (1.0 / 24 - x * (1.0 / 720 - x * (1.0 / 40320 - x / 3628800)));
        k.c1 = 1.0 / 6 - x * (1.0 / 120 - x * (1.0 / 5040 - x * (1.0 / 362880 - x / 39916800)));
        k.c2 = 1.0 / 24 - x * (1.0 / 720 - x * (1.0 / 40320 - x * (1.0 / 3628800 - x / 479001600)));
        k.c3 = 1.0 / 120 - x * (2.0 / 5040 - x * (3.0 / 362880 - x * (4.0 / 39916800 - x * (5.0 / 6227020800.0))));
        k.cp = 1.0 / 12 + x * (1.0 / 720 + x * (1.0 / 30240 + x * (1.0 / 1209600 + x / 47900160)));
        return k;
    }
    const double t = sqrt(th2);
    double s, c;
    sincos(t, &s, &c);
    k.a = s / t;
    k.b = (1.0 - c) / th2;
    k.c1 = (t - s) / (th2 * t);
    k.c2 = (th2 + 2.0 * c - 2.0) / (2.0 * th2 * th2);
    k.c3 = (2.0 * t - 3.0 * s + t * c) / (2.0 * th2 * th2 * t);
    k.cp = (1.0 - k.a / (2.0 * k.b)) / th2;
    return k;
}

// 3 x 3 matrices in registers: every index is a compile-time constant once the loops are unrolled
struct M3 { double m[3][3]; };
__device__ __forceinline__ M3 m3_hat(const double v[3]) { return M3{{{0.0, -v[2], v[1]}, {v[2], 0.0, -v[0]}, {-v[1], v[0], 0.0}}}; }
__device__ __forceinline__ M3 m3_mul(const M3& a, const M3& b) {
    M3 r;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) r.m[i][j] = a.m[i][0] * b.m[0][j] + a.m[i][1] * b.m[1][j] + a.m[i][2] * b.m[2][j];
    return r;
}
__device__ __forceinline__ M3 m3_tmul(const M3& a, const M3& b) {   // a' b
    M3 r;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) r.m[i][j] = a.m[0][i] * b.m[0][j] + a.m[1][i] * b.m[1][j] + a.m[2][i] * b.m[2][j];
    return r;
}
__device__ __forceinline__ M3 m3_t(const M3& a) {
    M3 r;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) r.m[i][j] = a.m[j][i];
    return r;
}
// x a + y b + z c (pass 0.0 and any matrix for a term that is absent)
__device__ __forceinline__ M3 m3_lin(double x, const M3& a, double y, const M3& b, double z, const M3& c) {
    M3 r;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) r.m[i][j] = x * a.m[i][j] + y * b.m[i][j] + z * c.m[i][j];
    return r;
}
__device__ __forceinline__ void m3_tvec(const M3& a, const double v[3], double out[3]) {   // a' v
#pragma unroll
    for (int i = 0; i < 3; ++i) out[i] = a.m[0][i] * v[0] + a.m[1][i] * v[1] + a.m[2][i] * v[2];
}
__device__ __forceinline__ M3 m3_eye() { return M3{{{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}}}; }

__device__ __forceinline__ void pg_load_pose(const double* p12, M3& R, double t[3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) R.m[i][j] = p12[4 * i + j];
        t[i] = p12[4 * i + 3];
    }
}

// One thread per edge: r = Log(Z^-1 P_i^-1 P_j), J_j = J_r^-1(r), J_i = -J_r^-1(r) Ad(M^-1), and the edge's pieces.  The 6 x 6
// Jacobians are [[X, 0], [Y, X]] with 3 x 3 blocks, which stay in registers; the 6 x 6 products go column by column of C, read
// from memory, so that no array is indexed by a runtime value (no scratch).
__global__ __launch_bounds__(64) void pg_linearize_kernel(PgGraph G, const double* __restrict__ poses, double* __restrict__ pieces) {
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= G.ne) return;
    const int i = G.ij[2 * e], j = G.ij[2 * e + 1];
    M3 Ri = m3_eye(), Rj, Rz;
    double ti[3] = {0.0, 0.0, 0.0}, tj[3], tz[3];
    if (i >= 0) pg_load_pose(poses + 12 * (size_t)i, Ri, ti);
    pg_load_pose(poses + 12 * (size_t)j, Rj, tj);
    pg_load_pose(G.Z + 12 * (size_t)e, Rz, tz);
    // M = P_i^-1 P_j, D = Z^-1 M
    const M3 Rm = m3_tmul(Ri, Rj);
    double d[3] = {tj[0] - ti[0], tj[1] - ti[1], tj[2] - ti[2]}, tm[3], td[3];
    m3_tvec(Ri, d, tm);
    const M3 Rd = m3_tmul(Rz, Rm);
    d[0] = tm[0] - tz[0]; d[1] = tm[1] - tz[1]; d[2] = tm[2] - tz[2];
    m3_tvec(Rz, d, td);
    // r = Log(D)
    const double v[3] = {0.5 * (Rd.m[2][1] - Rd.m[1][2]), 0.5 * (Rd.m[0][2] - Rd.m[2][0]), 0.5 * (Rd.m[1][0] - Rd.m[0][1])};
    const double sn = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    const double theta = atan2(sn, 0.5 * (((Rd.m[0][0] + Rd.m[1][1]) + Rd.m[2][2]) - 1.0));
    const PgCoef k = pg_coef(theta * theta);
    double r[6];
    r[0] = v[0] / k.a; r[1] = v[1] / k.a; r[2] = v[2] / k.a;
    {
        const M3 K = m3_hat(r), K2 = m3_mul(K, K);
        const M3 Vi = m3_lin(1.0, m3_eye(), -0.5, K, k.cp, K2);
#pragma unroll
        for (int a = 0; a < 3; ++a) r[3 + a] = Vi.m[a][0] * td[0] + Vi.m[a][1] * td[1] + Vi.m[a][2] * td[2];
    }
    // J_r^-1(r) = [[A, 0], [-A Q A, A]], A = J_l,SO3(-phi)^-1, Q = Q(-rho, -phi)
    const double np_[3] = {-r[0], -r[1], -r[2]}, nr[3] = {-r[3], -r[4], -r[5]};
    const M3 P = m3_hat(np_), Rh = m3_hat(nr);
    const M3 A = m3_lin(1.0, m3_eye(), -0.5, P, k.cp, m3_mul(P, P));
    M3 Y;
    {
        const M3 PR = m3_mul(P, Rh), RP = m3_mul(Rh, P), PRP = m3_mul(PR, P);
        const M3 q1 = m3_lin(1.0, PR, 1.0, RP, 1.0, PRP);
        const M3 q2 = m3_lin(1.0, m3_mul(P, PR), 1.0, m3_mul(RP, P), -3.0, PRP);
        const M3 q3 = m3_lin(1.0, m3_mul(PRP, P), 1.0, m3_mul(P, PRP), 0.0, PRP);
        const M3 Q = m3_lin(1.0, m3_lin(0.5, Rh, k.c1, q1, k.c2, q2), k.c3, q3, 0.0, q3);
        Y = m3_lin(-1.0, m3_mul(m3_mul(A, Q), A), 0.0, A, 0.0, A);
    }
    // J_i = -J_j Ad(M^-1), M^-1 = (Rn, tn) = (Rm', -Rm' tm): X_i = -A Rn, Y_i = -(Y Rn + A [tn]x Rn)
    const M3 Rn = m3_t(Rm);
    double tn[3];
    m3_tvec(Rm, tm, tn);
    tn[0] = -tn[0]; tn[1] = -tn[1]; tn[2] = -tn[2];
    const M3 ARn = m3_mul(A, Rn);
    const M3 Xi = m3_lin(-1.0, ARn, 0.0, A, 0.0, A);
    const M3 Yi = m3_lin(-1.0, m3_mul(Y, Rn), -1.0, m3_mul(A, m3_mul(m3_hat(tn), Rn)), 0.0, A);
    // B_a = J_a' C: rows 0..2 are X' C_top + Y' C_bottom, rows 3..5 are X' C_bottom; w = C' r
    double* out = pieces + (size_t)PG_PIECE * e;
    const double* C = G.C + 36 * (size_t)e;
    double cost = 0.0;
#pragma unroll 1
    for (int c = 0; c < 6; ++c) {
        double col[6];
#pragma unroll
        for (int q = 0; q < 6; ++q) col[q] = C[6 * q + c];
        double w = 0.0;
#pragma unroll
        for (int q = 0; q < 6; ++q) w += col[q] * r[q];
        out[72 + c] = w;
        cost += w * w;
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            const double ji = (Xi.m[0][p] * col[0] + Xi.m[1][p] * col[1] + Xi.m[2][p] * col[2]) +
                              (Yi.m[0][p] * col[3] + Yi.m[1][p] * col[4] + Yi.m[2][p] * col[5]);
            const double ji2 = Xi.m[0][p] * col[3] + Xi.m[1][p] * col[4] + Xi.m[2][p] * col[5];
            const double jj = (A.m[0][p] * col[0] + A.m[1][p] * col[1] + A.m[2][p] * col[2]) +
                              (Y.m[0][p] * col[3] + Y.m[1][p] * col[4] + Y.m[2][p] * col[5]);
            const double jj2 = A.m[0][p] * col[3] + A.m[1][p] * col[4] + A.m[2][p] * col[5];
            out[6 * p + c] = i >= 0 ? ji : 0.0;
            out[6 * (p + 3) + c] = i >= 0 ? ji2 : 0.0;
            out[36 + 6 * p + c] = jj;
            out[36 + 6 * (p + 3) + c] = jj2;
        }
    }
    out[78] = 0.5 * cost;
}

// One thread per (node, entry) of 84: the chain edges' diagonal block D (36), the block E = (k + 1, k) (36), the gradient (6) and
// diag H over all edges (6), each a walk of the node's edge list in edge-index order.  A fixed node's entries are zeros.
__global__ __launch_bounds__(256) void pg_assemble_kernel(PgGraph G, const double* __restrict__ pieces, double* __restrict__ D,
                                                          double* __restrict__ E, double* __restrict__ g, double* __restrict__ dH) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)G.n * 84) return;
    const int k = (int)(t / 84), ent = (int)(t % 84);
    const int kind = ent < 36 ? 0 : ent < 72 ? 1 : ent < 78 ? 2 : 3;
    const int x = kind == 0 ? ent : kind == 1 ? ent - 36 : kind == 2 ? ent - 72 : ent - 78;
    const int p = kind < 2 ? x / 6 : x, q = kind < 2 ? x % 6 : 0;
    double s = 0.0;
    if (!G.fixed[k]) {
        for (int it = G.node_ptr[k]; it < G.node_ptr[k + 1]; ++it) {
            const int en = G.node_ent[it], e = en >> 1, side = en & 1;
            const int other = G.ij[2 * e + (side ^ 1)];
            const bool chain = other < 0 || other - k == 1 || k - other == 1;
            const double* B = pieces + (size_t)PG_PIECE * e + 36 * side;
            if (kind == 0) {
                if (chain)
                    for (int c = 0; c < 6; ++c) s += B[6 * p + c] * B[6 * q + c];
            } else if (kind == 1) {
                if (other == k + 1 && !G.fixed[other]) {
                    const double* Bo = pieces + (size_t)PG_PIECE * e + 36 * (side ^ 1);
                    for (int c = 0; c < 6; ++c) s += Bo[6 * p + c] * B[6 * q + c];
                }
            } else if (kind == 2) {
                const double* w = pieces + (size_t)PG_PIECE * e + 72;
                for (int c = 0; c < 6; ++c) s += B[6 * p + c] * w[c];
            } else {
                for (int c = 0; c < 6; ++c) s += B[6 * p + c] * B[6 * p + c];
            }
        }
    }
    if (kind == 0) D[36 * (size_t)k + x] = s;
    else if (kind == 1) E[36 * (size_t)k + x] = s;
    else if (kind == 2) g[6 * (size_t)k + x] = s;
    else dH[6 * (size_t)k + x] = s;
}

// One workgroup: the cost, the edges' halves summed by thread in a fixed stride and then by block_sum's tree.
__global__ __launch_bounds__(256) void pg_cost_kernel(const double* __restrict__ pieces, int ne, double* __restrict__ scal) {
    __shared__ double red[4], tot[1];
    double acc[1] = {0.0};
    for (int e = threadIdx.x; e < ne; e += 256) acc[0] += pieces[(size_t)PG_PIECE * e + 78];
    block_sum<1, 4>(acc, red, tot);
    if (threadIdx.x == 0) {
        scal[PG_S_COST] = tot[0];
        scal[PG_S_COST_BAD] = isfinite(tot[0]) ? 0.0 : 1.0;
    }
}

// The block-tridiagonal Cholesky of T = chain blocks + lambda diag H, one wave per run, serial along the run; the 36 entries of
// a block are spread over the lanes.  Per node: S = D + lambda diag(dH) - F_prev F_prev', its Cholesky factor in LDS (a pivot must
// exceed PG_PIVOT times T's diagonal entry), the factor's inverse Li by the lanes 0..5 (a column each), F = E Li'.  A node's D, dH
// and E are asked for one node ahead, so that their way from memory runs beside the node before: what is left is the chain of
// barriers, LDS round trips, square roots and divisions of one 6 x 6 factorisation, the latency floor of the method.
__global__ __launch_bounds__(64) void pg_chain_factor_kernel(PgGraph G, const double* __restrict__ D, const double* __restrict__ dH,
                                                             const double* __restrict__ E, double lambda, double* __restrict__ Li,
                                                             double* __restrict__ F, double* __restrict__ scal) {
    __shared__ double a[36], f[36], li[36], od[6];
    const int run = blockIdx.x;
    if (run >= G.n_runs) return;
    const int k0 = G.runs[2 * run], k1 = G.runs[2 * run + 1];
    const int e = threadIdx.x, p = e / 6, q = e % 6;
    const bool act = e < 36;
    double dn = act ? D[36 * (size_t)k0 + e] : 0.0, hn = act && p == q ? dH[6 * (size_t)k0 + p] : 0.0;
    for (int k = k0; k < k1; ++k) {
        const bool more = k + 1 < k1;
        double s = dn, er[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (p == q) s += lambda * hn;
        if (act && more) {   // the next node's block, and this node's E for the end of the step
            dn = D[36 * (size_t)(k + 1) + e];
            if (p == q) hn = dH[6 * (size_t)(k + 1) + p];
#pragma unroll
            for (int c = 0; c < 6; ++c) er[c] = E[36 * (size_t)k + 6 * p + c];
        }
        if (act) {
            if (p == q) od[p] = s;
            if (k > k0)
                for (int c = 0; c < 6; ++c) s -= f[6 * p + c] * f[6 * q + c];
            a[e] = s;
        }
        __syncthreads();
#pragma unroll 1
        for (int c = 0; c < 6; ++c) {
            const double d = a[7 * c];
            if (!(d > PG_PIVOT * od[c])) {   // the same value in every lane: the wave leaves as one
                if (e == 0) scal[PG_S_CHAIN_FAIL] = 1.0;
                return;
            }
            __syncthreads();
            const double r = sqrt(d);
            if (act && q == c && p >= c) a[e] = p == c ? r : a[e] / r;
            __syncthreads();
            if (act && q > c && p >= q) a[e] -= a[6 * p + c] * a[6 * q + c];
            __syncthreads();
        }
        if (e < 6) {   // column e of L^-1: rows above it are zero
            for (int rr = 0; rr < 6; ++rr) {
                double x = rr == e ? 1.0 : 0.0;
                for (int m = e; m < rr; ++m) x -= a[6 * rr + m] * li[6 * m + e];
                li[6 * rr + e] = rr < e ? 0.0 : x / a[7 * rr];
            }
        }
        __syncthreads();
        if (act) {
            double v = 0.0;
#pragma unroll
            for (int c = 0; c < 6; ++c) v += er[c] * li[6 * q + c];   // er is zero at the run's last node
            f[e] = v;
            F[36 * (size_t)k + e] = v;
            Li[36 * (size_t)k + e] = li[e];
        }
        __syncthreads();
    }
}

// The sweeps, one lane per right-hand-side column, the column's 6-vector in registers.  Forward u_k = Li_k (b_k - F_{k-1} u_{k-1}),
// backward x_k = Li_k' (u_k - F_k' x_{k+1}).  b: column 6 l + c is the long edge l's block column c at its two end nodes, the last
// column is -g.  A step's Li and F (72 doubles, the same for every lane) are fetched by the wave one node ahead, a lane a double,
// and handed over through LDS, two buffers in turn; the lane's own operand (g forward, W backward) is asked for one node ahead
// too.  Lanes past the last column stay for the fetches and store nothing.  (Fetching eight nodes ahead, with W staged through
// LDS as well, was measured and is slower, 13.2 ms against 11.0 ms for 4541 nodes: the step is not waiting for memory any more.)
__global__ __launch_bounds__(64) void pg_chain_solve_kernel(PgGraph G, const double* __restrict__ pieces, const double* __restrict__ g,
                                                            const double* __restrict__ Li, const double* __restrict__ F,
                                                            double* __restrict__ W) {
    __shared__ double mat[2][72];   // Li | F of the step
    const int run = blockIdx.x, lane = threadIdx.x;
    if (run >= G.n_runs) return;
    const int col = blockIdx.y * 64 + lane;
    const bool on = col < G.ncol;
    const int k0 = G.runs[2 * run], k1 = G.runs[2 * run + 1];
    const size_t nc = (size_t)G.ncol;
    const bool last = col == G.ncol - 1;
    const int l = !on || last ? 0 : col / 6, c = col % 6;
    int ni = -1, nj = -1;
    const double* Bi = pieces;
    if (on && !last) {
        ni = G.long_ij[2 * l]; nj = G.long_ij[2 * l + 1];
        Bi = pieces + (size_t)PG_PIECE * G.long_edge[l];
    }
    // the lane's share of Li_k | F_kf: double `lane` of the 72, and for the lanes 0..7 double 64 + lane
    auto fetch = [&](int k, int kf, double& r0, double& r1) {
        r0 = lane < 36 ? Li[36 * (size_t)k + lane] : F[36 * (size_t)kf + (lane - 36)];
        r1 = lane < 8 ? F[36 * (size_t)kf + 28 + lane] : 0.0;
    };
    auto put = [&](int buf, double r0, double r1) {
        mat[buf][lane] = r0;
        if (lane < 8) mat[buf][64 + lane] = r1;
    };
    double r0, r1, nx[6], u[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    fetch(k0, k0, r0, r1);
    put(0, r0, r1);
#pragma unroll
    for (int p = 0; p < 6; ++p) nx[p] = last ? g[6 * (size_t)k0 + p] : 0.0;
    __syncthreads();
    for (int k = k0; k < k1; ++k) {
        const int buf = (k - k0) & 1;
        const double* L = mat[buf];
        const double* Fp = mat[buf] + 36;   // F_{k-1}
        const bool more = k + 1 < k1;
        double cur[6], b[6];
#pragma unroll
        for (int p = 0; p < 6; ++p) cur[p] = nx[p];
        if (more) {
            fetch(k + 1, k, r0, r1);
            if (last) {
#pragma unroll
                for (int p = 0; p < 6; ++p) nx[p] = g[6 * (size_t)(k + 1) + p];
            }
        }
#pragma unroll
        for (int p = 0; p < 6; ++p) {
            double v = 0.0;
            if (last) v = -cur[p];
            else if (k == ni) v = Bi[6 * p + c];
            else if (k == nj) v = Bi[36 + 6 * p + c];
            if (k > k0) {
#pragma unroll
                for (int m = 0; m < 6; ++m) v -= Fp[6 * p + m] * u[m];
            }
            b[p] = v;
        }
#pragma unroll
        for (int p = 0; p < 6; ++p) {
            double v = 0.0;
#pragma unroll
            for (int m = 0; m < 6; ++m) v += L[6 * p + m] * b[m];
            cur[p] = v;
        }
#pragma unroll
        for (int p = 0; p < 6; ++p) {
            u[p] = cur[p];
            if (on) W[((size_t)k * 6 + p) * nc + col] = u[p];
        }
        if (more) put(buf ^ 1, r0, r1);
        __syncthreads();
    }
    fetch(k1 - 1, k1 - 1, r0, r1);
    put(0, r0, r1);
#pragma unroll
    for (int p = 0; p < 6; ++p) nx[p] = on ? W[((size_t)(k1 - 1) * 6 + p) * nc + col] : 0.0;
    __syncthreads();
    for (int k = k1 - 1; k >= k0; --k) {
        const int buf = (k1 - 1 - k) & 1;
        const double* L = mat[buf];
        const double* Fk = mat[buf] + 36;   // F_k
        const bool more = k > k0;
        double cur[6], b[6];
#pragma unroll
        for (int p = 0; p < 6; ++p) cur[p] = nx[p];
        if (more) {
            fetch(k - 1, k - 1, r0, r1);
            if (on) {
#pragma unroll
                for (int p = 0; p < 6; ++p) nx[p] = W[((size_t)(k - 1) * 6 + p) * nc + col];
            }
        }
#pragma unroll
        for (int p = 0; p < 6; ++p) {
            double v = cur[p];
            if (k + 1 < k1) {
#pragma unroll
                for (int m = 0; m < 6; ++m) v -= Fk[6 * m + p] * u[m];
            }
            b[p] = v;
        }
#pragma unroll
        for (int p = 0; p < 6; ++p) {
            double v = 0.0;
#pragma unroll
            for (int m = 0; m < 6; ++m) v += L[6 * m + p] * b[m];
            cur[p] = v;
        }
#pragma unroll
        for (int p = 0; p < 6; ++p) {
            u[p] = cur[p];
            if (on) W[((size_t)k * 6 + p) * nc + col] = u[p];
        }
        if (more) put(buf ^ 1, r0, r1);
        __syncthreads();
    }
}

// S = I + U' W, with U' y as column 6 L: one thread per entry; W is read at the long edges' end nodes only.
__global__ __launch_bounds__(256) void pg_capacitance_kernel(PgGraph G, const double* __restrict__ pieces, const double* __restrict__ W,
                                                             double* __restrict__ S, double* __restrict__ d0) {
    const int m = 6 * G.nl;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)m * (m + 1)) return;
    const int row = (int)(t / (m + 1)), col = (int)(t % (m + 1));
    const int l = row / 6, c = row % 6;
    const double* B = pieces + (size_t)PG_PIECE * G.long_edge[l];
    double s = row == col ? 1.0 : 0.0;
    for (int side = 0; side < 2; ++side) {
        const int a = G.long_ij[2 * l + side];
        if (a < 0) continue;
        for (int p = 0; p < 6; ++p) s += B[36 * side + 6 * p + c] * W[((size_t)a * 6 + p) * (size_t)G.ncol + col];
    }
    S[(size_t)row * (m + 1) + col] = s;
    if (row == col) d0[row] = s;
}

// One workgroup: the Cholesky factor of S (order m <= 1536, row stride m + 1, lower triangle, in place in global memory) by
// block columns of PG_NB, left-looking: the block column takes the earlier columns' update with the block's own rows staged in LDS
// in chunks of PG_KC columns (whole ones), the diagonal block is factored in LDS, the rows below it are solved a thread each.  Then
// L y = v and L' z = y with the vector in LDS, one column (row) a step.  A pivot must exceed PG_PIVOT times S's diagonal entry.
__global__ __launch_bounds__(1024) void pg_dense_kernel(double* __restrict__ S, int m, const double* __restrict__ d0, double* __restrict__ z,
                                                        double* __restrict__ scal) {
    __shared__ double Ld[PG_NB][PG_NB + 1], Lj[PG_NB][PG_KC + 1], v[6 * PG_MAX_LONG], y[6 * PG_MAX_LONG];
    const int tid = threadIdx.x;
    const size_t ld = (size_t)m + 1;
    for (int c0 = 0; c0 < m; c0 += PG_NB) {
        const int nb = m - c0 < PG_NB ? m - c0 : PG_NB;
        for (int kc = 0; kc < c0; kc += PG_KC) {
            __syncthreads();
            for (int x = tid; x < PG_NB * PG_KC; x += 1024) {
                const int jj = x / PG_KC, kk = x % PG_KC;
                Lj[jj][kk] = jj < nb ? S[(size_t)(c0 + jj) * ld + kc + kk] : 0.0;
            }
            __syncthreads();
            for (int x = tid; x < (m - c0) * PG_NB; x += 1024) {
                const int i = c0 + x / PG_NB, jj = x % PG_NB;
                if (jj < nb && c0 + jj <= i) {
                    const double* Si = S + (size_t)i * ld + kc;
                    double acc = 0.0;
#pragma unroll
                    for (int kk = 0; kk < PG_KC; ++kk) acc += Si[kk] * Lj[jj][kk];   // a fixed count: the row's loads go out together
                    S[(size_t)i * ld + c0 + jj] -= acc;
                }
            }
        }
        __syncthreads();
        {
            const int a = tid / PG_NB, b = tid % PG_NB;
            Ld[a][b] = a < nb && b <= a ? S[(size_t)(c0 + a) * ld + c0 + b] : 0.0;
        }
        __syncthreads();
#pragma unroll 1
        for (int c = 0; c < nb; ++c) {
            const double d = Ld[c][c];
            if (!(d > PG_PIVOT * d0[c0 + c])) {   // the same value in every thread
                if (tid == 0) scal[PG_S_DENSE_FAIL] = 1.0;
                return;
            }
            __syncthreads();
            const double s = sqrt(d);
            if (tid < nb && tid >= c) Ld[tid][c] = tid == c ? s : Ld[tid][c] / s;
            __syncthreads();
            const int a = tid / PG_NB, b = tid % PG_NB;
            if (a < nb && b > c && b <= a) Ld[a][b] -= Ld[a][c] * Ld[b][c];
            __syncthreads();
        }
        {
            const int a = tid / PG_NB, b = tid % PG_NB;
            if (a < nb && b <= a) S[(size_t)(c0 + a) * ld + c0 + b] = Ld[a][b];
        }
        for (int i = c0 + nb + tid; i < m; i += 1024) {
            double* Si = S + (size_t)i * ld + c0;
            for (int b = 0; b < nb; ++b) {
                double x = Si[b];
                for (int t = 0; t < b; ++t) x -= Si[t] * Ld[b][t];
                Si[b] = x / Ld[b][b];
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < m; i += 1024) v[i] = S[(size_t)i * ld + m];
    __syncthreads();
    for (int c = 0; c < m; ++c) {
        const double yc = v[c] / S[(size_t)c * ld + c];
        if (tid == 0) y[c] = yc;
        for (int i = c + 1 + tid; i < m; i += 1024) v[i] -= S[(size_t)i * ld + c] * yc;
        __syncthreads();
    }
    for (int c = m - 1; c >= 0; --c) {
        const double zc = y[c] / S[(size_t)c * ld + c];
        if (tid == 0) z[c] = zc;
        __syncthreads();   // every thread has read y[c]
        for (int i = tid; i < c; i += 1024) y[i] -= S[(size_t)c * ld + i] * zc;
        __syncthreads();
    }
}

// delta = y - W z: one wave per row (node, component), the lanes stride the columns, the lanes' sums go through the wave's tree.
__global__ __launch_bounds__(256) void pg_delta_kernel(PgGraph G, const double* __restrict__ W, const double* __restrict__ z,
                                                       double* __restrict__ delta) {
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= (long long)G.n * 6) return;   // a whole wave
    const int m = G.ncol - 1;
    const double* Wr = W + (size_t)row * (size_t)G.ncol;
    double acc = 0.0;
    for (int c = lane; c < m; c += 64) acc += Wr[c] * z[c];
    acc = wave_sum_to_lane63(acc);
    if (lane == 63) delta[row] = G.fixed[row / 6] ? 0.0 : Wr[m] - acc;
}

// One workgroup: max |delta| and whether every component is finite.
__global__ __launch_bounds__(256) void pg_stepmax_kernel(const double* __restrict__ delta, int n6, double* __restrict__ scal) {
    __shared__ double mx[256], bad[256];
    double a = 0.0, b = 0.0;
    for (int i = threadIdx.x; i < n6; i += 256) {
        const double v = fabs(delta[i]);
        if (!isfinite(v)) b = 1.0;
        else if (v > a) a = v;
    }
    mx[threadIdx.x] = a; bad[threadIdx.x] = b;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            if (mx[threadIdx.x + s] > mx[threadIdx.x]) mx[threadIdx.x] = mx[threadIdx.x + s];
            if (bad[threadIdx.x + s] > 0.0) bad[threadIdx.x] = 1.0;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) { scal[PG_S_STEP] = mx[0]; scal[PG_S_STEP_BAD] = bad[0]; }
}

// The trial poses P_k Exp(delta_k), one thread per node; a fixed node's rows are copied.
__global__ __launch_bounds__(64) void pg_update_kernel(PgGraph G, const double* __restrict__ poses, const double* __restrict__ delta,
                                                       double* __restrict__ out) {
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= G.n) return;
    const double* P = poses + 12 * (size_t)k;
    double* O = out + 12 * (size_t)k;
    if (G.fixed[k]) {
        for (int x = 0; x < 12; ++x) O[x] = P[x];
        return;
    }
    const double* dk = delta + 6 * (size_t)k;
    const double phi[3] = {dk[0], dk[1], dk[2]}, rho[3] = {dk[3], dk[4], dk[5]};
    const PgCoef c = pg_coef((phi[0] * phi[0] + phi[1] * phi[1]) + phi[2] * phi[2]);
    const M3 K = m3_hat(phi), K2 = m3_mul(K, K);
    const M3 dR = m3_lin(1.0, m3_eye(), c.a, K, c.b, K2), V = m3_lin(1.0, m3_eye(), c.b, K, c.c1, K2);
    M3 R;
    double t[3], dt[3];
    pg_load_pose(P, R, t);
#pragma unroll
    for (int a = 0; a < 3; ++a) dt[a] = V.m[a][0] * rho[0] + V.m[a][1] * rho[1] + V.m[a][2] * rho[2];
    const M3 Rn = m3_mul(R, dR);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int b = 0; b < 3; ++b) O[4 * a + b] = Rn.m[a][b];
        O[4 * a + 3] = (R.m[a][0] * dt[0] + R.m[a][1] * dt[1] + R.m[a][2] * dt[2]) + t[a];
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
namespace {

struct PgHost {           // a checked graph, as the kernels want it
    int n = 0, ne = 0, nl = 0;
    std::vector<int> fixed, ij, node_ptr, node_ent, long_edge, long_ij, runs;
    std::vector<double> poses12, Z12, C;
};

inline bool pg_chain_edge(int i, int j) { return i < 0 || i - j == 1 || j - i == 1; }

// The checks that need no device, in the header's order; on VISO_OK h is filled.
int pg_check(const char* where, int n_poses, const double* poses, const int32_t* fixed, int n_edges, const int32_t* edge_ij, const double* edge_Z,
             const double* edge_info, PgHost* h) {
    if (n_poses < 1 || n_edges < 1 || !poses || !edge_ij || !edge_Z || !edge_info) {
        viso_set_error("%s: bad argument (n_poses >= 1, n_edges >= 1, non-null poses and edges)", where);
        return VISO_ERR_ARG;
    }
    if (n_poses > PG_MAX_POSES || n_edges > PG_MAX_EDGES) {
        viso_set_error("%s: %d poses and %d edges are beyond the %d poses and %d edges of this build", where, n_poses, n_edges, PG_MAX_POSES, PG_MAX_EDGES);
        return VISO_ERR_UNSUPPORTED;
    }
    const int n = n_poses, ne = n_edges;
    int nl = 0;
    for (int e = 0; e < ne; ++e) {
        const int i = edge_ij[2 * e], j = edge_ij[2 * e + 1];
        if (j < 0 || j >= n || i < -1 || i >= n || i == j) {
            viso_set_error("%s: edge %d joins %d and %d (j in 0 .. n_poses-1, i in -1 .. n_poses-1, i != j)", where, e, i, j);
            return VISO_ERR_ARG;
        }
        if (!pg_chain_edge(i, j)) ++nl;
    }
    if (nl > PG_MAX_LONG) {
        viso_set_error("%s: %d long edges, this build takes %d", where, nl, PG_MAX_LONG);
        return VISO_ERR_UNSUPPORTED;
    }
    {
        const size_t m = 6 * (size_t)nl;
        const size_t doubles = 24 * (size_t)n + 2 * PG_PIECE * (size_t)ne + 162 * (size_t)n + 6 * (size_t)n * (m + 1) + m * (m + 1) + 2 * m + 8 +
                               48 * (size_t)ne;
        if (doubles > PG_MAX_DOUBLES) {
            viso_set_error("%s: a workspace of %zu doubles (6 n_poses (6 L + 1) and the blocks), this build takes 2^28", where, doubles);
            return VISO_ERR_UNSUPPORTED;
        }
    }
    for (size_t x = 0; x < 16 * (size_t)n; ++x)
        if ((x & 15) < 12 && !isfinite(poses[x])) { viso_set_error("%s: pose %zu is not finite", where, x / 16); return VISO_ERR_ARG; }
    h->n = n; h->ne = ne; h->nl = nl;
    h->fixed.assign(n, 0);
    if (fixed) for (int k = 0; k < n; ++k) h->fixed[k] = fixed[k] != 0;
    h->ij.assign(edge_ij, edge_ij + 2 * (size_t)ne);
    h->poses12.resize(12 * (size_t)n);
    for (int k = 0; k < n; ++k) memcpy(&h->poses12[12 * (size_t)k], poses + 16 * (size_t)k, 12 * sizeof(double));
    h->Z12.resize(12 * (size_t)ne);
    h->C.assign(36 * (size_t)ne, 0.0);
    for (int e = 0; e < ne; ++e) {
        const double* Zs = edge_Z + 16 * (size_t)e;
        const double* Om = edge_info + 36 * (size_t)e;
        bool ok = true;
        for (int x = 0; x < 12; ++x) ok = ok && isfinite(Zs[x]);
        for (int x = 0; x < 36; ++x) ok = ok && isfinite(Om[x]);
        if (!ok) { viso_set_error("%s: edge %d has a Z or an information matrix that is not finite", where, e); return VISO_ERR_ARG; }
        memcpy(&h->Z12[12 * (size_t)e], Zs, 12 * sizeof(double));
        double sym[36];
        for (int p = 0; p < 6; ++p)
            for (int q = 0; q < 6; ++q) sym[6 * p + q] = Om[6 * (p > q ? p : q) + (p > q ? q : p)];   // the lower triangle is read
        if (!align_cholesky(sym, &h->C[36 * (size_t)e])) {
            viso_set_error("%s: the information matrix of edge %d is not positive definite (a pivot of its Cholesky factor is not > 1e-12 x its diagonal entry)",
                           where, e);
            return VISO_ERR_ARG;
        }
        for (int p = 0; p < 6; ++p)
            for (int q = p + 1; q < 6; ++q) h->C[36 * (size_t)e + 6 * p + q] = 0.0;
    }
    // the nodes' edge lists (edge-index order), the long edges
    h->node_ptr.assign((size_t)n + 1, 0);
    for (int e = 0; e < ne; ++e)
        for (int s = 0; s < 2; ++s) if (h->ij[2 * e + s] >= 0) ++h->node_ptr[h->ij[2 * e + s] + 1];
    for (int k = 0; k < n; ++k) h->node_ptr[k + 1] += h->node_ptr[k];
    h->node_ent.resize((size_t)h->node_ptr[n] + 1);
    {
        std::vector<int> at(h->node_ptr.begin(), h->node_ptr.end() - 1);
        for (int e = 0; e < ne; ++e)
            for (int s = 0; s < 2; ++s) if (h->ij[2 * e + s] >= 0) h->node_ent[at[h->ij[2 * e + s]]++] = 2 * e + s;
    }
    for (int e = 0; e < ne; ++e) {
        const int i = h->ij[2 * e], j = h->ij[2 * e + 1];
        if (pg_chain_edge(i, j)) continue;
        h->long_edge.push_back(e);
        h->long_ij.push_back(h->fixed[i] ? -1 : i);
        h->long_ij.push_back(h->fixed[j] ? -1 : j);
    }
    // T's runs: free nodes joined by chain edges; each needs an anchor (a prior, or a chain edge to a fixed node)
    std::vector<char> link((size_t)n, 0), anchor((size_t)n, 0), any((size_t)n, 0);   // link[k]: a chain edge joins k and k + 1
    for (int e = 0; e < ne; ++e) {
        const int i = h->ij[2 * e], j = h->ij[2 * e + 1];
        any[j] = 1;
        if (i >= 0) any[i] = 1;
        if (!pg_chain_edge(i, j)) continue;
        if (i < 0) { anchor[j] = 1; continue; }
        if (h->fixed[i] && !h->fixed[j]) anchor[j] = 1;
        else if (h->fixed[j] && !h->fixed[i]) anchor[i] = 1;
        else if (!h->fixed[i] && !h->fixed[j]) link[i < j ? i : j] = 1;
    }
    for (int k = 0; k < n;) {
        if (h->fixed[k]) { ++k; continue; }
        int k1 = k;
        bool anchored = anchor[k] != 0;
        while (k1 + 1 < n && !h->fixed[k1 + 1] && link[k1]) { ++k1; anchored = anchored || anchor[k1]; }
        if (k1 == k && !any[k]) { viso_set_error("%s: node %d is free and has no edge", where, k); return VISO_ERR_ARG; }
        if (!anchored) {
            viso_set_error("%s: the run of nodes that starts at node %d (%d nodes joined by chain edges) has neither a fixed neighbour nor a prior: "
                           "the chain is not definite on its own (bridge a gap with a weak edge, or fix a node)", where, k, k1 - k + 1);
            return VISO_ERR_ARG;
        }
        h->runs.push_back(k);
        h->runs.push_back(k1 + 1);
        k = k1 + 1;
    }
    return VISO_OK;
}

struct PgBlock {          // the call's one device allocation, freed behind a wait for the stream
    hipStream_t s; char* d = nullptr;
    explicit PgBlock(hipStream_t s_) : s(s_) {}
    ~PgBlock() { if (d) { (void)hipStreamSynchronize(s); (void)hipFree(d); } }
    PgBlock(const PgBlock&) = delete;
};

struct PgDev {            // where everything lies
    PgGraph G;
    double *poses[2], *pieces[2], *D, *E, *g, *dH, *Li, *F, *W, *S, *d0, *z, *delta, *scal;
};

struct PgLayout { size_t off = 0; size_t take(size_t bytes) { const size_t o = off; off = al256(off + bytes); return o; } };

// the graph onto the device and the workspace behind it
int pg_stage(const char* where, viso_ctx* c, const PgHost& h, PgBlock* blk, PgDev* dv, std::vector<char>* stage) {
    const size_t n = h.n, ne = h.ne, nl = h.nl, m = 6 * nl, ncol = m + 1, n_runs = h.runs.size() / 2;
    PgLayout lay;
    // staged part (copied from the host in one piece)
    const size_t o_fixed = lay.take(4 * n), o_ij = lay.take(8 * ne), o_Z = lay.take(96 * ne), o_C = lay.take(288 * ne),
                 o_ptr = lay.take(4 * (n + 1)), o_ent = lay.take(4 * h.node_ent.size()), o_le = lay.take(4 * (nl + 1)),
                 o_lij = lay.take(8 * (nl + 1)), o_runs = lay.take(8 * (n_runs + 1)), o_p0 = lay.take(96 * n);
    const size_t staged = lay.off;
    const size_t o_p1 = lay.take(96 * n), o_pc0 = lay.take(8 * PG_PIECE * ne), o_pc1 = lay.take(8 * PG_PIECE * ne), o_D = lay.take(288 * n),
                 o_E = lay.take(288 * n), o_g = lay.take(48 * n), o_dH = lay.take(48 * n), o_Li = lay.take(288 * n), o_F = lay.take(288 * n),
                 o_W = lay.take(48 * n * ncol), o_S = lay.take(8 * (m * (m + 1) + 1)), o_d0 = lay.take(8 * (m + 1)), o_z = lay.take(8 * (m + 1)),
                 o_delta = lay.take(48 * n), o_scal = lay.take(64);
    HIP_TRY(hipSetDevice(c->device));
    if (hipMalloc((void**)&blk->d, lay.off) != hipSuccess) {
        (void)hipGetLastError();
        blk->d = nullptr;
        viso_set_error("%s: cannot allocate the %zu-byte workspace", where, lay.off);
        return VISO_ERR_NOMEM;
    }
    stage->assign(staged, 0);
    char* hs = stage->data();
    memcpy(hs + o_fixed, h.fixed.data(), 4 * n);
    memcpy(hs + o_ij, h.ij.data(), 8 * ne);
    memcpy(hs + o_Z, h.Z12.data(), 96 * ne);
    memcpy(hs + o_C, h.C.data(), 288 * ne);
    memcpy(hs + o_ptr, h.node_ptr.data(), 4 * (n + 1));
    memcpy(hs + o_ent, h.node_ent.data(), 4 * h.node_ent.size());
    if (nl) { memcpy(hs + o_le, h.long_edge.data(), 4 * nl); memcpy(hs + o_lij, h.long_ij.data(), 8 * nl); }
    if (n_runs) memcpy(hs + o_runs, h.runs.data(), 8 * n_runs);
    memcpy(hs + o_p0, h.poses12.data(), 96 * n);
    hipStream_t s = c->stream;
    HIP_TRY(hipMemcpyAsync(blk->d, hs, staged, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(blk->d + staged, 0, lay.off - staged, s));   // W's rows of fixed nodes, F and Li outside the runs, scal
    char* d = blk->d;
    dv->G = PgGraph{(int)n, (int)ne, (int)nl, (int)ncol, (int)n_runs, (const int*)(d + o_fixed), (const int*)(d + o_ij), (const double*)(d + o_Z),
                    (const double*)(d + o_C), (const int*)(d + o_ptr), (const int*)(d + o_ent), (const int*)(d + o_le), (const int*)(d + o_lij),
                    (const int*)(d + o_runs)};
    dv->poses[0] = (double*)(d + o_p0); dv->poses[1] = (double*)(d + o_p1);
    dv->pieces[0] = (double*)(d + o_pc0); dv->pieces[1] = (double*)(d + o_pc1);
    dv->D = (double*)(d + o_D); dv->E = (double*)(d + o_E); dv->g = (double*)(d + o_g); dv->dH = (double*)(d + o_dH);
    dv->Li = (double*)(d + o_Li); dv->F = (double*)(d + o_F); dv->W = (double*)(d + o_W); dv->S = (double*)(d + o_S);
    dv->d0 = (double*)(d + o_d0); dv->z = (double*)(d + o_z); dv->delta = (double*)(d + o_delta); dv->scal = (double*)(d + o_scal);
    return VISO_OK;
}

void pg_launch_linearize(const PgDev& dv, int which, hipStream_t s) {   // the pieces and the cost of poses[which]
    hipLaunchKernelGGL(pg_linearize_kernel, dim3((dv.G.ne + 63) / 64), dim3(64), 0, s, dv.G, dv.poses[which], dv.pieces[which]);
    hipLaunchKernelGGL(pg_cost_kernel, dim3(1), dim3(256), 0, s, dv.pieces[which], dv.G.ne, dv.scal);
}
void pg_launch_assemble(const PgDev& dv, int which, hipStream_t s) {
    const long long t = (long long)dv.G.n * 84;
    hipLaunchKernelGGL(pg_assemble_kernel, dim3((unsigned)((t + 255) / 256)), dim3(256), 0, s, dv.G, dv.pieces[which], dv.D, dv.E, dv.g, dv.dH);
}
void pg_launch_step(const PgDev& dv, int which, double lambda, hipStream_t s) {   // delta and max |delta| from the assembled system
    const PgGraph& G = dv.G;
    if (G.n_runs) {
        hipLaunchKernelGGL(pg_chain_factor_kernel, dim3(G.n_runs), dim3(64), 0, s, G, dv.D, dv.dH, dv.E, lambda, dv.Li, dv.F, dv.scal);
        hipLaunchKernelGGL(pg_chain_solve_kernel, dim3(G.n_runs, (G.ncol + 63) / 64), dim3(64), 0, s, G, dv.pieces[which], dv.g, dv.Li, dv.F, dv.W);
    }
    if (G.nl) {
        const long long m = 6 * (long long)G.nl, t = m * (m + 1);
        hipLaunchKernelGGL(pg_capacitance_kernel, dim3((unsigned)((t + 255) / 256)), dim3(256), 0, s, G, dv.pieces[which], dv.W, dv.S, dv.d0);
        hipLaunchKernelGGL(pg_dense_kernel, dim3(1), dim3(1024), 0, s, dv.S, (int)m, dv.d0, dv.z, dv.scal);
    }
    hipLaunchKernelGGL(pg_delta_kernel, dim3((6 * G.n + 3) / 4), dim3(256), 0, s, G, dv.W, dv.z, dv.delta);
    hipLaunchKernelGGL(pg_stepmax_kernel, dim3(1), dim3(256), 0, s, dv.delta, 6 * G.n, dv.scal);
}

}   // namespace

extern "C" int viso_pose_graph_linearize(viso_ctx* ctx_or_null, int n_poses, const double* poses, const int32_t* fixed_or_null, int n_edges,
                                         const int32_t* edge_ij, const double* edge_Z, const double* edge_info, double lambda, double* cost_out,
                                         double* grad_out, double* step_out) {
    const char* where = "viso_pose_graph_linearize";
    if (!cost_out || !grad_out || !(lambda >= 0.0) || !isfinite(lambda)) {
        viso_set_error("%s: bad argument (non-null cost_out and grad_out, a finite lambda >= 0)", where);
        return VISO_ERR_ARG;
    }
    PgHost h;
    VISO_TRY(pg_check(where, n_poses, poses, fixed_or_null, n_edges, edge_ij, edge_Z, edge_info, &h));
    viso_ctx* c;
    VISO_TRY(ctx_resolve(where, ctx_or_null, &c));
    std::vector<char> stage;   // (before the block: the copy reads it until the block's wait)
    PgBlock blk(c->stream);
    PgDev dv;
    VISO_TRY(pg_stage(where, c, h, &blk, &dv, &stage));
    hipStream_t s = c->stream;
    pg_launch_linearize(dv, 0, s);
    pg_launch_assemble(dv, 0, s);
    if (step_out) pg_launch_step(dv, 0, lambda, s);
    HIP_TRY(hipGetLastError());
    double scal[8];
    HIP_TRY(hipMemcpyAsync(scal, dv.scal, sizeof(scal), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(grad_out, dv.g, 48 * (size_t)h.n, hipMemcpyDeviceToHost, s));
    if (step_out) HIP_TRY(hipMemcpyAsync(step_out, dv.delta, 48 * (size_t)h.n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    *cost_out = scal[PG_S_COST];
    if (step_out && (scal[PG_S_CHAIN_FAIL] != 0.0 || scal[PG_S_DENSE_FAIL] != 0.0)) {
        viso_set_error("%s: the system is not positive definite at lambda %g (a pivot of the %s factor is not > 1e-12 x its diagonal entry)", where,
                       lambda, scal[PG_S_CHAIN_FAIL] != 0.0 ? "chain" : "dense");
        return VISO_ERR_ARG;
    }
    return VISO_OK;
}

extern "C" int viso_pose_graph_optimize(viso_ctx* ctx_or_null, int n_poses, const double* poses, const int32_t* fixed_or_null, int n_edges,
                                        const int32_t* edge_ij, const double* edge_Z, const double* edge_info, int max_iters, double eps_step,
                                        double* poses_out, double report[8], double* trace_or_null, int trace_cap) {
    const char* where = "viso_pose_graph_optimize";
    if (!poses_out || !report || max_iters < 1 || max_iters > 200 || !(eps_step >= 0.0) || !isfinite(eps_step) || trace_cap < 0 ||
        (trace_cap > 0 && !trace_or_null)) {
        viso_set_error("%s: bad argument (non-null poses_out and report, max_iters in 1..200, a finite eps_step >= 0, a trace for trace_cap > 0)", where);
        return VISO_ERR_ARG;
    }
    PgHost h;
    VISO_TRY(pg_check(where, n_poses, poses, fixed_or_null, n_edges, edge_ij, edge_Z, edge_info, &h));
    viso_ctx* c;
    VISO_TRY(ctx_resolve(where, ctx_or_null, &c));
    std::vector<char> stage;
    PgBlock blk(c->stream);
    PgDev dv;
    VISO_TRY(pg_stage(where, c, h, &blk, &dv, &stage));
    hipStream_t s = c->stream;
    double scal[8];
    auto read_scal = [&]() -> int {
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(scal, dv.scal, sizeof(scal), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        return VISO_OK;
    };
    int cur = 0, status = 2, iters = 0, n_rejected = 0, n_trace = 0;
    double lambda = LM_LAMBDA0, F = 0.0, F0 = 0.0, last_step = 0.0;
    pg_launch_linearize(dv, cur, s);
    pg_launch_assemble(dv, cur, s);
    VISO_TRY(read_scal());
    F = F0 = scal[PG_S_COST];
    if (scal[PG_S_COST_BAD] != 0.0) status = -3;
    auto note = [&](double Ft, double step, bool accepted) {
        if (n_trace < trace_cap) {
            double* t = trace_or_null + 5 * (size_t)n_trace;
            t[0] = F; t[1] = Ft; t[2] = lambda; t[3] = step; t[4] = accepted ? 1.0 : 0.0;
        }
        ++n_trace;
    };
    while (status == 2 && iters < max_iters) {
        ++iters;
        // the solve, the trial poses and their linearise are queued as one; the host reads the words behind them
        pg_launch_step(dv, cur, lambda, s);
        hipLaunchKernelGGL(pg_update_kernel, dim3((h.n + 63) / 64), dim3(64), 0, s, dv.G, dv.poses[cur], dv.delta, dv.poses[cur ^ 1]);
        pg_launch_linearize(dv, cur ^ 1, s);
        VISO_TRY(read_scal());
        if (scal[PG_S_CHAIN_FAIL] != 0.0 || scal[PG_S_DENSE_FAIL] != 0.0) { status = -2; break; }
        if (scal[PG_S_STEP_BAD] != 0.0) { status = -3; break; }
        last_step = scal[PG_S_STEP];
        if (last_step <= eps_step) { note(F, last_step, false); status = 1; break; }
        const double Ft = scal[PG_S_COST];
        if (scal[PG_S_COST_BAD] != 0.0) { status = -3; break; }
        const bool accepted = Ft <= F * (1.0 + 0x1p-40);
        note(Ft, last_step, accepted);
        if (accepted) {
            cur ^= 1;
            F = Ft;
            pg_launch_assemble(dv, cur, s);
            lambda = lambda * 0.1 > LM_LAMBDA_MIN ? lambda * 0.1 : LM_LAMBDA_MIN;
        } else {
            lambda *= 10.0;
            ++n_rejected;
        }
    }
    std::vector<double> out12(12 * (size_t)h.n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out12.data(), dv.poses[cur], 96 * (size_t)h.n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    memcpy(poses_out, poses, 128 * (size_t)h.n);   // fixed nodes, and every node on a failure: as given, byte for byte
    if (status > 0)
        for (int k = 0; k < h.n; ++k)
            if (!h.fixed[k]) {
                memcpy(poses_out + 16 * (size_t)k, &out12[12 * (size_t)k], 96);
                poses_out[16 * (size_t)k + 12] = poses_out[16 * (size_t)k + 13] = poses_out[16 * (size_t)k + 14] = 0.0;
                poses_out[16 * (size_t)k + 15] = 1.0;
            }
    report[VISO_PG_STATUS] = status; report[VISO_PG_ITERS] = iters; report[VISO_PG_COST_INITIAL] = F0; report[VISO_PG_COST_FINAL] = F;
    report[VISO_PG_LAMBDA] = lambda; report[VISO_PG_LAST_STEP] = last_step; report[VISO_PG_N_LONG] = h.nl; report[VISO_PG_N_REJECTED] = n_rejected;
    return VISO_OK;
}
