// alignmath.h — the host arithmetic of the frame-to-model alignment (include/viso_hip.h, "TSDF align"; alignmath.cpp): the 6 x 6
// solve, the increment of a pose and the loop around the linearise, which its caller (tsdf_align.hip) passes in; for both kinds of
// linearise, the plain one and the one with the photometric row ("TSDF photometric align").
#ifndef VISO_ALIGNMATH_H_
#define VISO_ALIGNMATH_H_
#include "common.h"

#include <functional>

// One linearise of every frame f with active[f] != 0 at poses[f] ([n][16]) into out[f]; < 0: a VISO_ERR_*, which ends the loop.
using AlignLinearize = std::function<int(const double* poses, const unsigned long long* active, viso_tsdf_normal* out)>;

// Steps a..f and the final linearise for n frames, each on its own; every round linearises the frames that are not finished in
// one call.  guesses: [n][16], or null: the identity for all.  trace (or null): frame 0's linearises, at most trace_cap of them.
int align_run(const viso_tsdf_align_params& p, int n, const double* guesses, const AlignLinearize& linearize, viso_tsdf_alignment* records,
              viso_tsdf_align_step* trace, int trace_cap);

// The same machine on the combined sums of the photometric alignment ("TSDF photometric align"): min_pixels against n_used, the
// covariance's divisor with n_photo_used, the two costs from p; the trace's entries carry the whole linearise.
using AlignLinearizeGray = std::function<int(const double* poses, const unsigned long long* active, viso_tsdf_normal_gray* out)>;
int align_run_gray(const viso_tsdf_align_gray_params& p, int n, const double* guesses, const AlignLinearizeGray& linearize,
                   viso_tsdf_alignment_gray* records, viso_tsdf_align_gray_step* trace, int trace_cap);

// H = L L' (step c): false when a pivot is not greater than 1e-12 times its diagonal entry.  L: lower triangle, row-major [6][6].
bool align_cholesky(const double H[36], double L[36]);
void align_solve(const double L[36], const double r[6], double x[6]);   // L L' x = r
void align_increment(double T[16], const double xi[6]);                 // step e: T <- T D(xi), xi = (v, omega)
#endif /* VISO_ALIGNMATH_H_ */
