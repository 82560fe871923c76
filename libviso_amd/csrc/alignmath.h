// alignmath.h — the host arithmetic of the frame-to-model alignment (include/viso_hip.h, "TSDF align"; alignmath.cpp): the 6 x 6
// solve, the increment of a pose and the loop around the linearise, which its caller (tsdf_align.hip) passes in; for both kinds of
// linearise, the plain one and the one with the photometric row ("TSDF photometric align").
#ifndef VISO_ALIGNMATH_H_
#define VISO_ALIGNMATH_H_
#include "common.h"

#include <math.h>

#include <functional>

struct TsdfAlignArgs;
struct TsdfGrayAlignArgs;

// The two kinds of alignment as the loop (alignmath.cpp) and the launches (tsdf_align.hip) see them: the parameters, the
// linearise's sums and how many 64-bit words they are, the record, the trace's entry; where the geometric parameters, the counters
// of steps 1..9 and the plain record lie in them; the photometric weight and rows; what the final linearise adds to a record; the
// kernel's arguments and its launch (tsdf_align.hip's).
struct AlignPlain {
    using Params = viso_tsdf_align_params; using Normal = viso_tsdf_normal; using Record = viso_tsdf_alignment; using Step = viso_tsdf_align_step;
    using Args = TsdfAlignArgs;
    static constexpr size_t words = sizeof(Normal) / sizeof(unsigned long long);
    static const viso_tsdf_align_params& geo(const Params& p) { return p; }
    static double lambda(const Params&) { return 0.0; }
    static const viso_tsdf_normal& geo(const Normal& nm) { return nm; }
    static viso_tsdf_alignment& base(Record& r) { return r; }
    static uint64_t photo_rows(const Normal&) { return 0; }
    static void finish(Record&, const Normal&, double, double) {}
    static void launch(const Args& g, dim3 grid, hipStream_t s);
};
struct AlignGray {
    using Params = viso_tsdf_align_gray_params; using Normal = viso_tsdf_normal_gray; using Record = viso_tsdf_alignment_gray;
    using Step = viso_tsdf_align_gray_step; using Args = TsdfGrayAlignArgs;
    static constexpr size_t words = sizeof(Normal) / sizeof(unsigned long long);
    static const viso_tsdf_align_params& geo(const Params& p) { return p.geo; }
    static double lambda(const Params& p) { return p.photo_weight; }
    static const viso_tsdf_normal& geo(const Normal& nm) { return nm.normal; }
    static viso_tsdf_alignment& base(Record& r) { return r.a; }
    static uint64_t photo_rows(const Normal& nm) { return nm.n_photo_used; }
    static void finish(Record& r, const Normal& nm, double C, double lambda) {
        const double pp = (double)nm.p / 65536.0;
        r.cost_geo = sqrt((C - pp) / (double)nm.normal.n_used);
        r.cost_photo = nm.n_photo_used && lambda > 0.0 ? sqrt(pp / (double)nm.n_photo_used) / lambda : 0.0;
        r.n_photo_used = nm.n_photo_used;
    }
    static void launch(const Args& g, dim3 grid, hipStream_t s);
};

// One linearise of every frame f with active[f] != 0 at poses[f] ([n][16]) into out[f]; < 0: a VISO_ERR_*, which ends the loop.
template <class K>
using AlignLinearize = std::function<int(const double* poses, const unsigned long long* active, typename K::Normal* out)>;

// Steps a..f and the final linearise for n frames, each on its own; every round linearises the frames that are not finished in
// one call.  guesses: [n][16], or null: the identity for all.  trace (or null): frame 0's linearises, at most trace_cap of them.
// The gray kind runs the same machine on the combined sums: min_pixels against n_used, the covariance's divisor with
// n_photo_used, the two costs from p; its trace's entries carry the whole linearise.  (Instantiated in alignmath.cpp for both kinds.)
template <class K>
int align_run(const typename K::Params& p, int n, const double* guesses, const AlignLinearize<K>& linearize, typename K::Record* records,
              typename K::Step* trace, int trace_cap);

// H = L L' (step c): false when a pivot is not greater than 1e-12 times its diagonal entry.  L: lower triangle, row-major [6][6].
bool align_cholesky(const double H[36], double L[36]);
void align_solve(const double L[36], const double r[6], double x[6]);   // L L' x = r
void align_increment(double T[16], const double xi[6]);                 // step e: T <- T D(xi), xi = (v, omega)
#endif /* VISO_ALIGNMATH_H_ */
