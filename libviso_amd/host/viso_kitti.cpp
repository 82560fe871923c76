// viso_kitti — the reference's `kitti` driver (src/kitti.cpp:79-118) on the GPU
// pipeline: $KITTI_HOME/sequences/<seq>/{calib.txt,image_0/%06d.png,image_1/%06d.png}
// in, $KITTI_HOME/results/<seq>/<result_sha>/data/<seq>.txt out.  Images: KITTI's 8-bit
// grayscale PNGs (image_0/%06d.png, own decoder) or binary PGM (image_0/%06d.pgm).
//
//   KITTI_HOME=... viso_kitti result_sha seq_name [begin [end]] [options]
//
// One sequence over W GPUs (BASELINE configs[3], kitti_shard.hpp): frames shard into W contiguous
// ranges with a one-frame halo, each range is one process on one GPU, 64-byte records per frame pair
// are gathered once and chained on the host.  Any W writes the byte-identical pose file.
//   --gpus W            fork W rank processes (rank r on device r), wait, gather their rank files, write the poses
//   --rank r --world W  run range r only and write <result_dir>/shards/<seq>.<r>of<W>.rec   (one per GPU / node)
//   --gather W          read the W rank files and write the pose file
//   --device d          HIP device ordinal of this process (default: the rank, 0 without --rank)
//   --same-device       with --gpus: every rank on device 0 (rehearsal on a one-GPU box)
//   --chunk n           frames per device batch (default 64)      --seed s   RANSAC stream seed (default 0)
//   --decode-threads n  PNG decoding threads per rank (default: min(64, usable host threads / ranks): decoding bounds the run; usable = hardware, affinity, cgroup quota)
//   --reference-pose-list   write the list the reference's code actually produces, [P1, ..., Pn, Pn] (src/viso.cpp:1317-1321
//                       overwrites poses.back() before pushing the clone), instead of [I, P1, ..., Pn]
//   --subpixel m        opt-in sub-pixel stereo refinement (viso_batch_set_subpixel): 0 = off (default: the reference's
//                       arithmetic), 1 = uR, 2 = uR and vR.  Not in the reference: such poses are not comparable with its output
//   --rectify file      opt-in: the images are RAW (KITTI raw's unrectified drives, other rigs) and are undistorted and rectified
//                       on the device (viso_batch_set_rectify) with KITTI raw's calib_cam_to_cam.txt `file`, which is used in
//                       place of calib.txt (P_rect_00 / P_rect_01).  Not in the reference
//   --covariance file   opt-in: also write the per-frame motion covariance (viso_batch_set_covariance, mode 1: sigma
//                       estimated) to `file`, one line per frame pair: status n sigma2 gap and the 21 upper-triangle entries
//                       (%.17g); byte-identical for every chunk size, W and partition.  Pose files are unchanged.  Not in the
//                       reference
//   --covariance-sigma s  with --covariance: mode 2, sigma = s pixels
//   --disparity dir     opt-in: also write every frame's dense disparity map (viso_batch_set_disparity) to dir/%06d.png, named by
//                       the image index, in KITTI's stereo format (16-bit, value = 16 * disp16, i.e. disparity * 256; invalid =
//                       0, and a valid 0 px is 0 too: the format cannot tell them apart).  Uncompressed: about 0.93 MB per frame
//                       at 1241 x 376.  A chunk's or rank's halo frame is written by its owner only, so the directory is
//                       byte-identical for every chunk size, W and partition.  Pose files are unchanged.  Not in the reference
//   --disparity-params D,B,c,T,u,m  with --disparity: num_disp, block, prefilter_cap, texture_threshold, uniqueness,
//                       lr_max_diff (default 128,11,31,10,15,1)
//   --disparity-method bm|sgm  with --disparity: bm (the default) is the block matcher; sgm computes the same files by semi-global
//                       matching (viso_batch_set_sgm), with the same names, format and halo ownership
//   --sgm-params D,P1,P2,paths,u,m  with --disparity-method sgm: num_disp, p1, p2, paths, uniqueness, lr_max_diff (default
//                       128,10,120,8,10,1)
//   --speckle SIZE,DIFF  with --disparity, for either method: the speckle filter (viso_batch_set_speckle) over every map before it is
//                       written: max_size in pixels, max_diff in 1/16 px.  Same names, format and halo ownership
// Every rank reports where its wall time went: decode (PNG inflate on the worker threads; the calling thread's wait for
// it is the runner's critical path), upload and GPU seconds from time stamps on the device.
// libviso_amd/kitti_shard.py is the same runner with the gather as an RCCL all-gather (torch.distributed).
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <string>
#include <thread>
#include <sys/types.h>
#include <sys/wait.h>
#include <unistd.h>
#include <vector>

#include "kitti_io.hpp"
#include "kitti_shard.hpp"
#include "viso.hpp"

namespace {
struct Args {
    // --chunk, --seed, --decode-threads, --subpixel and the covariance mode are final after parse(); the lists of
    // --disparity-params, --sgm-params and --speckle wait in opt.disparity for main's checks (viso::set_disparity and friends)
    viso::RunOptions opt;
    const char* result_sha = nullptr;
    std::string seq_name;
    int begin = 0, end = INT_MAX;
    int gpus = 0, rank = -1, world = 0, gather = 0, device = -1;
    bool same_device = false, reference_pose_list = false;
    std::string rectify;      // calib_cam_to_cam.txt of --rectify ("" = off)
    std::string covariance;   // --covariance file ("" = off)
    std::string disparity;    // --disparity dir ("" = off)
    bool sigma_given = false, disp_params_given = false, method_given = false, sgm = false, sgm_params_given = false, speckle_given = false;
};

// an option's list: exactly N integers with commas between them and nothing behind; fmt ends in the %c that must not match
template <class... Int>
bool int_list(const char* s, const char* fmt, Int*... dst) {
    char tail = 0;
    return s && std::sscanf(s, fmt, dst..., &tail) == (int)sizeof...(dst);
}

bool parse(int argc, char** argv, Args& a) {
    int pos = 0;
    viso::DisparityOutput& d = a.opt.disparity;
    for (int i = 1; i < argc; ++i) {
        const std::string s = argv[i];
        auto value = [&]() -> const char* { return i + 1 < argc ? argv[++i] : nullptr; };   // the option needs one
        auto integer = [&](int& dst) { const char* v = value(); if (v) dst = std::atoi(v); return v != nullptr; };
        auto text = [&](std::string& dst) { const char* v = value(); if (v) dst = v; return v && *v; };   // not ""
        bool ok = true;
        if (s == "--gpus") ok = integer(a.gpus);
        else if (s == "--rank") ok = integer(a.rank);
        else if (s == "--world") ok = integer(a.world);
        else if (s == "--gather") ok = integer(a.gather);
        else if (s == "--device") ok = integer(a.device);
        else if (s == "--chunk") ok = integer(a.opt.chunk);
        else if (s == "--decode-threads") ok = integer(a.opt.decode_threads);
        else if (s == "--subpixel") { int m = 0; ok = integer(m) && viso::set_subpixel(a.opt, m).empty(); }
        else if (s == "--reference-pose-list") a.reference_pose_list = true;
        else if (s == "--rectify") ok = text(a.rectify);
        else if (s == "--covariance") ok = text(a.covariance);
        else if (s == "--disparity") ok = text(a.disparity);
        else if (s == "--disparity-params") {
            viso_disparity_params& p = d.params;
            ok = a.disp_params_given = int_list(value(), "%d,%d,%d,%d,%d,%d%c", &p.num_disp, &p.block, &p.prefilter_cap,
                                                &p.texture_threshold, &p.uniqueness, &p.lr_max_diff);
        }
        else if (s == "--disparity-method") {
            std::string m;
            ok = a.method_given = text(m) && (m == "bm" || m == "sgm");
            a.sgm = m == "sgm";
        }
        else if (s == "--sgm-params") {
            viso_sgm_params& p = d.sgm_params;
            ok = a.sgm_params_given = int_list(value(), "%d,%d,%d,%d,%d,%d%c", &p.num_disp, &p.p1, &p.p2, &p.paths, &p.uniqueness,
                                               &p.lr_max_diff);
        }
        else if (s == "--speckle") ok = a.speckle_given = int_list(value(), "%d,%d%c", &d.speckle_params.max_size, &d.speckle_params.max_diff);
        else if (s == "--covariance-sigma") {   // its range is set_covariance's to check, below
            const char* v = value();
            char* e = nullptr;
            if (v) a.opt.cov_sigma = std::strtod(v, &e);
            ok = a.sigma_given = v && !*e;
        }
        else if (s == "--seed") { const char* v = value(); if (v) a.opt.ransac_seed = std::strtoull(v, nullptr, 10); ok = v != nullptr; }
        else if (s == "--same-device") a.same_device = true;
        else if (s.rfind("--", 0) == 0) ok = false;
        else {
            if (pos == 0) a.result_sha = argv[i];
            else if (pos == 1) a.seq_name = s;
            else if (pos == 2) a.begin = std::atoi(argv[i]);                                   // src/kitti.cpp:86-94
            else if (pos == 3) a.end = std::atoi(argv[i]);
            else ok = false;
            ++pos;
        }
        if (!ok) return false;
    }
    if (pos < 2) return false;
    if ((a.rank >= 0) != (a.world > 0)) return false;
    if (a.rank >= a.world && a.world > 0) return false;
    if (a.sigma_given && a.covariance.empty()) return false;         // --covariance-sigma belongs to --covariance
    if (a.disp_params_given && a.disparity.empty()) return false;    // --disparity-params belongs to --disparity
    if (a.method_given && a.disparity.empty()) return false;         // and so does --disparity-method
    if (a.sgm_params_given && !a.sgm) return false;                  // --sgm-params belongs to --disparity-method sgm
    if (a.disp_params_given && a.sgm) return false;                  // --disparity-params to the block matcher
    if (a.speckle_given && a.disparity.empty()) return false;        // --speckle filters the maps of --disparity
    // --covariance: mode 1 (sigma estimated), mode 2 with --covariance-sigma
    return viso::set_covariance(a.opt, a.covariance.empty() ? 0 : a.sigma_given ? 2 : 1, a.opt.cov_sigma).empty();
}

bool write_covariances(const std::string& file, const std::vector<viso_motion_cov>& rec) {
    viso::mkdirs_for(file);
    if (viso::write_covariance_file(file, rec.data(), rec.size())) return true;
    std::fprintf(stderr, "cannot write %s\n", file.c_str());
    return false;
}

std::string rank_file(const std::string& result_dir, const std::string& seq, int r, int w) {
    return result_dir + "/shards/" + seq + "." + std::to_string(r) + "of" + std::to_string(w) + ".rec";
}

void print_stats(const char* who, const viso::OdometryStats& s) {
    std::printf("%s: %d frames in %.3f s (%.0f frames/s) | decode: %d threads, %.3f s of thread time, runner waited %.3f s | "
                "GPU stamps: upload %.3f s, kernels %.3f s | host: issue %.3f s, waiting for results %.3f s\n",
                who, s.frames, s.wall_s, s.wall_s > 0 ? s.frames / s.wall_s : 0.0, s.decode_threads, s.decode_cpu_s, s.decode_wait_s,
                s.upload_ms * 1e-3, s.gpu_ms * 1e-3, s.issue_s, s.drain_wait_s);
}

int threads_per_rank(int ranks) {
    const int share = viso::cpu_budget() / (ranks > 0 ? ranks : 1);   // hardware threads, affinity and cgroup quota
    return share < 1 ? 1 : (share > 64 ? 64 : share);
}
}  // namespace

int main(int argc, char** argv) {
    Args a;
    if (!parse(argc, argv, a)) {
        std::printf("usage: demo result_sha seq_name begin end [--gpus W | --rank r --world W | --gather W] "
                    "[--device d] [--same-device] [--chunk n] [--seed s] [--decode-threads n] [--reference-pose-list] [--subpixel 0|1|2] [--rectify calib_cam_to_cam.txt] "
                    "[--covariance file [--covariance-sigma s]] [--disparity dir [--disparity-params D,B,c,T,u,m] "
                    "[--disparity-method bm|sgm [--sgm-params D,P1,P2,paths,u,m]] [--speckle SIZE,DIFF]]\n");   // :81-85
        return 1;
    }
    const char* home = std::getenv("KITTI_HOME");                                              // :96
    if (!home) { std::fprintf(stderr, "KITTI_HOME is not set\n"); return 2; }
    const std::string seq_base = std::string(home) + "/sequences/" + a.seq_name;
    const std::string result_dir = std::string(home) + "/results/" + a.seq_name + "/" + a.result_sha;   // :100
    const std::string out = result_dir + "/data/" + a.seq_name + ".txt";                       // :114
    viso::Matd P1, P2;
    std::string err = viso::set_rectify(a.opt, P1, P2, a.rectify.c_str());
    if (!err.empty()) { std::fprintf(stderr, "%s\n", err.c_str()); return 2; }
    if (!a.opt.rect && !viso::loadCalib(seq_base + "/calib.txt", P1, P2)) { std::fprintf(stderr, "cannot read %s/calib.txt\n", seq_base.c_str()); return 2; }
    const int n_frames = viso::kitti_count_frames(seq_base, a.begin, a.end);
    if (!a.disparity.empty()) {   // --disparity: checked (and its directory made) here, before any rank is forked
        viso::DisparityOutput& d = a.opt.disparity;
        err = a.sgm ? viso::set_sgm(a.opt, a.disparity.c_str(), a.sgm_params_given ? &d.sgm_params : nullptr)
                    : viso::set_disparity(a.opt, a.disparity.c_str(), a.disp_params_given ? &d.params : nullptr);
        if (err.empty() && a.speckle_given) err = viso::set_speckle(a.opt, &d.speckle_params);
        if (!err.empty()) { std::fprintf(stderr, "%s\n", err.c_str()); return 2; }
    }

    // ---- --gpus W: fork the ranks BEFORE this process touches the GPU (the parent never does: nothing above makes a
    // HIP call), each child carries on below as `--rank r --world W`; the parent waits and gathers.  fork without exec:
    // a child initialises its own HIP runtime on its first call ----
    const auto t_start = std::chrono::steady_clock::now();
    if (a.opt.decode_threads <= 0 && !std::getenv("VISO_DECODE_THREADS"))
        a.opt.decode_threads = threads_per_rank(a.gpus > 1 ? a.gpus : 1);
    if (a.gpus > 1) {
        std::fflush(nullptr);
        std::vector<pid_t> kids;
        bool child = false;
        for (int r = 0; r < a.gpus && !child; ++r) {
            const pid_t pid = ::fork();
            if (pid < 0) { std::perror("fork"); return 5; }
            if (pid == 0) {
                child = true;
                a.rank = r; a.world = a.gpus; a.gpus = 0;
                if (a.device < 0) a.device = a.same_device ? 0 : r;
            } else {
                kids.push_back(pid);
            }
        }
        if (!child) {
            int bad = 0;
            for (pid_t pid : kids) {
                int st = 0;
                if (::waitpid(pid, &st, 0) < 0 || !WIFEXITED(st) || WEXITSTATUS(st) != 0) ++bad;
            }
            if (bad) { std::fprintf(stderr, "%d of %d rank processes failed\n", bad, (int)kids.size()); return 6; }
            a.gather = (int)kids.size();
        }
    }

    try {
        // ---- --gather W: rank files -> one pose file ----
        if (a.gather > 0) {
            const auto ranges = viso::partition(n_frames, a.gather);
            std::vector<std::vector<viso::FrameRecord>> parts((size_t)a.gather);
            for (int r = 0; r < a.gather; ++r) {
                int first = 0, last = 0;
                const std::string f = rank_file(result_dir, a.seq_name, r, a.gather);
                if (!viso::read_records(f, first, last, parts[(size_t)r])) { std::fprintf(stderr, "cannot read %s\n", f.c_str()); return 3; }
                if (first != ranges[(size_t)r].first || last != ranges[(size_t)r].second) {
                    std::fprintf(stderr, "%s covers frames %d..%d, expected %d..%d (begin/end changed?)\n", f.c_str(), first, last,
                                 ranges[(size_t)r].first, ranges[(size_t)r].second);
                    return 3;
                }
            }
            const std::vector<viso::FrameRecord> all = viso::stitch_records(parts, ranges);
            if (!a.covariance.empty()) {   // the ranks' covariance records, stitched the same way
                std::vector<std::vector<viso_motion_cov>> cparts((size_t)a.gather);
                for (int r = 0; r < a.gather; ++r) {
                    int first = 0, last = 0;
                    const std::string f = rank_file(result_dir, a.seq_name, r, a.gather) + ".cov";
                    if (!viso::read_records(f, first, last, cparts[(size_t)r]) || first != ranges[(size_t)r].first ||
                        last != ranges[(size_t)r].second || cparts[(size_t)r].size() != parts[(size_t)r].size()) {
                        std::fprintf(stderr, "cannot read %s (or it does not match the rank's records)\n", f.c_str());
                        return 3;
                    }
                }
                if (!write_covariances(a.covariance, viso::stitch_records(cparts, ranges))) return 3;
            }
            const std::vector<viso::Matd> poses = viso::chain_records(all.data(), (int)all.size(), a.reference_pose_list);
            viso::mkdirs(result_dir + "/data");
            if (!viso::savePoses(out, poses)) { std::fprintf(stderr, "cannot write %s\n", out.c_str()); return 3; }
            int solved = 0;
            for (const auto& r : all) solved += r.ok;
            const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
            std::printf("frames %zu solved %d poses %zu ranks %d -> %s (%.3f s, %.0f frames/s of the runner)\n", all.size() + (n_frames > 0),
                        solved, poses.size(), a.gather, out.c_str(), wall, wall > 0 ? (double)(all.size() + (n_frames > 0)) / wall : 0.0);
            return 0;
        }
        // ---- --rank r --world W: this rank's range -> its rank file ----
        if (a.world > 0) {
            const auto range = viso::partition(n_frames, a.world)[(size_t)a.rank];
            a.opt.device = a.device >= 0 ? a.device : a.rank;
            const viso::RangeResult res = viso::kitti_run_range(seq_base, P1, P2, a.begin, range.first, range.second, a.opt);
            viso::mkdirs(result_dir + "/shards");
            const std::string f = rank_file(result_dir, a.seq_name, a.rank, a.world);
            if (!a.covariance.empty() && !viso::write_records(f + ".cov", range.first, range.second, res.cov)) {
                std::fprintf(stderr, "cannot write %s.cov\n", f.c_str());
                return 3;
            }
            if (!viso::write_records(f, range.first, range.second, res.rec)) { std::fprintf(stderr, "cannot write %s\n", f.c_str()); return 3; }
            std::printf("rank %d/%d device %d frames %d..%d pairs %zu -> %s\n", a.rank, a.world, a.opt.device, a.begin + range.first,
                        a.begin + range.second, res.rec.size(), f.c_str());
            print_stats(("rank " + std::to_string(a.rank)).c_str(), res.stats);
            return 0;
        }
        // ---- one process, one GPU: the reference's flow (:108-116) ----
        const std::string ext = viso::kitti_image_ext(seq_base, a.begin);
        viso::StereoImageGenerator images({seq_base + "/image_0/%06d" + ext, seq_base + "/image_1/%06d" + ext}, a.begin, a.end);
        a.opt.first_frame_index = (uint64_t)a.begin;
        a.opt.device = a.device >= 0 ? a.device : 0;
        viso::OdometryResult res = viso::sequence_odometry(P1, P2, images, a.opt);             // :111
        if (!a.covariance.empty()) {   // one line per frame pair: the records of frames 1 .. (entry 0 is the first frame)
            const std::vector<viso_motion_cov> pairs(res.cov.size() > 1 ? res.cov.begin() + 1 : res.cov.end(), res.cov.end());
            if (!write_covariances(a.covariance, pairs)) return 3;
        }
        viso::mkdirs(result_dir + "/data");                                                    // :112-113
        if (a.reference_pose_list && res.poses.size() > 1) {                                   // [P1, ..., Pn, Pn], see kitti_shard.hpp
            res.poses.erase(res.poses.begin());
            res.poses.push_back(res.poses.back());
        }
        if (!viso::savePoses(out, res.poses)) { std::fprintf(stderr, "cannot write %s\n", out.c_str()); return 3; }
        int solved = 0;
        for (int v : res.ok) solved += v;
        std::printf("frames %zu solved %d poses %zu -> %s\n", res.ok.size(), solved, res.poses.size(), out.c_str());
        print_stats("one process", res.stats);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 4;
    }
    return 0;
}
