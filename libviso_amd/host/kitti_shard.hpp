// kitti_shard.hpp — one KITTI sequence over W GPUs (BASELINE configs[3]).
//
// The reference's `kitti` driver (src/kitti.cpp:79-118) is one process over one sequence.  The only cross-frame
// dependency of its loop is the *_prev state (src/viso.cpp:1208-1222): the relative motion of frame t needs frames
// t-1 and t, and the trajectory is the prefix product pose_t = pose_{t-1} * inv(Tr_t) (:1315-1321).  So:
//   partition   rank r of W takes a contiguous range of frame pairs, with a one-frame halo (it re-does detection,
//               description and the stereo match of its first frame); same rule as libviso_amd/shard.py
//   keys        RANSAC triples are drawn from a stream keyed on the ABSOLUTE KITTI frame index (the file number),
//               so a frame's record does not depend on the partition, on `begin`, or on the chunking
//   records     per frame pair {tr[6], ok, n_inl} = 64 B: what crosses ranks, once (RCCL all-gather in
//               libviso_amd/kitti_shard.py, or rank files read by `viso_kitti --gather`)
//   chain       the host prefix product over the gathered records and the KITTI pose file (src/kitti.cpp:49-64)
// Any W gives the byte-identical pose file (tests/test_gpu_kitti_shard.py).
#pragma once
#include <cstdint>
#include <cstdio>
#include <functional>
#include <string>
#include <utility>
#include <vector>

#include "viso.hpp"

namespace viso {

// one frame pair (t-1, t): what sequence_odometry's loop body leaves behind (src/viso.cpp:1313-1324)
struct FrameRecord {
    double tr[6];
    int32_t ok;
    int32_t n_inl;
    int32_t frame;      // absolute KITTI index of the pair's second frame (the file number)
    int32_t reserved;
};
static_assert(sizeof(FrameRecord) == 64, "FrameRecord is the 64-byte wire format");

// [(first, last)] per rank over frames 0..n_frames-1 (relative to `begin`): rank r solves the pairs (t-1, t) for
// t in (first, last]; frames first..last are read by it.  Sizes differ by at most one, larger ranges first.
std::vector<std::pair<int, int>> partition(int n_frames, int world);

// "<seq_base>/image_0/%06d" + ".png" if frame `begin` exists as PNG, ".pgm" otherwise (src/kitti.cpp:108-110)
std::string kitti_image_ext(const std::string& seq_base, int begin);
// number of consecutive frames begin, begin+1, ... <= end for which both image files can be opened
int kitti_count_frames(const std::string& seq_base, int begin, int end);

// What a range leaves behind
struct RangeResult {
    std::vector<FrameRecord> rec;       // rec[i] = record of the pair ending at frame first + 1 + i
    std::vector<viso_motion_cov> cov;   // one per record exactly when opt.cov_mode != 0
    OdometryStats stats;                // where the range's wall time went (decode / upload / GPU)
};
// Frames [begin + first, begin + last] of the sequence through sequence_odometry with `opt`, of which this function sets
// first_frame_index = begin + first and disparity.write_first = (first == 0) itself: maps are written for the frames first + 1 ..
// last, and for frame `first` only by the range that owns it (a later range's first frame is the previous range's last).  Fewer
// than last - first records come back when an image in the range cannot be decoded (the reference's generator stops there,
// src/viso.h:94-96).
RangeResult kitti_run_range(const std::string& seq_base, const Matd& P1, const Matd& P2, int begin, int first, int last,
                            const RunOptions& opt);

// The runners' option checks, one per option, shared by the C setters below and by viso_kitti.  Each stores a valid value in
// `opt` and returns "", or leaves `opt` as it was and returns the error text, which names the C setter.  A null or "" file or
// directory switches that option off; the last of set_disparity / set_sgm decides the method; set_speckle (null = off) sticks
// across both and does nothing while no maps are written.  set_disparity / set_sgm create the directory.  set_rectify also
// gives the rectified projections that replace the sequence's calib.txt.
std::string set_subpixel(RunOptions& opt, int mode);
std::string set_covariance(RunOptions& opt, int mode, double sigma_px);
std::string set_rectify(RunOptions& opt, Matd& P1, Matd& P2, const char* cam_to_cam_file);
std::string set_disparity(RunOptions& opt, const char* dir, const viso_disparity_params* params);
std::string set_sgm(RunOptions& opt, const char* dir, const viso_sgm_params* params);
std::string set_speckle(RunOptions& opt, const viso_speckle_params* params);

// The covariance file of the runners' --covariance option: one line per frame pair, "status n sigma2 gap" and the 21
// upper-triangle entries of cov (row by row), every value %.17g.  Written under a temporary name and renamed.
bool write_covariance_file(const std::string& file_name, const viso_motion_cov* rec, size_t n);

// poses[0] = I, then pose <- pose * inv(tr2mat(tr)) per solved record (src/viso.cpp:1189-1190, 1315-1321): the list
// [I, P1, ..., Pn] the reference's code reads as.
// reference_pose_list = true: the list the reference actually WRITES.  `Mat pose = poses.back(); pose =
// pose*tr_mat.inv(); poses.push_back(pose.clone());` (src/viso.cpp:1317-1321) assigns the product into a header that
// shares poses.back()'s buffer (cv::Mat is reference counted; the GEMM result is copied into the existing buffer), so
// the previous entry is overwritten before the clone is pushed: [P1, P2, ..., Pn, Pn] — no identity line, the last
// pose twice, the same number of lines.
std::vector<Matd> chain_records(const FrameRecord* rec, int n, bool reference_pose_list = false);

void mkdirs(const std::string& path);
// mkdirs of the directory file_name lies in
void mkdirs_for(const std::string& file_name);
// `write` fills file_name + ".tmp" (opened with `mode`), which is then renamed: a reader never sees a partial file
bool write_atomically(const std::string& file_name, const char* mode, const std::function<bool(FILE*)>& write);

// rank files of `viso_kitti --rank r --world W`: header {magic, first, last, n_done} + n_done records, of FrameRecord and,
// next to them, of the covariance records
template <class R> inline constexpr int32_t RECORD_MAGIC = 0;
template <> inline constexpr int32_t RECORD_MAGIC<FrameRecord> = 0x56534B52;       // "VSKR"
template <> inline constexpr int32_t RECORD_MAGIC<viso_motion_cov> = 0x56534B43;   // "VSKC"

template <class R>
bool write_records(const std::string& file_name, int first, int last, const std::vector<R>& rec) {
    return write_atomically(file_name, "wb", [&](FILE* fp) {
        const int32_t hdr[4] = {RECORD_MAGIC<R>, first, last, (int32_t)rec.size()};
        return std::fwrite(hdr, sizeof hdr, 1, fp) == 1 && (rec.empty() || std::fwrite(rec.data(), sizeof(R), rec.size(), fp) == rec.size());
    });
}

template <class R>
bool read_records(const std::string& file_name, int& first, int& last, std::vector<R>& rec) {
    FILE* fp = std::fopen(file_name.c_str(), "rb");
    if (!fp) return false;
    int32_t hdr[4];
    bool ok = std::fread(hdr, sizeof hdr, 1, fp) == 1 && hdr[0] == RECORD_MAGIC<R> && hdr[3] >= 0 && hdr[2] >= hdr[1] &&
              hdr[3] <= hdr[2] - hdr[1];
    if (ok) {
        first = hdr[1]; last = hdr[2];
        rec.resize((size_t)hdr[3]);
        if (hdr[3]) ok = std::fread(rec.data(), sizeof(R), rec.size(), fp) == rec.size();
    }
    std::fclose(fp);
    return ok;
}

// Records of all ranks in rank order -> one list; stops at the first rank that came back short (see above): the sequence
// ends there for one process too.
template <class R>
std::vector<R> stitch_records(const std::vector<std::vector<R>>& parts, const std::vector<std::pair<int, int>>& ranges) {
    std::vector<R> all;
    for (size_t r = 0; r < parts.size() && r < ranges.size(); ++r) {
        all.insert(all.end(), parts[r].begin(), parts[r].end());
        if ((int)parts[r].size() < ranges[r].second - ranges[r].first) break;
    }
    return all;
}

}  // namespace viso

// C entry points for the Python launcher (libviso_amd/kitti_shard.py: one rank per GPU under torch.distributed,
// records all-gathered over RCCL).  Return 1, or a negative code with the text in viso_host_last_error().
extern "C" {
int viso_kitti_count_frames(const char* seq_base, int begin, int end);
// rec8: [(last - first)][8] doubles = tr[6], ok, n_inl per pair; *n_done = pairs actually solved or failed (not skipped)
int viso_kitti_run_range(const char* seq_base, int begin, int first, int last, int device, int chunk,
                         uint64_t ransac_seed, double* rec8, int* n_done);
// OdometryStats of this thread's last viso_kitti_run_range: frames, decode_threads, wall_s, decode_wait_s,
// decode_cpu_s, issue_s, drain_wait_s, upload_ms, gpu_ms
void viso_kitti_last_stats(double out[9]);
// worker threads the next viso_kitti_run_range calls of this thread decode with (0 = default)
void viso_kitti_set_decode_threads(int n);
// sub-pixel stereo refinement mode (viso_batch_set_subpixel: 0 = off, 1, 2) of the next viso_kitti_run_range calls of this
// thread; returns VISO_ERR_ARG for another value
int viso_kitti_set_subpixel(int mode);
// KITTI raw calib_cam_to_cam.txt (viso::loadCalibCamToCam): K [2][9], D [2][5], R [2][9] (R_rect), P [2][12] (P_rect),
// geometry = raw_rows, raw_cols, out_rows, out_cols.  Camera 0 = left (*_00), 1 = right (*_01).  No device needed.
int viso_kitti_load_cam_to_cam(const char* file_name, double K[18], double D[10], double R[18], double P[24], int geometry[4]);
// the next viso_kitti_run_range calls of this thread read RAW images and rectify them on the device with the calibration of
// this calib_cam_to_cam.txt, whose P_rect_00 / P_rect_01 replace the sequence's calib.txt; null or "" = off.  VISO_ERR_ARG
// when the file cannot be read.
int viso_kitti_set_rectify(const char* cam_to_cam_file);
// the motion covariance (viso_batch_set_covariance) of the next viso_kitti_run_range calls of this thread: mode 0 (off), 1, or 2
// with sigma_px; VISO_ERR_ARG for anything else
int viso_kitti_set_covariance(int mode, double sigma_px);
// the records of this thread's last viso_kitti_run_range (one per record it returned): *n = their number, copied up to cap
int viso_kitti_last_covariances(viso_motion_cov* out, int cap, int* n);
// the covariance file of --covariance (viso::write_covariance_file)
int viso_kitti_write_covariances(const char* file_name, const viso_motion_cov* rec, int n);
// the dense disparity maps (viso_batch_set_disparity) of the next viso_kitti_run_range calls of this thread, written to
// dir/%06d.png (the directory is created); dir null or "" = off.  params null = viso_disparity_params_default.  VISO_ERR_ARG for
// invalid parameters or a directory that cannot be created.
int viso_kitti_set_disparity(const char* dir, const viso_disparity_params* params);
// the same maps by semi-global matching (viso_batch_set_sgm): same directory, names and ownership of halo frames; the last of the
// two calls decides the method.  params null = viso_sgm_params_default
int viso_kitti_set_sgm(const char* dir, const viso_sgm_params* params);
// the speckle filter (viso_batch_set_speckle) over those maps, for either method, in the next viso_kitti_run_range calls of this
// thread; params null = off.  It does nothing while no maps are written.  VISO_ERR_ARG for invalid parameters.
int viso_kitti_set_speckle(const viso_speckle_params* params);
// One disparity map (int16 rows x cols, 1/16 px, VISO_DISP_INVALID = -16) as KITTI's stereo PNG: 16-bit grayscale, value =
// 16 * disp16 (disparity = value / 256), 0 = invalid.  A valid disparity of 0 px is written as 0 as well: the format cannot tell it
// from invalid.  zlib stored blocks (no compression: about 0.93 MB at 1241 x 376), Adler-32 and CRC-32 computed here; written under
// a temporary name and renamed.  No device needed.  VISO_ERR_ARG: null pointers, sizes <= 0, a file that cannot be written.
int viso_write_disparity_png(const char* path, const int16_t* d16, int rows, int cols);
// chain n records and write the KITTI pose file (directories are created); *n_poses = lines written
int viso_kitti_write_poses(const char* file_name, const double* rec8, int n, int* n_poses);
// the same with the pose list the reference writes ([P1..Pn, Pn], see chain_records) when reference_pose_list != 0
int viso_kitti_write_poses2(const char* file_name, const double* rec8, int n, int reference_pose_list, int* n_poses);
const char* viso_host_last_error(void);
}
