// kitti_shard.cpp — see kitti_shard.hpp.  Host code only: ranges, record files, the pose chain; every frame's
// arithmetic happens in viso::sequence_odometry -> libviso_hip.so.
#include "kitti_shard.hpp"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <sys/stat.h>

#include "kitti_io.hpp"

namespace viso {

std::vector<std::pair<int, int>> partition(int n_frames, int world) {
    std::vector<std::pair<int, int>> out;
    if (world < 1) world = 1;
    const int n_pairs = n_frames > 1 ? n_frames - 1 : 0;
    const int base = n_pairs / world, rem = n_pairs % world;
    int t = 0;
    for (int r = 0; r < world; ++r) {
        const int k = base + (r < rem ? 1 : 0);
        out.emplace_back(t, t + k);
        t += k;
    }
    return out;
}

static std::string frame_file(const std::string& seq_base, int side, int index, const std::string& ext) {
    char buf[64];
    std::snprintf(buf, sizeof buf, "/image_%d/%06d", side, index);
    return seq_base + buf + ext;
}

static bool readable(const std::string& f) {
    FILE* fp = std::fopen(f.c_str(), "rb");
    if (fp) std::fclose(fp);
    return fp != nullptr;
}

std::string kitti_image_ext(const std::string& seq_base, int begin) {
    return readable(frame_file(seq_base, 0, begin, ".png")) ? ".png" : ".pgm";
}

int kitti_count_frames(const std::string& seq_base, int begin, int end) {
    const std::string ext = kitti_image_ext(seq_base, begin);
    int n = 0;
    for (long i = begin; i <= end; ++i, ++n)
        if (!readable(frame_file(seq_base, 0, (int)i, ext)) || !readable(frame_file(seq_base, 1, (int)i, ext))) break;
    return n;
}

RangeResult kitti_run_range(const std::string& seq_base, const Matd& P1, const Matd& P2, int begin, int first, int last,
                            const RunOptions& opt) {
    RangeResult out;
    if (last <= first) return out;
    const std::string ext = kitti_image_ext(seq_base, begin);
    StereoImageGenerator images({seq_base + "/image_0/%06d" + ext, seq_base + "/image_1/%06d" + ext},
                                begin + first, begin + last);
    RunOptions o = opt;
    o.first_frame_index = (uint64_t)(begin + first);
    o.disparity.write_first = first == 0;   // frame `first` of a later range is the previous range's last frame
    const OdometryResult res = sequence_odometry(P1, P2, images, o);
    out.stats = res.stats;
    // res.ok / res.tr / res.n_inliers: one entry per frame read, entry 0 = this range's first frame (no pose)
    for (size_t t = 1; t < res.ok.size(); ++t) {
        FrameRecord r;
        for (int j = 0; j < 6; ++j) r.tr[j] = res.tr[t][(size_t)j];
        r.ok = res.ok[t];
        r.n_inl = res.n_inliers[t];
        r.frame = begin + first + (int)t;
        r.reserved = 0;
        out.rec.push_back(r);
        if (t < res.cov.size()) out.cov.push_back(res.cov[t]);
    }
    return out;
}

bool write_atomically(const std::string& file_name, const char* mode, const std::function<bool(FILE*)>& write) {
    const std::string tmp = file_name + ".tmp";
    FILE* fp = std::fopen(tmp.c_str(), mode);
    if (!fp) return false;
    bool ok = write(fp);
    ok = (std::fclose(fp) == 0) && ok;
    return ok && std::rename(tmp.c_str(), file_name.c_str()) == 0;
}

bool write_covariance_file(const std::string& file_name, const viso_motion_cov* rec, size_t n) {
    return write_atomically(file_name, "w", [&](FILE* fp) {
        bool ok = true;
        for (size_t i = 0; i < n && ok; ++i) {
            const viso_motion_cov& c = rec[i];
            ok = std::fprintf(fp, "%d %d %.17g %.17g", (int)c.status, (int)c.n, c.sigma2, c.gap) > 0;
            for (int p = 0; p < 6 && ok; ++p)
                for (int q = p; q < 6 && ok; ++q) ok = std::fprintf(fp, " %.17g", c.cov[6 * p + q]) > 0;
            ok = ok && std::fputc('\n', fp) != EOF;
        }
        return ok;
    });
}

std::vector<Matd> chain_records(const FrameRecord* rec, int n, bool reference_pose_list) {
    std::vector<Matd> poses;
    poses.push_back(Matd::eye(4));                                   // src/viso.cpp:1189-1190
    double pose[16];
    std::memcpy(pose, poses[0].ptr(), sizeof pose);
    for (int i = 0; i < n; ++i) {
        if (!rec[i].ok) continue;                                    // :1287, :1323: nothing is pushed
        viso_pose_update(pose, rec[i].tr, pose);                     // :1315-1321
        Matd P(4, 4);
        std::memcpy(P.ptr(), pose, sizeof pose);
        if (reference_pose_list) poses.back() = P;                   // :1317-1319: the product lands in poses.back()'s buffer
        poses.push_back(P);                                          // :1321: ... and its clone is pushed
    }
    return poses;
}

void mkdirs(const std::string& path) {
    for (size_t i = 1; i <= path.size(); ++i)
        if (i == path.size() || path[i] == '/') ::mkdir(path.substr(0, i).c_str(), 0777);
}

void mkdirs_for(const std::string& file_name) {
    const size_t slash = file_name.rfind('/');
    if (slash != std::string::npos && slash > 0) mkdirs(file_name.substr(0, slash));
}

std::string set_subpixel(RunOptions& opt, int mode) {
    if (mode < 0 || mode > 2) return "viso_kitti_set_subpixel: mode must be 0, 1 or 2";
    opt.subpixel = mode;
    return "";
}

std::string set_covariance(RunOptions& opt, int mode, double sigma_px) {
    if (mode != 0 && mode != 1 && !(mode == 2 && std::isfinite(sigma_px) && sigma_px > 0.0))
        return "viso_kitti_set_covariance: mode 0, 1, or 2 with a finite sigma_px > 0";
    opt.cov_mode = mode;
    opt.cov_sigma = mode == 2 ? sigma_px : 0.0;
    return "";
}

std::string set_rectify(RunOptions& opt, Matd& P1, Matd& P2, const char* cam_to_cam_file) {
    if (!cam_to_cam_file || !*cam_to_cam_file) { opt.rect.reset(); return ""; }
    StereoRectification r;
    Matd p1, p2;
    if (!loadCalibCamToCam(cam_to_cam_file, r, p1, p2))
        return std::string("viso_kitti_set_rectify: cannot read a KITTI raw calib_cam_to_cam file from ") + cam_to_cam_file;
    opt.rect = r; P1 = p1; P2 = p2;
    return "";
}

// the tail that set_disparity and set_sgm share: the directory, then the switch to the method of `who`
static std::string write_maps_to(RunOptions& opt, const char* who, const char* dir, bool params_ok, bool sgm) {
    if (!params_ok) return std::string(who) + ": parameters outside the ranges of include/viso_hip.h";
    mkdirs(dir);
    struct stat st;
    if (::stat(dir, &st) != 0 || !S_ISDIR(st.st_mode)) return std::string(who) + ": cannot create " + dir;
    opt.disparity.dir = dir; opt.disparity.write_first = true; opt.disparity.sgm = sgm; opt.disparity_on = true;
    return "";
}

std::string set_disparity(RunOptions& opt, const char* dir, const viso_disparity_params* params) {
    if (!dir || !*dir) { opt.disparity_on = false; return ""; }
    viso_disparity_params p;
    viso_disparity_params_default(&p);
    if (params) p = *params;
    const bool ok = p.num_disp >= 16 && p.num_disp <= 256 && p.num_disp % 16 == 0 && p.block >= 5 && p.block <= 21 && p.block % 2 == 1 &&
                    p.prefilter_cap >= 1 && p.prefilter_cap <= 63 && p.texture_threshold >= 0 && p.uniqueness >= 0 &&
                    p.uniqueness <= 100 && p.lr_max_diff >= -1 && p.lr_max_diff <= p.num_disp;
    const std::string err = write_maps_to(opt, "viso_kitti_set_disparity", dir, ok, false);
    if (err.empty()) opt.disparity.params = p;
    return err;
}

std::string set_sgm(RunOptions& opt, const char* dir, const viso_sgm_params* params) {
    if (!dir || !*dir) { opt.disparity_on = false; return ""; }
    viso_sgm_params p;
    viso_sgm_params_default(&p);
    if (params) p = *params;
    const bool ok = p.num_disp >= 16 && p.num_disp <= 256 && p.num_disp % 16 == 0 && p.p1 >= 1 && p.p1 <= p.p2 && p.p2 <= 192 &&
                    (p.paths == 4 || p.paths == 8) && p.uniqueness >= 0 && p.uniqueness <= 100 && p.lr_max_diff >= -1 &&
                    p.lr_max_diff <= p.num_disp;
    const std::string err = write_maps_to(opt, "viso_kitti_set_sgm", dir, ok, true);
    if (err.empty()) opt.disparity.sgm_params = p;
    return err;
}

std::string set_speckle(RunOptions& opt, const viso_speckle_params* params) {
    if (!params) { opt.disparity.speckle = false; return ""; }
    if (params->max_size < 0 || params->max_diff < 0 || params->max_diff > 4096)
        return "viso_kitti_set_speckle: parameters outside the ranges of include/viso_hip.h";
    opt.disparity.speckle = true; opt.disparity.speckle_params = *params;
    return "";
}

}  // namespace viso

// ---- C entry points ---------------------------------------------------------------------------------------
static thread_local std::string g_host_err;
// what the viso_kitti_set_* calls of this thread have asked of its next viso_kitti_run_range calls, the rectified projections
// of viso_kitti_set_rectify (used in place of calib.txt while g_opt.rect is set), and what the last range left behind
static thread_local viso::RunOptions g_opt;
static thread_local viso::Matd g_rect_P1, g_rect_P2;
static thread_local viso::RangeResult g_last;

static int report(const std::string& err) {
    if (err.empty()) return VISO_OK;
    g_host_err = err;
    return VISO_ERR_ARG;
}

extern "C" const char* viso_host_last_error(void) { return g_host_err.c_str(); }
namespace viso { void set_host_error(const std::string& s) { g_host_err = s; } }   // for the other C entry points (drop_in.cpp)

extern "C" int viso_kitti_count_frames(const char* seq_base, int begin, int end) {
    if (!seq_base || begin < 0 || end < begin) { g_host_err = "viso_kitti_count_frames: bad argument"; return VISO_ERR_ARG; }
    return viso::kitti_count_frames(seq_base, begin, end);
}

extern "C" int viso_kitti_run_range(const char* seq_base, int begin, int first, int last, int device, int chunk,
                                    uint64_t ransac_seed, double* rec8, int* n_done) {
    if (!seq_base || begin < 0 || first < 0 || last < first || !n_done || (last > first && !rec8)) {
        g_host_err = "viso_kitti_run_range: bad argument";
        return VISO_ERR_ARG;
    }
    *n_done = 0;
    try {
        viso::Matd P1 = g_rect_P1, P2 = g_rect_P2;
        if (!g_opt.rect && !viso::loadCalib(std::string(seq_base) + "/calib.txt", P1, P2)) {
            g_host_err = std::string("cannot read ") + seq_base + "/calib.txt";
            return VISO_ERR_ARG;
        }
        g_last = viso::RangeResult();
        g_opt.device = device; g_opt.chunk = chunk; g_opt.ransac_seed = ransac_seed;
        g_last = viso::kitti_run_range(seq_base, P1, P2, begin, first, last, g_opt);
        const std::vector<viso::FrameRecord>& rec = g_last.rec;
        for (size_t i = 0; i < rec.size(); ++i) {
            for (int j = 0; j < 6; ++j) rec8[i * 8 + (size_t)j] = rec[i].tr[j];
            rec8[i * 8 + 6] = rec[i].ok;
            rec8[i * 8 + 7] = rec[i].n_inl;
        }
        *n_done = (int)rec.size();
        return VISO_OK;
    } catch (const std::exception& e) {
        g_host_err = e.what();
        return VISO_ERR_HIP;
    }
}

extern "C" void viso_kitti_last_stats(double out[9]) {
    const viso::OdometryStats& s = g_last.stats;
    const double v[9] = {(double)s.frames, (double)s.decode_threads, s.wall_s, s.decode_wait_s, s.decode_cpu_s, s.issue_s,
                         s.drain_wait_s, s.upload_ms, s.gpu_ms};
    for (int i = 0; i < 9; ++i) out[i] = v[i];
}

extern "C" void viso_kitti_set_decode_threads(int n) { g_opt.decode_threads = n > 0 ? n : 0; }
extern "C" int viso_kitti_set_subpixel(int mode) { return report(viso::set_subpixel(g_opt, mode)); }
extern "C" int viso_kitti_set_covariance(int mode, double sigma_px) { return report(viso::set_covariance(g_opt, mode, sigma_px)); }
extern "C" int viso_kitti_set_rectify(const char* cam_to_cam_file) {
    return report(viso::set_rectify(g_opt, g_rect_P1, g_rect_P2, cam_to_cam_file));
}
extern "C" int viso_kitti_set_disparity(const char* dir, const viso_disparity_params* params) {
    return report(viso::set_disparity(g_opt, dir, params));
}
extern "C" int viso_kitti_set_sgm(const char* dir, const viso_sgm_params* params) { return report(viso::set_sgm(g_opt, dir, params)); }
extern "C" int viso_kitti_set_speckle(const viso_speckle_params* params) { return report(viso::set_speckle(g_opt, params)); }

extern "C" int viso_kitti_last_covariances(viso_motion_cov* out, int cap, int* n) {
    if (!n || cap < 0 || (cap > 0 && !out)) { g_host_err = "viso_kitti_last_covariances: bad argument"; return VISO_ERR_ARG; }
    const std::vector<viso_motion_cov>& cov = g_last.cov;
    const size_t k = cov.size() < (size_t)cap ? cov.size() : (size_t)cap;
    if (k) std::memcpy(out, cov.data(), sizeof(viso_motion_cov) * k);
    *n = (int)cov.size();
    return VISO_OK;
}

extern "C" int viso_kitti_write_covariances(const char* file_name, const viso_motion_cov* rec, int n) {
    if (!file_name || n < 0 || (n > 0 && !rec)) { g_host_err = "viso_kitti_write_covariances: bad argument"; return VISO_ERR_ARG; }
    viso::mkdirs_for(file_name);
    if (!viso::write_covariance_file(file_name, rec, (size_t)n)) { g_host_err = std::string("cannot write ") + file_name; return VISO_ERR_ARG; }
    return VISO_OK;
}

extern "C" int viso_kitti_load_cam_to_cam(const char* file_name, double K[18], double D[10], double R[18], double P[24], int geometry[4]) {
    if (!file_name || !K || !D || !R || !P || !geometry) { g_host_err = "viso_kitti_load_cam_to_cam: bad argument"; return VISO_ERR_ARG; }
    viso::StereoRectification r;
    viso::Matd P1, P2;
    if (!viso::loadCalibCamToCam(file_name, r, P1, P2)) {
        g_host_err = std::string("cannot read a KITTI raw calib_cam_to_cam file (S, K, D, R_rect, P_rect, S_rect of cameras 00 and 01) from ") +
                     file_name;
        return VISO_ERR_ARG;
    }
    for (int c = 0; c < 2; ++c) {
        for (int i = 0; i < 9; ++i) { K[9 * c + i] = r.K[c].data[(size_t)i]; R[9 * c + i] = r.R[c].data[(size_t)i]; }
        for (int i = 0; i < 5; ++i) D[5 * c + i] = r.D[c].data[(size_t)i];
        for (int i = 0; i < 12; ++i) P[12 * c + i] = r.P[c].data[(size_t)i];
    }
    geometry[0] = r.raw_rows; geometry[1] = r.raw_cols; geometry[2] = r.out_rows; geometry[3] = r.out_cols;
    return VISO_OK;
}

// ---- KITTI stereo PNG (16-bit grayscale) without zlib: stored deflate blocks, checksums computed here ----
namespace {
uint32_t crc32_update(uint32_t c, const uint8_t* p, size_t n) {
    static const std::array<uint32_t, 256> table = [] {   // the reflected polynomial 0xEDB88320 of PNG / zlib
        std::array<uint32_t, 256> t{};
        for (uint32_t i = 0; i < 256; ++i) {
            uint32_t v = i;
            for (int k = 0; k < 8; ++k) v = (v & 1u) ? 0xEDB88320u ^ (v >> 1) : v >> 1;
            t[i] = v;
        }
        return t;
    }();
    for (size_t i = 0; i < n; ++i) c = table[(c ^ p[i]) & 0xFFu] ^ (c >> 8);
    return c;
}
void put32(std::vector<uint8_t>& v, uint32_t x) {
    v.push_back((uint8_t)(x >> 24)); v.push_back((uint8_t)(x >> 16)); v.push_back((uint8_t)(x >> 8)); v.push_back((uint8_t)x);
}
void put_chunk(std::vector<uint8_t>& png, const char type[4], const std::vector<uint8_t>& data) {
    put32(png, (uint32_t)data.size());
    const size_t at = png.size();
    png.insert(png.end(), type, type + 4);
    png.insert(png.end(), data.begin(), data.end());
    put32(png, crc32_update(0xFFFFFFFFu, png.data() + at, 4 + data.size()) ^ 0xFFFFFFFFu);
}
}  // namespace

extern "C" int viso_write_disparity_png(const char* path, const int16_t* d16, int rows, int cols) {
    if (!path || !*path || !d16 || rows <= 0 || cols <= 0 || (long long)cols * 2 + 1 > (1ll << 30)) {
        g_host_err = "viso_write_disparity_png: bad argument";
        return VISO_ERR_ARG;
    }
    // raw scanlines: filter byte 0, then cols big-endian 16-bit values; Adler-32 over them
    const size_t line = (size_t)cols * 2 + 1, total = line * (size_t)rows;
    std::vector<uint8_t> raw(total);
    uint32_t a = 1, b = 0;
    for (int y = 0; y < rows; ++y) {
        uint8_t* o = raw.data() + (size_t)y * line;
        o[0] = 0;
        for (int x = 0; x < cols; ++x) {
            const int v = d16[(size_t)y * cols + x];
            const uint32_t u = v < 0 ? 0u : (uint32_t)v * 16u;   // VISO_DISP_INVALID and every negative value: 0
            o[1 + 2 * x] = (uint8_t)(u >> 8); o[2 + 2 * x] = (uint8_t)u;
        }
    }
    for (size_t i = 0; i < total; ) {   // Adler-32 in runs short enough that the sums cannot overflow before the modulo
        const size_t n = std::min<size_t>(5552, total - i);
        for (size_t k = 0; k < n; ++k) { a += raw[i + k]; b += a; }
        a %= 65521u; b %= 65521u;
        i += n;
    }
    std::vector<uint8_t> z;
    z.reserve(total + total / 65535 * 5 + 16);
    z.push_back(0x78); z.push_back(0x01);   // deflate, 32 K window, no dictionary; (0x7801 % 31 == 0)
    size_t i = 0;
    do {   // stored blocks of at most 65 535 bytes
        const size_t n = std::min<size_t>(65535, total - i);
        const bool last = i + n == total;
        z.push_back(last ? 1 : 0);
        z.push_back((uint8_t)n); z.push_back((uint8_t)(n >> 8));
        z.push_back((uint8_t)~n); z.push_back((uint8_t)(~n >> 8));
        z.insert(z.end(), raw.begin() + (long)i, raw.begin() + (long)(i + n));
        i += n;
    } while (i < total);
    put32(z, (b << 16) | a);
    std::vector<uint8_t> png = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1A, '\n'};
    std::vector<uint8_t> ihdr;
    put32(ihdr, (uint32_t)cols); put32(ihdr, (uint32_t)rows);
    ihdr.push_back(16); ihdr.push_back(0); ihdr.push_back(0); ihdr.push_back(0); ihdr.push_back(0);   // 16-bit gray, no interlace
    put_chunk(png, "IHDR", ihdr);
    put_chunk(png, "IDAT", z);
    put_chunk(png, "IEND", {});
    if (!viso::write_atomically(path, "wb", [&](FILE* fp) { return std::fwrite(png.data(), 1, png.size(), fp) == png.size(); })) {
        g_host_err = std::string("viso_write_disparity_png: cannot write ") + path;
        return VISO_ERR_ARG;
    }
    return VISO_OK;
}

extern "C" int viso_kitti_write_poses(const char* file_name, const double* rec8, int n, int* n_poses) {
    return viso_kitti_write_poses2(file_name, rec8, n, 0, n_poses);
}

extern "C" int viso_kitti_write_poses2(const char* file_name, const double* rec8, int n, int reference_pose_list, int* n_poses) {
    if (!file_name || n < 0 || (n > 0 && !rec8)) { g_host_err = "viso_kitti_write_poses: bad argument"; return VISO_ERR_ARG; }
    std::vector<viso::FrameRecord> rec((size_t)n);
    for (int i = 0; i < n; ++i) {
        for (int j = 0; j < 6; ++j) rec[(size_t)i].tr[j] = rec8[(size_t)i * 8 + (size_t)j];
        rec[(size_t)i].ok = (int32_t)rec8[(size_t)i * 8 + 6];
        rec[(size_t)i].n_inl = (int32_t)rec8[(size_t)i * 8 + 7];
        rec[(size_t)i].frame = rec[(size_t)i].reserved = 0;
    }
    std::vector<viso::Matd> poses = viso::chain_records(rec.data(), n, reference_pose_list != 0);
    viso::mkdirs_for(file_name);
    if (!viso::savePoses(file_name, poses)) { g_host_err = std::string("cannot write ") + file_name; return VISO_ERR_ARG; }
    if (n_poses) *n_poses = (int)poses.size();
    return VISO_OK;
}
