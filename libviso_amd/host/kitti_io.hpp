// kitti_io.hpp — the two file formats the reference's kitti driver reads and
// writes (alexkreimer/libviso src/kitti.cpp:23-64), restated:
//   calib.txt : "P0: <12 doubles>\nP1: <12 doubles>" (3x4 row-major each; the
//               driver reads the first two lines, :31-44)
//   poses     : one line per pose, 12 x "%lf" = first three rows of the 4x4
//               pose, six decimals (:56-60)
// and, for the opt-in rectification of raw images (not in the reference), KITTI raw's calib_cam_to_cam.txt.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

#include "viso.hpp"

namespace viso {

inline bool loadCalib(const std::string& file_name, Matd& p1, Matd& p2) {
    FILE* fp = std::fopen(file_name.c_str(), "r");
    if (!fp) return false;
    p1.create(3, 4); p2.create(3, 4);
    int n = 0;
    bool ok = std::fscanf(fp, "P%d:", &n) == 1;
    for (int i = 0; ok && i < 12; ++i) ok = std::fscanf(fp, "%lf", &p1.data[(size_t)i]) == 1;
    ok = ok && std::fscanf(fp, " P%d:", &n) == 1;
    for (int i = 0; ok && i < 12; ++i) ok = std::fscanf(fp, "%lf", &p2.data[(size_t)i]) == 1;
    std::fclose(fp);
    return ok;
}

// KITTI raw calib_cam_to_cam.txt: lines "<key>: <values>".  Camera 0 (keys *_00) is the left one, camera 1 (*_01) the right
// one; per camera S (raw width height), K (3x3), D (k1 k2 p1 p2 k3), R_rect (3x3), P_rect (3x4) and S_rect (rectified width
// height).  Fills rect (border 0) and P1 = P_rect_00, P2 = P_rect_01 (for F_from_P and the solver's param).  false when the
// file cannot be read, a key is missing or has the wrong number of values, the two cameras disagree on a geometry, or a
// geometry is not a positive integer pair.
inline bool loadCalibCamToCam(const std::string& file_name, StereoRectification& rect, Matd& P1, Matd& P2) {
    FILE* fp = std::fopen(file_name.c_str(), "r");
    if (!fp) return false;
    std::map<std::string, std::vector<double>> kv;
    std::string line;
    for (int ch = 0; ch != EOF;) {
        line.clear();
        while ((ch = std::fgetc(fp)) != EOF && ch != '\n') line += (char)ch;
        const size_t colon = line.find(':');
        if (colon == std::string::npos) continue;
        std::vector<double> v;
        const char* p = line.c_str() + colon + 1;
        for (;;) {   // the numbers of the line (calib_time's value is not one: it gets none)
            char* end = nullptr;
            const double x = std::strtod(p, &end);
            if (end == p) break;
            v.push_back(x);
            p = end;
        }
        kv[line.substr(0, colon)] = v;
    }
    std::fclose(fp);
    auto get = [&kv](const std::string& key, size_t n, std::vector<double>& out) {
        auto it = kv.find(key);
        if (it == kv.end() || it->second.size() != n) return false;
        out = it->second;
        return true;
    };
    auto as_int = [](double x, int& out) {
        if (!(x >= 1.0 && x <= 1e6) || x != (double)(int)x) return false;
        out = (int)x;
        return true;
    };
    StereoRectification r;
    int geo[2][4];
    for (int c = 0; c < 2; ++c) {
        const std::string id = c ? "01" : "00";
        std::vector<double> S, K, D, R, P, Sr;
        if (!get("S_" + id, 2, S) || !get("K_" + id, 9, K) || !get("D_" + id, 5, D) || !get("R_rect_" + id, 9, R) ||
            !get("P_rect_" + id, 12, P) || !get("S_rect_" + id, 2, Sr))
            return false;
        if (!as_int(S[0], geo[c][1]) || !as_int(S[1], geo[c][0]) || !as_int(Sr[0], geo[c][3]) || !as_int(Sr[1], geo[c][2])) return false;
        r.K[c].create(3, 3); r.K[c].data = K;
        r.D[c].create(1, 5); r.D[c].data = D;
        r.R[c].create(3, 3); r.R[c].data = R;
        r.P[c].create(3, 4); r.P[c].data = P;
    }
    for (int k = 0; k < 4; ++k)
        if (geo[0][k] != geo[1][k]) return false;
    r.raw_rows = geo[0][0]; r.raw_cols = geo[0][1]; r.out_rows = geo[0][2]; r.out_cols = geo[0][3];
    rect = r;
    P1 = r.P[0];
    P2 = r.P[1];
    return true;
}

inline bool savePoses(const std::string& file_name, const std::vector<Matd>& poses) {
    FILE* fp = std::fopen(file_name.c_str(), "w+");
    if (!fp) return false;
    for (const Matd& pose : poses) {
        std::fprintf(fp, "%lf %lf %lf %lf %lf %lf %lf %lf %lf %lf %lf %lf\n",
                     pose.at(0, 0), pose.at(0, 1), pose.at(0, 2), pose.at(0, 3),
                     pose.at(1, 0), pose.at(1, 1), pose.at(1, 2), pose.at(1, 3),
                     pose.at(2, 0), pose.at(2, 1), pose.at(2, 2), pose.at(2, 3));
    }
    std::fclose(fp);
    return true;
}

}  // namespace viso
