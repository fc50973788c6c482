// Calls sage_icp::DeSkewScan through the opt-in Deskew shim the way pipeline/sageICP.cpp:36-52 does
// (tests/test_deskew_gpu.py).
// usage: deskew_user <frame.f64> <timestamps.f64> <poses.f64> <out.f64>
//   (files: raw little-endian doubles; 4 per point, 1 per point, 14 = start pose then finish pose)
#include <cstdio>
#include <exception>
#include <vector>

#include "sage_icp/core/Deskew.hpp"

int main(int argc, char **argv) {
    if (argc != 5) return 2;
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    std::vector<Eigen::Vector4d> frame;
    Eigen::Vector4d p;
    while (std::fread(p.data(), sizeof(double), 4, f) == 4) frame.push_back(p);
    std::fclose(f);
    std::vector<double> ts(frame.size());
    f = std::fopen(argv[2], "rb");
    if (!f || std::fread(ts.data(), sizeof(double), ts.size(), f) != ts.size()) return 3;
    std::fclose(f);
    Sophus::SE3d start, finish;
    f = std::fopen(argv[3], "rb");
    if (!f || std::fread(start.data(), sizeof(double), 7, f) != 7 || std::fread(finish.data(), sizeof(double), 7, f) != 7)
        return 3;
    std::fclose(f);
    std::vector<Eigen::Vector4d> out;
    try {
        out = sage_icp::DeSkewScan(frame, ts, start, finish);
    } catch (const std::exception &e) {
        std::printf("error: %s\n", e.what());
        return 4;
    }
    std::FILE *g = std::fopen(argv[4], "wb");
    if (!g) return 5;
    for (const auto &q : out) std::fwrite(q.data(), sizeof(double), 4, g);
    std::fclose(g);
    std::printf("deskewed %zu\n", out.size());
    return 0;
}
