// Calls sage_icp::Preprocess(..., dynamic_vehicle_filter = true, ...) through the opt-in Preprocessing shim the way
// pipeline/sageICP.cpp:58-65 does with the SemanticKITTI launch settings (tests/test_dynfilter_gpu.py).
// usage: dynfilter_user <frame.f64> <out.f64> <dy_th>   (files: raw little-endian doubles, 4 per point)
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <vector>

#include "sage_icp/core/Preprocessing.hpp"

int main(int argc, char **argv) {
    if (argc != 4) return 2;
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    std::vector<Eigen::Vector4d> frame;
    Eigen::Vector4d p;
    while (std::fread(p.data(), sizeof(double), 4, f) == 4) frame.push_back(p);
    std::fclose(f);
    const std::vector<int> vehicles{10, 11, 13, 15, 16, 18, 20};     // voxel_labels[dynamic_vehicle_voxid = 5]
    const std::vector<int> lankmark{44, 48};
    std::vector<Eigen::Vector4d> out;
    try {
        out = sage_icp::Preprocess(frame, 100.0, 5.0, 50.0, true, std::atof(argv[3]), vehicles, lankmark);
    } catch (const std::exception &e) {
        std::printf("error: %s\n", e.what());
        return 4;
    }
    std::FILE *g = std::fopen(argv[2], "wb");
    if (!g) return 5;
    for (const auto &q : out) std::fwrite(q.data(), sizeof(double), 4, g);
    std::fclose(g);
    std::printf("filtered %zu -> %zu\n", frame.size(), out.size());
    return 0;
}
