// The host path a caller of the odometry node has without the device entries: the raw frame moved into the last key
// frame's coordinates, its bird's-eye grid drawn into nested vectors and the overlap with the key grid counted — the
// node's own data structures (ros/ros2/Utils.hpp:221-260, OdometryServer.cpp:233-235), restated here in plain C++.
// Reads <frame.bin>: uint64 n, then n rows of 4 doubles, then a pose (qx qy qz qw tx ty tz); prints the median
// microseconds of transform + grid + overlap, and of one grid alone, over `reps` calls.
#include <algorithm>
#include <array>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <vector>

using Rows = std::vector<std::array<double, 4>>;
using Grid = std::vector<std::vector<int>>;

static const double B[3][2] = {{-51.2, 51.2}, {-51.2, 51.2}, {-4.0, 2.4}};
static const int H = 128, W = 128;

static Grid grid_of(const Rows &pts) {
    Grid g(H, std::vector<int>(W, 0));
    const double xr = (B[0][1] - B[0][0]) / W, yr = (B[1][1] - B[1][0]) / H;
    for (const auto &p : pts) {
        if (p[0] < B[0][0] || p[0] > B[0][1] || p[1] < B[1][0] || p[1] > B[1][1] || p[2] < B[2][0] || p[2] > B[2][1])
            continue;
        const double vx = (p[0] + B[0][1]) / xr, vy = (p[1] + B[1][1]) / yr;
        if (vx > -1.0 && vx < W && vy > -1.0 && vy < H) g[static_cast<int>(vy)][static_cast<int>(vx)] = 1;
    }
    return g;
}

static double overlap(const Grid &k, const Grid &c) {
    long inter = 0, total = 0;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            inter += k[y][x] == 1 && c[y][x] == 1;
            total += k[y][x] == 1;
        }
    return static_cast<double>(inter) / total;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    const int reps = argc > 2 ? std::atoi(argv[2]) : 50;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint64_t n = 0;
    if (std::fread(&n, 8, 1, f) != 1) return 2;
    Rows pts(n);
    double q[7];
    if (std::fread(pts.data(), 32, n, f) != n || std::fread(q, 8, 7, f) != 7) return 2;
    std::fclose(f);
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    const double R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                         2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                         2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)};
    const Grid key = grid_of(pts);
    std::vector<double> t_full, t_grid;
    double sink = 0;
    for (int r = 0; r < reps; ++r) {
        const auto t0 = std::chrono::steady_clock::now();
        Rows moved = pts;                                   // TransformToLastFrame copies the frame
        for (auto &p : moved) {
            const double a = p[0], b = p[1], c = p[2];
            p[0] = R[0] * a + R[1] * b + R[2] * c + q[4];
            p[1] = R[3] * a + R[4] * b + R[5] * c + q[5];
            p[2] = R[6] * a + R[7] * b + R[8] * c + q[6];
        }
        const Grid cur = grid_of(moved);
        sink += overlap(key, cur);
        const auto t1 = std::chrono::steady_clock::now();
        const Grid g = grid_of(pts);
        const auto t2 = std::chrono::steady_clock::now();
        sink += g[H / 2][W / 2];
        t_full.push_back(std::chrono::duration<double, std::micro>(t1 - t0).count());
        t_grid.push_back(std::chrono::duration<double, std::micro>(t2 - t1).count());
    }
    std::sort(t_full.begin(), t_full.end());
    std::sort(t_grid.begin(), t_grid.end());
    std::printf("host transform+grid+overlap_us %.1f grid_us %.1f (n=%llu, reps=%d, sink %.3f)\n", t_full[reps / 2],
                t_grid[reps / 2], static_cast<unsigned long long>(n), reps, sink);
    return 0;
}
