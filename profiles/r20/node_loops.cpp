// The odometry node's two host loops, written out for profiles/r20/msg_probe.py: the parent's way of producing the bytes
// the message entries produce on the device.  Single-threaded; built with g++ -O2 -shared -fPIC by the probe.
//   fill_xyzlrgb   the node's FillPointCloud2XYZlRGB: one pass over double[n][4] rows with a std::map<int, int>::at
//                  colour lookup, writing 21-byte records (x, y, z float32, label uint8, rgb uint32, 4 bytes left zero)
//   expand_xyzl    the node's PointCloud2ToEigen: float32 x, y, z and a uint8 or float32 label at byte offsets of a
//                  point_step-strided blob into double[n][4]; expand_stamps: uint32 stamps cast and divided by their maximum
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <map>

extern "C" {

void *colors_new(const int *keys, const int *values, int n) {
    auto *m = new std::map<int, int>();
    for (int i = 0; i < n; ++i) (*m)[keys[i]] = values[i];
    return m;
}
void colors_free(void *m) { delete static_cast<std::map<int, int> *>(m); }

void fill_xyzlrgb(const double *rows, size_t n, const void *colors, uint8_t *out) {
    const auto &color_list = *static_cast<const std::map<int, int> *>(colors);
    for (size_t i = 0; i < n; ++i) {
        const double *p = rows + 4 * i;
        uint8_t *r = out + 21 * i;
        const float x = static_cast<float>(p[0]), y = static_cast<float>(p[1]), z = static_cast<float>(p[2]);
        std::memcpy(r, &x, 4);
        std::memcpy(r + 4, &y, 4);
        std::memcpy(r + 8, &z, 4);
        r[12] = static_cast<uint8_t>(p[3]);
        const uint32_t rgb = static_cast<uint32_t>(color_list.at(static_cast<int>(p[3])));
        std::memcpy(r + 13, &rgb, 4);
    }
}

void expand_xyzl(const uint8_t *blob, size_t n, uint32_t step, uint32_t xo, uint32_t yo, uint32_t zo, uint32_t lo,
                 int label_is_u8, double *out) {
    for (size_t i = 0; i < n; ++i) {
        const uint8_t *r = blob + i * step;
        float x, y, z;
        std::memcpy(&x, r + xo, 4);
        std::memcpy(&y, r + yo, 4);
        std::memcpy(&z, r + zo, 4);
        double l;
        if (label_is_u8) {
            l = r[lo];
        } else {
            float f;
            std::memcpy(&f, r + lo, 4);
            l = f;
        }
        double *o = out + 4 * i;
        o[0] = x; o[1] = y; o[2] = z; o[3] = l;
    }
}

void expand_stamps(const uint8_t *blob, size_t n, uint32_t step, uint32_t to, double *out) {
    for (size_t i = 0; i < n; ++i) {
        uint32_t t;
        std::memcpy(&t, blob + i * step + to, 4);
        out[i] = static_cast<double>(t);
    }
    if (!n) return;
    const double m = *std::max_element(out, out + n);
    if (m < 1.0) return;
    for (size_t i = 0; i < n; ++i) out[i] = out[i] / m;
}
}
