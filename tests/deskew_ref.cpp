// Independent CPU restatement of the reference's deskew (core/Deskew.cpp:31-50, DeSkewScan) for the tests: the SE(3)
// arithmetic is written out here from Sophus 1.22's formulas (the version 3rdparty/sophus/sophus.cmake pins), not from
// csrc/se3_math.h, so that the product's exp / log / point action are checked against a second statement of them.
// Pose layout {qx, qy, qz, qw, tx, ty, tz} == Sophus::SE3d::data(); tangent (upsilon, omega), translation first.
//   SO3::expAndTheta          theta^2 < eps^2: series for the quaternion factors (and theta = 0), else sin / cos
//   SO3::leftJacobian         theta^2 < eps^2: I + 1/2 Omega, else I + (1 - cos)/th^2 Omega + (th - sin)/th^3 Omega^2
//   SO3::logAndTheta          |q.vec|^2 < eps^2: series of 2 atan(n / w) / n, else atan2 with the sign of w folded
//   SO3::leftJacobianInverse  theta^2 < eps: I - 1/2 Omega + 1/12 Omega^2, else the half-angle cot form
//   SO3::operator*(point)     p + w (2 v x p) + v x (2 v x p)
//   SO3 * SO3                 Eigen's quaternion product, rescaled by 2 / (1 + |q|^2) when |q|^2 != 1
//   SO3(quaternion)           normalises (SE3::inverse builds its rotation that way)
// eps = Sophus::Constants<double>::epsilon() = 1e-10.  Matrices are formed and applied as Eigen would (row times
// column, left to right); -ffp-contract=off keeps every product and sum a separate rounding.
#include <cmath>
#include <cstdint>

namespace {

constexpr double kEps = 1e-10;

struct M3 {
    double m[3][3];
};

M3 hat(const double w[3]) {
    return M3{{{0.0, -w[2], w[1]}, {w[2], 0.0, -w[0]}, {-w[1], w[0], 0.0}}};
}
M3 mul(const M3 &a, const M3 &b) {
    M3 r{};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) r.m[i][j] = (a.m[i][0] * b.m[0][j] + a.m[i][1] * b.m[1][j]) + a.m[i][2] * b.m[2][j];
    return r;
}
void apply(const M3 &a, const double v[3], double o[3]) {
    for (int i = 0; i < 3; ++i) o[i] = (a.m[i][0] * v[0] + a.m[i][1] * v[1]) + a.m[i][2] * v[2];
}
// I + a A + b B
M3 combo(double a, const M3 &A, double b, const M3 &B) {
    M3 r{};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) r.m[i][j] = ((i == j ? 1.0 : 0.0) + a * A.m[i][j]) + b * B.m[i][j];
    return r;
}

// SO3 * point, Sophus's cross-product form
void rotate(const double q[4], const double p[3], double o[3]) {
    const double v[3] = {q[0], q[1], q[2]};
    double uv[3] = {v[1] * p[2] - v[2] * p[1], v[2] * p[0] - v[0] * p[2], v[0] * p[1] - v[1] * p[0]};
    for (double &x : uv) x += x;
    const double c[3] = {v[1] * uv[2] - v[2] * uv[1], v[2] * uv[0] - v[0] * uv[2], v[0] * uv[1] - v[1] * uv[0]};
    for (int i = 0; i < 3; ++i) o[i] = (p[i] + q[3] * uv[i]) + c[i];
}

}  // namespace

extern "C" {

void dsr_exp(const double a[6], double T[7]) {
    const double w[3] = {a[3], a[4], a[5]};
    const double theta_sq = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
    double theta, imag, real;
    if (theta_sq < kEps * kEps) {
        theta = 0.0;
        const double theta_po4 = theta_sq * theta_sq;
        imag = (0.5 - (1.0 / 48.0) * theta_sq) + (1.0 / 3840.0) * theta_po4;
        real = (1.0 - (1.0 / 8.0) * theta_sq) + (1.0 / 384.0) * theta_po4;
    } else {
        theta = std::sqrt(theta_sq);
        const double half = 0.5 * theta;
        imag = std::sin(half) / theta;
        real = std::cos(half);
    }
    T[0] = imag * w[0]; T[1] = imag * w[1]; T[2] = imag * w[2]; T[3] = real;
    // leftJacobian(omega, theta)
    const M3 O = hat(w), O2 = mul(O, O);
    const double th2 = theta * theta;
    M3 V;
    if (th2 < kEps * kEps) {
        V = combo(0.5, O, 0.0, O2);
    } else {
        V = combo((1.0 - std::cos(theta)) / th2, O, (theta - std::sin(theta)) / (th2 * theta), O2);
    }
    apply(V, a, T + 4);
}

void dsr_log(const double T[7], double a[6]) {
    const double squared_n = (T[0] * T[0] + T[1] * T[1]) + T[2] * T[2];
    const double w = T[3];
    double k, theta;
    if (squared_n < kEps * kEps) {
        const double squared_w = w * w;
        k = 2.0 / w - (2.0 / 3.0) * squared_n / (w * squared_w);
        theta = 2.0 * squared_n / w;
    } else {
        const double n = std::sqrt(squared_n);
        const double atan_nbyw = (w < 0.0) ? std::atan2(-n, -w) : std::atan2(n, w);
        k = 2.0 * atan_nbyw / n;
        theta = k * n;
    }
    const double om[3] = {k * T[0], k * T[1], k * T[2]};
    const M3 O = hat(om), O2 = mul(O, O);
    const double theta_sq = theta * theta;
    M3 Vi;
    if (theta_sq < kEps) {
        Vi = combo(-0.5, O, 1.0 / 12.0, O2);
    } else {
        const double half = 0.5 * theta;
        Vi = combo(-0.5, O, (1.0 - 0.5 * theta * std::cos(half) / std::sin(half)) / (theta * theta), O2);
    }
    apply(Vi, T + 4, a);
    a[3] = om[0]; a[4] = om[1]; a[5] = om[2];
}

void dsr_inv(const double T[7], double O[7]) {
    double q[4] = {-T[0], -T[1], -T[2], T[3]};
    const double len = std::sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
    for (double &x : q) x /= len;
    const double mt[3] = {T[4] * -1.0, T[5] * -1.0, T[6] * -1.0};
    rotate(q, mt, O + 4);
    for (int i = 0; i < 4; ++i) O[i] = q[i];
}

void dsr_mul(const double A[7], const double B[7], double O[7]) {
    double t[3];
    rotate(A, B + 4, t);
    const double ax = A[0], ay = A[1], az = A[2], aw = A[3], bx = B[0], by = B[1], bz = B[2], bw = B[3];
    double q[4] = {((aw * bx + ax * bw) + ay * bz) - az * by, ((aw * by + ay * bw) + az * bx) - ax * bz,
                   ((aw * bz + az * bw) + ax * by) - ay * bx, ((aw * bw - ax * bx) - ay * by) - az * bz};
    const double sq = ((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3];
    if (sq != 1.0) {
        const double scale = 2.0 / (1.0 + sq);
        for (double &x : q) x *= scale;
    }
    for (int i = 0; i < 4; ++i) O[i] = q[i];
    for (int i = 0; i < 3; ++i) O[4 + i] = A[4 + i] + t[i];
}

void dsr_apply(const double T[7], const double p[3], double o[3]) {
    rotate(T, p, o);
    for (int i = 0; i < 3; ++i) o[i] += T[4 + i];
}

// Deskew.cpp:36: (start_pose.inverse() * finish_pose).log()
void dsr_delta(const double start[7], const double finish[7], double delta[6]) {
    double inv[7], rel[7];
    dsr_inv(start, inv);
    dsr_mul(inv, finish, rel);
    dsr_log(rel, delta);
}

// Deskew.cpp:31-50 with a given delta; out may equal frame
void dsr_deskew_delta(const double *frame, const double *ts, uint64_t n, const double delta[6], double *out) {
    for (uint64_t i = 0; i < n; ++i) {
        const double s = ts[i] - 0.5;
        double a[6], T[7], o[3];
        for (int j = 0; j < 6; ++j) a[j] = s * delta[j];
        dsr_exp(a, T);
        const double p[3] = {frame[4 * i], frame[4 * i + 1], frame[4 * i + 2]};
        dsr_apply(T, p, o);
        const double l = frame[4 * i + 3];
        out[4 * i] = o[0]; out[4 * i + 1] = o[1]; out[4 * i + 2] = o[2]; out[4 * i + 3] = l;
    }
}

void dsr_deskew(const double *frame, const double *ts, uint64_t n, const double start[7], const double finish[7],
                double *out) {
    double delta[6];
    dsr_delta(start, finish, delta);
    dsr_deskew_delta(frame, ts, n, delta, out);
}

}  // extern "C"
