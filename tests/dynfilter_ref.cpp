// An independent CPU restatement of SAGE-ICP's Preprocess() with the dynamic vehicle filter on
// (cpp/sage_icp/core/Preprocessing.cpp:95-172, NeSC-IV/sage-icp @ 2024_10_08), written for the tests of the
// device filter (csrc/dyn_filter.hip).  It shares no code with the library: the radius searches are brute force
// over all points, the clustering is PCL's seed-queue loop (pcl::extractEuclideanClusters), and the cluster order
// comes from the same std::sort(rbegin, rend) call PCL's EuclideanClusterExtraction::extract ends with, applied to
// clusters that carry their index lists.
//
// Built by the tests with g++ -O2 -ffp-contract=off -shared (no FMA: FLANN's L2_Simple is plain mul / add).
// -DSQNORM_A selects the other association of the crop's squared norm (the library's SAGE_SQNORM3_ORDER=0 build).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace {

struct P3 {                      // pcl::PointXYZL: float coordinates, uint32_t label
    float x, y, z;
    uint32_t label;
};

double crop_norm(const double *p) {
#ifdef SQNORM_A
    return std::sqrt(p[0] * p[0] + (p[1] * p[1] + p[2] * p[2]));
#else
    return std::sqrt((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]);   // Eigen's packet order for head<3>().norm()
#endif
}

// FLANN L2_Simple between a query and a data point, accumulated from zero in x, y, z order
float l2_simple(const P3 &a, const P3 &b) {
    float r = 0.0f;
    const float dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
    r += dx * dx;
    r += dy * dy;
    r += dz * dz;
    return r;
}

// radiusSearch(q, 0.5): every point of `cloud` whose squared distance is below 0.5f * 0.5f (strict)
void radius_search(const std::vector<P3> &cloud, const P3 &q, std::vector<int> &hits) {
    const float r2 = 0.5f * 0.5f;
    hits.clear();
    for (size_t j = 0; j < cloud.size(); ++j)
        if (l2_simple(q, cloud[j]) < r2) hits.push_back(static_cast<int>(j));
}

bool listed(const std::vector<int> &v, uint32_t label) {
    // std::find over std::vector<int> with a uint32_t value: the ints convert to unsigned
    return std::find(v.begin(), v.end(), label) != v.end();
}

struct Cluster {                 // pcl::PointIndices
    std::vector<int> indices;
};

bool smaller(const Cluster &a, const Cluster &b) { return a.indices.size() < b.indices.size(); }   // comparePointClusters

// pcl::extractEuclideanClusters + the sort of EuclideanClusterExtraction::extract
std::vector<Cluster> euclidean_clusters(const std::vector<P3> &cloud, size_t min_size, size_t max_size) {
    std::vector<Cluster> clusters;
    std::vector<bool> processed(cloud.size(), false);
    std::vector<int> nn;
    for (size_t i = 0; i < cloud.size(); ++i) {
        if (processed[i]) continue;
        std::vector<int> seed_queue{static_cast<int>(i)};
        processed[i] = true;
        for (size_t sq = 0; sq < seed_queue.size(); ++sq) {
            radius_search(cloud, cloud[seed_queue[sq]], nn);
            for (int j : nn) {
                if (processed[j]) continue;
                seed_queue.push_back(j);
                processed[j] = true;
            }
        }
        if (seed_queue.size() >= min_size && seed_queue.size() <= max_size) {
            Cluster c;
            c.indices = seed_queue;
            std::sort(c.indices.begin(), c.indices.end());
            clusters.push_back(std::move(c));
        }
    }
    std::sort(clusters.rbegin(), clusters.rend(), smaller);
    return clusters;
}

}  // namespace

extern "C" {

// info[5]: vehicle points, landmark points, clusters (>= 5 points), clusters kept, vehicle points removed.
// Returns 0, or -1 when a kept point's label is not finite (the library refuses such a frame as a whole).
int dynref_preprocess(const double *frame, uint64_t n, double max_range, double min_range, double label_max_range,
                      double dy_th, const int *dyn, int n_dyn, const int *lm, int n_lm, double *out, uint64_t *n_out,
                      uint64_t *info) {
    const std::vector<int> dynamic_labels(dyn, dyn + n_dyn), lankmark(lm, lm + n_lm);
    std::vector<P3> map_all, map_vehicle;
    std::vector<const double *> vehicle_rows;
    std::vector<double> zeroed(4 * n);
    std::vector<double> inliers;
    // Preprocessing.cpp:100-124: crop, zero far labels, fp32 copies, split vehicles from the rest
    for (uint64_t i = 0; i < n; ++i) {
        const double *p = frame + 4 * i;
        double *q = zeroed.data() + 4 * i;
        std::memcpy(q, p, 4 * sizeof(double));
        const double norm = crop_norm(p);
        if (!(norm < max_range && norm > min_range)) continue;
        if (norm > label_max_range) q[3] = 0.0;
        if (!std::isfinite(q[3])) return -1;
        P3 t{static_cast<float>(p[0]), static_cast<float>(p[1]), static_cast<float>(p[2]),
             static_cast<uint32_t>(static_cast<long long>(q[3]))};
        map_all.push_back(t);
        if (listed(dynamic_labels, t.label)) {
            map_vehicle.push_back(t);
            vehicle_rows.push_back(q);
        } else {
            inliers.insert(inliers.end(), q, q + 4);
        }
    }
    // :126-137: clusters of the vehicle points (tolerance 0.5, min 5, max = all of them)
    const std::vector<Cluster> clusters = euclidean_clusters(map_vehicle, 5, map_vehicle.size());
    // :139-169: the landmark neighbours of a cluster's points, early exit once the threshold is passed.  Only the
    // landmark points of map_all can count, so the brute-force search runs over those.
    std::vector<P3> landmarks;
    for (const P3 &p : map_all)
        if (listed(lankmark, p.label)) landmarks.push_back(p);
    std::vector<int> nn;
    uint64_t kept = 0, kept_points = 0;
    for (const Cluster &c : clusters) {
        bool is_static = false;
        const int cluster_size = static_cast<int>(c.indices.size());
        int count_size = 0;
        for (int idx : c.indices) {
            radius_search(landmarks, map_vehicle[idx], nn);
            for (size_t k = 0; k < nn.size() && !is_static; ++k) {
                ++count_size;
                if (count_size > static_cast<int>(dy_th * static_cast<double>(cluster_size))) is_static = true;
            }
            if (is_static) break;
        }
        if (!is_static) continue;
        ++kept;
        kept_points += c.indices.size();
        for (int idx : c.indices) inliers.insert(inliers.end(), vehicle_rows[idx], vehicle_rows[idx] + 4);
    }
    if (!inliers.empty()) std::memcpy(out, inliers.data(), inliers.size() * sizeof(double));
    *n_out = inliers.size() / 4;
    if (info) {
        info[0] = map_vehicle.size();
        info[1] = landmarks.size();
        info[2] = clusters.size();
        info[3] = kept;
        info[4] = map_vehicle.size() - kept_points;
    }
    return 0;
}

// PCL's cluster order for clusters found with these sizes: order[j] = which of them comes j-th
void dynref_emission_order(const uint32_t *sizes, uint64_t n, uint32_t *order) {
    std::vector<Cluster> clusters(n);
    for (uint64_t k = 0; k < n; ++k) clusters[k].indices.assign(sizes[k], static_cast<int>(k));
    std::sort(clusters.rbegin(), clusters.rend(), smaller);
    for (uint64_t k = 0; k < n; ++k) order[k] = static_cast<uint32_t>(clusters[k].indices.empty() ? ~0u : clusters[k].indices[0]);
}

}  // extern "C"
