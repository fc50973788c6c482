// csrc/rebuild_rule.h on its own: the closed form of the retention policy on a fresh voxel, stepped in groups of lanes as
// rebuild.hip steps it, against a literal transcription of VoxelBlock::AddPoint (reference core/VoxelHashMap.hpp:45-70,
// VoxelHashMap.cpp:171) applied one arrival after another.  Plain C++: g++, also under -fsanitize=address,undefined.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rebuild_rule.h"

using namespace sageicp;

namespace {

const int kBasicLabels[] = {40, 44, 48};
const int kLabelOf[3] = {0, 44, 71};         // unlabelled, one of basic_parts_labels, any other

struct Voxel {
    std::vector<int> stored;                 // arrival indices in slot order
    bool operator==(const Voxel &o) const { return stored == o.stored; }
};

// ---- the transcription -------------------------------------------------------------------------------------------------
bool is_basic(int label) { return std::find(std::begin(kBasicLabels), std::end(kBasicLabels), label) != std::end(kBasicLabels); }

void replace_first_unlabelled(Voxel &v, const std::vector<int> &labels, int arrival) {
    for (size_t j = 0; j < v.stored.size(); ++j)
        if (labels[v.stored[j]] == 0) {
            v.stored[j] = arrival;
            break;
        }
}

Voxel sequential(const std::vector<int> &labels, int basic, int critical) {
    Voxel v;
    for (int a = 0; a < static_cast<int>(labels.size()); ++a) {
        if (a == 0) {                        // a new voxel takes its first point unconditionally (VoxelHashMap.cpp:171)
            v.stored.push_back(a);
            continue;
        }
        const int label = labels[a];
        if (static_cast<int>(v.stored.size()) < basic) {
            v.stored.push_back(a);
            continue;
        }
        if (label == 0) continue;
        if (is_basic(label)) replace_first_unlabelled(v, labels, a);
        else if (static_cast<int>(v.stored.size()) < basic + critical) v.stored.push_back(a);
        else replace_first_unlabelled(v, labels, a);
    }
    return v;
}

// ---- the closed form, G lanes at a time (k_rb_resolve's steps: ballots become loops over the lanes) -----------------------
struct Resolved {
    Voxel v;
    uint32_t count = 0, zeros = 0;
    int slot0 = -1;                          // the arrival the crop looks at
};

Resolved grouped(const std::vector<int> &labels, int basic, int critical, uint32_t G) {
    const RulePolicy rp = rule_policy(basic, critical);
    const uint32_t L = static_cast<uint32_t>(labels.size());
    std::vector<int> code(L);
    for (uint32_t p = 0; p < L; ++p) code[p] = rule_code(labels[p], kBasicLabels, 3);
    std::vector<uint32_t> slot(L, kRuleNoSlot);
    uint32_t K = 0, R = 0;
    int first_repl = -1;
    RuleZ z;
    rule_z_clear(z);
    for (uint32_t at = 0; at < L; at += G) {
        const uint32_t lanes = std::min(G, L - at);
        uint64_t bz = 0, bc = 0, br = 0;
        for (uint32_t gl = 0; gl < lanes; ++gl) {
            const uint32_t p = at + gl;
            if (p < rp.P1 && code[p] == kRuleUnlabelled) bz |= 1ull << gl;
            if (p >= rp.P1 && code[p] == kRuleCritical) bc |= 1ull << gl;
        }
        if (at < 256) rule_z_or(z, at >> 6, at & 63u, bz);
        std::vector<int> kind(lanes);
        std::vector<uint32_t> k(lanes);
        for (uint32_t gl = 0; gl < lanes; ++gl) {
            k[gl] = K + rule_popc(bc & ((1ull << gl) - 1ull));
            kind[gl] = rule_kind(rp, at + gl, code[at + gl], k[gl]);
            if (kind[gl] == kRuleReplace) br |= 1ull << gl;
        }
        for (uint32_t gl = 0; gl < lanes; ++gl) {
            const uint32_t m = R + rule_popc(br & ((1ull << gl) - 1ull));
            if (kind[gl] == kRuleReplace && m == 0) first_repl = static_cast<int>(at + gl);
            if (kind[gl] != kRuleFirst) slot[at + gl] = rule_later_slot(rp, kind[gl], k[gl], m, z);
        }
        K += rule_popc(bc);
        R += rule_popc(br);
    }
    for (uint32_t p = 0; p < std::min(L, rp.P1); ++p) slot[p] = rule_first_slot(p, code[p], R, z);
    Resolved out;
    out.count = rule_final_count(rp, L, K);
    out.zeros = rule_final_zeros(R, z);
    out.slot0 = rule_slot0_replaced(R, z) ? first_repl : 0;
    out.v.stored.assign(out.count, -1);
    for (uint32_t p = 0; p < L; ++p) {
        if (slot[p] == kRuleNoSlot) continue;
        if (slot[p] >= out.count || out.v.stored[slot[p]] != -1) {       // every slot below count exactly once
            out.v.stored.assign(1, -2);
            return out;
        }
        out.v.stored[slot[p]] = static_cast<int>(p);
    }
    return out;
}

long checked = 0;

bool check(const std::vector<int> &labels, int basic, int critical) {
    const Voxel want = sequential(labels, basic, critical);
    uint32_t zeros = 0;
    for (int a : want.stored) zeros += labels[a] == 0 ? 1u : 0u;
    for (uint32_t G : {16u, 64u}) {
        const Resolved got = grouped(labels, basic, critical, G);
        if (!(got.v == want) || got.count != want.stored.size() || got.zeros != zeros || got.slot0 != want.stored[0]) {
            std::printf("MISMATCH basic %d critical %d G %u length %zu:", basic, critical, G, labels.size());
            for (size_t i = 0; i < labels.size() && i < 40; ++i) std::printf(" %d", labels[i]);
            std::printf("\n want:");
            for (int a : want.stored) std::printf(" %d", a);
            std::printf("\n got (count %u zeros %u slot0 %d):", got.count, got.zeros, got.slot0);
            for (int a : got.v.stored) std::printf(" %d", a);
            std::printf("\n");
            return false;
        }
    }
    ++checked;
    return true;
}

// xorshift: the same runs everywhere
uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return static_cast<uint32_t>(rng_state >> 32);
}

}  // namespace

int main() {
    // every label sequence of length <= 9
    const int policies[][2] = {{1, 0}, {1, 1}, {2, 2}, {3, 1}, {2, 0}, {0, 1}, {0, 3}};
    for (const auto &pc : policies) {
        long before = checked;
        for (int len = 1; len <= 9; ++len) {
            long total = 1;
            for (int i = 0; i < len; ++i) total *= 3;
            std::vector<int> labels(len);
            for (long s = 0; s < total; ++s) {
                long v = s;
                for (int i = 0; i < len; ++i, v /= 3) labels[i] = kLabelOf[v % 3];
                if (!check(labels, pc[0], pc[1])) return 1;
            }
        }
        std::printf("(basic %d, critical %d): %ld sequences of length <= 9\n", pc[0], pc[1], checked - before);
    }
    // seeded runs around the group widths, a workgroup's 256 positions and beyond, at the default policy
    const int lengths[] = {15, 16, 17, 63, 64, 65, 255, 256, 257, 320};
    // shares (of 16) of unlabelled and basic-part labels: mostly unlabelled first rows with few / many replacers, mostly critical
    const int mixes[][2] = {{8, 4}, {14, 1}, {2, 2}, {5, 10}, {0, 0}, {16, 0}, {12, 4}};
    long before = checked;
    for (int len : lengths)
        for (const auto &mix : mixes)
            for (int rep = 0; rep < 40; ++rep) {
                std::vector<int> labels(len);
                for (int i = 0; i < len; ++i) {
                    const int r = static_cast<int>(rnd() % 16u);
                    labels[i] = r < mix[0] ? 0 : r < mix[0] + mix[1] ? kBasicLabels[rnd() % 3u] : 71 + static_cast<int>(rnd() % 3u);
                }
                if (!check(labels, 20, 20)) return 1;
                if (!check(labels, 3, 2)) return 1;
                if (!check(labels, 100, 155)) return 1;       // Z beyond one 64-bit word, the largest voxel
            }
    std::printf("seeded runs of 15 .. 320 arrivals: %ld\n", checked - before);
    std::printf("rebuild_rule_check: ok (%ld runs, groups of 16 and of 64)\n", checked);
    return 0;
}
