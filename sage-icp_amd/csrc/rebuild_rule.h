// The retention policy of VoxelBlock::AddPoint (reference core/VoxelHashMap.hpp:45-70; HostMap::add_point) on a FRESH
// voxel, in closed form.  Plain C++, host and device: rebuild.hip resolves a voxel's run of arrivals
// with it, a group of lanes at a time, and tests/rebuild_rule_check.cpp holds it to a transcription of AddPoint.
//
// A voxel that starts empty takes its first P1 = max(basic, 1) arrivals unconditionally, in slots 0 .. P1 - 1 (the very
// first by VoxelHashMap.cpp:171, the others because count < basic).  From then on count >= basic for good, so what a
// LATER arrival does depends on its label class and on two counts of later arrivals before it, never on the rows:
//   unlabelled                       dropped
//   critical, k < cap - P1           appended at slot P1 + k     (k: critical later arrivals before it; cap = max(basic +
//                                                                 critical, P1); appends are the only thing that moves
//                                                                 the count, so count == P1 + min(k, cap - P1) there)
//   any other labelled arrival       a replacer: the m-th replacer overwrites the first slot that is still unlabelled.
//                                    Only slots below P1 can be unlabelled (an appended row is critical), each is
//                                    overwritten at most once and in ascending order: it overwrites Z[m], Z the ascending
//                                    list of the unlabelled slots among the first min(L, P1); nothing if m >= |Z|.
// A lane therefore needs its position p in the run, its label class, k and m (two prefix counts over the run, carried
// from group step to group step) and Z (a bit mask of at most 255 bits).  Nothing here depends on the group's width.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SAGE_RULE_HD __host__ __device__ __forceinline__
#else
#define SAGE_RULE_HD inline
#endif

namespace sageicp {

constexpr int kRuleUnlabelled = 0, kRuleBasicPart = 1, kRuleCritical = 2;      // label classes
constexpr int kRuleFirst = 0, kRuleDrop = 1, kRuleAppend = 2, kRuleReplace = 3; // what an arrival is
constexpr uint32_t kRuleNoSlot = 0xFFu;      // (a voxel holds at most 255 rows: slots 0 .. 254)

struct RulePolicy {
    uint32_t P1, cap;
};

SAGE_RULE_HD RulePolicy rule_policy(int basic, int critical) {
    RulePolicy r;
    r.P1 = static_cast<uint32_t>(basic > 1 ? basic : 1);
    const uint32_t bc = static_cast<uint32_t>(basic + critical);
    r.cap = bc > r.P1 ? bc : r.P1;
    return r;
}

SAGE_RULE_HD int rule_code(int label, const int *basic_labels, int n_labels) {
    if (label == 0) return kRuleUnlabelled;
    for (int i = 0; i < n_labels; ++i)
        if (basic_labels[i] == label) return kRuleBasicPart;
    return kRuleCritical;
}

// Z: bit p set iff arrival p < P1 is unlabelled
struct RuleZ {
    uint64_t w[4];
};

SAGE_RULE_HD void rule_z_clear(RuleZ &z) { z.w[0] = z.w[1] = z.w[2] = z.w[3] = 0; }
// bits of positions [64 * word + shift, ..): a group step's ballot (the group's width divides 64: no straddle)
SAGE_RULE_HD void rule_z_or(RuleZ &z, uint32_t word, uint32_t shift, uint64_t bits) {
    const uint64_t b = bits << shift;
    if (word == 0) z.w[0] |= b;
    else if (word == 1) z.w[1] |= b;
    else if (word == 2) z.w[2] |= b;
    else if (word == 3) z.w[3] |= b;
}
SAGE_RULE_HD uint32_t rule_popc(uint64_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return static_cast<uint32_t>(__popcll(v));
#else
    return static_cast<uint32_t>(__builtin_popcountll(v));
#endif
}
SAGE_RULE_HD uint32_t rule_z_count(const RuleZ &z) {
    return rule_popc(z.w[0]) + rule_popc(z.w[1]) + rule_popc(z.w[2]) + rule_popc(z.w[3]);
}
// |{q in Z : q < p}|
SAGE_RULE_HD uint32_t rule_z_rank(const RuleZ &z, uint32_t p) {
    uint32_t n = 0;
    for (uint32_t k = 0; k < 4; ++k) {
        if (p >= 64 * (k + 1)) n += rule_popc(z.w[k]);
        else if (p > 64 * k) n += rule_popc(z.w[k] & ((1ull << (p - 64 * k)) - 1ull));
    }
    return n;
}
// Z[m], or kRuleNoSlot if m >= |Z|
SAGE_RULE_HD uint32_t rule_z_select(const RuleZ &z, uint32_t m) {
    for (uint32_t k = 0; k < 4; ++k) {
        uint64_t w = z.w[k];
        const uint32_t c = rule_popc(w);
        if (m >= c) {
            m -= c;
            continue;
        }
        for (uint32_t j = 0; j < m; ++j) w &= w - 1;       // drop the m lowest set bits
        uint32_t bit = 0;                                  // the lowest one left (w != 0)
        for (uint32_t s = 32; s; s >>= 1)
            if (!(w & ((1ull << s) - 1ull))) {
                w >>= s;
                bit += s;
            }
        return 64 * k + bit;
    }
    return kRuleNoSlot;
}

// arrival p of a run with label class `code`; k: the critical arrivals among the later ones (positions >= P1) before it
SAGE_RULE_HD int rule_kind(const RulePolicy &pol, uint32_t p, int code, uint32_t k) {
    if (p < pol.P1) return kRuleFirst;
    if (code == kRuleUnlabelled) return kRuleDrop;
    if (code == kRuleCritical && k < pol.cap - pol.P1) return kRuleAppend;
    return kRuleReplace;
}
// the slot a later arrival writes (kRuleNoSlot: none); m: the replacers before it; z: complete (every arrival below P1 seen)
SAGE_RULE_HD uint32_t rule_later_slot(const RulePolicy &pol, int kind, uint32_t k, uint32_t m, const RuleZ &z) {
    if (kind == kRuleAppend) return pol.P1 + k;
    if (kind == kRuleReplace) return rule_z_select(z, m);
    return kRuleNoSlot;
}
// the slot arrival p < P1 ends in, once the run's replacers are counted (R): its own, unless a replacer took it
SAGE_RULE_HD uint32_t rule_first_slot(uint32_t p, int code, uint32_t R, const RuleZ &z) {
    if (code == kRuleUnlabelled && rule_z_rank(z, p) < R) return kRuleNoSlot;
    return p;
}
// a run of L arrivals with K critical ones among the later ones and R replacers
SAGE_RULE_HD uint32_t rule_final_count(const RulePolicy &pol, uint32_t L, uint32_t K) {
    const uint32_t first = L < pol.P1 ? L : pol.P1, room = pol.cap - pol.P1;
    return first + (K < room ? K : room);
}
SAGE_RULE_HD uint32_t rule_final_zeros(uint32_t R, const RuleZ &z) {
    const uint32_t nz = rule_z_count(z);
    return nz - (R < nz ? R : nz);
}
// slot 0 ends as the first replacer's row iff the first arrival is unlabelled and there is a replacer
SAGE_RULE_HD bool rule_slot0_replaced(uint32_t R, const RuleZ &z) { return (z.w[0] & 1ull) && R > 0; }

}  // namespace sageicp
