// The host books of a replay's priorities (include/hsrsim.h: hsr_replay_priority_*): the spec and argument checks, the sizes of the sum
// tree's stored levels, the clamp of an updated priority and the rule that decides whether a sampled cell still holds the transition it
// was sampled from - plain C++ without a HIP call or header, as replay_logic.h, so that a stand-alone program can exercise it under a
// sanitizer (tests/replay_prio_logic_main.cpp).  host_replay.h asks these functions and launches only what they allow; replay_prio.h
// clamps and tests staleness with the same functions.
#pragma once
#include "replay_logic.h"

// The tree: level 0 = the T N float32 leaves, cell (slot, e) at slot N + e; stored level k >= 1 = ceil(n[k-1] / 64) float64 nodes, node v the
// sum of entries 64 v .. 64 v + 63 of the level below in the order of a binary tree (absent entries are 0); the last level has one node,
// the total.  T N <= 2^30 bounds the stored levels by 5 (64^5 = 2^30).
enum { PRIO_RADIX_LOG2 = 6, PRIO_RADIX = 64, PRIO_MAX_LEVELS = 5 };
static const uint64_t PRIO_MAX_LEAVES = (uint64_t)1 << 30;
struct PrioLevels {
    int levels;                            // stored float64 levels, 1 .. 5
    uint32_t n[PRIO_MAX_LEVELS + 1];       // n[0] leaves, n[k] nodes of level k; n[levels] == 1
    uint32_t offset[PRIO_MAX_LEVELS + 1];  // of level k >= 1 in one array of all nodes
    uint32_t nodes;                        // sum of n[1 ..]
};
static inline PrioLevels prio_levels(uint64_t leaves) {       // 1 <= leaves <= 2^30
    PrioLevels P{};
    P.n[0] = (uint32_t)leaves;
    do {
        const int k = ++P.levels;
        P.n[k] = (P.n[k - 1] + PRIO_RADIX - 1) / PRIO_RADIX;
        P.offset[k] = P.nodes;
        P.nodes += P.n[k];
    } while (P.n[P.levels] > 1);
    return P;
}

struct PrioBooks {
    bool enabled;
    float p_init, p_min, p_max;
    int max_batch;
};

// NULL when priorities may be switched on with these numbers, else why not
static inline const char *prio_enable_error(const ReplayBooks *k, const PrioBooks *p, float p_init, float p_min, float p_max, int max_batch) {
    if (p->enabled) return "priorities are enabled already";
    if (k->state != REPLAY_EMPTY) return "priorities can be enabled only on an empty replay, before the first commit (or right after a clear)";
    if (!isfinite(p_init) || !isfinite(p_min) || !isfinite(p_max)) return "p_init, p_min and p_max must be finite";
    if (!(0.f < p_min && p_min <= p_init && p_init <= p_max)) return "0 < p_min <= p_init <= p_max does not hold";
    if (max_batch < 1) return "max_batch < 1";
    if ((uint64_t)k->T * (uint64_t)k->N > PRIO_MAX_LEAVES) return "capacity_steps x envs above 2^30 leaves";
    return nullptr;
}
static inline const char *prio_sample_error(const ReplayBooks *k, const PrioBooks *p, int batch, float her_ratio) {
    if (!p->enabled) return "priorities are not enabled";
    const char *why = replay_sample_error(k, batch, her_ratio);
    if (why) return why;
    if (batch > p->max_batch) return "batch above the spec's max_batch";
    return nullptr;
}
static inline const char *prio_sample_seq_error(const ReplayBooks *k, const PrioBooks *p, int batch, int seq_len, float her_ratio, float gamma, bool has_out) {
    if (!p->enabled) return "priorities are not enabled";
    const char *why = replay_sample_seq_error(k, batch, seq_len, her_ratio, gamma, has_out);
    if (why) return why;
    if (batch > p->max_batch) return "batch above the spec's max_batch";
    return nullptr;
}
static inline const char *prio_update_error(const ReplayBooks *k, const PrioBooks *p, uint64_t sampled_at, int batch, bool has_arrays) {
    if (!p->enabled) return "priorities are not enabled";
    if (replay_count(k) == 0) return "update of an empty replay";
    if (batch < 1) return "batch < 1";
    if (batch > p->max_batch) return "batch above the spec's max_batch";
    if (!has_arrays) return "null d_index / d_priority";
    if (sampled_at > k->pushed) return "sampled_at above pushed: no sample can have seen that many transitions";
    return nullptr;
}
// records written so far, the pending one included: the cells that hold a transition are those of records W - min(W, T) .. W - 1
static inline uint64_t prio_written(const ReplayBooks *k) { return k->pushed + (k->state == REPLAY_PENDING ? 1u : 0u); }

#ifndef REPLAY_HD
#ifdef __HIPCC__
#define REPLAY_HD __host__ __device__
#else
#define REPLAY_HD
#endif
#endif
// Staleness.  Record k (0-based since the last clear) writes slot k mod T.  With W records written, slot `slot` holds record
// k_s = the largest k < W with k mod T == slot, if there is one.  A sample taken when `sampled_at` records were closed saw records
// < sampled_at only, so the cell still holds what it saw iff k_s exists and k_s < sampled_at.
REPLAY_HD static inline bool prio_cell_live(uint64_t written, int T, int64_t slot, uint64_t sampled_at) {
    if (slot < 0 || slot >= (int64_t)T || written == 0) return false;
    const uint64_t last = written - 1;
    const uint64_t back = (last % (uint64_t)T + (uint64_t)T - (uint64_t)slot) % (uint64_t)T;      // steps from the newest record's slot back to `slot`
    if (back > last) return false;         // the ring has not reached that slot yet
    return last - back < sampled_at;
}
// the value an update stores: x clamped into [p_min, p_max], NaN as p_max
REPLAY_HD static inline float prio_clamp(float x, float p_min, float p_max) {
    if (x != x) return p_max;
    return x < p_min ? p_min : x > p_max ? p_max : x;
}
