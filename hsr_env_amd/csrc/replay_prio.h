// Prioritised replay on the device (include/hsrsim.h: hsr_replay_priority_*): a sum tree over the ring's cells and the kernels that keep
// and search it.  Opt-in per replay; nothing here is launched for a replay that never enables it, and nothing touches the simulation state.
//
// Storage (replay_prio_logic.h has the level sizes): leaf [T N] float32, cell (slot, e) at slot N + e - one record writes one contiguous run
// of N leaves; node: the stored float64 levels, radix 64, in one array; p_new: the bit pattern of the priority a new transition gets;
// cell [max_batch]: the leaf of every sample of the draw in flight (descent -> row copy) or of every row of an update (mark -> max -> re-sum).
//
// One wave per node.  A wave loads the node's 64 children, one per lane, widened to float64 (exact), and adds them with an xor-butterfly:
// after stage t every lane holds the sum of the 2^t-aligned block of children it belongs to, and because a + b == b + a bit for bit both
// halves of a block compute the same value - the six stages ARE the six binary levels below the node, every inner sum one float64
// addition of its two children.  Absent children are +0, which changes no sum of non-negative values.  A float64 crosses lanes as two
// 32-bit moves.  No floating-point atomics: the only atomics are integer maxima on bit patterns of positive floats (update), whose
// result does not depend on their order.
#pragma once
#include "replay_prio_logic.h"

enum { EP_STREAM_PRIO = 6 };
enum { PRIO_BLOCK = 256, PRIO_WAVE = 64, PRIO_WAVES = PRIO_BLOCK / PRIO_WAVE };

struct PrioDev {
    float *leaf;
    double *node;
    uint32_t *p_new;
    int32_t *cell;
    PrioLevels L;
    float p_min, p_max;
};

__device__ __forceinline__ double prio_shfl_xor(double v, int mask) {
    return __hiloint2double(__shfl_xor(__double2hiint(v), mask, PRIO_WAVE), __shfl_xor(__double2loint(v), mask, PRIO_WAVE));
}
__device__ __forceinline__ double prio_shfl(double v, int lane) {
    return __hiloint2double(__shfl(__double2hiint(v), lane, PRIO_WAVE), __shfl(__double2loint(v), lane, PRIO_WAVE));
}
// entry c of level k - 1 as a float64; level 0 is the float32 leaves
__device__ __forceinline__ double prio_child(const PrioDev &P, int k, uint32_t c) {
    if (c >= P.L.n[k - 1]) return 0.0;
    return k == 1 ? (double)P.leaf[c] : P.node[P.L.offset[k - 1] + c];
}
// s[t] = the sum of this lane's 2^t-block of the node's children, t = 0 .. 6; the whole wave calls it
__device__ __forceinline__ void prio_butterfly(double own, double s[PRIO_RADIX_LOG2 + 1]) {
    s[0] = own;
#pragma unroll
    for (int t = 0; t < PRIO_RADIX_LOG2; t++) s[t + 1] = s[t] + prio_shfl_xor(s[t], 1 << t);
}
__device__ __forceinline__ void prio_resum_node(const PrioDev &P, int k, uint32_t v, int lane) {     // v < n[k], wave-uniform
    double s[PRIO_RADIX_LOG2 + 1];
    prio_butterfly(prio_child(P, k, v * PRIO_RADIX + (uint32_t)lane), s);
    if (lane == 0) P.node[P.L.offset[k] + v] = s[PRIO_RADIX_LOG2];
}

// record: the N leaves of the slot just written take p_new
__global__ void __launch_bounds__(PRIO_BLOCK) k_prio_set_leaves(PrioDev P, uint32_t lo, uint32_t n) {
    const uint32_t i = blockIdx.x * (uint32_t)PRIO_BLOCK + threadIdx.x;
    if (i < n && lo + i < P.L.n[0]) P.leaf[lo + i] = __uint_as_float(*P.p_new);
}
// re-sum nodes lo .. lo + count - 1 of level k from their children; launched level by level, so the children are final
__global__ void __launch_bounds__(PRIO_BLOCK) k_prio_resum_range(PrioDev P, int k, uint32_t lo, uint32_t count) {
    const uint32_t w = blockIdx.x * (uint32_t)PRIO_WAVES + threadIdx.x / PRIO_WAVE;
    if (w >= count || lo + w >= P.L.n[k]) return;
    prio_resum_node(P, k, lo + w, threadIdx.x % PRIO_WAVE);
}
// re-sum the level-k ancestor of every marked row's leaf (cell[row] < 0: a skipped row).  Rows that share an ancestor store the same
// value: it is a function of the children alone.
__global__ void __launch_bounds__(PRIO_BLOCK) k_prio_resum_rows(PrioDev P, int k, int batch) {
    const int row = blockIdx.x * PRIO_WAVES + threadIdx.x / PRIO_WAVE;
    if (row >= batch) return;
    const int32_t c = P.cell[row];
    if (c < 0 || (uint32_t)c >= P.L.n[0]) return;
    prio_resum_node(P, k, (uint32_t)c >> (PRIO_RADIX_LOG2 * k), threadIdx.x % PRIO_WAVE);
}

// descent: one wave per sample.  u = ((i + r) / batch) total with r the 53-bit fraction of words 0 and 1, each operation a float64
// operation of its own (no contraction).  At every stored node the wave rebuilds the six binary levels below it with the butterfly and
// walks them: at a binary node with children (l, r) go left if u < l or r == 0, else u -= l and go right.  l and r are read from the lanes
// that start the two blocks; the walk is the same in every lane.  A positive total leads to a positive leaf (DESIGN.md has the argument),
// so the leaf is a stored cell; the index is clamped below n[0] all the same, and nothing is read past a level's end (prio_child).
__global__ void __launch_bounds__(PRIO_BLOCK) k_prio_descend(PrioDev P, uint32_t key0, uint32_t key1, uint32_t env_offset, uint32_t draw, int batch,
                                                             float *prob) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * PRIO_WAVES + threadIdx.x / PRIO_WAVE, lane = threadIdx.x % PRIO_WAVE;
    if (i >= batch) return;
    const Philox4 p = philox4x32_10((uint32_t)i, draw, EP_STREAM_PRIO, env_offset, key0, key1);
    const double total = P.node[P.L.offset[P.L.levels]];
    const double r = (double)(((uint64_t)(p.x >> 5) << 26) + (uint64_t)(p.y >> 6)) * 0x1p-53;
    double u = ((double)i + r) / (double)batch;
    u = u * total;
    uint32_t v = 0;
    double leaf = 0.0;
    for (int k = P.L.levels; k >= 1; k--) {
        double s[PRIO_RADIX_LOG2 + 1];
        prio_butterfly(prio_child(P, k, v * PRIO_RADIX + (uint32_t)lane), s);
        int at = 0;
#pragma unroll
        for (int t = PRIO_RADIX_LOG2 - 1; t >= 0; t--) {
            const double l = prio_shfl(s[t], at), rt = prio_shfl(s[t], at + (1 << t));
            if (!(u < l || rt == 0.0)) { u = u - l; at += 1 << t; }
        }
        v = v * PRIO_RADIX + (uint32_t)at;
        leaf = prio_shfl(s[0], at);
    }
    if (lane != 0) return;
    P.cell[i] = (int32_t)(v < P.L.n[0] ? v : P.L.n[0] - 1);
    if (prob) prob[i] = (float)(leaf / total);
}

// the draw of a prioritised sample from the cell the descent left: (e, slot) = the leaf, age = (slot - first + T) mod T; relabel and the
// goal word are words 2 and 3 of the same Philox block, used as replay_draw uses them
__device__ __forceinline__ ReplayDraw prio_draw(const ReplayDev &R, const int32_t *cell, int i, uint32_t draw, int first, int count, float her_ratio) {
    const Philox4 p = philox4x32_10((uint32_t)i, draw, EP_STREAM_PRIO, R.env_offset, R.key0, R.key1);
    const int c = cell[i], slot = c / R.N;
    ReplayDraw d;
    d.e = c - slot * R.N;
    d.j = slot - first + (slot < first ? R.T : 0);
    if (d.j >= count) d.j = count - 1;     // never for a leaf with a priority: only stored cells have one; keeps every age the sampler forms below count
    d.relabel = (float)(p.z >> 8) * 5.9604644775390625e-8f < her_ratio;
    d.goal_word = p.w;
    return d;
}
// the samplers: the bodies of k_replay_sample and k_replay_sample_seq (replay.h) from the prioritised draw
__global__ void __launch_bounds__(REPLAY_BLOCK) k_prio_sample(ReplayDev R, const int32_t *cell, int first, int count, uint32_t draw, int batch, float her_ratio,
                                                              uint32_t *obs, uint32_t *act, uint32_t *next_obs, uint32_t *goal, uint32_t *achieved_next,
                                                              uint32_t *reward, uint8_t *done, int32_t *index) {
    const int i = blockIdx.x * REPLAY_PER_BLOCK + threadIdx.x / REPLAY_GROUP, lane = threadIdx.x % REPLAY_GROUP;
    if (i >= batch) return;
    replay_sample_rows(R, first, count, prio_draw(R, cell, i, draw, first, count, her_ratio), i, lane, obs, act, next_obs, goal, achieved_next, reward, done, index);
}
__global__ void __launch_bounds__(REPLAY_BLOCK) k_prio_sample_seq(ReplayDev R, const int32_t *cell, int first, int count, uint32_t draw, int batch, int seq_len,
                                                                  float her_ratio, float gamma, hsr_replay_seq_out O) {
    const uint32_t gi = blockIdx.x * (uint32_t)REPLAY_PER_BLOCK + threadIdx.x / REPLAY_GROUP;
    const int lane = threadIdx.x % REPLAY_GROUP;
    if (gi >= (uint32_t)batch * (uint32_t)seq_len) return;
    const int i = (int)(gi / (uint32_t)seq_len), k = (int)(gi - (uint32_t)i * (uint32_t)seq_len);
    replay_sample_seq_rows(R, first, count, prio_draw(R, cell, i, draw, first, count, her_ratio), gi, i, k, lane, seq_len, gamma, O);
}

// update, first launch: decide every row (range, staleness: replay_prio_logic.h), leave its leaf in cell[] (-1: skipped) and store 0 to it
__global__ void __launch_bounds__(PRIO_BLOCK) k_prio_update_mark(PrioDev P, int T, int N, uint64_t written, uint64_t sampled_at, int batch, const int32_t *index) {
    const int row = blockIdx.x * PRIO_BLOCK + threadIdx.x;
    if (row >= batch) return;
    const int32_t e = index[(size_t)row * 4], slot = index[(size_t)row * 4 + 1];
    const bool ok = e >= 0 && e < N && prio_cell_live(written, T, slot, sampled_at);
    const int32_t c = ok ? slot * N + e : -1;          // < T N <= 2^30
    P.cell[row] = c;
    if (ok) P.leaf[c] = 0.f;
}
// second launch: the largest clamped value of the rows that name a leaf wins (positive floats order as their bit patterns); p_new follows
__global__ void __launch_bounds__(PRIO_BLOCK) k_prio_update_max(PrioDev P, int batch, const float *priority) {
    const int row = blockIdx.x * PRIO_BLOCK + threadIdx.x;
    if (row >= batch) return;
    const int32_t c = P.cell[row];
    if (c < 0) return;
    const uint32_t v = __float_as_uint(prio_clamp(priority[row], P.p_min, P.p_max));
    atomicMax(reinterpret_cast<uint32_t *>(P.leaf) + c, v);
    atomicMax(P.p_new, v);
}
