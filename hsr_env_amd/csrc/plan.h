// A cross-entropy-method planner over forked envs (include/hsrsim.h: hsr_plan): the kernels between the env-steps of a planning batch of
// N = P K envs, candidate k of group p = env p K + k.  The arithmetic of a draw, a cost step, a rank and a refit is plan_logic.h's; this file
// moves the values.  The planning batch's state is only read (accumulate: the goal body's pose, the mocap point, the done / bad flags).
//
//   k_plan_reset / k_plan_shift   one lane per (group, actuator), the H steps in order
//   k_plan_begin                  one lane per candidate
//   k_plan_sample                 one lane per (candidate, actuator), actuator fastest: ctrl [N][nu] is written contiguously; the action as
//                                 sampled is kept in act [P][H][nu][K], candidate fastest, for the refit
//   k_plan_accumulate             one lane per candidate, coalesced on the batch's [row][N] fields
//   k_plan_add_cost               one lane per candidate
//   k_plan_update                 one workgroup of ceil(K / 64) waves per group: cost keys in LDS, one lane per candidate for the rank, a
//                                 ballot per wave for the finite count, elite flags in LDS; then wave w refits the entries (h, a) = w, w + W, ..
//                                 with the two fp64 sums in the fixed shape plan_logic.h states (non-elites add +0.0 in place)
// No atomics.  Draws: Philox4x32-10 of episode.h, stream 7: key = (seed & 0xffffffff, seed >> 32),
// counter = (env_offset + p, call 256 + iter, 7, (k H + h) nu + a); the block's four words make one Irwin-Hall normal (plan_z).
#pragma once
#include "plan_logic.h"

enum { EP_STREAM_PLAN = 7 };
enum { PLAN_BLOCK = 256 };
static_assert(PLAN_WAVE == 64, "a lane group of the refit is one wave64");
static_assert(PLAN_SAMPLES_MAX == 1024, "k_plan_update: one workgroup holds a group's candidates");

struct PlanDev {
    float *mean, *sigma;           // [P][H][nu]
    float *act;                    // [P][H][nu][K] the actions as sampled
    float *J, *g;                  // [N]
    uint8_t *alive;                // [N]
    int32_t *reach;                // [N]
    uint32_t *failed;              // [P]
    int32_t *best_index;           // [P]
    float *best_cost;              // [P]
    int P, K, H, nu, N, elites;
    uint32_t key0, key1, env_offset;
    int goal_body;
    float gamma, alpha, init_std, min_std;
};

__device__ __forceinline__ void plan_act_range(const float *ctrlrange, int a, float *lo, float *hi) { plan_range(ctrlrange[2 * a], ctrlrange[2 * a + 1], lo, hi); }

// reset (shift == 0): mean <- clamp(0), sigma <- its initial value; shift: mean[h] <- mean[h + 1], the last step repeats, sigma likewise back
__global__ void __launch_bounds__(PLAN_BLOCK) k_plan_reset(PlanDev R, const float *ctrlrange, const uint8_t *mask, int shift) {
    const int i = blockIdx.x * PLAN_BLOCK + threadIdx.x;
    if (i >= R.P * R.nu) return;
    const int p = i / R.nu, a = i - p * R.nu;
    if (mask && !mask[p]) return;
    float lo, hi;
    plan_act_range(ctrlrange, a, &lo, &hi);
    const float s0 = plan_sigma0(R.init_std, plan_half_range(lo, hi)), m0 = plan_clamp(0.f, lo, hi);
    float *mean = R.mean + (size_t)p * R.H * R.nu + a, *sigma = R.sigma + (size_t)p * R.H * R.nu + a;
    for (int h = 0; h < R.H; h++) {
        if (shift) { if (h + 1 < R.H) mean[(size_t)h * R.nu] = mean[(size_t)(h + 1) * R.nu]; }
        else mean[(size_t)h * R.nu] = m0;
        sigma[(size_t)h * R.nu] = s0;
    }
}

__global__ void __launch_bounds__(PLAN_BLOCK) k_plan_begin(PlanDev R) {
    const int e = blockIdx.x * PLAN_BLOCK + threadIdx.x;
    if (e >= R.N) return;
    const PlanCost c = plan_cost_begin();
    R.J[e] = c.J; R.g[e] = c.g; R.alive[e] = c.alive; R.reach[e] = c.reach_step;
}

__global__ void __launch_bounds__(PLAN_BLOCK) k_plan_sample(PlanDev R, const float *ctrlrange, uint32_t call, int iter, int h, float *ctrl) {
    const size_t i = (size_t)blockIdx.x * PLAN_BLOCK + threadIdx.x;
    if (i >= (size_t)R.N * R.nu) return;
    const int e = (int)(i / R.nu), a = (int)(i - (size_t)e * R.nu), p = e / R.K, k = e - p * R.K;
    float z = 0.f;                 // candidate 0 is the current mean
    if (k > 0) {
        const Philox4 w = philox4x32_10(R.env_offset + (uint32_t)p, plan_second(call, iter), EP_STREAM_PLAN, plan_block(k, h, a, R.H, R.nu), R.key0, R.key1);
        z = plan_z(w.x, w.y, w.z, w.w);
    }
    float lo, hi;
    plan_act_range(ctrlrange, a, &lo, &hi);
    const size_t row = ((size_t)p * R.H + h) * R.nu + a;
    const float x = plan_action(R.mean[row], R.sigma[row], z, lo, hi);
    ctrl[i] = x;
    R.act[row * R.K + k] = x;
}

// after hsr_batch_step_dev of step h.  The goal body's position is k_body_xpos's expression (util_kernels.h)
__global__ void __launch_bounds__(PLAN_BLOCK) k_plan_accumulate(DevModel m, DevState s, PlanDev R, int h) {
    const int e = blockIdx.x * PLAN_BLOCK + threadIdx.x;
    if (e >= R.N) return;
    PlanCost c;
    c.J = R.J[e]; c.g = R.g[e]; c.alive = R.alive[e]; c.reach_step = R.reach[e];
    if (!c.alive) return;
    const int N = s.N, l = m.body_link[R.goal_body];
    const View xpos{s.xpos + e, N}, xmat{s.xmat + e, N};
    const v3 pos = xpos.get3(l) + mulmv(xmat.getm(l), ld3(m.body_pos, R.goal_body));
    const float d = plan_dist(pos.x, pos.y, pos.z, s.mocap[e], s.mocap[(size_t)N + e], s.mocap[2 * (size_t)N + e]);
    plan_cost_step(&c, d, R.gamma, s.done[e] != 0, s.bad[e] != 0, h);
    R.J[e] = c.J; R.g[e] = c.g; R.alive[e] = c.alive; R.reach[e] = c.reach_step;
}

__global__ void __launch_bounds__(PLAN_BLOCK) k_plan_add_cost(PlanDev R, const float *extra) {
    const int e = blockIdx.x * PLAN_BLOCK + threadIdx.x;
    if (e < R.N) R.J[e] = R.J[e] + extra[e];
}

// one sum of the refit by one whole wave, in plan_logic.h's shape; every lane returns it
template <typename F>
__device__ __forceinline__ double plan_wave_sum(int K, int lane, F leaf) {
    double acc = 0.0;
    for (int k = lane; k < K; k += PLAN_WAVE) acc = acc + leaf(k);
    acc = wave_sum_fixed(acc);
    return __shfl(acc, 0, 64);
}

// blockDim.x = K rounded up to whole waves; blockIdx.x = the group
__global__ void __launch_bounds__(PLAN_SAMPLES_MAX) k_plan_update(PlanDev R, const float *ctrlrange) {
    __shared__ float key[PLAN_SAMPLES_MAX];
    __shared__ uint8_t elite[PLAN_SAMPLES_MAX];
    __shared__ int wave_finite[PLAN_SAMPLES_MAX / PLAN_WAVE];
    const int K = R.K, p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, waves = blockDim.x >> 6;
    const bool mine = tid < K;
    const float kv = mine ? plan_cost_key(R.J[(size_t)p * K + tid]) : INFINITY;
    if (mine) key[tid] = kv;
    const unsigned long long fin = __ballot(mine && plan_finite32(kv));
    if (lane == 0) wave_finite[wave] = __popcll(fin);
    __syncthreads();
    int finite = 0;
    for (int w = 0; w < waves; w++) finite += wave_finite[w];
    const int E = plan_elite_count(R.elites, finite);
    if (mine) {
        const int rank = plan_rank(key, K, tid);
        elite[tid] = rank < E ? 1 : 0;
        if (rank == 0) { R.best_index[p] = tid; R.best_cost[p] = kv; }       // exactly one candidate has rank 0
    }
    if (E == 0) {                  // no finite cost: mean and sigma stay
        if (tid == 0) R.failed[p] += 1u;
        return;
    }
    __syncthreads();
    const int nu = R.nu, entries = R.H * nu;
    for (int c = wave; c < entries; c += waves) {
        const float *x = R.act + ((size_t)p * entries + c) * K;
        const double m = plan_elite_mean(plan_wave_sum(K, lane, [&](int k) { return plan_leaf((double)x[k], elite[k] != 0); }), E);
        const double sq = plan_wave_sum(K, lane, [&](int k) { return plan_leaf(plan_sq_dev((double)x[k], m), elite[k] != 0); });
        if (lane == 0) {
            float lo, hi;
            plan_act_range(ctrlrange, c % nu, &lo, &hi);
            plan_refit(m, sq, E, R.alpha, R.min_std, plan_half_range(lo, hi), R.mean + (size_t)p * entries + c, R.sigma + (size_t)p * entries + c);
        }
    }
}

// mean[p][0] of every group -> ctrl [P][nu]
__global__ void __launch_bounds__(PLAN_BLOCK) k_plan_action(PlanDev R, float *ctrl) {
    const int i = blockIdx.x * PLAN_BLOCK + threadIdx.x;
    if (i >= R.P * R.nu) return;
    const int p = i / R.nu, a = i - p * R.nu;
    ctrl[i] = R.mean[(size_t)p * R.H * R.nu + a];
}
