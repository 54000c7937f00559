// On-policy rollouts on the device (include/hsrsim.h: hsr_rollout): a store of T env-steps of every env, generalised advantage estimation
// with the time-limit bootstrap, the advantage statistics and shuffled minibatches.  Nothing here reads or writes the simulation state.
//
// Storage (rollout_logic.h has the row layout): rows [T][N][stride] - obs | act of one stored step, one contiguous 16-byte aligned row, so a
// group of 16 lanes moves it with 16-byte accesses as k_replay_record does; planes [T][N], env fastest, one 32-bit word each - logp, value,
// reward, kind, v_term, adv, ret - so that the GAE chain, lane = env, reads and writes coalesced; head [N][obs_dim] - the observation the
// next stage pairs with its action.  Words move as uint32_t bit patterns (NaN payloads and -0 survive).
//
// The float arithmetic is the GAE recursion and the normalisation of a minibatch's advantages, every operation rounded to float32 on its own
// (#pragma clang fp contract(off), as ep_uniform of episode.h: the header's __fmul_rn / __fadd_rn are plain operators that hipcc fuses).
// The statistics are fp64 sums of a fixed shape: per-lane serial, a shuffle tree per wave, waves in order, partials in order - no atomics.
//
// Shuffle: Philox4x32-10 of episode.h, stream 5.  key = (seed & 0xffffffff, seed >> 32), counter = (epoch, 0, 5, env_offset); the four words
// are the round keys of a Feistel network over 2 h bits, walked until the value falls below M (include/hsrsim.h states it).
#pragma once
#include "rollout_logic.h"

enum { EP_STREAM_ROLLOUT = 5 };
enum { ROLLOUT_GROUP = 16, ROLLOUT_BLOCK = 256, ROLLOUT_PER_BLOCK = ROLLOUT_BLOCK / ROLLOUT_GROUP };
// k_rollout_gae: one wave per workgroup - at 8192 envs 128 workgroups, one for every other compute unit, instead of 32 of four waves; the
// loads of ROLLOUT_GAE_AHEAD steps are in flight before the chain needs the first of them
enum { ROLLOUT_GAE_BLOCK = 64, ROLLOUT_GAE_AHEAD = 8 };
enum { ROLLOUT_VAR_BLOCKS = 1024 };        // most workgroups of the second-moment pass (each leaves one partial)

struct RolloutDev {
    uint32_t *rows, *head;
    uint32_t *logp, *value, *reward, *kind, *v_term, *adv, *ret;      // planes [T][N]
    double *partial;               // [max(ceil(N / 64), ROLLOUT_VAR_BLOCKS)] per-workgroup sums of the pass that runs
    double *mean64;                // [1] what the second pass subtracts
    float *stats;                  // [3] mean, std, rstd as float32
    RolloutLayout L;
    int T, N;
    uint32_t key0, key1, env_offset;
    float gamma, gl;               // gl = gamma * lam, one float32 product on the host
};

// stage: a workgroup takes 16 envs.  Its first 16 lanes move the two scalars, env fastest; then 16 lanes per env write that env's row, 16
// bytes per lane, contiguous over the group.
__global__ void __launch_bounds__(ROLLOUT_BLOCK) k_rollout_stage(RolloutDev R, int slot, const uint32_t *act, const uint32_t *logp, const uint32_t *value) {
    const int N = R.N, e0 = blockIdx.x * ROLLOUT_PER_BLOCK;
    if (threadIdx.x < ROLLOUT_PER_BLOCK && e0 + (int)threadIdx.x < N) {
        const int e = e0 + threadIdx.x;
        R.logp[(size_t)slot * N + e] = logp[e];
        R.value[(size_t)slot * N + e] = value[e];
    }
    const int g = threadIdx.x / ROLLOUT_GROUP, lane = threadIdx.x % ROLLOUT_GROUP, e = e0 + g;
    if (e >= N) return;
    const RolloutLayout &L = R.L;
    uint32_t *row = R.rows + ((size_t)slot * N + e) * L.stride;
    const uint32_t *h = R.head + (size_t)e * L.obs_dim, *a = act + (size_t)e * L.nu;
    for (int w0 = 4 * lane; w0 < L.stride; w0 += 4 * ROLLOUT_GROUP) {
        uint32_t v[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int w = w0 + k;
            v[k] = w < L.o_act ? h[w] : w < L.words ? a[w - L.o_act] : 0u;
        }
        *reinterpret_cast<uint4 *>(row + w0) = make_uint4(v[0], v[1], v[2], v[3]);
    }
}

// close: the head observation is one flat coalesced copy; lane = env for the scalars of the slot
__global__ void __launch_bounds__(ROLLOUT_BLOCK) k_rollout_close(RolloutDev R, int slot, const uint32_t *reward, const uint8_t *kind, const uint32_t *next_obs) {
    const size_t i = (size_t)blockIdx.x * ROLLOUT_BLOCK + threadIdx.x;
    if (i < (size_t)R.N * R.L.obs_dim) R.head[i] = next_obs[i];
    if (i < (size_t)R.N) {
        const size_t p = (size_t)slot * R.N + i;
        R.reward[p] = reward[i];
        R.kind[p] = kind[i];
        R.v_term[p] = 0u;
    }
}
// begin (slot < 0: the head alone) and bootstrap (v_term of `slot`) are the two halves of close
__global__ void __launch_bounds__(ROLLOUT_BLOCK) k_rollout_rows(RolloutDev R, int slot, const uint32_t *src) {
    const size_t i = (size_t)blockIdx.x * ROLLOUT_BLOCK + threadIdx.x;
    if (slot < 0) { if (i < (size_t)R.N * R.L.obs_dim) R.head[i] = src[i]; }
    else if (i < (size_t)R.N) R.v_term[(size_t)slot * R.N + i] = src[i];
}

struct GaeIn { float reward, value, v_term; uint32_t kind; };
__device__ __forceinline__ GaeIn gae_load(const RolloutDev &R, int t, int e) {
    GaeIn g{0.f, 0.f, 0.f, 1u};
    if (t >= 0) {
        const size_t p = (size_t)t * R.N + e;
        g.reward = __uint_as_float(R.reward[p]); g.value = __uint_as_float(R.value[p]); g.v_term = __uint_as_float(R.v_term[p]); g.kind = R.kind[p];
    }
    return g;
}
// one step of the recursion as include/hsrsim.h states it: five float32 operations, each rounded on its own
__device__ __forceinline__ float gae_step(const GaeIn &g, float gamma, float gl, float next_value, float next_adv) {
#pragma clang fp contract(off)
    const float nv = g.kind == 0u ? next_value : g.kind == 2u ? g.v_term : 0.f;
    const float carry = g.kind == 0u ? next_adv : 0.f;
    const float discounted = gamma * nv;
    const float target = g.reward + discounted;
    const float delta = target - g.value;
    const float tail = gl * carry;
    return delta + tail;
}
__device__ __forceinline__ float f32_add(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}
// the 64 lanes' values in a fixed tree; the sum is lane 0's
__device__ __forceinline__ double wave_sum_fixed(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// GAE: lane = env, t = T-1 .. 0.  The chain is serial in its arithmetic only: what a step loads does not depend on it, so the loads of the
// next ROLLOUT_GAE_AHEAD steps are issued before the current ones are consumed.  Each lane sums its advantages in fp64 as it goes.
__global__ void __launch_bounds__(ROLLOUT_GAE_BLOCK) k_rollout_gae(RolloutDev R, const float *last_value) {
    const int e = blockIdx.x * ROLLOUT_GAE_BLOCK + threadIdx.x, T = R.T;
    double sum = 0.0;
    if (e < R.N) {
        float next_value = last_value[e], next_adv = 0.f;        // kind == 0 at t == T-1 bootstraps from last_value and carries nothing
        GaeIn cur[ROLLOUT_GAE_AHEAD], nxt[ROLLOUT_GAE_AHEAD];
#pragma unroll
        for (int k = 0; k < ROLLOUT_GAE_AHEAD; k++) cur[k] = gae_load(R, T - 1 - k, e);
        for (int base = T - 1; base >= 0; base -= ROLLOUT_GAE_AHEAD) {
#pragma unroll
            for (int k = 0; k < ROLLOUT_GAE_AHEAD; k++) nxt[k] = gae_load(R, base - ROLLOUT_GAE_AHEAD - k, e);
#pragma unroll
            for (int k = 0; k < ROLLOUT_GAE_AHEAD; k++) {
                const int t = base - k;
                if (t < 0) break;
                const float adv = gae_step(cur[k], R.gamma, R.gl, next_value, next_adv);
                const size_t p = (size_t)t * R.N + e;
                R.adv[p] = __float_as_uint(adv);
                R.ret[p] = __float_as_uint(f32_add(adv, cur[k].value));
                sum += (double)adv;
                next_value = cur[k].value; next_adv = adv;
            }
#pragma unroll
            for (int k = 0; k < ROLLOUT_GAE_AHEAD; k++) cur[k] = nxt[k];
        }
    }
    sum = wave_sum_fixed(sum);
    if (threadIdx.x == 0) R.partial[blockIdx.x] = sum;
}

// the sum of a workgroup of ROLLOUT_BLOCK threads, in thread 0: a shuffle tree per wave, then the waves in order
__device__ __forceinline__ double block_sum_fixed(double v) {
    __shared__ double wave_part[ROLLOUT_BLOCK / 64];
    v = wave_sum_fixed(v);
    if ((threadIdx.x & 63) == 0) wave_part[threadIdx.x / 64] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < ROLLOUT_BLOCK / 64; w++) s += wave_part[w];
    return s;
}
// second pass: a workgroup's share of sum((adv - mean)^2), element i to thread i mod (grid x block)
__global__ void __launch_bounds__(ROLLOUT_BLOCK) k_rollout_var(RolloutDev R, int items) {
    const double mean = *R.mean64;
    double acc = 0.0;
    for (size_t i = (size_t)blockIdx.x * ROLLOUT_BLOCK + threadIdx.x; i < (size_t)items; i += (size_t)gridDim.x * ROLLOUT_BLOCK) {
        const double d = (double)__uint_as_float(R.adv[i]) - mean;
        acc += d * d;
    }
    acc = block_sum_fixed(acc);
    if (threadIdx.x == 0) R.partial[blockIdx.x] = acc;
}
// one workgroup adds the partials of a pass in a fixed order.  pass 0: the mean; pass 1: variance -> std and rstd
__global__ void __launch_bounds__(ROLLOUT_BLOCK) k_rollout_moment(RolloutDev R, int npartial, int items, int pass) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < npartial; i += ROLLOUT_BLOCK) acc += R.partial[i];
    acc = block_sum_fixed(acc);
    if (threadIdx.x != 0) return;
    const double m = acc / (double)items;
    if (pass == 0) { *R.mean64 = m; R.stats[0] = (float)m; }
    else {
        const double sd = sqrt(m);
        R.stats[1] = (float)sd;
        R.stats[2] = (float)(1.0 / (sd + 1e-8));
    }
}

__device__ __forceinline__ uint32_t rollout_feistel_f(uint32_t v, uint32_t k, uint32_t mask) {
    v ^= k; v *= 0x9E3779B1u; v ^= v >> 15; v *= 0x85EBCA77u; v ^= v >> 13;
    return v & mask;
}
// the shuffle: i < M -> perm(i) < M.  The four rounds are a bijection of [0, 2^(2h)), so the walk comes back below M (i itself lies there)
__device__ __forceinline__ uint32_t rollout_perm(uint32_t i, uint32_t items, int h, const Philox4 &key) {
    const uint32_t mask = (1u << h) - 1u;          // h <= 16
    uint32_t x = i;
    do {
        uint32_t l = x >> h, r = x & mask;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t f = rollout_feistel_f(r, philox_word(key, k), mask);
            const uint32_t nr = l ^ f;
            l = r; r = nr;
        }
        x = l << h | r;
    } while (x >= items);
    return x;
}
__device__ __forceinline__ float rollout_normalized(float adv, float mean, float rstd) {
#pragma clang fp contract(off)
    const float centred = adv - mean;
    return centred * rstd;
}

// minibatch: 16 lanes per row.  Every lane of a group computes the same element p = perm(first + i) < M = T N, which is the plane index
// t N + e itself; the group copies the row, 16 bytes per lane, and routes its words to the caller's arrays; lane 0 moves the scalars.  A
// group past `count` leaves at once: nothing is read outside the store or written outside the first `count` rows of an output.
__global__ void __launch_bounds__(ROLLOUT_BLOCK) k_rollout_minibatch(RolloutDev R, uint32_t epoch, int first, int count, int normalize, int h, uint32_t *obs,
                                                                    uint32_t *act, uint32_t *logp, uint32_t *value, uint32_t *adv, uint32_t *ret, int32_t *index) {
    const int i = blockIdx.x * ROLLOUT_PER_BLOCK + threadIdx.x / ROLLOUT_GROUP, lane = threadIdx.x % ROLLOUT_GROUP;
    if (i >= count) return;
    const RolloutLayout &L = R.L;
    const Philox4 key = philox4x32_10(epoch, 0u, EP_STREAM_ROLLOUT, R.env_offset, R.key0, R.key1);
    const uint32_t p = rollout_perm((uint32_t)(first + i), (uint32_t)R.T * (uint32_t)R.N, h, key);
    const uint32_t *row = R.rows + (size_t)p * L.stride;
    for (int w0 = 4 * lane; w0 < L.stride; w0 += 4 * ROLLOUT_GROUP) {
        const uint4 q = *reinterpret_cast<const uint4 *>(row + w0);
        const uint32_t v[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int w = w0 + k;
            if (w < L.o_act) { if (obs) obs[(size_t)i * L.obs_dim + w] = v[k]; }
            else if (w < L.words) { if (act) act[(size_t)i * L.nu + (w - L.o_act)] = v[k]; }
        }
    }
    if (lane != 0) return;
    if (logp) logp[i] = R.logp[p];
    if (value) value[i] = R.value[p];
    if (ret) ret[i] = R.ret[p];
    if (adv) adv[i] = normalize ? __float_as_uint(rollout_normalized(__uint_as_float(R.adv[p]), R.stats[0], R.stats[2])) : R.adv[p];
    if (index) { index[(size_t)i * 2] = (int32_t)(p / (uint32_t)R.N); index[(size_t)i * 2 + 1] = (int32_t)(p % (uint32_t)R.N); }
}
