// Hindsight replay on the device (include/hsrsim.h: hsr_replay): an episode-aware transition ring per env and the four kernels that fill
// and sample it.  Nothing here touches the simulation state: record READS the batch's pose and mocap arrays, sample and sample_seq read
// the ring only.
//
// Storage (replay_logic.h has the row layout): rows [T][N][stride] - one transition = one contiguous, 16-byte aligned row, so a group of 16
// lanes moves a row with 16-byte accesses, four words per lane and pass; ep_plane [T][N] - the rows' ep_id once more, env fastest, so that
// the scan for an episode's end reads 4 bytes per step instead of striding through rows; head [N][obs_dim] - the observation the next record
// pairs with its action; ep_id / ep_step [N] - the replay's own episode counters.
// Words move as uint32_t bit patterns (NaN payloads and -0 survive, as in k_snapshot_copy); the one float computation is the relabelled
// reward, norm(achieved - goal) < geofence, the expression of the env-step's own goal test (persist.h, solve_mf.h); sample_seq adds the
// n-step reduction of replay_logic.h, every operation rounded to float32 on its own.
//
// Draws: Philox4x32-10 of episode.h, stream 4.  key = (seed & 0xffffffff, seed >> 32), counter = (sample i, draw, 4, env_offset);
//   word 0 -> env = mulhi(word, N); word 1 -> age = mulhi(word, count); word 2 -> relabel = (word >> 8) 2^-24 < her_ratio;
//   word 3 -> goal age = age + mulhi(word, last age of the episode - age + 1)
#pragma once
#include "replay_logic.h"

enum { EP_STREAM_REPLAY = 4 };
enum { REPLAY_GROUP = 16, REPLAY_BLOCK = 256, REPLAY_PER_BLOCK = REPLAY_BLOCK / REPLAY_GROUP };

struct ReplayDev {
    uint32_t *rows, *ep_plane, *head, *ep_id, *ep_step;
    ReplayLayout L;
    int T, N;
    uint32_t key0, key1, env_offset;
    int goal_body;
    float geofence;
};

// commit: the head observation is one flat coalesced copy; lane = env for the counters (reset == NULL: every env opens an episode)
__global__ void __launch_bounds__(REPLAY_BLOCK) k_replay_commit(ReplayDev R, const uint32_t *obs, const uint8_t *reset) {
    const size_t i = (size_t)blockIdx.x * REPLAY_BLOCK + threadIdx.x;
    if (i < (size_t)R.N * R.L.obs_dim) R.head[i] = obs[i];
    if (i < (size_t)R.N) {
        const bool open = reset ? reset[i] != 0 : true;
        if (open) { R.ep_id[i] += 1u; R.ep_step[i] = 0u; }
        else R.ep_step[i] += 1u;
    }
}

// record: a workgroup takes 16 envs.  Its first 16 lanes read what the batch keeps [row][N] - the goal body's pose, the mocap point, the
// latched done flag - with the env fastest and leave the ten tail words of each row in LDS; then 16 lanes per env write that env's row,
// 16 bytes per lane, contiguous over the group.  achieved_next is k_body_xpos's expression (util_kernels.h).
__global__ void __launch_bounds__(REPLAY_BLOCK) k_replay_record(DevModel m, DevState s, ReplayDev R, int slot, const uint32_t *ctrl, const uint32_t *next_obs,
                                                                const uint32_t *reward, const uint8_t *done) {
    __shared__ uint32_t tail[REPLAY_PER_BLOCK][REPLAY_TAIL_WORDS];
    const int N = R.N, e0 = blockIdx.x * REPLAY_PER_BLOCK;
    if (threadIdx.x < REPLAY_PER_BLOCK && e0 + (int)threadIdx.x < N) {
        const int e = e0 + threadIdx.x, l = m.body_link[R.goal_body];
        const View xpos{s.xpos + e, N}, xmat{s.xmat + e, N};
        const v3 p = xpos.get3(l) + mulmv(xmat.getm(l), ld3(m.body_pos, R.goal_body));
        const bool d = done ? done[e] != 0 : s.done[e] != 0;
        uint32_t *t = tail[threadIdx.x];
        t[0] = __float_as_uint(p.x); t[1] = __float_as_uint(p.y); t[2] = __float_as_uint(p.z);
        for (int k = 0; k < 3; k++) t[3 + k] = __float_as_uint(s.mocap[(size_t)k * N + e]);
        t[6] = reward ? reward[e] : __float_as_uint(d ? 1.f : 0.f);
        t[7] = d ? 1u : 0u;
        t[8] = R.ep_id[e];
        t[9] = R.ep_step[e];
        R.ep_plane[(size_t)slot * N + e] = t[8];
    }
    __syncthreads();
    const int g = threadIdx.x / REPLAY_GROUP, lane = threadIdx.x % REPLAY_GROUP, e = e0 + g;
    if (e >= N) return;
    const ReplayLayout &L = R.L;
    uint32_t *row = R.rows + ((size_t)slot * N + e) * L.stride;
    const uint32_t *h = R.head + (size_t)e * L.obs_dim, *a = ctrl + (size_t)e * L.nu, *o = next_obs + (size_t)e * L.obs_dim;
    for (int w0 = 4 * lane; w0 < L.stride; w0 += 4 * REPLAY_GROUP) {
        uint32_t v[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int w = w0 + k;
            v[k] = w < L.o_act ? h[w] : w < L.o_next ? a[w - L.o_act] : w < L.o_achieved ? o[w - L.o_next] : w < L.words ? tail[g][w - L.o_achieved] : 0u;
        }
        *reinterpret_cast<uint4 *>(row + w0) = make_uint4(v[0], v[1], v[2], v[3]);
    }
}

// The pieces k_replay_sample and k_replay_sample_seq share: the draw, the ring's slot arithmetic, the scan and the goal test.
struct ReplayDraw { int e, j; bool relabel; uint32_t goal_word; };
__device__ __forceinline__ ReplayDraw replay_draw(const ReplayDev &R, int i, uint32_t draw, int count, float her_ratio) {
    const Philox4 p = philox4x32_10((uint32_t)i, draw, EP_STREAM_REPLAY, R.env_offset, R.key0, R.key1);
    ReplayDraw d;
    d.e = (int)__umulhi(p.x, (uint32_t)R.N); d.j = (int)__umulhi(p.y, (uint32_t)count);
    d.relabel = (float)(p.z >> 8) * 5.9604644775390625e-8f < her_ratio;       // 24 bits: exact
    d.goal_word = p.w;
    return d;
}
__device__ __forceinline__ int replay_slot_of(const ReplayDev &R, int first, int age) {       // first < T, age < count <= T
    const int sl = first + age;
    return sl >= R.T ? sl - R.T : sl;
}
// the last age with the ep_id of age j; the 16 lanes of a group call it together
__device__ __forceinline__ int replay_episode_end(const ReplayDev &R, int first, int count, int e, int j, int lane) {
    const int N = R.N;
    const uint32_t id = R.ep_plane[(size_t)replay_slot_of(R, first, j) * N + e];
    const int shift = threadIdx.x & 63 & ~(REPLAY_GROUP - 1);      // this group's 16 bits of the wave's ballot
    for (int base = j + 1; base < count; base += REPLAY_GROUP) {
        const int a = base + lane;
        const bool same = a < count && R.ep_plane[(size_t)replay_slot_of(R, first, a < count ? a : j) * N + e] == id;
        const uint32_t miss = ~(uint32_t)(__ballot(same) >> shift) & 0xffffu;
        if (miss) return base + __ffs((int)miss) - 2;      // the first age that differs, less one
    }
    return count - 1;
}
// reward (as its bit pattern) and done of a row under goal g: as stored, or the env-step's own goal test on a relabelled goal
struct ReplayWord { uint32_t reward, done; };
__device__ __forceinline__ ReplayWord replay_step_words(const ReplayDev &R, const uint32_t *row, bool relabel, uint32_t g0, uint32_t g1, uint32_t g2) {
    const ReplayLayout &L = R.L;
    ReplayWord s{row[L.o_reward], row[L.o_done]};
    if (relabel) {
        const v3 a = mk3(__uint_as_float(row[L.o_achieved]), __uint_as_float(row[L.o_achieved + 1]), __uint_as_float(row[L.o_achieved + 2]));
        const v3 gp = mk3(__uint_as_float(g0), __uint_as_float(g1), __uint_as_float(g2));
        const bool reach = norm(a - gp) < R.geofence;
        s.reward = __float_as_uint(reach ? 1.f : 0.f);
        s.done = reach ? 1u : 0u;      // success is the env's only terminal (hsr/env.py:133); a time limit never is
    }
    return s;
}

// sample: 16 lanes per sample.  Every lane of a group draws the same indices (one Philox block); the scan for the last age of the episode
// checks 16 ages per pass, one per lane, on the ep_id plane; then the group copies the row, 16 bytes per lane, and routes its words to the
// caller's arrays.  e < N, age < count and slot < T hold for every 32-bit draw (mulhi(w, n) < n), and a group past `batch` leaves at once:
// nothing is read or written outside the ring or the first `batch` rows of an output.  `first` = slot of age 0.
// The body is a function of the sample's draw, so that the prioritised sampler (replay_prio.h) runs the same code from its own draw.
__device__ __forceinline__ void replay_sample_rows(const ReplayDev &R, int first, int count, const ReplayDraw &d, int i, int lane,
                                                   uint32_t *obs, uint32_t *act, uint32_t *next_obs, uint32_t *goal, uint32_t *achieved_next,
                                                   uint32_t *reward, uint8_t *done, int32_t *index) {
    const ReplayLayout &L = R.L;
    const int N = R.N;
    const int e = d.e, j = d.j;
    const bool relabel = d.relabel;
    const int sj = replay_slot_of(R, first, j);
    const uint32_t *row = R.rows + ((size_t)sj * N + e) * L.stride;
    int sg = -1;
    if (relabel) {
        const int j_end = replay_episode_end(R, first, count, e, j, lane);
        sg = replay_slot_of(R, first, j + (int)__umulhi(d.goal_word, (uint32_t)(j_end - j + 1)));
    }
    for (int w0 = 4 * lane; w0 < L.stride; w0 += 4 * REPLAY_GROUP) {
        const uint4 q = *reinterpret_cast<const uint4 *>(row + w0);
        const uint32_t v[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int w = w0 + k;
            if (w < L.o_act) { if (obs) obs[(size_t)i * L.obs_dim + w] = v[k]; }
            else if (w < L.o_next) { if (act) act[(size_t)i * L.nu + (w - L.o_act)] = v[k]; }
            else if (w < L.o_achieved) { if (next_obs) next_obs[(size_t)i * L.obs_dim + (w - L.o_next)] = v[k]; }
            else if (w < L.o_desired) { if (achieved_next) achieved_next[(size_t)i * 3 + (w - L.o_achieved)] = v[k]; }
        }
    }
    if (lane != 0) return;
    const uint32_t *gsrc = relabel ? R.rows + ((size_t)sg * N + e) * L.stride + L.o_achieved : row + L.o_desired;
    const uint32_t g0 = gsrc[0], g1 = gsrc[1], g2 = gsrc[2];
    const ReplayWord s = replay_step_words(R, row, relabel, g0, g1, g2);
    if (goal) { goal[(size_t)i * 3] = g0; goal[(size_t)i * 3 + 1] = g1; goal[(size_t)i * 3 + 2] = g2; }
    if (reward) reward[i] = s.reward;
    if (done) done[i] = (uint8_t)(s.done != 0u);
    if (index) { int32_t *x = index + (size_t)i * 4; x[0] = e; x[1] = sj; x[2] = sg; x[3] = relabel ? 1 : 0; }
}
__global__ void __launch_bounds__(REPLAY_BLOCK) k_replay_sample(ReplayDev R, int first, int count, uint32_t draw, int batch, float her_ratio,
                                                                uint32_t *obs, uint32_t *act, uint32_t *next_obs, uint32_t *goal, uint32_t *achieved_next,
                                                                uint32_t *reward, uint8_t *done, int32_t *index) {
    const int i = blockIdx.x * REPLAY_PER_BLOCK + threadIdx.x / REPLAY_GROUP, lane = threadIdx.x % REPLAY_GROUP;
    if (i >= batch) return;
    replay_sample_rows(R, first, count, replay_draw(R, i, draw, count, her_ratio), i, lane, obs, act, next_obs, goal, achieved_next, reward, done, index);
}

// sample_seq: 16 lanes per (sample, step) - batch x seq_len rows in flight.  Every group of a sample redraws the sample's Philox block and
// rescans j_end on the ep_id plane (4-byte reads, cheaper than a dependency between kernels), so it knows the window's length by itself:
// a group inside the window copies the row of age j + k and lane 0 writes that step's reward and done; a group past it writes zero words.
// The group of step 0 also writes the per-sample outputs.  For the n-step chain lane l of that group reads reward, done and, when relabelled,
// the three achieved_next words of step c + l, 16 steps per pass, and the chain (replay_logic.h: replay_nstep) takes them by shuffles inside
// the group, all 16 lanes alike, so that the loads of a pass are in flight together; then the group copies next_obs of step m - 1.
// Bounds: ages j .. j + length - 1 <= j_end < count; (sample, step) < batch seq_len < 2^31 (replay_sample_seq_error); a group past that
// leaves at once.  No LDS, no atomics, no scratch.
// The body, from the sample's draw on (as replay_sample_rows): gi = the (sample, step) of the group, i its sample, k its step.
__device__ __forceinline__ void replay_sample_seq_rows(const ReplayDev &R, int first, int count, const ReplayDraw &d, uint32_t gi, int i, int k, int lane,
                                                       int seq_len, float gamma, const hsr_replay_seq_out &O) {
    const ReplayLayout &L = R.L;
    const int N = R.N;
    const int e = d.e, j = d.j;
    const int j_end = replay_episode_end(R, first, count, e, j, lane);
    const int length = min(seq_len, j_end - j + 1);
    const bool valid = k < length;
    auto row_of = [&](int age) { return R.rows + ((size_t)replay_slot_of(R, first, age) * N + e) * L.stride; };
    const uint32_t *row = row_of(valid ? j + k : j);
    uint32_t *obs = (uint32_t *)O.obs, *act = (uint32_t *)O.act, *next_obs = (uint32_t *)O.next_obs, *achieved_next = (uint32_t *)O.achieved_next;
    for (int w0 = 4 * lane; w0 < L.stride; w0 += 4 * REPLAY_GROUP) {
        const uint4 q = valid ? *reinterpret_cast<const uint4 *>(row + w0) : make_uint4(0u, 0u, 0u, 0u);
        const uint32_t v[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const int w = w0 + c;
            if (w < L.o_act) { if (obs) obs[(size_t)gi * L.obs_dim + w] = v[c]; }
            else if (w < L.o_next) { if (act) act[(size_t)gi * L.nu + (w - L.o_act)] = v[c]; }
            else if (w < L.o_achieved) { if (next_obs) next_obs[(size_t)gi * L.obs_dim + (w - L.o_next)] = v[c]; }
            else if (w < L.o_desired) { if (achieved_next) achieved_next[(size_t)gi * 3 + (w - L.o_achieved)] = v[c]; }
        }
    }
    if (!valid) {
        if (lane == 0) {
            if (O.reward) ((uint32_t *)O.reward)[gi] = 0u;
            if (O.done) O.done[gi] = 0;
        }
        return;
    }
    // one goal for the whole window; every lane reads the same three words
    const int sj = replay_slot_of(R, first, j);
    const int sg = d.relabel ? replay_slot_of(R, first, j + (int)__umulhi(d.goal_word, (uint32_t)(j_end - j + 1))) : -1;
    const uint32_t *gsrc = d.relabel ? R.rows + ((size_t)sg * N + e) * L.stride + L.o_achieved : row_of(j) + L.o_desired;
    const uint32_t g0 = gsrc[0], g1 = gsrc[1], g2 = gsrc[2];
    if (lane == 0) {
        const ReplayWord s = replay_step_words(R, row, d.relabel, g0, g1, g2);
        if (O.reward) ((uint32_t *)O.reward)[gi] = s.reward;
        if (O.done) O.done[gi] = (uint8_t)(s.done != 0u);
    }
    if (k != 0) return;
    ReplayWord mine{0u, 0u};       // this lane's step of the pass
    const ReplayNstep n = replay_nstep(length, gamma, [&](int c) {
        const int l = c % REPLAY_GROUP;
        if (l == 0) mine = c + lane < length ? replay_step_words(R, row_of(j + c + lane), d.relabel, g0, g1, g2) : ReplayWord{0u, 0u};
        return ReplayStep{__uint_as_float(__shfl(mine.reward, l, REPLAY_GROUP)), __shfl(mine.done, l, REPLAY_GROUP)};
    });
    if (O.nstep_obs) {
        const uint32_t *last = row_of(j + n.m - 1);
        uint32_t *dst = (uint32_t *)O.nstep_obs + (size_t)i * L.obs_dim;
        for (int w0 = (L.o_next & ~3) + 4 * lane; w0 < L.o_achieved; w0 += 4 * REPLAY_GROUP) {
            const uint4 q = *reinterpret_cast<const uint4 *>(last + w0);
            const uint32_t v[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const int w = w0 + c;
                if (w >= L.o_next && w < L.o_achieved) dst[w - L.o_next] = v[c];
            }
        }
    }
    if (lane != 0) return;
    if (O.goal) { uint32_t *g = (uint32_t *)O.goal + (size_t)i * 3; g[0] = g0; g[1] = g1; g[2] = g2; }
    if (O.length) O.length[i] = length;
    if (O.nstep) O.nstep[i] = n.m;
    if (O.nstep_return) O.nstep_return[i] = n.ret;
    if (O.nstep_discount) O.nstep_discount[i] = n.discount;
    if (O.nstep_done) O.nstep_done[i] = (uint8_t)(n.done != 0u);
    if (O.index) { int32_t *x = O.index + (size_t)i * 4; x[0] = e; x[1] = sj; x[2] = sg; x[3] = d.relabel ? 1 : 0; }
}
__global__ void __launch_bounds__(REPLAY_BLOCK) k_replay_sample_seq(ReplayDev R, int first, int count, uint32_t draw, int batch, int seq_len, float her_ratio,
                                                                    float gamma, hsr_replay_seq_out O) {
    const uint32_t gi = blockIdx.x * (uint32_t)REPLAY_PER_BLOCK + threadIdx.x / REPLAY_GROUP;
    const int lane = threadIdx.x % REPLAY_GROUP;
    if (gi >= (uint32_t)batch * (uint32_t)seq_len) return;
    const int i = (int)(gi / (uint32_t)seq_len), k = (int)(gi - (uint32_t)i * (uint32_t)seq_len);
    replay_sample_seq_rows(R, first, count, replay_draw(R, i, draw, count, her_ratio), gi, i, k, lane, seq_len, gamma, O);
}
