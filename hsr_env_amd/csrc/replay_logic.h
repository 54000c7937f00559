// The host books of a replay (include/hsrsim.h: hsr_replay): row layout, the EMPTY -> READY -> PENDING state machine, slot arithmetic and
// the argument checks, and the n-step reduction of a sampled window, in plain C++ without a HIP call or header, so that a stand-alone
// program can exercise them under a sanitizer (tests/replay_logic_main.cpp, tests/replay_seq_logic_main.cpp).  host_replay.h asks these
// functions and launches only what they allow; replay.h indexes with the same row layout and runs the same reduction.
#pragma once
#include <math.h>
#include <stdint.h>

// One transition = one row of 32-bit words, padded to a multiple of 4 (16-byte rows):
//   obs[obs_dim] | act[nu] | next_obs[obs_dim] | achieved_next[3] | desired[3] | reward | done | ep_id | ep_step | padding
enum { REPLAY_TAIL_WORDS = 10 };
struct ReplayLayout {
    int obs_dim, nu;
    int o_act, o_next, o_achieved, o_desired, o_reward, o_done, o_ep_id, o_ep_step;
    int words, stride;             // W = 2 obs_dim + nu + 10, and W rounded up to 4
};
static inline ReplayLayout replay_layout(int obs_dim, int nu) {
    ReplayLayout L;
    L.obs_dim = obs_dim; L.nu = nu;
    L.o_act = obs_dim; L.o_next = L.o_act + nu; L.o_achieved = L.o_next + obs_dim; L.o_desired = L.o_achieved + 3;
    L.o_reward = L.o_desired + 3; L.o_done = L.o_reward + 1; L.o_ep_id = L.o_done + 1; L.o_ep_step = L.o_ep_id + 1;
    L.words = L.o_ep_step + 1;
    L.stride = (L.words + 3) & ~3;
    return L;
}

enum ReplayState { REPLAY_EMPTY = 0, REPLAY_READY = 1, REPLAY_PENDING = 2 };
struct ReplayBooks {
    int T, N;                      // capacity_steps, envs
    int state;
    uint64_t pushed;               // transitions closed per env since the last clear
};
static inline void replay_books_init(ReplayBooks *k, int T, int N) { k->T = T; k->N = N; k->state = REPLAY_EMPTY; k->pushed = 0; }
static inline int replay_count(const ReplayBooks *k) { return k->pushed < (uint64_t)k->T ? (int)k->pushed : k->T; }
static inline int replay_head_slot(const ReplayBooks *k) { return (int)(k->pushed % (uint64_t)k->T); }      // the slot the next record writes
static inline int replay_first_slot(const ReplayBooks *k) { return (int)((k->pushed - (uint64_t)replay_count(k)) % (uint64_t)k->T); }    // slot of age 0
static inline int replay_slot(const ReplayBooks *k, int age) { return (int)(((uint64_t)replay_first_slot(k) + (uint64_t)age) % (uint64_t)k->T); }

// NULL when the spec's numbers are acceptable, else what is wrong with them.  nbody / mocap flags come from the model.
static inline const char *replay_spec_error(int capacity_steps, int obs_dim, int goal_body, float geofence, int nbody, const int *body_mocap, int ngoal_terms) {
    if (capacity_steps < 1) return "capacity_steps < 1";
    if (obs_dim < 1) return "obs_dim < 1";
    if (obs_dim > (1 << 20)) return "obs_dim above 2^20";      // keeps every row offset far inside an int
    if (goal_body < 0 || goal_body >= nbody) return "goal_body out of range";
    if (body_mocap[goal_body]) return "goal_body is the mocap body (the goal point itself, not what has to reach it)";
    if (!isfinite(geofence) || !(geofence > 0.f)) return "geofence is not a finite positive number";
    if (ngoal_terms > 0) return "the batch has extra goal terms (hsr_batch_set_goals): a reward of several terms cannot be recomputed from one relabelled point";
    return nullptr;
}
// bytes of the ring's rows, or 0 when T N stride words do not fit the 2^40 bytes this layer is willing to ask a device for
static inline uint64_t replay_ring_bytes(int T, int N, int stride) {
    const uint64_t words = (uint64_t)T * (uint64_t)N;     // < 2^62
    if (words > ((uint64_t)1 << 40) / 4 / (uint64_t)stride) return 0;
    return words * (uint64_t)stride * 4;
}

// The protocol: each returns NULL when the call may run (and the *_done twin then moves the books), else why not.
static inline const char *replay_commit_error(const ReplayBooks *) { return nullptr; }     // a commit is in order from every state
static inline void replay_commit_done(ReplayBooks *k) {
    if (k->state == REPLAY_PENDING) k->pushed += 1;
    k->state = REPLAY_READY;
}
static inline const char *replay_record_error(const ReplayBooks *k) {
    if (k->state == REPLAY_EMPTY) return "record before the first commit";
    if (k->state == REPLAY_PENDING) return "two records without a commit between them";
    return nullptr;
}
static inline void replay_record_done(ReplayBooks *k) { k->state = REPLAY_PENDING; }
static inline const char *replay_sample_error(const ReplayBooks *k, int batch, float her_ratio) {
    if (k->state == REPLAY_PENDING) return "sample while a recorded transition waits for its commit";
    if (replay_count(k) == 0) return "sample from an empty replay";
    if (batch < 1) return "batch < 1";
    if (!isfinite(her_ratio) || her_ratio < 0.f || her_ratio > 1.f) return "her_ratio outside [0, 1]";
    return nullptr;
}
// hsr_replay_sample_seq_dev: what hsr_replay_sample_dev refuses, and the window's own numbers.  seq_len <= T keeps every per-sample loop
// finite; batch seq_len < 2^31 keeps the (sample, step) index of the kernel and of every per-step output row inside an int.
static inline const char *replay_sample_seq_error(const ReplayBooks *k, int batch, int seq_len, float her_ratio, float gamma, bool has_out) {
    const char *why = replay_sample_error(k, batch, her_ratio);
    if (why) return why;
    if (!has_out) return "null out";
    if (seq_len < 1) return "seq_len < 1";
    if (seq_len > k->T) return "seq_len above capacity_steps";
    if (!isfinite(gamma) || gamma < 0.f || gamma > 1.f) return "gamma outside [0, 1]";
    if ((uint64_t)batch * (uint64_t)seq_len >= ((uint64_t)1 << 31)) return "batch x seq_len reaches 2^31";
    return nullptr;
}
static inline void replay_clear_done(ReplayBooks *k) { k->state = REPLAY_EMPTY; k->pushed = 0; }

// The n-step reduction of a window (include/hsrsim.h: hsr_replay_sample_seq_dev), for the kernel and for a host program alike.
// step_at(k) gives reward and done of step k and is called for k = 0, 1, .. in order, once each, and not past the first done step.
// m = the smallest k + 1 with done_k != 0 over k < length, else length; ret = sum over k < m of gamma^k reward_k, summed in that order;
// discount = gamma^m; done = done_{m-1}.  Every product and every sum is a float32 operation of its own.
#ifdef __HIPCC__
#define REPLAY_HD __host__ __device__
#else
#define REPLAY_HD
#endif
struct ReplayStep { float reward; uint32_t done; };
struct ReplayNstep { int m; float ret, discount; uint32_t done; };
template <class StepAt> REPLAY_HD static inline ReplayNstep replay_nstep(int length, float gamma, StepAt step_at) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    ReplayNstep r{0, 0.f, 1.f, 0u};
    for (int k = 0; k < length; k++) {
        const ReplayStep s = step_at(k);
        const float term = r.discount * s.reward;
        r.ret = r.ret + term;
        r.discount = r.discount * gamma;
        r.m = k + 1; r.done = s.done;
        if (s.done != 0u) break;
    }
    return r;
}
