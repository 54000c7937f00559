// The host books of an on-policy rollout (include/hsrsim.h: hsr_rollout): row layout, the EMPTY -> READY -> STAGED -> DONE state machine,
// slot arithmetic, the shuffle's domain and the argument checks, in plain C++ without a HIP call or header, so that a stand-alone program can
// exercise them under a sanitizer (tests/rollout_logic_main.cpp).  host_rollout.h asks these functions and launches only what they allow;
// rollout.h indexes with the same layout.
#pragma once
#include <math.h>
#include <stdint.h>

// One stored step of one env = one row of 32-bit words, padded to a multiple of 4 (16-byte rows):  obs[obs_dim] | act[nu] | padding
struct RolloutLayout {
    int obs_dim, nu;
    int o_act, words, stride;      // W = obs_dim + nu, and W rounded up to 4
};
static inline RolloutLayout rollout_layout(int obs_dim, int nu) {
    RolloutLayout L;
    L.obs_dim = obs_dim; L.nu = nu;
    L.o_act = obs_dim;
    L.words = obs_dim + nu;
    L.stride = (L.words + 3) & ~3;
    return L;
}
enum { ROLLOUT_PLANES = 7 };       // logp, value, reward, kind, v_term, adv, ret: one 32-bit word per (step, env) each

enum RolloutState { ROLLOUT_EMPTY = 0, ROLLOUT_READY = 1, ROLLOUT_STAGED = 2, ROLLOUT_DONE = 3 };
struct RolloutBooks {
    int T, N;                      // horizon, envs
    int state;
    int t;                         // steps closed since begin / next: the slot the next stage writes
};
static inline void rollout_books_init(RolloutBooks *k, int T, int N) { k->T = T; k->N = N; k->state = ROLLOUT_EMPTY; k->t = 0; }
static inline int64_t rollout_items(const RolloutBooks *k) { return (int64_t)k->T * (int64_t)k->N; }       // M
static inline int rollout_stage_slot(const RolloutBooks *k) { return k->t; }
static inline int rollout_bootstrap_slot(const RolloutBooks *k) { return k->t - 1; }      // the step closed last

// NULL when the spec's numbers are acceptable, else what is wrong with them
static inline const char *rollout_spec_error(int horizon, int obs_dim, float gamma, float lam, int n_envs) {
    if (horizon < 1) return "horizon < 1";
    if (obs_dim < 1) return "obs_dim < 1";
    if (obs_dim > (1 << 20)) return "obs_dim above 2^20";      // keeps every row offset far inside an int
    if (!isfinite(gamma) || gamma < 0.f || gamma > 1.f) return "gamma outside [0, 1]";
    if (!isfinite(lam) || lam < 0.f || lam > 1.f) return "lam outside [0, 1]";
    if (n_envs < 1) return "no envs";
    if ((int64_t)horizon * (int64_t)n_envs >= ((int64_t)1 << 31)) return "horizon x envs does not fit 31 bits";
    return nullptr;
}
// bytes of rows, planes and head together, or 0 beyond the 2^40 bytes this layer is willing to ask a device for.  T N < 2^31 and
// stride, obs_dim < 2^21 + nu: nothing here leaves 64 bits
static inline uint64_t rollout_storage_bytes(int T, int N, int stride, int obs_dim) {
    const uint64_t items = (uint64_t)T * (uint64_t)N;
    const uint64_t words = items * ((uint64_t)stride + ROLLOUT_PLANES) + (uint64_t)N * (uint64_t)obs_dim;
    if (words > ((uint64_t)1 << 40) / 4) return 0;
    return words * 4;
}

// The shuffle's domain: h bits per Feistel half; the domain 2^(2h) holds M and is below 4 M
static inline int rollout_half_bits(int64_t items) {
    int bits = 0;
    for (uint64_t v = (uint64_t)(items - 1); v; v >>= 1) bits++;
    const int h = (bits + 1) / 2;
    return h < 1 ? 1 : h;
}

// The protocol: each returns NULL when the call may run (and the *_done twin then moves the books), else why not.
static inline const char *rollout_begin_error(const RolloutBooks *) { return nullptr; }       // a begin is in order from every state
static inline void rollout_begin_done(RolloutBooks *k) { k->state = ROLLOUT_READY; k->t = 0; }
static inline const char *rollout_stage_error(const RolloutBooks *k) {
    if (k->state == ROLLOUT_EMPTY) return "stage before begin";
    if (k->state == ROLLOUT_STAGED) return "two stages without a close between them";
    if (k->state == ROLLOUT_DONE) return "stage after finish (next or begin first)";
    if (k->t >= k->T) return "stage past the horizon: the rollout is full (finish)";
    return nullptr;
}
static inline void rollout_stage_done(RolloutBooks *k) { k->state = ROLLOUT_STAGED; }
static inline const char *rollout_close_error(const RolloutBooks *k) {
    if (k->state != ROLLOUT_STAGED) return "close without a staged step";
    return nullptr;
}
static inline void rollout_close_done(RolloutBooks *k) { k->state = ROLLOUT_READY; k->t += 1; }
static inline const char *rollout_bootstrap_error(const RolloutBooks *k) {
    if (k->state != ROLLOUT_READY) return "bootstrap outside READY";
    if (k->t < 1) return "bootstrap before the first step was closed";
    return nullptr;
}
static inline const char *rollout_finish_error(const RolloutBooks *k) {
    if (k->state != ROLLOUT_READY) return "finish outside READY";
    if (k->t < k->T) return "finish before the horizon";
    return nullptr;
}
static inline void rollout_finish_done(RolloutBooks *k) { k->state = ROLLOUT_DONE; }
static inline const char *rollout_read_error(const RolloutBooks *k) {      // stats, planes, next
    if (k->state != ROLLOUT_DONE) return "the rollout is not finished";
    return nullptr;
}
static inline void rollout_next_done(RolloutBooks *k) { k->state = ROLLOUT_READY; k->t = 0; }
static inline const char *rollout_minibatch_error(const RolloutBooks *k, int first, int count) {
    if (k->state != ROLLOUT_DONE) return "the rollout is not finished";
    if (count < 1) return "count < 1";
    if (first < 0) return "first < 0";
    if ((int64_t)first + (int64_t)count > rollout_items(k)) return "first + count beyond horizon x envs";
    return nullptr;
}
