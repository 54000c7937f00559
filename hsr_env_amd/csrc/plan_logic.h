// The arithmetic and the argument checks of the cross-entropy-method planner (include/hsrsim.h: hsr_plan) in plain C++ without a HIP call or
// header: every HSR_EINVAL condition, the Irwin-Hall normal, the clamp, the cost recursion, the rank rule, the shape of the refit's sums and
// the refit itself.  plan.h's kernels and host_plan.h compile these very functions, and so does a stand-alone program under a sanitizer
// (tests/plan_logic_main.cpp).  A refused call launches nothing.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#ifdef __HIPCC__
#define PLAN_HD __host__ __device__
#else
#define PLAN_HD
#endif

enum { PLAN_SAMPLES_MIN = 2, PLAN_SAMPLES_MAX = 1024, PLAN_HORIZON_MAX = 64, PLAN_ITER_MAX = 255, PLAN_WAVE = 64 };

// ---- checks: NULL when the numbers are acceptable, else what is wrong with them.  nbody / mocap flags / goal terms come from the batch.
static inline const char *plan_spec_error(int n_envs, int groups, int samples, int horizon, int elites, int goal_body, float gamma, float alpha,
                                          float init_std, float min_std, int nu, int nbody, const int *body_mocap, int ngoal_terms) {
    if (nu < 1) return "the model has no actuators";
    if (samples < PLAN_SAMPLES_MIN || samples > PLAN_SAMPLES_MAX) return "samples outside 2..1024";
    if (groups < 1 || (int64_t)groups * samples != (int64_t)n_envs) return "the batch's envs are not groups x samples";
    if (horizon < 1 || horizon > PLAN_HORIZON_MAX) return "horizon outside 1..64";
    if (elites < 1 || elites > samples) return "elites outside 1..samples";
    if (goal_body < 0 || goal_body >= nbody) return "goal_body out of range";
    if (body_mocap[goal_body]) return "goal_body is the mocap body (the goal point itself, not what has to reach it)";
    if (ngoal_terms > 0) return "the batch has extra goal terms (hsr_batch_set_goals): a cost of several terms cannot be computed from one goal point";
    if (!(gamma >= 0.f && gamma <= 1.f)) return "gamma outside [0, 1]";
    if (!(alpha > 0.f && alpha <= 1.f)) return "alpha outside (0, 1]";
    if (!isfinite(init_std) || !(init_std > 0.f)) return "init_std is not a finite positive number";
    if (!isfinite(min_std) || !(min_std > 0.f)) return "min_std is not a finite positive number";
    if ((uint64_t)samples * (uint64_t)horizon * (uint64_t)nu >= ((uint64_t)1 << 32)) return "samples x horizon x nu does not fit the 32-bit block counter";
    return nullptr;
}
static inline const char *plan_sample_error(int64_t iter, int64_t h, int horizon, const void *d_ctrl) {
    if (iter < 0 || iter > PLAN_ITER_MAX) return "iter outside 0..255";
    if (h < 0 || h >= horizon) return "h outside 0..horizon-1";
    if (!d_ctrl) return "null d_ctrl";
    return nullptr;
}
static inline const char *plan_step_error(int64_t h, int horizon) {
    if (h < 0 || h >= horizon) return "h outside 0..horizon-1";
    return nullptr;
}

// ---- the draw.  Philox counter word 3 of (candidate k, step h, actuator a)
PLAN_HD static inline uint32_t plan_block(int k, int h, int a, int horizon, int nu) { return ((uint32_t)k * (uint32_t)horizon + (uint32_t)h) * (uint32_t)nu + (uint32_t)a; }
PLAN_HD static inline uint32_t plan_second(uint32_t call, int iter) { return call * 256u + (uint32_t)iter; }

// Irwin-Hall normal of one Philox block: the sum of four uniforms has mean 2 and variance 1/3.  u = (w >> 8) 2^-24 is exact; the three sums,
// the difference and the product are float32 operations, each rounded on its own.  |z| <= 2 sqrt(3).
PLAN_HD static inline float plan_z(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const float s = 5.9604644775390625e-8f;
    const float u0 = (float)(w0 >> 8) * s, u1 = (float)(w1 >> 8) * s, u2 = (float)(w2 >> 8) * s, u3 = (float)(w3 >> 8) * s;
    const float a = u0 + u1, b = u2 + u3;
    const float sum = a + b;
    const float centred = sum - 2.f;
    return centred * 1.7320508075688772f;
}
// the range an actuator is clamped into: a side without a limit (not finite, or the compiled models' marker 1e30) counts as -1 / +1
PLAN_HD static inline void plan_range(float lo_in, float hi_in, float *lo, float *hi) {
    *lo = fabsf(lo_in) < 1e30f ? lo_in : -1.f;
    *hi = fabsf(hi_in) < 1e30f ? hi_in : 1.f;
}
PLAN_HD static inline float plan_half_range(float lo, float hi) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const float span = hi - lo;
    return span * 0.5f;
}
PLAN_HD static inline float plan_clamp(float x, float lo, float hi) { return x < lo ? lo : x > hi ? hi : x; }
// ctrl = clamp(mean + sigma z, lo, hi): a float32 product and a float32 sum, each rounded on its own.  Candidate 0 passes z = 0.
PLAN_HD static inline float plan_action(float mean, float sigma, float z, float lo, float hi) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const float step = sigma * z;
    const float x = mean + step;
    return plan_clamp(x, lo, hi);
}
PLAN_HD static inline float plan_sigma0(float init_std, float half_range) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    return init_std * half_range;
}

// ---- the cost.  d = sqrt((dx dx + dy dy) + dz dz) of the difference of two points: three differences, three products, two sums and an IEEE
// square root, each a float32 operation rounded on its own.  It is the expression of the env-step's goal test, which the step kernels are free
// to contract and whose square root is the 1-ulp hardware one: the two may differ in the last bit, and only the step's own test decides `done`.
PLAN_HD static inline float plan_dist(float ax, float ay, float az, float gx, float gy, float gz) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const float dx = ax - gx, dy = ay - gy, dz = az - gz;
    const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
    const float s = xx + yy;
    const float t = s + zz;
    return sqrtf(t);
}
struct PlanCost { float J, g; uint8_t alive; int32_t reach_step; };
PLAN_HD static inline PlanCost plan_cost_begin() { PlanCost c; c.J = 0.f; c.g = 1.f; c.alive = 1; c.reach_step = -1; return c; }
// after env-step h of a candidate: a dead candidate keeps everything; a bad env costs +inf; else J = J + g d, g = g gamma, and a latched done
// ends the candidate (the rest of the horizon costs nothing)
PLAN_HD static inline void plan_cost_step(PlanCost *c, float d, float gamma, bool done, bool bad, int h) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    if (!c->alive) return;
    if (bad) { c->J = INFINITY; c->alive = 0; return; }
    const float term = c->g * d;
    c->J = c->J + term;
    c->g = c->g * gamma;
    if (done) { c->alive = 0; c->reach_step = h; }
}

// ---- the rank.  A NaN or an infinity of either sign counts as +inf, by the bits
PLAN_HD static inline bool plan_finite32(float x) {
    uint32_t u;
    memcpy(&u, &x, sizeof u);
    return (u & 0x7f800000u) != 0x7f800000u;
}
PLAN_HD static inline float plan_cost_key(float J) { return plan_finite32(J) ? J : INFINITY; }
// rank(k) = #{ j : key_j < key_k or (key_j == key_k and j < k) } over keys made by plan_cost_key
PLAN_HD static inline int plan_rank(const float *key, int K, int k) {
    const float mine = key[k];
    int r = 0;
    for (int j = 0; j < K; j++) r += (key[j] < mine || (key[j] == mine && j < k)) ? 1 : 0;
    return r;
}
PLAN_HD static inline int plan_elite_count(int elites, int finite) { return elites < finite ? elites : finite; }

// ---- THE SHAPE OF THE REFIT'S SUMS depends on K only.  One sum runs over all K leaves, candidate k at leaf k; a candidate that is no elite
// adds +0.0 in its place:
//   1. lane l of 64 adds, serially from 0.0 and in this order, the leaves l, l + 64, l + 128, .. below K (plan_lane_terms(K, l) of them);
//   2. the 64 lane values in the shuffle tree of wave_sum_fixed (rollout.h): for off = 32, 16, 8, 4, 2, 1: v[l] += v[l + off], l + off < 64;
//      the sum is lane 0's.
// An addition chain is at most PLAN_TREE_DEPTH(K) = ceil(K / 64) + 6 long.
PLAN_HD static inline int plan_lane_terms(int K, int lane) { return lane < K ? (K - 1 - lane) / PLAN_WAVE + 1 : 0; }
PLAN_HD static inline int plan_tree_depth(int K) { return (K + PLAN_WAVE - 1) / PLAN_WAVE + 6; }
PLAN_HD static inline double plan_leaf(double term, bool elite) { return elite ? term : 0.0; }
PLAN_HD static inline double plan_sq_dev(double x, double m) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double d = x - m;
    return d * d;
}
// the same sum on the host (the sanitized program and nothing else): term(k) is the leaf of candidate k
template <typename F>
static inline double plan_tree_sum_host(int K, F term) {
    double v[PLAN_WAVE];
    for (int l = 0; l < PLAN_WAVE; l++) {
        double acc = 0.0;
        for (int i = 0, n = plan_lane_terms(K, l); i < n; i++) acc = acc + term(l + PLAN_WAVE * i);
        v[l] = acc;
    }
    for (int off = 32; off >= 1; off >>= 1)
        for (int l = 0; l + off < PLAN_WAVE; l++) v[l] = v[l] + v[l + off];     // ascending l: v[l + off] still holds its value of the previous level
    return v[0];
}

// ---- the refit of one (h, a) entry from its two sums over the E' elites, in double, every operation rounded on its own:
//   m = sum_x / E'; v = sum_sq / E'; mean <- (float)(mean + alpha (m - mean)); sigma <- (float)max(sigma + alpha (sqrt(v) - sigma), min_std half_range)
PLAN_HD static inline double plan_elite_mean(double sum_x, int e) { return sum_x / (double)e; }
PLAN_HD static inline void plan_refit(double m, double sum_sq, int e, float alpha, float min_std, float half_range, float *mean, float *sigma) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double v = sum_sq / (double)e, al = (double)alpha;
    const double mu = (double)*mean, sg = (double)*sigma;
    const double dm = m - mu;
    const double mstep = al * dm;
    const double sd = sqrt(v);
    const double ds = sd - sg;
    const double sstep = al * ds;
    const double snew = sg + sstep;
    const double floor_ = (double)min_std * (double)half_range;
    *mean = (float)(mu + mstep);
    *sigma = (float)(snew > floor_ ? snew : floor_);
}
