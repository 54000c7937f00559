// Stand-alone exerciser of hsr_env_amd/csrc/plan_logic.h - the arithmetic and the argument checks of the CEM planner: every HSR_EINVAL
// condition, the Irwin-Hall normal, the clamp, the cost recursion, the rank rule, the indexing and the shape of the refit's sums at
// K = 2, 5, 64, 70, 1024, and the refit - for a build with -ffp-contract=off -fsanitize=address,undefined
// (tests/test_plan_logic_sanitized.py).  No HIP, no GPU.  It prints the values it computed from inputs that tests/test_plan_logic_sanitized.py
// builds the same way and compares with tests/plan_ref.py, then "ok <checks>", and returns 0; or says what failed and returns 1.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "../hsr_env_amd/csrc/plan_logic.h"

static long checks = 0;
#define CHECK(x) do { checks++; if (!(x)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

static uint32_t bits32(float x) { uint32_t u; memcpy(&u, &x, sizeof u); return u; }
static unsigned long long bits64(double x) { unsigned long long u; memcpy(&u, &x, sizeof u); return u; }
// the inputs: word(i) = i 2654435761 + 12345 (mod 2^32), val(i) = (word(i) >> 8) 2^-24 in [0, 1), exact in float32
static uint32_t word(uint32_t i) { return i * 2654435761u + 12345u; }
static float val(uint32_t i) { return (float)(word(i) >> 8) * 5.9604644775390625e-8f; }
// planted costs: eighths (ties), every 7th + 3 infinite, every 11th + 5 a NaN
static float planted_cost(int k) {
    if (k % 7 == 3) return (k & 1) ? INFINITY : -INFINITY;
    if (k % 11 == 5) return NAN;
    return floorf(val(300u + (uint32_t)k) * 8.f) * 0.125f;
}

static int spec_ok(int n, int p, int k, int h, int e, int body, float gamma, float alpha, float s0, float smin, int nu, int ngoal) {
    static const int mocap[4] = {0, 1, 0, 0};
    return plan_spec_error(n, p, k, h, e, body, gamma, alpha, s0, smin, nu, 4, mocap, ngoal) == nullptr;
}

int main() {
    // ---- the checks
    CHECK(spec_ok(12, 3, 4, 5, 2, 2, 1.f, 1.f, 0.5f, 0.05f, 7, 0));
    CHECK(spec_ok(2, 1, 2, 1, 1, 0, 0.f, 1e-6f, 1e-30f, 1e30f, 1, 0) && spec_ok(3072, 3, 1024, 64, 1024, 3, 0.5f, 0.5f, 1.f, 1.f, 7, 0));
    CHECK(!spec_ok(13, 3, 4, 5, 2, 2, 1.f, 1.f, 0.5f, 0.05f, 7, 0) && !spec_ok(12, 4, 4, 5, 2, 2, 1.f, 1.f, 0.5f, 0.05f, 7, 0));      // N != P K
    CHECK(!spec_ok(0, 0, 4, 5, 2, 2, 1.f, 1.f, 0.5f, 0.05f, 7, 0) && !spec_ok(-4, -1, 4, 5, 2, 2, 1.f, 1.f, 0.5f, 0.05f, 7, 0));
    CHECK(!spec_ok(3, 3, 1, 5, 1, 2, 1.f, 1.f, 0.5f, 0.05f, 7, 0) && !spec_ok(3075, 3, 1025, 5, 2, 2, 1.f, 1.f, 0.5f, 0.05f, 7, 0));   // samples
    CHECK(!spec_ok(12, 3, 4, 0, 2, 2, 1.f, 1.f, 0.5f, 0.05f, 7, 0) && !spec_ok(12, 3, 4, 65, 2, 2, 1.f, 1.f, 0.5f, 0.05f, 7, 0));      // horizon
    CHECK(!spec_ok(12, 3, 4, 5, 0, 2, 1.f, 1.f, 0.5f, 0.05f, 7, 0) && !spec_ok(12, 3, 4, 5, 5, 2, 1.f, 1.f, 0.5f, 0.05f, 7, 0));       // elites
    CHECK(!spec_ok(12, 3, 4, 5, 2, -1, 1.f, 1.f, 0.5f, 0.05f, 7, 0) && !spec_ok(12, 3, 4, 5, 2, 4, 1.f, 1.f, 0.5f, 0.05f, 7, 0));      // goal body
    CHECK(!spec_ok(12, 3, 4, 5, 2, 1, 1.f, 1.f, 0.5f, 0.05f, 7, 0));                                                                   // the mocap body
    CHECK(!spec_ok(12, 3, 4, 5, 2, 2, 1.f, 1.f, 0.5f, 0.05f, 7, 1));                                                                   // extra goal terms
    CHECK(!spec_ok(12, 3, 4, 5, 2, 2, 1.f, 1.f, 0.5f, 0.05f, 0, 0));                                                                   // no actuators
    for (float bad : {-0.01f, 1.01f, NAN, INFINITY, -INFINITY}) CHECK(!spec_ok(12, 3, 4, 5, 2, 2, bad, 1.f, 0.5f, 0.05f, 7, 0));
    for (float bad : {0.f, -0.5f, 1.01f, NAN, INFINITY}) CHECK(!spec_ok(12, 3, 4, 5, 2, 2, 1.f, bad, 0.5f, 0.05f, 7, 0));
    for (float bad : {0.f, -0.5f, NAN, INFINITY, -INFINITY}) {
        CHECK(!spec_ok(12, 3, 4, 5, 2, 2, 1.f, 1.f, bad, 0.05f, 7, 0));
        CHECK(!spec_ok(12, 3, 4, 5, 2, 2, 1.f, 1.f, 0.5f, bad, 7, 0));
    }
    CHECK(spec_ok(1024, 1, 1024, 64, 2, 2, 1.f, 1.f, 0.5f, 0.05f, 65535, 0) && !spec_ok(1024, 1, 1024, 64, 2, 2, 1.f, 1.f, 0.5f, 0.05f, 65536, 0));   // 2^32 blocks
    float buf[1];
    CHECK(!plan_sample_error(0, 0, 3, buf) && !plan_sample_error(255, 2, 3, buf));
    CHECK(plan_sample_error(-1, 0, 3, buf) && plan_sample_error(256, 0, 3, buf) && plan_sample_error(0, -1, 3, buf) && plan_sample_error(0, 3, 3, buf) &&
          plan_sample_error(0, 0, 3, nullptr));
    CHECK(!plan_step_error(0, 1) && plan_step_error(1, 1) && plan_step_error(-1, 1));
    CHECK(plan_block(1023, 63, 6, 64, 7) == (1023u * 64u + 63u) * 7u + 6u && plan_second(3u, 2) == 770u && plan_second(0x01000000u, 255) == 255u);

    // ---- z: bounds, and values for the reference
    CHECK(plan_z(0u, 0u, 0u, 0u) == -2.f * 1.7320508075688772f && fabsf(plan_z(~0u, ~0u, ~0u, ~0u)) <= 2.f * 1.7320508075688772f);
    printf("z");
    float z[8];
    for (uint32_t i = 0; i < 8; i++) { z[i] = plan_z(word(4 * i), word(4 * i + 1), word(4 * i + 2), word(4 * i + 3)); printf(" %08x", bits32(z[i])); }
    printf("\n");

    // ---- range, clamp, action
    float lo, hi;
    plan_range(-0.5f, 0.75f, &lo, &hi);
    CHECK(lo == -0.5f && hi == 0.75f && plan_half_range(lo, hi) == 0.625f);
    plan_range(-1e30f, INFINITY, &lo, &hi);
    CHECK(lo == -1.f && hi == 1.f);
    plan_range(NAN, 1e30f, &lo, &hi);
    CHECK(lo == -1.f && hi == 1.f);
    CHECK(plan_clamp(0.f, 0.25f, 1.f) == 0.25f && plan_clamp(0.f, -1.f, -0.25f) == -0.25f && plan_clamp(0.f, -1.f, 1.f) == 0.f);
    CHECK(plan_action(0.3f, 0.7f, 0.f, -1.f, 1.f) == 0.3f && plan_action(0.3f, 0.7f, 0.f, -1.f, 0.2f) == 0.2f);       // candidate 0: the clamped mean
    CHECK(plan_sigma0(0.5f, 0.625f) == 0.3125f);
    printf("act");
    for (uint32_t i = 0; i < 8; i++) printf(" %08x", bits32(plan_action(val(i) * 2.f - 1.f, val(100u + i), z[i], -0.5f, 0.75f)));
    printf("\n");

    // ---- the cost recursion: six steps, gamma = 0.5, done at step 4; then a bad env at step 2
    CHECK(plan_dist(1.f, 2.f, 3.f, 1.f, 2.f, 3.f) == 0.f && plan_dist(3.f, 0.f, 4.f, 0.f, 0.f, 0.f) == 5.f);
    PlanCost c = plan_cost_begin();
    CHECK(c.J == 0.f && c.g == 1.f && c.alive == 1 && c.reach_step == -1);
    for (int h = 0; h < 6; h++) plan_cost_step(&c, plan_dist(val(200u + h), val(210u + h), val(220u + h), 0.25f, 0.5f, 0.75f), 0.5f, h == 4, false, h);
    CHECK(c.alive == 0 && c.reach_step == 4 && c.g == 0.03125f);
    printf("cost %08x %08x %d %d\n", bits32(c.J), bits32(c.g), (int)c.alive, (int)c.reach_step);
    c = plan_cost_begin();
    for (int h = 0; h < 6; h++) plan_cost_step(&c, 1.f, 0.5f, h == 3, h == 2, h);
    CHECK(c.J == INFINITY && c.alive == 0 && c.reach_step == -1 && c.g == 0.25f);

    // ---- keys
    CHECK(plan_cost_key(NAN) == INFINITY && plan_cost_key(-INFINITY) == INFINITY && plan_cost_key(INFINITY) == INFINITY && plan_cost_key(-3.f) == -3.f);
    CHECK(plan_finite32(3.4e38f) && plan_finite32(-0.f) && !plan_finite32(NAN) && !plan_finite32(-NAN));
    CHECK(plan_elite_count(3, 5) == 3 && plan_elite_count(3, 2) == 2 && plan_elite_count(3, 0) == 0);

    // ---- rank, tree and refit at every K whose tree has another shape
    for (int K : {2, 5, 64, 70, 1024}) {
        std::vector<float> key(K);
        int finite = 0;
        for (int k = 0; k < K; k++) { key[k] = plan_cost_key(planted_cost(k)); finite += plan_finite32(key[k]) ? 1 : 0; }
        std::vector<int> rank(K), seen(K, 0);
        for (int k = 0; k < K; k++) { rank[k] = plan_rank(key.data(), K, k); CHECK(rank[k] >= 0 && rank[k] < K); seen[rank[k]]++; }
        for (int k = 0; k < K; k++) CHECK(seen[k] == 1);                   // a permutation
        printf("rank %d", K);
        for (int k = 0; k < K; k++) printf(" %d", rank[k]);
        printf("\n");
        // indexing: every leaf is visited once, by the lane and at the position the shape states
        int total = 0;
        std::vector<int> visits(K, 0);
        for (int l = 0; l < PLAN_WAVE; l++) {
            const int n = plan_lane_terms(K, l);
            total += n;
            for (int i = 0; i < n; i++) { CHECK(l + PLAN_WAVE * i < K); visits[l + PLAN_WAVE * i]++; }
            CHECK(l + PLAN_WAVE * n >= K);
        }
        CHECK(total == K);
        for (int k = 0; k < K; k++) CHECK(visits[k] == 1);
        CHECK(plan_tree_depth(K) == (K + 63) / 64 + 6);
        const int E = plan_elite_count(std::max(1, K / 4), finite);
        CHECK(E >= 1);
        std::vector<double> x(K);
        for (int k = 0; k < K; k++) x[k] = (double)(val(500u + (uint32_t)k) - 0.5f);
        const double sum = plan_tree_sum_host(K, [&](int k) { return plan_leaf(x[k], rank[k] < E); });
        const double m = plan_elite_mean(sum, E);
        const double sq = plan_tree_sum_host(K, [&](int k) { return plan_leaf(plan_sq_dev(x[k], m), rank[k] < E); });
        // against the plain serial sum: the bound the tree's depth gives
        long double plain = 0.0L, mag = 0.0L;
        for (int k = 0; k < K; k++) if (rank[k] < E) { plain += x[k]; mag += fabsl((long double)x[k]); }
        CHECK(fabsl((long double)sum - plain) <= (long double)plan_tree_depth(K) * ldexpl(1.0L, -53) * mag * 1.0001L);
        float mean = 0.1f, sigma = 0.3f;
        plan_refit(m, sq, E, 0.7f, 0.05f, 1.5f, &mean, &sigma);
        CHECK(sigma >= 0.05f * 1.5f);
        printf("tree %d %d %016llx %016llx %08x %08x\n", K, E, bits64(sum), bits64(sq), bits32(mean), bits32(sigma));
        // the floor holds when the elites agree
        float m2 = 0.f, s2 = 0.3f;
        plan_refit(0.25, 0.0, E, 1.f, 0.05f, 1.5f, &m2, &s2);
        CHECK(m2 == 0.25f && s2 == (float)((double)0.05f * (double)1.5f));
    }
    printf("ok %ld\n", checks);
    return 0;
}
