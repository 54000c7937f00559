// Stand-alone exerciser of hsr_env_amd/csrc/normalize_logic.h - the arithmetic and the argument checks of the running-moments normaliser:
// the checks, the finite test, Chan's merge, the publish rule, the apply, m == 0, count == 0 - for a build with
// -ffp-contract=off -fsanitize=address,undefined (tests/test_normalize_logic_sanitized.py).  No HIP, no GPU.  It keeps the rows the plain
// way (one vector, two passes in long double) next to the merged state and compares; prints "ok <checks>" and returns 0, or says what
// differed and returns 1.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <limits>
#include <vector>

#include "../hsr_env_amd/csrc/normalize_logic.h"

static long checks = 0;
#define CHECK(x) do { checks++; if (!(x)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static double uniform() {          // xorshift64*, in [0, 1)
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return (double)((rng_state * 0x2545F4914F6CDD1Dull) >> 11) / 9007199254740992.0;
}
static uint64_t bits(double x) { uint64_t u; memcpy(&u, &x, sizeof u); return u; }
static uint32_t bits32(float x) { uint32_t u; memcpy(&u, &x, sizeof u); return u; }

// `updates` batches of `m` values offset + scale u merged one by one against all of them at once
static int merge_against_two_pass(int updates, int m, double offset, double scale) {
    std::vector<float> all;
    double count = 0.0, mean = 0.0, m2 = 0.0;
    for (int u = 0; u < updates; u++) {
        std::vector<float> batch(m);
        for (float &x : batch) { x = (float)(offset + scale * (uniform() - 0.5)); all.push_back(x); }
        double s = 0.0, q = 0.0;
        for (float x : batch) s += (double)x;
        const double mean_b = s / m;
        for (float x : batch) q += ((double)x - mean_b) * ((double)x - mean_b);
        norm_merge(count, (double)m, mean_b, q, &mean, &m2);
        count += m;
    }
    long double s = 0.0L, q = 0.0L, mag = 0.0L;
    for (float x : all) { s += x; mag += fabsl((long double)x); }
    const long double ref_mean = s / all.size();
    for (float x : all) q += (x - ref_mean) * (x - ref_mean);
    // the bound of tests/test_gpu_normalize.py: (M + 8 U) 2^-52 mean|x| on the mean
    const double M = (double)all.size(), bound = (M + 8.0 * updates) * ldexp(1.0, -52) * (double)(mag / all.size());
    const double sd = sqrt((double)(q / all.size()));
    CHECK(count == M);
    CHECK(fabs(mean - (double)ref_mean) <= bound);
    CHECK(bound < 1e-3 * sd);
    CHECK(fabsl(m2 - q) <= 1e-9L * q);
    return 0;
}

int main() {
    // the checks
    CHECK(norm_create_error(1, 0.01f, 5.f) == nullptr && norm_create_error(1024, 1e-30f, 1e30f) == nullptr && norm_create_error(27, 0.01f, 5.f) == nullptr);
    CHECK(norm_create_error(0, 0.01f, 5.f) && norm_create_error(-1, 0.01f, 5.f) && norm_create_error(1025, 0.01f, 5.f));
    for (float bad : {0.f, -0.01f, NAN, INFINITY, -INFINITY}) {
        CHECK(norm_create_error(3, bad, 5.f));
        CHECK(norm_create_error(3, 0.01f, bad));
    }
    const float some = 0.f;
    const void *p = &some, *q = &checks;         // stand-ins for device pointers and batch handles: compared, never followed
    CHECK(norm_update_error(27, 0, 27, p) == nullptr && norm_update_error(27, 65536, 27, p) == nullptr && norm_update_error(27, 1, 1 << 20, p) == nullptr);
    CHECK(norm_update_error(27, 0x7fffffff, 27, p) == nullptr && norm_update_error(27, (int64_t)1 << 31, 27, p));
    CHECK(norm_update_error(27, -1, 27, p) && norm_update_error(27, 4, 26, p) && norm_update_error(27, 4, 0, p) && norm_update_error(27, 4, -27, p));
    CHECK(norm_update_error(27, 4, 27, nullptr) && norm_update_error(27, 0, 27, nullptr) == nullptr);
    CHECK(norm_apply_error(3, 0, 3, 3, p, p) == nullptr && norm_apply_error(3, 9, 3, 8, p, p) == nullptr && norm_apply_error(3, 9, 8, 3, p, p) == nullptr);
    CHECK(norm_apply_error(3, -1, 3, 3, p, p) && norm_apply_error(3, 9, 2, 3, p, p) && norm_apply_error(3, 9, 3, 2, p, p) && norm_apply_error(3, (int64_t)1 << 31, 3, 3, p, p));
    CHECK(norm_apply_error(3, 9, 3, 3, nullptr, p) && norm_apply_error(3, 9, 3, 3, p, nullptr) && norm_apply_error(3, 0, 3, 3, nullptr, nullptr) == nullptr);
    CHECK(norm_batch_error(p, 1) == nullptr && norm_batch_error(p, NORM_BATCH_ITEMS) == nullptr);
    CHECK(norm_batch_error(nullptr, 1) && norm_batch_error(p, 0) && norm_batch_error(p, -1) && norm_batch_error(p, NORM_BATCH_ITEMS + 1));
    CHECK(norm_item_error(0, 1, 0, nullptr) == nullptr && norm_item_error(4096, 1, 1, p) == nullptr && norm_item_error(4096 * 8, 8, 0, p) == nullptr);
    CHECK(norm_item_error(-1, 1, 0, p) && norm_item_error(10, 0, 0, p) && norm_item_error(10, -2, 0, p) && norm_item_error(10, 3, 0, p) &&
          norm_item_error((int64_t)1 << 31, 1, 0, p));
    CHECK(norm_item_error(10, 1, 2, p) && norm_item_error(10, 1, -1, p) && norm_item_error(10, 1, 0, nullptr));
    CHECK(norm_owner_error(p, p) == nullptr && norm_owner_error(p, q) && norm_owner_error(nullptr, p));
    {
        const double mean[3] = {0.0, -1e300, 5.0}, m2[3] = {0.0, 1e300, 2.0};
        CHECK(norm_state_error(3, 0.0, mean, m2) == nullptr && norm_state_error(3, 490.0, mean, m2) == nullptr && norm_state_error(3, 1.0, nullptr, nullptr) == nullptr);
        CHECK(norm_state_error(3, -1.0, mean, m2) && norm_state_error(3, NAN, mean, m2) && norm_state_error(3, INFINITY, mean, m2));
        for (double bad : {(double)NAN, (double)INFINITY, -(double)INFINITY}) {
            double a[3] = {0.0, bad, 0.0};
            CHECK(norm_state_error(3, 1.0, a, m2) && norm_state_error(3, 1.0, mean, a));
        }
        const double neg[3] = {0.0, 0.0, -1e-300};
        CHECK(norm_state_error(3, 1.0, mean, neg) && norm_state_error(3, 1.0, neg, m2) == nullptr);
    }
    // the shape
    CHECK(norm_tiles(0) == 0 && norm_tiles(1) == 1 && norm_tiles(128) == 1 && norm_tiles(129) == 2 && norm_tiles(65536) == 512 && norm_tiles(0x7fffffff) == (1 << 24));
    CHECK(norm_chunks(1) == 1 && norm_chunks(64) == 1 && norm_chunks(65) == 2 && norm_chunks(1024) == 16);
    CHECK(norm_partial_doubles(65536, 27) == 512 * (29 + 27) && norm_partial_doubles(1, 1) == 4 && norm_partial_doubles(0, 27) == 0);
    CHECK(norm_partial_doubles(0x7fffffff, 1024) == ((int64_t)1 << 24) * 2050);
    // the finite test
    {
        const float inf = std::numeric_limits<float>::infinity(), tiny = std::numeric_limits<float>::denorm_min(), big = std::numeric_limits<float>::max();
        CHECK(norm_finite32(0.f) && norm_finite32(-0.f) && norm_finite32(tiny) && norm_finite32(-big) && norm_finite32(big));
        CHECK(!norm_finite32(inf) && !norm_finite32(-inf) && !norm_finite32(NAN) && !norm_finite32(-NAN));
        std::vector<float> row(53, 1.f);
        CHECK(norm_row_finite(row.data(), 53));
        for (int at : {0, 26, 52}) {
            for (float bad : {inf, -inf, (float)NAN}) {
                row[at] = bad;
                CHECK(!norm_row_finite(row.data(), 53) && norm_row_finite(row.data(), at) && norm_row_finite(row.data() + at + 1, 52 - at));
                row[at] = 1.f;
            }
        }
    }
    // merge: m == 0 writes nothing (the bits of a NaN batch mean never reach the state); the first batch becomes the state; two halves of
    // a two-point column
    {
        double mean = 1.25, m2 = 7.5;
        const uint64_t b_mean = bits(mean), b_m2 = bits(m2);
        norm_merge(10.0, 0.0, NAN, NAN, &mean, &m2);
        CHECK(bits(mean) == b_mean && bits(m2) == b_m2);
        norm_merge(0.0, 0.0, NAN, 0.0, &mean, &m2);
        CHECK(bits(mean) == b_mean && bits(m2) == b_m2);
        mean = 0.0; m2 = 0.0;
        norm_merge(0.0, 70.0, 1000.5, 0.25, &mean, &m2);
        CHECK(mean == 1000.5 && m2 == 0.25);
        mean = -1.0; m2 = 0.0;                       // 8 rows of -1, then 8 rows of +1: mean 0, m2 = 16
        norm_merge(8.0, 8.0, 1.0, 0.0, &mean, &m2);
        CHECK(mean == 0.0 && m2 == 16.0);
    }
    // merge against two passes over everything: easy data, and the offset case of the GPU test (and ten times its offset)
    if (merge_against_two_pass(7, 33, 0.0, 2.0)) return 1;
    if (merge_against_two_pass(200, 70, 1000.0, 0.04)) return 1;
    if (merge_against_two_pass(200, 70, 10000.0, 0.04)) return 1;
    if (merge_against_two_pass(1, 14000, 1000.0, 0.04)) return 1;
    // publish: count == 0 is the identity; the eps floor; an ordinary column
    {
        float mean32 = 7.f, rstd32 = 7.f;
        norm_publish(0.0, 3.0, 4.0, 0.01, &mean32, &rstd32);
        CHECK(mean32 == 0.f && rstd32 == 1.f);
        norm_publish(100.0, 1000.0, 0.0, 0.25, &mean32, &rstd32);          // a constant column: std = eps
        CHECK(mean32 == 1000.f && rstd32 == 4.f);
        norm_publish(100.0, -2.0, 100.0 * 1e-6, 0.25, &mean32, &rstd32);   // std 1e-3 below the floor
        CHECK(mean32 == -2.f && rstd32 == 4.f);
        norm_publish(16.0, 0.5, 64.0, 0.01, &mean32, &rstd32);             // var 4, std 2
        CHECK(mean32 == 0.5f && rstd32 == 0.5f);
        const double third = 1.0 / 3.0;
        norm_publish(1.0, third, 0.0, 1.0, &mean32, &rstd32);
        CHECK(mean32 == (float)third && rstd32 == 1.f);
    }
    // apply: the two roundings, the clip at exactly +-clip, NaN stays NaN, the identity
    {
        CHECK(norm_apply(3.f, 1.f, 0.5f, 5.f) == 1.f);
        CHECK(norm_apply(100.f, 0.f, 1.f, 5.f) == 5.f && norm_apply(-100.f, 0.f, 1.f, 5.f) == -5.f);
        CHECK(norm_apply(5.f, 0.f, 1.f, 5.f) == 5.f && norm_apply(-5.f, 0.f, 1.f, 5.f) == -5.f && norm_apply(4.999f, 0.f, 1.f, 5.f) == 4.999f);
        CHECK(isnan(norm_apply(NAN, 0.f, 1.f, 5.f)));
        CHECK(norm_apply(INFINITY, 0.f, 1.f, 5.f) == 5.f && norm_apply(-INFINITY, 0.f, 1.f, 5.f) == -5.f);
        CHECK(bits32(norm_apply(-0.f, 0.f, 1.f, 5.f)) == bits32(-0.f - 0.f));
        // the difference is rounded to float32 before the product: x - mean = 1 + 2^-24 rounds to 1 (ties to even); carried on in a
        // wider format it would give 3 + 3 2^-24, which rounds to 3 + 2^-22
        const float x = 1.f, mean = -5.9604644775390625e-8f;        // -2^-24
        volatile float centred = x - mean;
        CHECK(centred == 1.f);
        CHECK(norm_apply(x, mean, 3.f, 5.f) == 3.f);
        for (int k = 0; k < 1000; k++) {
            const float v = (float)(200.0 * (uniform() - 0.5)), mu = (float)(uniform() - 0.5), rs = (float)(0.01 + uniform());
            volatile float c = v - mu;
            volatile float y = c * rs;
            const float want = y > 5.f ? 5.f : y < -5.f ? -5.f : y;
            CHECK(bits32(norm_apply(v, mu, rs, 5.f)) == bits32(want));
        }
    }
    printf("ok %ld\n", checks);
    return 0;
}
