// Stand-alone exerciser of hsr_env_amd/csrc/rollout_logic.h - the host books of the on-policy rollout: row layout, state machine, slot
// arithmetic, the shuffle's domain, argument checks - for a build with -fsanitize=address,undefined
// (tests/test_rollout_logic_sanitized.py).  No HIP, no GPU.  It keeps the store the plain way (an array of who wrote which slot, with a guard
// element on either side) next to the books and compares them after every call; prints "ok <checks>" and returns 0, or says what differed
// and returns 1.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../hsr_env_amd/csrc/rollout_logic.h"

static long checks = 0;
#define CHECK(x) do { checks++; if (!(x)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

// every call the state does not allow is refused, and a refusal moves nothing
static int refused_elsewhere(const RolloutBooks *k) {
    const RolloutBooks before = *k;
    const int s = k->state, t = k->t, T = k->T;
    CHECK(rollout_begin_error(k) == nullptr);
    CHECK((rollout_stage_error(k) == nullptr) == (s == ROLLOUT_READY && t < T));
    CHECK((rollout_close_error(k) == nullptr) == (s == ROLLOUT_STAGED));
    CHECK((rollout_bootstrap_error(k) == nullptr) == (s == ROLLOUT_READY && t >= 1));
    CHECK((rollout_finish_error(k) == nullptr) == (s == ROLLOUT_READY && t == T));
    CHECK((rollout_read_error(k) == nullptr) == (s == ROLLOUT_DONE));
    CHECK((rollout_minibatch_error(k, 0, 1) == nullptr) == (s == ROLLOUT_DONE));
    CHECK(before.T == k->T && before.N == k->N && before.state == k->state && before.t == k->t);
    return 0;
}

static int run_protocol(int T, int N, int rollouts) {
    RolloutBooks k;
    rollout_books_init(&k, T, N);
    CHECK(k.state == ROLLOUT_EMPTY && k.t == 0 && rollout_items(&k) == (int64_t)T * N);
    if (refused_elsewhere(&k)) return 1;
    rollout_begin_done(&k);
    for (int r = 0; r < rollouts; r++) {
        std::vector<int> written(T + 2, 0), boot(T + 2, 0);       // slots 1..T with a guard on either side
        CHECK(k.state == ROLLOUT_READY && k.t == 0);
        for (int t = 0; t < T; t++) {
            if (refused_elsewhere(&k)) return 1;
            CHECK(rollout_stage_error(&k) == nullptr);
            const int slot = rollout_stage_slot(&k);
            CHECK(slot == t && slot >= 0 && slot < T);
            written[1 + slot] += 1;
            rollout_stage_done(&k);
            if (refused_elsewhere(&k)) return 1;
            CHECK(rollout_stage_slot(&k) == t);                   // close writes the slot stage wrote
            rollout_close_done(&k);
            CHECK(k.state == ROLLOUT_READY && k.t == t + 1);
            for (int again = 0; again < 2; again++) {             // the last bootstrap wins: both name the step closed last
                CHECK(rollout_bootstrap_error(&k) == nullptr);
                const int b = rollout_bootstrap_slot(&k);
                CHECK(b == t && b >= 0 && b < T);
                boot[1 + b] += 1;
            }
        }
        if (refused_elsewhere(&k)) return 1;
        CHECK(rollout_stage_error(&k) != nullptr && rollout_finish_error(&k) == nullptr);
        rollout_finish_done(&k);
        if (refused_elsewhere(&k)) return 1;
        CHECK(!written[0] && !written[T + 1] && !boot[0] && !boot[T + 1]);
        for (int t = 0; t < T; t++) CHECK(written[1 + t] == 1 && boot[1 + t] == 2);
        // minibatch arguments
        const int64_t M = rollout_items(&k);
        CHECK(rollout_minibatch_error(&k, 0, (int)M) == nullptr && rollout_minibatch_error(&k, (int)M - 1, 1) == nullptr);
        CHECK(rollout_minibatch_error(&k, 0, 0) && rollout_minibatch_error(&k, 0, -1) && rollout_minibatch_error(&k, -1, 1) &&
              rollout_minibatch_error(&k, (int)M, 1) && rollout_minibatch_error(&k, 0, (int)M + 1) && rollout_minibatch_error(&k, 1, (int)M) &&
              rollout_minibatch_error(&k, 0x7fffffff, 0x7fffffff));
        if (r % 2) { rollout_next_done(&k); } else { rollout_begin_done(&k); }     // either way back to READY(0)
    }
    // a begin in the middle of a rollout, and from STAGED, starts again
    rollout_stage_done(&k);
    rollout_begin_done(&k);
    CHECK(k.state == ROLLOUT_READY && k.t == 0);
    return 0;
}

int main() {
    // row layout: the cases of the tests and the extremes the checks admit
    const int dims[][4] = {{17, 2, 19, 20}, {27, 7, 34, 36}, {25, 7, 32, 32}, {1, 1, 2, 4}, {1 << 20, 32, (1 << 20) + 32, (1 << 20) + 32}, {1 << 20, 33, (1 << 20) + 33, (1 << 20) + 36}};
    for (const auto &d : dims) {
        const RolloutLayout L = rollout_layout(d[0], d[1]);
        CHECK(L.words == d[2] && L.stride == d[3] && L.stride % 4 == 0 && L.stride - L.words < 4 && L.stride >= L.words);
        CHECK(L.o_act == d[0] && L.obs_dim == d[0] && L.nu == d[1]);
    }
    // spec checks
    CHECK(rollout_spec_error(5, 17, 0.99f, 0.95f, 70) == nullptr);
    CHECK(rollout_spec_error(1, 1, 0.f, 0.f, 1) == nullptr && rollout_spec_error(1, 1 << 20, 1.f, 1.f, 1) == nullptr);
    CHECK(rollout_spec_error(0, 17, 0.99f, 0.95f, 70) && rollout_spec_error(-3, 17, 0.99f, 0.95f, 70));
    CHECK(rollout_spec_error(5, 0, 0.99f, 0.95f, 70) && rollout_spec_error(5, -1, 0.99f, 0.95f, 70) && rollout_spec_error(5, (1 << 20) + 1, 0.99f, 0.95f, 70));
    for (float bad : {-0.01f, 1.01f, NAN, INFINITY, -INFINITY}) {
        CHECK(rollout_spec_error(5, 17, bad, 0.95f, 70));
        CHECK(rollout_spec_error(5, 17, 0.99f, bad, 70));
    }
    CHECK(rollout_spec_error(5, 17, 0.99f, 0.95f, 0));
    // T N at 2^31 - 1 (a prime: 1 x it, and it x 1) and at 2^31
    CHECK(rollout_spec_error(0x7fffffff, 1, 0.99f, 0.95f, 1) == nullptr && rollout_spec_error(1, 1, 0.99f, 0.95f, 0x7fffffff) == nullptr);
    CHECK(rollout_spec_error(1 << 16, 1, 0.99f, 0.95f, 1 << 15) && rollout_spec_error(1 << 15, 1, 0.99f, 0.95f, 1 << 16));
    CHECK(rollout_spec_error((1 << 16) - 1, 1, 0.99f, 0.95f, 1 << 15) == nullptr);
    CHECK(rollout_spec_error(0x7fffffff, 1, 0.99f, 0.95f, 0x7fffffff));
    // storage: rows + seven planes + head, up to 2^40 bytes and not beyond
    CHECK(rollout_storage_bytes(5, 70, 20, 17) == (5ull * 70 * (20 + 7) + 70 * 17) * 4);
    CHECK(rollout_storage_bytes(1, 1, 4, 1) == (4 + 7 + 1) * 4);
    CHECK(rollout_storage_bytes(1 << 10, 1 << 10, (1 << 18) - 8, 1 << 10) == (1ull << 40));        // 2^20 (2^18 - 1) + 2^20 words = 2^38
    CHECK(rollout_storage_bytes(1 << 10, 1 << 10, (1 << 18) - 8, (1 << 10) + 1) == 0);
    CHECK(rollout_storage_bytes(0x7fffffff, 1, (1 << 20) + 36, 1 << 20) == 0 && rollout_storage_bytes(1, 0x7fffffff, (1 << 20) + 36, 1 << 20) == 0);
    // the shuffle's domain holds M and is below 4 M
    const int64_t sizes[] = {1, 2, 3, 4, 5, 255, 256, 257, 350, 4096, 32769, 1 << 20, (1ll << 31) - 1};
    for (int64_t M : sizes) {
        const int h = rollout_half_bits(M);
        CHECK(h >= 1 && h <= 16 && ((int64_t)1 << (2 * h)) >= M && (M == 1 || ((int64_t)1 << (2 * h)) < 4 * M));
    }
    CHECK(rollout_half_bits(1) == 1 && rollout_half_bits(256) == 4 && rollout_half_bits(257) == 5 && rollout_half_bits(350) == 5 &&
          rollout_half_bits((1ll << 31) - 1) == 16);
    // the protocol: T = 1, small, and one env or many
    const int shapes[][2] = {{1, 1}, {1, 70}, {2, 3}, {5, 70}, {32, 8192}};
    for (const auto &s : shapes) if (run_protocol(s[0], s[1], 3)) return 1;
    printf("ok %ld\n", checks);
    return 0;
}
