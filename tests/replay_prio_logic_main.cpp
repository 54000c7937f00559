// Stand-alone exerciser of the priorities' host logic in hsr_env_amd/csrc/replay_prio_logic.h - the spec and argument checks, the level
// sizes, the clamp and the staleness rule - for a build with -fsanitize=address,undefined (tests/test_replay_prio_logic_sanitized.py).
// No HIP, no GPU.  The staleness rule is walked exhaustively for small rings against a brute-force history: an array that remembers which
// record every slot holds.  Prints "ok <checks>" and returns 0, or says what differed and returns 1.
#include <math.h>
#include <stdio.h>

#include <limits>
#include <vector>

#include "../hsr_env_amd/csrc/replay_prio_logic.h"

static long checks = 0;
#define CHECK(x) do { checks++; if (!(x)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

int main() {
    const float inf = std::numeric_limits<float>::infinity();
    // ---- enable: only on an empty replay, only with 0 < p_min <= p_init <= p_max, all finite
    ReplayBooks k;
    PrioBooks off{};
    replay_books_init(&k, 7, 70);
    CHECK(prio_enable_error(&k, &off, 1.f, 1e-6f, 1e6f, 256) == nullptr);
    CHECK(prio_enable_error(&k, &off, 1.f, 1.f, 1.f, 1) == nullptr);
    CHECK(prio_enable_error(&k, &off, 1.f, 1e-30f, 1e30f, 0x7fffffff) == nullptr);
    CHECK(prio_enable_error(&k, &off, 1.f, 0.f, 2.f, 256) && prio_enable_error(&k, &off, 1.f, -1.f, 2.f, 256));
    CHECK(prio_enable_error(&k, &off, 0.5f, 1.f, 2.f, 256) && prio_enable_error(&k, &off, 3.f, 1.f, 2.f, 256) && prio_enable_error(&k, &off, 1.f, 2.f, 1.f, 256));
    CHECK(prio_enable_error(&k, &off, NAN, 1.f, 2.f, 256) && prio_enable_error(&k, &off, 1.f, NAN, 2.f, 256) && prio_enable_error(&k, &off, 1.f, 1.f, NAN, 256));
    CHECK(prio_enable_error(&k, &off, 1.f, 1.f, inf, 256) && prio_enable_error(&k, &off, inf, 1.f, inf, 256));
    CHECK(prio_enable_error(&k, &off, 1.f, 1e-6f, 1e6f, 0) && prio_enable_error(&k, &off, 1.f, 1e-6f, 1e6f, -5));
    PrioBooks on{true, 1.f, 1e-6f, 1e6f, 256};
    CHECK(prio_enable_error(&k, &on, 1.f, 1e-6f, 1e6f, 256));                                   // twice
    replay_commit_done(&k);
    CHECK(prio_enable_error(&k, &off, 1.f, 1e-6f, 1e6f, 256));                                  // after a commit
    replay_clear_done(&k);
    CHECK(prio_enable_error(&k, &off, 1.f, 1e-6f, 1e6f, 256) == nullptr);                       // a clear makes it empty again
    ReplayBooks big, huge;
    replay_books_init(&big, 1 << 15, 1 << 15);                                                  // 2^30 leaves: the most
    replay_books_init(&huge, (1 << 15) + 1, 1 << 15);
    CHECK(prio_enable_error(&big, &off, 1.f, 1e-6f, 1e6f, 256) == nullptr && prio_enable_error(&huge, &off, 1.f, 1e-6f, 1e6f, 256));
    replay_books_init(&huge, 0x7fffffff, 0x7fffffff);                                           // the product does not wrap
    CHECK(prio_enable_error(&huge, &off, 1.f, 1e-6f, 1e6f, 256));

    // ---- samplers and update: refusals
    CHECK(prio_sample_error(&k, &on, 4, 0.5f) && prio_update_error(&k, &on, 0, 4, true));       // empty
    replay_commit_done(&k); replay_record_done(&k); replay_commit_done(&k);                     // one transition
    CHECK(prio_sample_error(&k, &on, 4, 0.5f) == nullptr && prio_sample_error(&k, &on, 256, 0.5f) == nullptr);
    CHECK(prio_sample_error(&k, &off, 4, 0.5f) && prio_sample_error(&k, &on, 257, 0.5f) && prio_sample_error(&k, &on, 0, 0.5f) && prio_sample_error(&k, &on, 4, 1.5f));
    CHECK(prio_sample_seq_error(&k, &on, 4, 2, 0.5f, 0.9f, true) == nullptr);
    CHECK(prio_sample_seq_error(&k, &off, 4, 2, 0.5f, 0.9f, true) && prio_sample_seq_error(&k, &on, 257, 2, 0.5f, 0.9f, true) &&
          prio_sample_seq_error(&k, &on, 4, 8, 0.5f, 0.9f, true) && prio_sample_seq_error(&k, &on, 4, 2, 0.5f, 0.9f, false));
    CHECK(prio_update_error(&k, &on, 0, 4, true) == nullptr && prio_update_error(&k, &on, 1, 256, true) == nullptr);
    CHECK(prio_update_error(&k, &on, 2, 4, true));                                              // sampled_at > pushed
    CHECK(prio_update_error(&k, &off, 1, 4, true) && prio_update_error(&k, &on, 1, 0, true) && prio_update_error(&k, &on, 1, 257, true) &&
          prio_update_error(&k, &on, 1, 4, false) && prio_update_error(&k, &on, ~(uint64_t)0, 4, true));
    replay_record_done(&k);
    CHECK(prio_sample_error(&k, &on, 4, 0.5f) && prio_sample_seq_error(&k, &on, 4, 2, 0.5f, 0.9f, true));     // a pending record
    CHECK(prio_update_error(&k, &on, 1, 4, true) == nullptr && prio_written(&k) == 2);          // an update may run; the pending record counts as written

    // ---- level sizes
    PrioLevels P = prio_levels(1);
    CHECK(P.levels == 1 && P.n[0] == 1 && P.n[1] == 1 && P.nodes == 1 && P.offset[1] == 0);
    P = prio_levels(64);
    CHECK(P.levels == 1 && P.n[1] == 1);
    P = prio_levels(65);
    CHECK(P.levels == 2 && P.n[1] == 2 && P.n[2] == 1 && P.nodes == 3 && P.offset[2] == 2);
    P = prio_levels(490);
    CHECK(P.levels == 2 && P.n[1] == 8 && P.n[2] == 1);
    P = prio_levels(4690);
    CHECK(P.levels == 3 && P.n[1] == 74 && P.n[2] == 2 && P.n[3] == 1 && P.offset[3] == 76 && P.nodes == 77);
    P = prio_levels(PRIO_MAX_LEAVES);
    CHECK(P.levels == PRIO_MAX_LEVELS && P.n[1] == 1u << 24 && P.n[4] == 64 && P.n[5] == 1);
    for (uint64_t n = 1; n < 70000; n += (n < 5000 ? 1 : 997)) {
        P = prio_levels(n);
        uint32_t sum = 0;
        CHECK(P.levels >= 1 && P.levels <= PRIO_MAX_LEVELS && P.n[P.levels] == 1);
        for (int l = 1; l <= P.levels; l++) {
            CHECK(P.offset[l] == sum && (uint64_t)P.n[l] * PRIO_RADIX >= P.n[l - 1] && (uint64_t)(P.n[l] - 1) * PRIO_RADIX < P.n[l - 1]);
            sum += P.n[l];
        }
        CHECK(P.nodes == sum);
    }

    // ---- the clamp
    CHECK(prio_clamp(0.5f, 0.1f, 2.f) == 0.5f && prio_clamp(0.1f, 0.1f, 2.f) == 0.1f && prio_clamp(2.f, 0.1f, 2.f) == 2.f);
    CHECK(prio_clamp(0.f, 0.1f, 2.f) == 0.1f && prio_clamp(-0.f, 0.1f, 2.f) == 0.1f && prio_clamp(-3.f, 0.1f, 2.f) == 0.1f && prio_clamp(-inf, 0.1f, 2.f) == 0.1f);
    CHECK(prio_clamp(1e38f, 0.1f, 2.f) == 2.f && prio_clamp(inf, 0.1f, 2.f) == 2.f && prio_clamp(NAN, 0.1f, 2.f) == 2.f && prio_clamp(-NAN, 0.1f, 2.f) == 2.f);

    // ---- staleness against a brute-force history: holds[s] = the record slot s holds, -1 none
    for (int T = 1; T <= 6; T++) {
        std::vector<long> holds((size_t)T, -1);
        for (uint64_t written = 0; written <= (uint64_t)(3 * T + 2); written++) {
            if (written > 0) holds[(size_t)((written - 1) % (uint64_t)T)] = (long)(written - 1);
            for (int64_t slot = -2; slot <= T + 1; slot++)
                for (uint64_t sampled_at = 0; sampled_at <= written + 1; sampled_at++) {
                    const bool in = slot >= 0 && slot < T;
                    const bool want = in && holds[(size_t)(in ? slot : 0)] >= 0 && (uint64_t)holds[(size_t)(in ? slot : 0)] < sampled_at;
                    CHECK(prio_cell_live(written, T, slot, sampled_at) == want);
                }
        }
    }
    // far from zero: no wrap in the 64-bit arithmetic
    const uint64_t far = ((uint64_t)1 << 40) + 3;       // record far - 1 is the newest
    CHECK(prio_cell_live(far, 7, (int64_t)((far - 1) % 7), far) && !prio_cell_live(far, 7, (int64_t)((far - 1) % 7), far - 1));
    CHECK(prio_cell_live(far, 7, (int64_t)((far - 7) % 7), far - 6) && !prio_cell_live(far, 7, (int64_t)((far - 7) % 7), far - 7));
    CHECK(!prio_cell_live(far, 0x7fffffff, 0x7fffffff, far) && prio_cell_live(far, 0x7fffffff, 0x7ffffffe, far));
    CHECK(!prio_cell_live(5, 0x7fffffff, 5, 5) && prio_cell_live(5, 0x7fffffff, 4, 5));
    printf("ok %ld\n", checks);
    return 0;
}
