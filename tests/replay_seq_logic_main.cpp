// Stand-alone exerciser of the window sampler's host logic in hsr_env_amd/csrc/replay_logic.h - replay_sample_seq_error and replay_nstep -
// for a build with -fsanitize=address,undefined (tests/test_replay_seq_logic_sanitized.py).  No HIP, no GPU.  The windows are hand-made
// arrays with a guard element on either side: replay_nstep may call step_at only for k < length, in order, and not past the first done
// step.  Prints "ok <checks>" and returns 0, or says what differed and returns 1.
#include <math.h>
#include <stdio.h>

#include <vector>

#include "../hsr_env_amd/csrc/replay_logic.h"

static long checks = 0;
#define CHECK(x) do { checks++; if (!(x)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

struct Window {
    std::vector<float> reward;
    std::vector<uint32_t> done;
    std::vector<int> asked;        // the k of every step_at call, in order
    Window(std::initializer_list<float> r, std::initializer_list<uint32_t> d) : reward(r), done(d) {}
    ReplayNstep run(int length, float gamma) {
        asked.clear();
        return replay_nstep(length, gamma, [this](int k) {
            asked.push_back(k);
            return ReplayStep{reward.at((size_t)k), done.at((size_t)k)};       // .at(): a step outside the window throws
        });
    }
    bool asked_in_order(int m) const {
        if ((int)asked.size() != m) return false;
        for (int k = 0; k < m; k++) if (asked[(size_t)k] != k) return false;
        return true;
    }
};

int main() {
    // ---- refusals: a ring of 5 steps holding 2
    ReplayBooks k;
    replay_books_init(&k, 5, 3);
    CHECK(replay_sample_seq_error(&k, 4, 2, 0.5f, 0.9f, true) != nullptr);                      // empty
    replay_commit_done(&k);
    CHECK(replay_sample_seq_error(&k, 4, 2, 0.5f, 0.9f, true) != nullptr);                      // committed, still empty
    replay_record_done(&k); replay_commit_done(&k); replay_record_done(&k);
    CHECK(replay_sample_seq_error(&k, 4, 2, 0.5f, 0.9f, true) != nullptr);                      // a pending record
    replay_commit_done(&k);
    CHECK(replay_count(&k) == 2);
    CHECK(replay_sample_seq_error(&k, 4, 2, 0.5f, 0.9f, true) == nullptr);
    CHECK(replay_sample_seq_error(&k, 1, 1, 0.f, 0.f, true) == nullptr && replay_sample_seq_error(&k, 1, 5, 1.f, 1.f, true) == nullptr);   // seq_len up to T, not count
    CHECK(replay_sample_seq_error(&k, 0, 2, 0.5f, 0.9f, true) && replay_sample_seq_error(&k, -1, 2, 0.5f, 0.9f, true));
    CHECK(replay_sample_seq_error(&k, 4, 2, -0.01f, 0.9f, true) && replay_sample_seq_error(&k, 4, 2, 1.01f, 0.9f, true) && replay_sample_seq_error(&k, 4, 2, NAN, 0.9f, true));
    CHECK(replay_sample_seq_error(&k, 4, 2, 0.5f, 0.9f, false));                                // out == NULL
    CHECK(replay_sample_seq_error(&k, 4, 0, 0.5f, 0.9f, true) && replay_sample_seq_error(&k, 4, -3, 0.5f, 0.9f, true) && replay_sample_seq_error(&k, 4, 6, 0.5f, 0.9f, true));
    CHECK(replay_sample_seq_error(&k, 4, 2, 0.5f, NAN, true) && replay_sample_seq_error(&k, 4, 2, 0.5f, INFINITY, true) && replay_sample_seq_error(&k, 4, 2, 0.5f, -0.1f, true) &&
          replay_sample_seq_error(&k, 4, 2, 0.5f, 1.5f, true));
    // batch x seq_len: 2^31 - 1 passes, 2^31 and beyond do not, and the product does not wrap
    ReplayBooks big;
    replay_books_init(&big, 0x7fffffff, 1);
    replay_commit_done(&big); replay_record_done(&big); replay_commit_done(&big);
    CHECK(replay_sample_seq_error(&big, 0x7fffffff, 1, 0.5f, 0.9f, true) == nullptr && replay_sample_seq_error(&big, 1, 0x7fffffff, 0.5f, 0.9f, true) == nullptr);
    CHECK(replay_sample_seq_error(&big, 1 << 30, 2, 0.5f, 0.9f, true) && replay_sample_seq_error(&big, 0x7fffffff, 0x7fffffff, 0.5f, 0.9f, true) &&
          replay_sample_seq_error(&big, 1 << 16, 1 << 16, 0.5f, 0.9f, true));
    CHECK(replay_sample_seq_error(&big, (1 << 15) - 1, 1 << 16, 0.5f, 0.9f, true) == nullptr);

    // ---- the n-step chain on hand-made windows (gamma 0.5: every value exact)
    Window first({1.f, 1.f, 1.f}, {1u, 0u, 0u}), middle({0.f, 1.f, 1.f}, {0u, 1u, 0u}), never({1.f, 1.f, 1.f}, {0u, 0u, 0u});
    ReplayNstep n = first.run(3, 0.5f);
    CHECK(n.m == 1 && n.ret == 1.f && n.discount == 0.5f && n.done == 1u && first.asked_in_order(1));
    n = middle.run(3, 0.5f);
    CHECK(n.m == 2 && n.ret == 0.5f && n.discount == 0.25f && n.done == 1u && middle.asked_in_order(2));
    n = never.run(3, 0.5f);
    CHECK(n.m == 3 && n.ret == 1.75f && n.discount == 0.125f && n.done == 0u && never.asked_in_order(3));
    n = middle.run(1, 0.5f);                                   // the window ends before the done step
    CHECK(n.m == 1 && n.ret == 0.f && n.discount == 0.5f && n.done == 0u && middle.asked_in_order(1));
    Window one({3.f}, {0u}), one_done({1.f}, {7u});           // length 1; a done word that is not 1 is kept as it is
    n = one.run(1, 0.9f);
    CHECK(n.m == 1 && n.ret == 3.f && n.discount == 0.9f && n.done == 0u && one.asked_in_order(1));
    n = one_done.run(1, 0.9f);
    CHECK(n.m == 1 && n.ret == 1.f && n.discount == 0.9f && n.done == 7u);
    n = never.run(3, 0.f);
    CHECK(n.m == 3 && n.ret == 1.f && n.discount == 0.f && n.done == 0u);
    n = never.run(3, 1.f);
    CHECK(n.m == 3 && n.ret == 3.f && n.discount == 1.f && n.done == 0u);
    // every product and every sum is rounded on its own: 0.9 by hand, in the stated order
    Window w({0.3f, 0.7f, 0.2f, 0.6f}, {0u, 0u, 0u, 0u});
    n = w.run(4, 0.9f);
    volatile float acc = 0.f, g = 1.f, term;
    for (int c = 0; c < 4; c++) { term = g * w.reward[(size_t)c]; acc = acc + term; g = g * 0.9f; }
    CHECK(n.m == 4 && n.ret == acc && n.discount == g && w.asked_in_order(4));
    printf("ok %ld\n", checks);
    return 0;
}
