// Stand-alone exerciser of hsr_env_amd/csrc/replay_logic.h - the host books of the hindsight replay: row layout, state machine, slot
// arithmetic, argument checks - for a build with -fsanitize=address,undefined (tests/test_replay_logic_sanitized.py).  No HIP, no GPU.
// It keeps a ring the plain way (a list of the env-steps still held) next to the books and compares them after every call; prints
// "ok <checks>" and returns 0, or says what differed and returns 1.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../hsr_env_amd/csrc/replay_logic.h"

static long checks = 0;
#define CHECK(x) do { checks++; if (!(x)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

static int run_protocol(int T, int steps, unsigned seed) {
    ReplayBooks k;
    replay_books_init(&k, T, 3);
    std::vector<int> slot_step(T, -1);         // which env-step every slot holds
    std::vector<char> touched(T + 2, 0);       // the ring as an array with a guard element on either side
    int pushed = 0;
    CHECK(replay_record_error(&k) != nullptr && replay_sample_error(&k, 4, 0.5f) != nullptr);
    replay_commit_done(&k);
    CHECK(k.state == REPLAY_READY && k.pushed == 0 && replay_sample_error(&k, 4, 0.5f) != nullptr);
    srand(seed);
    for (int s = 0; s < steps; s++) {
        if (rand() % 4 == 0) { CHECK(replay_commit_error(&k) == nullptr); replay_commit_done(&k); CHECK(k.pushed == (uint64_t)pushed); }   // a commit without a record replaces the head only
        CHECK(replay_record_error(&k) == nullptr);
        const int head = replay_head_slot(&k);
        CHECK(head >= 0 && head < T && head == pushed % T);
        touched[1 + head] = 1; slot_step[head] = s;
        replay_record_done(&k);
        CHECK(replay_record_error(&k) != nullptr && replay_sample_error(&k, 4, 0.5f) != nullptr);
        replay_commit_done(&k);
        pushed++;
        const int count = replay_count(&k);
        CHECK(k.pushed == (uint64_t)pushed && count == (pushed < T ? pushed : T) && replay_sample_error(&k, 1, 0.f) == nullptr);
        for (int age = 0; age < count; age++) {
            const int sl = replay_slot(&k, age);
            CHECK(sl >= 0 && sl < T && touched[1 + sl] && slot_step[sl] == pushed - count + age);
        }
        CHECK(replay_slot(&k, 0) == replay_first_slot(&k) && replay_slot(&k, count - 1) == (pushed - 1) % T);
    }
    CHECK(!touched[0] && !touched[T + 1]);
    replay_clear_done(&k);
    CHECK(k.state == REPLAY_EMPTY && k.pushed == 0 && replay_count(&k) == 0 && replay_head_slot(&k) == 0 && replay_record_error(&k) != nullptr);
    return 0;
}

int main() {
    // row layout: the cases of the tests and the extremes the checks admit
    const int dims[][4] = {{17, 2, 46, 48}, {27, 7, 71, 72}, {25, 7, 67, 68}, {1, 1, 13, 16}, {1 << 20, 32, 2 * (1 << 20) + 42, 2 * (1 << 20) + 44}};
    for (const auto &d : dims) {
        const ReplayLayout L = replay_layout(d[0], d[1]);
        CHECK(L.words == d[2] && L.stride == d[3] && L.stride % 4 == 0 && L.stride - L.words < 4);
        CHECK(L.o_act == d[0] && L.o_next == d[0] + d[1] && L.o_achieved == 2 * d[0] + d[1] && L.o_ep_step == L.words - 1);
        CHECK(L.o_ep_step - L.o_achieved + 1 == REPLAY_TAIL_WORDS);
    }
    // spec checks
    const int mocap[4] = {0, 1, 0, 0};
    CHECK(replay_spec_error(7, 17, 2, 0.05f, 4, mocap, 0) == nullptr);
    CHECK(replay_spec_error(0, 17, 2, 0.05f, 4, mocap, 0) && replay_spec_error(-1, 17, 2, 0.05f, 4, mocap, 0));
    CHECK(replay_spec_error(7, 0, 2, 0.05f, 4, mocap, 0) && replay_spec_error(7, (1 << 20) + 1, 2, 0.05f, 4, mocap, 0));
    CHECK(replay_spec_error(7, 17, 1, 0.05f, 4, mocap, 0) && replay_spec_error(7, 17, 4, 0.05f, 4, mocap, 0) && replay_spec_error(7, 17, -1, 0.05f, 4, mocap, 0));
    CHECK(replay_spec_error(7, 17, 2, 0.f, 4, mocap, 0) && replay_spec_error(7, 17, 2, -1.f, 4, mocap, 0) && replay_spec_error(7, 17, 2, NAN, 4, mocap, 0) &&
          replay_spec_error(7, 17, 2, INFINITY, 4, mocap, 0));
    CHECK(replay_spec_error(7, 17, 2, 0.05f, 4, mocap, 1));
    CHECK(replay_ring_bytes(7, 70, 48) == 7ull * 70 * 48 * 4 && replay_ring_bytes(0x7fffffff, 0x7fffffff, 2 * (1 << 20) + 44) == 0 &&
          replay_ring_bytes(1 << 20, 1 << 12, 64) == (1ull << 40) && replay_ring_bytes((1 << 20) + 1, 1 << 12, 64) == 0);
    // sample checks
    ReplayBooks k;
    replay_books_init(&k, 3, 2);
    replay_commit_done(&k); replay_record_done(&k); replay_commit_done(&k);
    CHECK(replay_sample_error(&k, 1, 0.f) == nullptr && replay_sample_error(&k, 1, 1.f) == nullptr && replay_sample_error(&k, 0x7fffffff, 0.8f) == nullptr);
    CHECK(replay_sample_error(&k, 0, 0.5f) && replay_sample_error(&k, -3, 0.5f) && replay_sample_error(&k, 1, -0.01f) && replay_sample_error(&k, 1, 1.01f) &&
          replay_sample_error(&k, 1, NAN) && replay_sample_error(&k, 1, INFINITY));
    // the counter is 64 bits wide: the ring goes on past 2^32 steps
    k.pushed = 0xffffffffull;
    const int before = replay_head_slot(&k);
    replay_record_done(&k); replay_commit_done(&k);
    CHECK(k.pushed == 0x100000000ull && replay_head_slot(&k) == (before + 1) % 3 && replay_count(&k) == 3 && replay_slot(&k, 2) == before);
    // protocol against the plain ring: T = 1, a power of two, not one, and more steps than slots
    for (int T : {1, 2, 7, 64}) if (run_protocol(T, 3 * T + 5, 17u + T)) return 1;
    printf("ok %ld\n", checks);
    return 0;
}
