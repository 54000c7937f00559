// Stand-alone exerciser of hsr_env_amd/csrc/split_logic.h and launch_plan.h - the pure decisions of the hand-over of hard envs inside a launch of the
// persistent kernel: which envs a wave gives away at a check point (split_decide) and whether a launch splits at all (split_plan, and plan_launch which asks it)
// (tests/test_split_logic.py).  No HIP, no GPU.  split_decide is checked exhaustively over small inputs - 0-4 live envs in every pattern,
// window trips around the threshold, substeps left around min_left - against the rules written out here; prints "ok <checks>" and returns 0,
// or says what differed and returns 1.
#include <stdio.h>
#include <string.h>

#include <initializer_list>

#include "../hsr_env_amd/csrc/launch_plan.h"

static long checks = 0;
#define CHECK(x) do { checks++; if (!(x)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

static int popcount(unsigned v) { int n = 0; for (; v; v &= v - 1) n++; return n; }

static int decide_rules(int groups, int period, int trips_x4, int min_left) {
    // the per-env window trips that matter: around the threshold trips_x4 * period / 4 (below, at, above, well above) and zero
    const int thr = (trips_x4 * period + 3) / 4;           // the smallest count that is hard
    const int vals[5] = {0, thr - 1 < 0 ? 0 : thr - 1, thr, thr + 1, thr + 7};
    const int n_sub = 2 * (period + min_left) + 3;
    int t[SPLIT_MAX_GROUPS];
    for (unsigned alive = 0; alive < (1u << SPLIT_MAX_GROUPS); alive++)       // (bits beyond `groups` are set too: an out-of-range group never leaves)
        for (int code = 0; code < 5 * 5 * 5 * 5; code++) {
            for (int j = 0, k = code; j < SPLIT_MAX_GROUPS; j++, k /= 5) t[j] = vals[k % 5];
            for (int left = min_left - 2; left <= min_left + 2; left++) {
                const int sub = n_sub - left;
                const unsigned d = split_decide(t, alive, groups, sub, left, period, trips_x4, min_left);
                unsigned hard = 0;
                for (int j = 0; j < groups; j++) if (((alive >> j) & 1u) && 4 * t[j] >= trips_x4 * period) hard |= 1u << j;
                CHECK((d & ~hard) == 0);                    // never an env that is done, out of range or easy
                CHECK((d >> groups) == 0);
                if (popcount(hard) < 2 || left < min_left || left <= 0) { CHECK(d == 0); continue; }      // never with fewer than two hard envs, never too late
                CHECK(popcount(d) == popcount(hard) - 1);   // all the hard ones but one ...
                const unsigned kept = hard & ~d;
                int keep = 0;
                while (!((kept >> keep) & 1u)) keep++;
                for (int j = 0; j < groups; j++) {          // ... which is the hardest; ties go to the lower lane group
                    if (!((hard >> j) & 1u)) continue;
                    CHECK(t[j] <= t[keep]);
                    if (t[j] == t[keep]) CHECK(keep <= j);
                }
            }
        }
    return 0;
}

static int decide_edges() {
    int t[4] = {100, 100, 100, 100};
    CHECK(split_decide(t, 0xfu, 4, 16, 100, 16, 14, 40) == 0xeu);
    CHECK(split_decide(t, 0xfu, 4, 0, 100, 16, 14, 40) == 0u);                      // no check point at substep 0 (a ticket's substep is positive)
    CHECK(split_decide(t, 0xfu, 4, SPLIT_MAX_SUBSTEPS, 100, 16, 14, 40) == 0u);     // the substep must fit the ticket
    CHECK(split_decide(t, 0xfu, 4, SPLIT_MAX_SUBSTEPS - 1, 100, 16, 14, 40) == 0xeu);
    CHECK(split_decide(t, 0xfu, 4, 16, 100, 0, 14, 40) == 0u);                      // period 0: off
    CHECK(split_decide(t, 0xfu, 1, 16, 100, 16, 14, 40) == 0u);                     // a wave of one env has nothing to give
    CHECK(split_decide(t, 0xfu, 5, 16, 100, 16, 14, 40) == 0u);
    CHECK(split_decide(t, 0xfu, 2, 16, 100, 16, 14, 40) == 0x2u);
    CHECK(split_decide(t, 0xfu, 4, 16, 0, 16, 0, 0) == 0u);                         // nothing left to run
    int z[4] = {0, 0, 0, 0};
    CHECK(split_decide(z, 0xfu, 4, 8, 52, 8, 0, 8) == 0xeu);                        // threshold 0 (tests): every live env counts as hard
    CHECK(split_decide(z, 0x5u, 4, 8, 52, 8, 0, 8) == 0x4u);
    CHECK(split_decide(z, 0x4u, 4, 8, 52, 8, 0, 8) == 0u);
    return 0;
}

static int plan_rules() {
    // enabled, group, const_instance, schedule, queued, tasks, n_envs, slots, n_substeps, period, trips, min_left, extra
    SplitPlan p = split_plan(1, 16, 1, 1, 0, 2048, 8192, 2048, 300, 16, 3.5f, 40, 0);
    CHECK(p.on == 1 && p.extra == 0 && p.period == 16 && p.trips_x4 == 14 && p.min_left == 40);
    CHECK(split_plan(0, 16, 1, 1, 0, 2048, 8192, 2048, 300, 16, 3.5f, 40, 0).on == 0);         // switched off
    CHECK(split_plan(1, 32, 1, 1, 0, 2048, 8192, 2048, 300, 16, 3.5f, 40, 0).on == 0);         // the 32-lane models
    CHECK(split_plan(1, 16, 0, 1, 0, 2048, 8192, 2048, 300, 16, 3.5f, 40, 0).on == 0);         // a generic kernel instance
    CHECK(split_plan(1, 16, 1, 0, 0, 2048, 8192, 2048, 300, 16, 3.5f, 40, 0).on == 0);         // no env -> slot table
    CHECK(split_plan(1, 16, 1, 1, 1, 2048, 8192, 2048, 300, 16, 3.5f, 40, 0).on == 0);         // a queued launch
    CHECK(split_plan(1, 16, 1, 1, 0, 2048, 8192, 2048, 2048, 16, 3.5f, 40, 0).on == 0);        // the ticket's substep field
    CHECK(split_plan(1, 16, 1, 1, 0, 2048, 8192, 2048, 2047, 16, 3.5f, 40, 0).on == 1);
    CHECK(split_plan(1, 16, 1, 1, 0, 1 << 18, (1 << 20) + 1, 1 << 18, 300, 16, 3.5f, 40, 0).on == 0);  // ... and its env field
    CHECK(split_plan(1, 16, 1, 1, 0, 1 << 18, 1 << 20, 1 << 18, 300, 16, 3.5f, 40, 0).on == 1);
    CHECK(split_plan(1, 16, 1, 1, 0, 2049, 8196, 2048, 300, 16, 3.5f, 40, 0).on == 0);         // more tasks than slots without the queue: helpers would hold the slots the late workgroups need
    CHECK(split_plan(1, 16, 1, 1, 0, 2048, 8192, 0, 300, 16, 3.5f, 40, 0).on == 0);            // unknown residency
    CHECK(split_plan(1, 16, 1, 1, 0, 2048, 8192, 2048, 55, 16, 3.5f, 40, 0).on == 0);          // too short for any check point to donate
    CHECK(split_plan(1, 16, 1, 1, 0, 2048, 8192, 2048, 56, 16, 3.5f, 40, 0).on == 1);
    CHECK(split_plan(1, 16, 1, 1, 0, 2048, 8192, 2048, 300, 0, 3.5f, 40, 0).on == 0);
    CHECK(split_plan(1, 16, 1, 1, 0, 2048, 8192, 2048, 300, 16, -1.f, 40, 0).on == 0);
    CHECK(split_plan(1, 16, 1, 1, 0, 2048, 8192, 2048, 300, 16, 3.5f, 0, 0).on == 0);
    p = split_plan(1, 16, 1, 1, 0, 16, 64, 2048, 60, 8, 0.f, 8, 16);                           // the GPU test's shape: forced, 16 extra helpers
    CHECK(p.on == 1 && p.extra == 16 && p.period == 8 && p.trips_x4 == 0 && p.min_left == 8);
    CHECK(split_plan(1, 16, 1, 1, 0, 2040, 8160, 2048, 300, 16, 3.5f, 40, 8).on == 1);         // extra helpers fit exactly
    CHECK(split_plan(1, 16, 1, 1, 0, 2041, 8164, 2048, 300, 16, 3.5f, 40, 8).on == 0);         // ... or the launch does not split at all
    CHECK(split_plan(1, 16, 1, 1, 0, 16, 64, 0, 60, 8, 0.f, 8, 16).on == 0);                   // unknown residency: no extra workgroups
    CHECK(split_plan(1, 16, 1, 1, 0, 16, 64, 2048, 60, 8, 0.f, 8, SPLIT_MAX_EXTRA + 1).on == 0);
    CHECK(split_plan(1, 16, 1, 1, 0, 16, 64, 2048, 60, 8, 0.f, 8, -1).on == 0);
    return 0;
}

// plan_launch's own lines: the queue's decision goes into the split's, and the grid of a splitting launch is one workgroup per task plus the extra ones
static int launch_rules() {
    const SplitSettings on{true, true, 8, 2.5f, 40, 0}, off{false, true, 8, 2.5f, 40, 0}, generic{true, false, 8, 2.5f, 40, 0}, extra{true, true, 8, 0.f, 8, 16};
    // N, group, slots, n_substeps, queue, queue_chunk, queue_chunk_set, solo_servers, solo_trips, has_sv, schedule, split settings
    PersistLaunch p = plan_launch(8192, 16, 2048, 300, -1, 20, false, 0, 3.5f, true, true, on);
    CHECK(p.tasks == 2048 && p.grid == 2048 && p.rounds == 0 && p.solo_servers == 0);
    CHECK(p.split.on == 1 && p.split.extra == 0 && p.split.period == 8 && p.split.trips_x4 == 10 && p.split.min_left == 40);
    p = plan_launch(8192, 16, 2048, 300, -1, 20, false, 0, 3.5f, true, true, off);
    CHECK(p.grid == 2048 && p.rounds == 0 && p.split.on == 0);
    p = plan_launch(8192, 16, 2048, 300, -1, 20, false, 0, 3.5f, true, true, generic);
    CHECK(p.grid == 2048 && p.rounds == 0 && p.split.on == 0);
    p = plan_launch(8192, 16, 2048, 300, -1, 20, false, 0, 3.5f, true, false, on);          // no wave packing
    CHECK(p.grid == 2048 && p.rounds == 0 && p.split.on == 0);
    p = plan_launch(8192, 16, 2048, 300, 1, 20, false, 0, 3.5f, true, true, on);             // queue forced on: no split, the queue's grid
    CHECK(p.rounds == 15 && p.grid == 2048 && p.split.on == 0);
    p = plan_launch(16384, 16, 2048, 300, -1, 20, false, 0, 3.5f, true, true, on);          // more tasks than slots: the queue, no split
    CHECK(p.tasks == 4096 && p.rounds == 15 && p.grid == 2048 && p.split.on == 0);
    p = plan_launch(16384, 16, 2048, 300, 0, 20, false, 0, 3.5f, true, true, on);           // ... queue forced off: one workgroup per task, no split (residency)
    CHECK(p.rounds == 0 && p.grid == 4096 && p.split.on == 0);
    p = plan_launch(4096, 16, 2048, 300, -1, 20, false, 64, 3.5f, true, true, on);          // solo servers bring the queue: their grid, no split
    CHECK(p.rounds == 15 && p.solo_servers == 64 && p.grid == 1024 + 64 && p.split.on == 0);
    p = plan_launch(4096, 16, 2048, 300, -1, 20, false, 64, 3.5f, false, true, on);         // ... an instance without the server path: no queue, the split
    CHECK(p.rounds == 0 && p.solo_servers == 0 && p.grid == 1024 && p.split.on == 1);
    p = plan_launch(8192, 16, 2048, 30, -1, 20, false, 0, 3.5f, true, true, on);             // too short to donate
    CHECK(p.grid == 2048 && p.split.on == 0);
    p = plan_launch(64, 16, 2048, 60, -1, 20, false, 0, 3.5f, true, true, extra);           // the GPU test's shape
    CHECK(p.tasks == 16 && p.grid == 32 && p.rounds == 0 && p.split.on == 1 && p.split.extra == 16 && p.split.trips_x4 == 0);
    p = plan_launch(67, 16, 2048, 60, -1, 20, false, 0, 3.5f, true, true, extra);
    CHECK(p.tasks == 17 && p.grid == 33 && p.split.on == 1);
    p = plan_launch(64, 16, 24, 60, -1, 20, false, 0, 3.5f, true, true, extra);             // the extra workgroups do not fit: a plain launch
    CHECK(p.grid == 16 && p.rounds == 0 && p.split.on == 0);
    p = plan_launch(64, 32, 2048, 60, -1, 20, false, 0, 3.5f, true, true, extra);           // 32 lanes per env
    CHECK(p.tasks == 32 && p.grid == 32 && p.split.on == 0);
    return 0;
}

int main() {
    for (int groups = 2; groups <= SPLIT_MAX_GROUPS; groups++)
        for (int period : {1, 8, 16})
            for (int trips_x4 : {0, 1, 14, 17})
                for (int min_left : {0, 1, 8, 40})
                    if (decide_rules(groups, period, trips_x4, min_left)) return 1;
    if (decide_edges() || plan_rules() || launch_rules()) return 1;
    printf("ok %ld\n", checks);
    return 0;
}
