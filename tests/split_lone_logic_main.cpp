// Stand-alone exerciser of the lone rule of hsr_env_amd/csrc/split_logic.h (split_decide_lone: a wave's one hard env leaves its easier
// neighbours) and of the way launch_plan.h carries its setting (tests/test_split_lone_logic.py).  No HIP, no GPU.  The properties are
// checked exhaustively over 2-4 lane groups, every alive mask, window trips of {0, 1, 2, 3, 5} iterations per substep for periods of 4 and
// 8, both thresholds in {0, 1.5, 2.5, 4.5} iterations per substep and substeps left on both sides of min_left; prints "ok <checks>" and
// returns 0, or says what differed and returns 1.
#include <stdio.h>

#include <initializer_list>

#include "../hsr_env_amd/csrc/launch_plan.h"

static long checks = 0;
#define CHECK(x) do { checks++; if (!(x)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

static bool guards_hold(int groups, int sub, int left, int period, int min_left) {
    return period > 0 && groups >= 2 && groups <= SPLIT_MAX_GROUPS && sub > 0 && sub < SPLIT_MAX_SUBSTEPS && left > 0 && left >= min_left;
}

static int lone_rules(int groups, int period, int trips_x4, int lone_x4, int min_left) {
    const int vals[5] = {0, period, 2 * period, 3 * period, 5 * period};
    const int n_sub = 2 * (period + min_left) + 3;
    int t[SPLIT_MAX_GROUPS];
    for (unsigned alive = 0; alive < (1u << SPLIT_MAX_GROUPS); alive++)       // (bits beyond `groups` are set too: an out-of-range group never leaves)
        for (int code = 0; code < 5 * 5 * 5 * 5; code++) {
            for (int j = 0, k = code; j < SPLIT_MAX_GROUPS; j++, k /= 5) t[j] = vals[k % 5];
            for (int left = min_left - 2; left <= min_left + 2; left++) {
                const int sub = n_sub - left;
                const unsigned base = split_decide(t, alive, groups, sub, left, period, trips_x4, min_left);
                const unsigned d = split_decide_lone(t, alive, groups, sub, left, period, trips_x4, min_left, lone_x4);
                const unsigned live = alive & ((1u << groups) - 1u);
                // (i) the rule off: split_decide, for every input
                CHECK(split_decide_lone(t, alive, groups, sub, left, period, trips_x4, min_left, 0) == base);
                CHECK(split_decide_lone(t, alive, groups, sub, left, period, trips_x4, min_left, -1) == base);
                // (ii) never a dead or out-of-range group; nothing where split_decide's guards say nothing
                CHECK((d & ~live) == 0);
                if (!guards_hold(groups, sub, left, period, min_left)) { CHECK(d == 0); continue; }
                // split_decide's envs leave as before
                CHECK((d & base) == base);
                // (iii) never every live env (so never the only one)
                CHECK(live == 0 || (d & live) != live);
                if (lone_x4 <= 0) { CHECK(d == base); continue; }
                // (iv) before credits: no env at or above the lone threshold stays next to a live env below it
                bool stays_hard = false, stays_easy = false;
                for (int j = 0; j < groups; j++) {
                    if (!((live >> j) & 1u) || ((d >> j) & 1u)) continue;
                    if (4 * t[j] >= lone_x4 * period) stays_hard = true; else stays_easy = true;
                }
                CHECK(!(stays_hard && stays_easy));
                // what the rule adds is at or above its threshold, and only where an easier live env stays
                for (int j = 0; j < groups; j++)
                    if (((d & ~base) >> j) & 1u) { CHECK(4 * t[j] >= lone_x4 * period); CHECK(stays_easy); }
                // a wave whose remaining live envs are all at or above the threshold, or all below, adds nothing
                bool any_easy = false, any_hard = false;
                for (int j = 0; j < groups; j++) {
                    if (!((live >> j) & 1u) || ((base >> j) & 1u)) continue;
                    if (4 * t[j] >= lone_x4 * period) any_hard = true; else any_easy = true;
                }
                if (!(any_easy && any_hard)) CHECK(d == base);
                // the first env the rule adds is the hardest that split_decide left; ties go to the lower group
                if (d != base) {
                    int k = -1;
                    for (int j = 0; j < groups; j++)
                        if (((live >> j) & 1u) && !((base >> j) & 1u) && (k < 0 || t[j] > t[k])) k = j;
                    CHECK(k >= 0 && ((d >> k) & 1u));
                }
                // (v) every subset of the result leaves a live env behind as well: split_acquire may grant only a part
                for (unsigned part = d; ; part = (part - 1) & d) {
                    CHECK(live == 0 || (part & live) != live);
                    if (part == 0) break;
                }
            }
        }
    return 0;
}

static int lone_edges() {
    int t[4] = {40, 0, 8, 0};      // period 8: 5, 0, 1, 0 iterations per substep
    CHECK(split_decide_lone(t, 0xfu, 4, 8, 52, 8, 4000, 8, 10) == 0x1u);            // the one hard env leaves its three easy neighbours
    CHECK(split_decide_lone(t, 0x1u, 4, 8, 52, 8, 4000, 8, 10) == 0u);              // alone in its wave (a helper): nothing to leave
    CHECK(split_decide_lone(t, 0x5u, 4, 8, 52, 8, 4000, 8, 10) == 0x1u);
    CHECK(split_decide_lone(t, 0x5u, 4, 8, 52, 8, 4000, 8, 4) == 0u);               // both at or above the threshold: the wave keeps them, as split_decide does
    CHECK(split_decide_lone(t, 0xfu, 4, 8, 7, 8, 4000, 8, 10) == 0u);               // too late
    CHECK(split_decide_lone(t, 0xfu, 4, 0, 52, 8, 4000, 8, 10) == 0u);              // no check point at substep 0
    CHECK(split_decide_lone(t, 0xfu, 1, 8, 52, 8, 4000, 8, 10) == 0u);
    int u[4] = {40, 24, 8, 40};    // 5, 3, 1, 5
    CHECK(split_decide(u, 0xfu, 4, 8, 52, 8, 10, 8) == 0xau);                       // two-hard rule at 2.5: keeps group 0 (tie: the lower), gives 1 and 3
    CHECK(split_decide_lone(u, 0xfu, 4, 8, 52, 8, 10, 8, 14) == 0xbu);              // ... and the kept one leaves the easy env in group 2
    CHECK(split_decide_lone(u, 0xbu, 4, 8, 52, 8, 10, 8, 14) == 0xau);              // without that env: as split_decide
    CHECK(split_decide_lone(u, 0xfu, 4, 8, 52, 8, 4000, 8, 10) == 0xbu);            // lone threshold below the two-hard one: every env at or above it leaves the easy one
    return 0;
}

// the settings travel through plan_launch: SplitPlan::lone_x4 is set only where the launch splits and the rule is on; the initialisers the
// other exerciser uses still name every member they used to
static int plan_rules() {
    const SplitSettings old_form{true, true, 8, 2.5f, 40, 0};
    CHECK(!old_form.lone);
    SplitPlan z = {0, 0, 0, 0, 0};
    CHECK(z.lone_x4 == 0);
    CHECK(split_plan(1, 16, 1, 1, 0, 2048, 8192, 2048, 300, 8, 2.5f, 40, 0).lone_x4 == 0);
    SplitSettings sp{true, true, 8, 2.5f, 40, 0};
    // N, group, slots, n_substeps, queue, queue_chunk, queue_chunk_set, solo_servers, solo_trips, has_sv, schedule, split settings
    PersistLaunch p = plan_launch(8192, 16, 2048, 300, -1, 20, false, 0, 3.5f, true, true, sp);
    CHECK(p.split.on == 1 && p.split.lone_x4 == 0);
    sp.lone = true;
    sp.lone_trips = 3.5f;
    p = plan_launch(8192, 16, 2048, 300, -1, 20, false, 0, 3.5f, true, true, sp);
    CHECK(p.split.on == 1 && p.split.lone_x4 == 14 && p.split.trips_x4 == 10 && p.grid == 2048);
    sp.lone_trips = 2.5f;
    p = plan_launch(8192, 16, 2048, 300, -1, 20, false, 0, 3.5f, true, true, sp);
    CHECK(p.split.lone_x4 == 10);
    sp.lone_trips = 0.f;                                                            // no threshold: off
    CHECK(plan_launch(8192, 16, 2048, 300, -1, 20, false, 0, 3.5f, true, true, sp).split.lone_x4 == 0);
    sp.lone_trips = 3.5f;
    CHECK(plan_launch(16384, 16, 2048, 300, -1, 20, false, 0, 3.5f, true, true, sp).split.lone_x4 == 0);      // a queued launch does not split
    sp.on = false;
    CHECK(plan_launch(8192, 16, 2048, 300, -1, 20, false, 0, 3.5f, true, true, sp).split.lone_x4 == 0);       // the split itself off
    return 0;
}

int main() {
    for (int groups = 2; groups <= SPLIT_MAX_GROUPS; groups++)
        for (int period : {4, 8})
            for (int trips_x4 : {0, 6, 10, 18})
                for (int lone_x4 : {0, 6, 10, 18})
                    for (int min_left : {1, 8})
                        if (lone_rules(groups, period, trips_x4, lone_x4, min_left)) return 1;
    if (lone_edges() || plan_rules()) return 1;
    printf("ok %ld\n", checks);
    return 0;
}
