// Splitting a lagging wave of the persistent kernel (persist.h: "hand-over of hard envs inside a launch"): the two decisions that are pure
// arithmetic - which envs a wave gives away at a check point (split_decide and, with the lone rule, split_decide_lone, asked by the kernel) and whether a launch splits at all
// (split_plan, asked by plan_launch in host_step.h) - in plain C++ without a HIP call or header, so that a stand-alone program can exercise
// them (tests/split_logic_main.cpp, tests/split_lone_logic_main.cpp).
#pragma once

#ifdef __HIPCC__
#define SPLIT_HD __host__ __device__
#else
#define SPLIT_HD
#endif

enum {
    SPLIT_MAX_GROUPS = 4,              // lane groups (envs) of a wave: the split exists for the 16-lane instances only
    SPLIT_MAX_SUBSTEPS = 2048,         // a hand-over ticket packs env | substep << 20 into one non-negative int ...
    SPLIT_MAX_ENVS = 1 << 20,          // ... so fewer than 2048 substeps and at most 2^20 envs
    SPLIT_MAX_EXTRA = 4096,            // workgroups without a task of their own (tests): the env -> slot table has rows for that many
};

// The donor's decision at a check point: bit j of the result = lane group j's env leaves the wave.
//   trips[j]   Newton iterations of group j's env over the window (the `period` substeps before the check point)
//   alive      bit j = group j holds an env that is in range and not done
//   sub, left  substeps of the env-step behind the check point and still ahead of it
// A wave donates by this rule only if at least two of its live envs were hard over the window (trips_x4 / 4 iterations per substep or
// more, each) and only if min_left substeps or more remain.  It keeps its hardest env (ties: the lower lane group) and gives the other
// hard ones away.  (An easy neighbour leaves the Newton loop after its first iteration, but it is not free: its narrowphase items, its
// item-list rebuilds and the arms the hard env would skip wave-uniformly cost a hard env 2-5 % even where the neighbours are the three
// easiest envs of the batch, which touch nothing - tools/experiments/neighbour_cost.py, DESIGN.md.  That is what split_decide_lone below is for.)
SPLIT_HD static inline unsigned split_decide(const int *trips, unsigned alive, int groups, int sub, int left, int period, int trips_x4, int min_left) {
    if (period <= 0 || groups < 2 || groups > SPLIT_MAX_GROUPS || sub <= 0 || sub >= SPLIT_MAX_SUBSTEPS || left <= 0 || left < min_left) return 0u;
    unsigned hard = 0u;
    int nhard = 0, keep = -1;
    for (int j = 0; j < groups; j++) {
        if (!((alive >> j) & 1u) || 4 * trips[j] < trips_x4 * period) continue;
        hard |= 1u << j;
        nhard++;
        if (keep < 0 || trips[j] > trips[keep]) keep = j;
    }
    return nhard >= 2 ? hard & ~(1u << keep) : 0u;
}

// The donor's decision with the lone rule: split_decide's envs, and - lone_x4 > 0, the same guards - the hardest env the wave would keep
// (ties: the lower lane group) if it ran lone_x4 / 4 iterations per substep or more over the window while a live env that stays ran
// fewer: the hard env goes to a helper, where it has the wave to itself, and the wave goes on with the easier ones.  The step repeats
// with the envs that are left, so that no env at or above the lone threshold stays next to a live env below it; with lone_x4 >= trips_x4
// (every production setting) split_decide has left at most one such env and it applies once.  A wave whose live envs are all at or
// above the threshold keeps its hardest, as split_decide leaves it.  The result never covers every live env - the env below the
// threshold stays - so a wave with one live env never donates (every helper is one), an env is handed over at most once per launch, and
// every subset of the result (split_acquire grants credits in group order and stops at the first refusal) leaves a live env behind too.
SPLIT_HD static inline unsigned split_decide_lone(const int *trips, unsigned alive, int groups, int sub, int left, int period, int trips_x4, int min_left,
                                                  int lone_x4) {
    unsigned give = split_decide(trips, alive, groups, sub, left, period, trips_x4, min_left);
    if (lone_x4 <= 0 || period <= 0 || groups < 2 || groups > SPLIT_MAX_GROUPS || sub <= 0 || sub >= SPLIT_MAX_SUBSTEPS || left <= 0 || left < min_left) return give;
    for (int round = 0; round < SPLIT_MAX_GROUPS; round++) {
        int k = -1;
        bool below = false;                // a live env that stays ran fewer than lone_x4 / 4 iterations per substep
        for (int j = 0; j < groups; j++) {
            if (!((alive >> j) & 1u) || ((give >> j) & 1u)) continue;
            if (4 * trips[j] < lone_x4 * period) below = true;
            if (k < 0 || trips[j] > trips[k]) k = j;
        }
        if (k < 0 || !below || 4 * trips[k] < lone_x4 * period) break;
        give |= 1u << k;
    }
    return give;
}

// Whether one launch of the persistent kernel splits, and with which settings (DevState::split_*).  The split exists for launches
// without the work queue, with the env -> slot table (wave packing on), of the kernel instances the host's table allows (`const_instance`).  `extra`
// workgroups own no task and start as helpers (a test setting; production launches one workgroup per task): the tasks' workgroups and
// they must all fit the `slots` the GPU holds at once, else the launch runs without the split.
struct SplitPlan {
    int on;                            // 0: the launch behaves exactly as one without the feature
    int extra;                         // workgroups launched beyond the tasks'
    int period, trips_x4, min_left;
    int lone_x4 = 0;                   // the lone rule's threshold (split_decide_lone), set by plan_launch; 0: the rule is off
};
static inline SplitPlan split_plan(int enabled, int group, int const_instance, int schedule, int queued, int tasks, int n_envs, int slots,
                                   int n_substeps, int period, float trips, int min_left, int extra) {
    SplitPlan p = {0, 0, 0, 0, 0};
    if (!enabled || group != 16 || !const_instance || !schedule || queued) return p;
    if (period < 1 || period >= SPLIT_MAX_SUBSTEPS || !(trips >= 0.f) || trips > 1000.f || min_left < 1 || extra < 0 || extra > SPLIT_MAX_EXTRA) return p;
    if (tasks < 1 || n_envs > SPLIT_MAX_ENVS || n_substeps >= SPLIT_MAX_SUBSTEPS || n_substeps < period + min_left) return p;      // (no check point could ever donate)
    // every workgroup must be resident at once: a finished workgroup keeps its wave slot as a helper until the launch ends, so with more
    // workgroups than slots the launch would run in generations, each with its own tail, where a plain launch reuses a slot at once
    if (slots <= 0 || tasks + extra > slots) return p;
    p.on = 1;
    p.extra = extra;
    p.period = period;
    p.trips_x4 = (int)(4.f * trips + 0.5f);
    p.min_left = min_left;
    return p;
}
