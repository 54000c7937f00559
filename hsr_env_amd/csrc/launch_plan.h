// The launch plan of the persistent kernel: how one env-step runs on it - work queue or not, solo servers, the hand-over of hard envs inside
// the launch - from the batch's settings alone.  Plain C++ without a HIP call or header (split_logic.h likewise), so that a stand-alone program
// can exercise it (tests/split_logic_main.cpp); host_step.h asks plan_launch and launches what it says.
#pragma once
#include "split_logic.h"

enum { QUEUE_ROUNDS = 64 };        // rounds the work queue of the persistent kernel has room for (DevState::q_head / q_wpos / q_items)

// How one env-step runs on the persistent kernel.  More tasks than the GPU holds workgroups at once: persistent workgroups + the work
// queue (persist.h), else one task per workgroup.  Pure arithmetic on the batch's settings: no HIP call, no state.
struct PersistLaunch {
    int tasks, grid;               // tasks = the envs of one workgroup each; workgroups launched
    int chunk, rounds;             // substeps per round of the work queue and its rounds; rounds == 0: no queue
    int solo_servers, solo_trips_x4, solo_min_left;      // DevState fields of a launch with solo servers; solo_servers == 0: none
    SplitPlan split;               // hard envs handed over inside a launch without the queue (split_logic.h); split.on == 0: none
};
// the split settings of a batch, as plan_launch takes them
struct SplitSettings {
    bool on, const_instance; int period; float trips; int min_left, extra;
    bool lone = false; float lone_trips = 4.5f;        // the lone rule (split_decide_lone) and its threshold in Newton iterations per substep
};
static inline PersistLaunch plan_launch(int N, int group, int slots, int n_substeps, int queue, int queue_chunk, bool queue_chunk_set,
                                 int solo_servers, float solo_trips, bool has_sv, bool schedule, const SplitSettings &sp) {
    PersistLaunch p{};
    const int epb = 64 / group, T = (N + epb - 1) / epb;
    int chunk = queue_chunk;
    // many tasks per resident workgroup (65536 envs: eight) balance themselves: longer rounds there, fewer hand-overs through the state arrays
    // and fewer rebuilds of the item lists (measured at 65536 envs, cfg3: rounds of 20 / 50 / 100 / 300 substeps: 833 / 856 / 841 / 779 k env-steps/s)
    if (!queue_chunk_set && slots > 0 && T >= 4 * slots) chunk = 50;
    while ((n_substeps + chunk - 1) / chunk > QUEUE_ROUNDS) chunk *= 2;
    // solo servers need the queue (a hard env leaves its task at the end of a round) and the env -> slot table
    // (a hand-over ticket packs env | substep << 20 into one int that must stay non-negative: fewer than 2048 substeps, at most 2^20 envs - beyond
    // that the launch simply runs without servers)
    const bool solo = has_sv && solo_servers > 0 && solo_servers <= 4096 && schedule && slots > 0 && n_substeps >= 3 * chunk && n_substeps < 2048 && N <= (1 << 20)
                      && (T + solo_servers <= slots || 4 * solo_servers <= slots);
    const bool qon = slots > 0 && n_substeps >= 2 * chunk && (solo || queue == 1 || (queue < 0 && T > slots));
    p.tasks = T;
    p.grid = T;
    p.chunk = chunk;
    if (qon) {
        p.rounds = (n_substeps + chunk - 1) / chunk;
        p.grid = T < slots ? T : slots;
        if (solo) {
            p.solo_servers = solo_servers;
            p.solo_trips_x4 = (int)(4.f * solo_trips + 0.5f);
            p.solo_min_left = 2 * chunk;
            p.grid = (slots < T + solo_servers ? slots : T + solo_servers);
        }
    }
    p.split = split_plan(sp.on, group, sp.const_instance, schedule, qon, T, N, slots, n_substeps, sp.period, sp.trips, sp.min_left, sp.extra);
    if (p.split.on) p.grid = T + p.split.extra;
    if (p.split.on && sp.lone && sp.lone_trips > 0.f && sp.lone_trips <= 1000.f) p.split.lone_x4 = (int)(4.f * sp.lone_trips + 0.5f);
    return p;
}
