// libhsrsim.so - host side of the C-ABI declared in include/hsrsim.h (gfx950 only).
//
// Owns: model tables on the device (fp32), per-batch SoA state, one HIP stream per batch, and the launches: one persistent
// kernel per env-step (persist.h: all substeps, ctrl in, obs / reward / done out; a work queue when the batch has more tasks than
// resident workgroups), or - for models outside its lane maps, and as the cross-check of the tests - the per-substep chain
// k_kinematics -> k_cull + k_narrow -> k_solve_mf, optionally replayed from a captured hipGraph.
//
// One translation unit; the host layer is cut by concern into the host_*.h files included at the end (DESIGN.md (b) has the map).
#include <hip/hip_runtime.h>
#include <math.h>
#include <algorithm>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <string>
#include <tuple>
#include <type_traits>
#include <vector>

#include "../../include/hsrsim.h"
#include "collide.h"
#include "model.h"
#include "solve_g.h"
#include "solve_mf.h"
#include "persist.h"
#include "render.h"
#include "episode.h"
#include "snapshot.h"
#include "replay.h"
#include "replay_prio.h"
#include "rollout.h"
#include "normalize.h"
#include "plan.h"
#include "cfg_consts.h"

#include "host_model.h"      // error message, blob loader, hsr_model_*, hull planes: plain C++, no HIP
#include "launch_plan.h"     // QUEUE_ROUNDS, plan_launch: the persistent launch plan, plain C++ (tests/split_logic_main.cpp)
#include "host_batch.h"      // the hsr_batch record; error / entry-guard macros; allocation, upload and staging helpers
#include "util_kernels.h"    // layout / IO / reset / observation / capture kernels, k_queue_init, k_schedule
#include "host_create.h"     // environment switches, kernel-instance table, plan_persist, model upload, hsr_batch_create / destroy
#include "host_step.h"       // launch_substep, forward, reset, the persistent launch plan, hsr_batch_step*
#include "host_episode.h"   // episodes on the device: spec upload, sampled reset, episode end, action sampling (kernels: episode.h)
#include "host_access.h"     // settings, state / field getters and setters, diagnostics
#include "host_render.h"     // ray-caster front end and in-step frame capture
#include "host_snapshot.h"   // env records on the device: save / load / env-to-env copy, the host image (kernel: snapshot.h)
#include "host_replay.h"     // hindsight replay: the transition ring and its sampler (kernels: replay.h, replay_prio.h; books and checks: replay_logic.h, replay_prio_logic.h)
#include "host_rollout.h"    // on-policy rollouts: store, GAE, statistics, shuffled minibatches (kernels: rollout.h; books and checks: rollout_logic.h)
#include "host_normalize.h"  // running mean / std normalisation of rows: fp64 moments, publish, apply (kernels: normalize.h; arithmetic and checks: normalize_logic.h)
#include "host_plan.h"       // cross-entropy-method planner over forked envs: draws, costs, rank and refit (kernels: plan.h; arithmetic and checks: plan_logic.h)
