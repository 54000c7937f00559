/*
 * hsrsim.h - C-ABI of libhsrsim.so: the MI355X-native batched replacement for the slice of
 * mujoco_py that ethanabrooks/hsr-env touches on its hot path (HSREnv.step -> sim.step()).
 *
 * Every entry point cites the reference interface it replaces (paths relative to the reference
 * repository root).  All functions return 0 on success or a negative HSR_E* code; they never
 * throw across the ABI.  hsr_last_error() returns a thread-local message for the last failure.
 * Host arrays are caller-owned, row-major, float32 unless stated; "dev" variants take device
 * pointers (same layout) and do not synchronise the stream.
 *
 * A batch is NOT thread-safe; it owns one HIP stream and all device buffers (SoA [field][env]).
 */
#ifndef HSRSIM_H
#define HSRSIM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HSR_OK 0
#define HSR_EINVAL (-1)   /* bad argument / shape (reference: AssertionError, hsr/mujoco_env.py:88-89) */
#define HSR_EBLOB (-2)    /* not a model blob (reference: IOError on a missing XML, hsr/mujoco_env.py:30-31) */
#define HSR_EDEVICE (-3)  /* HIP runtime failure / no GPU (reference: DependencyNotInstalled, hsr/mujoco_env.py:12-15) */
#define HSR_ENAME (-4)    /* unknown body / joint name */
#define HSR_EBADSTATE (-5) /* some env hit a non-finite state (reference: mujoco_py.MujocoException) */

typedef struct hsr_model hsr_model;
typedef struct hsr_batch hsr_batch;
typedef struct hsr_snapshot hsr_snapshot;
typedef struct hsr_replay hsr_replay;

/* indices for hsr_model_size() */
enum hsr_size { HSR_NQ = 0, HSR_NV, HSR_NU, HSR_NLINK, HSR_NBODY, HSR_NGEOM, HSR_NPAIR, HSR_NMESHVERT,
                HSR_NSLOT, HSR_NLIMIT, HSR_NCONMAX, HSR_NJMAX, HSR_NMOCAP };

const char *hsr_last_error(void);

/* ---- model: replaces mujoco_py.load_model_from_path (hsr/mujoco_env.py:33) on the XML produced by
 *      hsr/util.py:87-182; the blob is emitted offline by hsr_env_amd/compiler.py ---------------- */
int hsr_model_load(const void *blob, size_t len, hsr_model **out);
void hsr_model_destroy(hsr_model *m);
int hsr_model_size(const hsr_model *m, int which);                 /* sim.model.nq / nv / nu (hsr/mujoco_env.py:88-89) */
double hsr_model_timestep(const hsr_model *m);                     /* sim.model.opt.timestep (hsr/mujoco_env.py:98) */
int hsr_model_ctrlrange(const hsr_model *m, float *out /*[nu,2]*/); /* model.actuator_ctrlrange (hsr/mujoco_env.py:44) */
int hsr_model_qpos0(const hsr_model *m, float *out /*[nq]*/);       /* sim.data.qpos after MjSim() (hsr/mujoco_env.py:49) */
int hsr_model_body_id(const hsr_model *m, const char *name);       /* name lookup behind data.get_body_xpos (hsr/env.py:144,180,184) */
int hsr_model_joint_qpos_addr(const hsr_model *m, const char *name, int *start, int *end); /* model.get_joint_qpos_addr (hsr/env.py:153) */
/* face planes (n, w), n.x <= w inside, of a mesh geom's convex hull in the geom frame (computed in double from the hull vertices on
 * first use; coplanar facets merged).  Writes min(count, cap) planes and returns the count, or HSR_EINVAL for a geom that is not a mesh. */
int hsr_model_hull_planes(const hsr_model *m, int geom, float *out /*[cap,4]*/, int cap);

/* ---- batch of N independent envs on one GPU: replaces N x mujoco_py.MjSim(model) (hsr/mujoco_env.py:34) */
int hsr_batch_create(const hsr_model *m, int n_envs, int device_id, hsr_batch **out);
void hsr_batch_destroy(hsr_batch *b);                              /* sim.__exit__ (hsr/env.py:209) */
int hsr_batch_size(const hsr_batch *b);
void *hsr_batch_stream(const hsr_batch *b);                        /* hipStream_t the batch launches on */
int hsr_batch_sync(hsr_batch *b);

/* sim.reset() + reset_model() writes (hsr/mujoco_env.py:83-85, hsr/env.py:158-177): for envs with
 * mask[e] != 0 (all if mask == NULL): qpos <- qpos0[e] (model qpos0 if NULL), qvel <- 0, ctrl <- 0,
 * warm start <- 0, time <- 0, mocap_pos <- mocap[e] (0 if NULL); then sim.forward(). */
int hsr_batch_reset(hsr_batch *b, const uint8_t *mask, const float *qpos0 /*[N,nq]*/, const float *mocap /*[N,3]*/);

/* same for device pointers, asynchronous; d_mask == NULL means "the envs whose done flag the last step
 * latched" - the batched form of `if done: env.reset()` (hsr/control.py:73-75) */
int hsr_batch_reset_dev(hsr_batch *b, const uint8_t *d_mask, const float *d_qpos0, const float *d_mocap);

/* sim.get_state() / sim.set_state(MjSimState(time,qpos,qvel,act,udd_state)) + forward
 * (hsr/mujoco_env.py:87-94, hsr/env.py:69,150,175); act and udd_state are empty for this model */
int hsr_batch_get_state(hsr_batch *b, float *time /*[N]*/, float *qpos /*[N,nq]*/, float *qvel /*[N,nv]*/);
int hsr_batch_set_state(hsr_batch *b, const float *time, const float *qpos, const float *qvel);
int hsr_batch_set_mocap(hsr_batch *b, const float *mocap /*[N,3]*/);   /* sim.data.mocap_pos[:] = ... (hsr/env.py:169) */
int hsr_batch_set_warmstart(hsr_batch *b, const float *qacc_warmstart /*[N,nv]*/);
int hsr_batch_get_warmstart(hsr_batch *b, float *qacc_warmstart /*[N,nv]*/);
int hsr_batch_forward(hsr_batch *b);                               /* sim.forward() (hsr/env.py:176) */

/* HSREnv.step (hsr/env.py:115-135) for all envs: ctrl[:] = action; up to n_substeps x { sim.step();
 * done = |xpos(goal_body) - mocap_pos| < geofence; break if done }; obs = concat(qpos, qvel);
 * reward = float(done).  goal_body < 0 reproduces `goals is None` (done stays 0).
 * Outputs may be NULL.  nsteps (optional) receives the substeps each env actually ran. */
int hsr_batch_step(hsr_batch *b, const float *ctrl /*[N,nu]*/, int n_substeps, int goal_body, float geofence,
                   float *obs /*[N,nq+nv]*/, float *reward /*[N]*/, uint8_t *done /*[N]*/, int32_t *nsteps /*[N]*/);
/* same with device pointers, asynchronous on hsr_batch_stream() */
int hsr_batch_step_dev(hsr_batch *b, const float *d_ctrl, int n_substeps, int goal_body, float geofence,
                       float *d_obs, float *d_reward, uint8_t *d_done, int32_t *d_nsteps);

/* Further goal terms, AND-ed per substep with the main term of hsr_batch_step* - `all(in_range(*g) for g in goals)`,
 * hsr/env.py:124-126,137-147: term k holds when |p(body_a[k]) - p(body_b[k])| < dist[k], p(body) = its xpos, or the env's mocap
 * point when the body is the mocap body.  n = 0..4 (0 clears); with goal_body < 0 in hsr_batch_step* the terms alone decide. */
int hsr_batch_set_goals(hsr_batch *b, int n, const int *body_a, const int *body_b, const float *dist);

/* sim.data.get_body_xpos(name) for every env (hsr/env.py:144,180,184); valid after forward/step */
int hsr_batch_body_xpos(hsr_batch *b, int body_id, float *out /*[N,3]*/);


/* the reference's 'openai' observation (hsr/env.py:72-110, restored to its evident intent), fused in
 * one kernel: out[N,25] = grip_pos 3 | object_pos 3 | object_rel_pos 3 | gripper_state 2 | object_rot 3 (mat2euler,
 * hsr/env.py:256-272) | object_velp 3 | object_velr 3 | grip_velp 3 | gripper_vel 2.
 * ids[7] = {finger body l, finger body r (hsr/env.py:59), object body (hsr/env.py:58), qpos address of the two finger
 * joints, dof address of the two finger joints}.  Positions / velocities are those of the last forward pass. */
int hsr_batch_obs_openai(hsr_batch *b, const int *ids, float *out /*[N,25]*/);
int hsr_batch_obs_openai_dev(hsr_batch *b, const int *ids, float *d_out);
/* render (hsr/mujoco_env.py:105-125, batched): cam[9] = lookat3 distance azimuth elevation (degrees) fovy (degrees) znear zfar,
 * MuJoCo free-camera convention; track_body >= 0: per-env lookat = xpos(track_body) + lookat. geom_rgba [ngeom,4] or NULL
 * (the model's default palette). Outputs may be NULL. Poses are those of the last reset / forward / step.
 * A ray caster over the collision geoms (the blob carries no visual-only geoms): rgb uint8 [N,H,W,3], depth float [N,H,W] (distance
 * along the camera axis, zfar on background), segid int32 [N,H,W] (geom id, -1 on background); row 0 is the top of the image.
 * Shading: rgb = rgba.rgb (0.1 + 0.4 max(0, n.v) + 0.5 max(0, n.z)), clamped, no shadows / specular / textures.
 * Never writes simulation state.  HSR_EINVAL: width / height outside 1..4096, a non-finite camera, fovy outside (0, 180),
 * znear <= 0 or zfar <= znear, a track_body out of range or the mocap body. */
int hsr_batch_render(hsr_batch *b, const float *cam, int track_body, int width, int height, const float *geom_rgba,
                     uint8_t *rgb /*[N,H,W,3]*/, float *depth /*[N,H,W]*/, int32_t *segid /*[N,H,W]*/);
int hsr_batch_render_dev(hsr_batch *b, const float *cam, int track_body, int width, int height, const float *geom_rgba,
                         uint8_t *d_rgb, float *d_depth, int32_t *d_segid);   /* asynchronous on hsr_batch_stream() */
/* In-step frame capture (hsr/env.py:118-131: VideoRecorder.capture_frame every record_freq substeps before sim.step(), 50 frames of the
 * final poses after a step that reached the goal).  The n envs env_ids[0..n) get capture slots 0..n-1; every > 0 is the period in
 * substeps, every = 0 turns capture off (the default; n and env_ids are then ignored).  In each later hsr_batch_step* a slot takes frame k
 * at substep k * every if its env is live then (not done at an earlier substep of the step): the link poses of that substep's forward
 * pass, what mujoco-py draws before sim.step().  An env that ran s substeps has s == 0 ? 0 : (s - 1) / every + 1 frames.  Each slot
 * also gets a final frame: the poses after the step (HSR_F_XPOS / HSR_F_XMAT).  A step of S substeps keeps rows = (S == 0 ? 0 :
 * (S - 1) / every + 1) + 1 rows per slot, the final frame in the last row; rows past a slot's count (other than the last) are not written.
 * The frame buffer holds NaN when it is allocated and after every hsr_batch_set_capture with every > 0.
 * Capture does not change any result of the step.  HSR_EINVAL: every < 0, n outside 1..HSR_CAPTURE_MAX, an env id out of range or
 * repeated.  Synchronises. */
#define HSR_CAPTURE_MAX 1024
int hsr_batch_set_capture(hsr_batch *b, int every, int n, const int *env_ids);
/* frames per slot in the last step (counts[n], may be NULL); returns the rows per slot (> 0), HSR_EINVAL when capture is off or no
 * step ran since hsr_batch_set_capture.  Synchronises. */
int hsr_batch_capture_counts(hsr_batch *b, int32_t *counts);
/* host copy of the captured rows of the last step: xpos [n, rows, nlink, 3], xmat [n, rows, nlink, 9] (either may be NULL); final frame
 * last.  Rows past a slot's count hold what the buffer held before (NaN if no step wrote them since hsr_batch_set_capture).  Synchronises. */
int hsr_batch_capture_poses(hsr_batch *b, float *xpos, float *xmat);
/* hsr_batch_render of the captured rows: image (slot, row) at index slot * rows + row of rgb [n, rows, H, W, 3], depth [n, rows, H, W],
 * segid [n, rows, H, W]; the images of rows past a slot's count (other than the last) are not written.  track_body reads the frame's own
 * poses.  Same checks as hsr_batch_render, and HSR_EINVAL when there is no captured step. */
int hsr_batch_render_frames(hsr_batch *b, const float *cam, int track_body, int width, int height, const float *geom_rgba,
                            uint8_t *rgb, float *depth, int32_t *segid);
int hsr_batch_render_frames_dev(hsr_batch *b, const float *cam, int track_body, int width, int height, const float *geom_rgba,
                                uint8_t *d_rgb, float *d_depth, int32_t *d_segid);   /* asynchronous on hsr_batch_stream() */
/* per-env error flags (non-finite or |q| > 1e10), the batched form of MuJoCo's mj_checkPos/Vel */
int hsr_batch_bad_state(hsr_batch *b, uint8_t *out /*[N]*/);

/* ---- introspection used by the parity tests (stage-by-stage comparison with the oracle) ------ */
/* HSR_F_XPOS / HSR_F_XMAT: the link poses of the last forward pass.  After hsr_batch_reset / _set_state / _forward that is the pass over the
 * current state; after hsr_batch_step* it is the forward pass of every env's LAST substep, that is the poses of the state that substep
 * STARTED from (mj_step runs mj_forward, then integrates: sim.data.xpos after sim.step() lags qpos by one substep in the same way),
 * with the free-joint quaternions normalised; persistent kernel and per-substep chain alike. */
enum hsr_field { HSR_F_XPOS = 0 /*[N,nlink,3]*/, HSR_F_XMAT /*[N,nlink,9]*/, HSR_F_M /*[N,nv,nv]*/,
                 HSR_F_QACC /*[N,nv]*/, HSR_F_QACC_SMOOTH /*[N,nv]*/, HSR_F_QFRC_SMOOTH /*[N,nv]*/,
                 HSR_F_QFRC_CONSTRAINT /*[N,nv]*/, HSR_F_NCON /*[N] (as float)*/, HSR_F_NEFC /*[N]*/,
                 HSR_F_CONTACT /*[N,nslot,7] pos3 normal3 dist; dist=+1 marks an empty slot*/,
                 HSR_F_NITER /*[N]*/ };
int hsr_batch_get_field(hsr_batch *b, int field, float *out);
/* timing of the last hsr_batch_step*: total ms and per-kernel ms (HIP events on the batch stream);
 * enable with hsr_batch_set_profiling(b, 1).  kernel order: kinematics, collide, solve */
int hsr_batch_set_profiling(hsr_batch *b, int on);
int hsr_batch_last_timing(hsr_batch *b, float *total_ms, float *kernel_ms /*[3]*/, int *launches /*[3]*/);
/* hsr_batch_set_profiling(b, 2): log an event pair around EVERY launch of the persistent kernel without synchronising (what bench.py
 * times its roofline with).  hsr_batch_kernel_times synchronises, writes the durations (ms) of the launches logged since the last
 * call into out_ms[0..cap) and returns how many there were. */
int hsr_batch_kernel_times(hsr_batch *b, float *out_ms, int cap);
/* use a captured hipGraph for the substep loop of the per-substep-kernel path (default on) */
int hsr_batch_set_graph(hsr_batch *b, int on);
/* whole env-step in ONE persistent kernel (default on when the model fits: nv <= 32, LDS budget); returns the
 * resulting setting.  With it on, hsr_batch_last_timing() reports the persistent kernel in slot 2 (slots 0,1 = 0). */
int hsr_batch_set_persistent(hsr_batch *b, int on);
int hsr_batch_is_persistent(const hsr_batch *b);                  /* 0 = per-substep chain; else bit 0 set, bit 1: the kernel instance carries the model's scalars as
                                                                    * compile-time constants, bit 2: and its kinematic tree (straight-line kinematics / inertia).
                                                                    * The instance is the one hsr_batch_create chose for the batch. */
/* introspection after hsr_batch_step*: with it on, the persistent kernel also stores what hsr_batch_forward stores - the
 * per-pair contact counts (HSR_F_CONTACT), HSR_F_NCON / NEFC / NITER and HSR_F_QACC of every env's LAST substep (default off:
 * the fields then describe the last hsr_batch_forward).  Parity tests of the hot path's own narrowphase use it.
 * `on` is a bit mask: 1 = the above; 2 and 4 are test hooks that force rarely taken branches of the Newton solver of the persistent
 * kernel (2: J v per contact instead of per link; 4: every iteration takes the PSD-majorant Hessian) - same minimiser, other path;
 * 16 makes the convex-pair section trust a cached separation margin whatever its stamp - the round-2 behaviour, kept so that the test of
 * the stamps can show what they prevent; 64 makes the persistent kernel cull every substep instead of keeping its narrowphase item list
 * until a geom may have moved half a skin (the behaviour up to round 3; the contact sets are the same either way); 128 keeps the dense factorisation of the Newton Hessian where the sparse one applies (32-lane instances with several free bodies, envs whose contacts couple at most one body to the robot: same minimiser, fewer instructions); 32 raises the work queue's watchdog flag after every persistent launch (what a ticket that is
 * never served does): the flag is sticky on the device, the next synchronising call (hsr_batch_sync, _step, _kernel_times, _cap_counts,
 * _bad_state, _get_state) returns HSR_EDEVICE once and clears it. */
int hsr_batch_set_debug(hsr_batch *b, int on);
/* Solo servers of the persistent kernel (queued launches; the 16-lane instances of the reference configurations).  `servers` workgroups
 * of the launch take no tasks: they wait for envs that a worker has found hard - `trips` or more Newton iterations per substep over a
 * round of the work queue (0 keeps the current threshold) - and run each of them alone in a wave, from the substep its worker left it at to
 * the end of the env-step, while the task it came from goes on without it.  The launch ends with its slowest env's chain (hsr/env.py:118-131
 * is one serial loop per env); this shortens that chain.  0 servers = off.  A server's replicas sum the contact terms of the Hessian and
 * of J^T f in another order than a worker does, and which envs get a server depends on timing: with servers on, results are reproducible to
 * rounding (median |dobs| 1e-5 after an env-step, tests/test_gpu_hotpath.py::test_solo_servers_follow_the_plain_run), not bit for bit.  Launches of
 * 2048 or more substeps or of more than 2^20 envs run without servers (the hand-over ticket is one int).  Returns 1 (not an error) when the
 * model's kernel instance has no server path. */
int hsr_batch_set_solo(hsr_batch *b, int servers, float trips);
/* envs handed over by the last persistent launch - to solo servers, or inside a splitting launch (below) (synchronises) */
int hsr_batch_solo_handovers(hsr_batch *b, int *out);
/* Hand-over of hard envs inside a launch WITHOUT the work queue (persist.h): a wave advances at the pace of its hardest env, so every
 * `period` substeps it checks whether two or more of its live envs ran `trips` Newton iterations per substep or more over that window; if so,
 * and with `min_left` substeps or more ahead, it keeps the hardest and gives the others to workgroups that have already finished their own
 * task, one env each.  The env runs the ordinary code path there: every result is bit-identical with the split on or off, whoever ran the env
 * from whichever substep.  Applies to launches of the arm models' constant-configuration kernel instances (cfg3, the cupboard) with wave packing on; any other launch
 * (queued, more workgroups than the GPU holds at once, 2048 or more substeps, more than 2^20 envs) runs exactly as without it.  on = 0: off (on by default; HSR_SPLIT=0 / 1 override).
 * period = 0, trips < 0, min_left = 0 keep the current value (defaults 8, 2.0, 40; HSR_SPLIT_PERIOD / _TRIPS / _MIN_LEFT); trips = 0
 * counts every live env as hard (tests).  extra_helpers (tests; 0 in production) launches that many workgroups without a task which start as
 * helpers; they must fit next to the tasks' workgroups among those the GPU holds at once, else the launch does not split.  Returns 1 (not an
 * error) when the batch's kernel instance never splits. */
int hsr_batch_set_split(hsr_batch *b, int on, int period, float trips, int min_left, int extra_helpers);
/* The lone rule of a splitting launch (split_logic.h: split_decide_lone): even the easiest neighbours cost a hard env several per cent of its
 * wave's pace, so at a check point a wave whose hardest remaining env ran `trips` Newton iterations per substep or more over the window, while a
 * live env that stays ran fewer, gives that env to a helper as well and goes on with the easier ones.  A wave whose live envs are all at or above
 * the threshold keeps its hardest, and a wave never gives away its last live env.  Same launches, period, min_left and helpers as
 * hsr_batch_set_split, which must be on; results stay bit-identical.  on = 0: off (on by default, measured: DESIGN.md; HSR_SPLIT_LONE=0 / 1 override);
 * trips <= 0 keeps the current threshold (default 4.5; HSR_SPLIT_LONE_TRIPS).  Returns 1 (not an error) when the batch's kernel instance never splits. */
int hsr_batch_set_split_lone(hsr_batch *b, int on, float trips);
/* wave packing of the persistent kernel (default on; HSR_SCHEDULE=0 turns it off at creation): before every launch the envs are re-distributed over the waves by the
 * Newton iterations they needed at the end of their previous launch (hard envs one per wave, with the easiest as neighbours).
 * A pure scheduling decision: every env's result is bit-identical with it on or off. */
int hsr_batch_set_schedule(hsr_batch *b, int on);
/* Convex pairs (mesh / cylinder vs box / mesh: MPR, libccd's ccdMPRPenetration behind mjc_Convex).  A pair that penetrates keeps the
 * vertex ids of the portal its run ended on; placed with the next substep's poses they are a portal again (checked: the origin ray
 * still crosses their triangle, else the run starts from scratch), so the refinement confirms the face it found last time with 2-3
 * support calls instead of rediscovering it with 8.  The refinement itself is libccd's.  Where the origin projects into the final
 * triangle the result (the face's plane) does not depend on how the run got there; where it does not (libccd then measures to the
 * triangle's edge) a warm-started run is repeated from scratch and nothing is kept for the next substep - the warm start is as close
 * to the cold-started fp64 oracle as a cold fp32 run is (tests/test_gpu_hotpath.py::test_pinched_block_contacts_follow_the_oracle).
 * Default on (HSR_MPR_WARM=0 at creation, or this call, turns it off). */
int hsr_batch_set_mpr_warm(hsr_batch *b, int on);
/* Work queue of the persistent kernel.  When a batch has more tasks (groups of 4 or 2 envs) than the GPU holds workgroups at once
 * (BASELINE configs 4 / 5: 4096 two-env tasks on 2048 resident workgroups), the env-step is cut into rounds of `chunk` substeps and
 * persistent workgroups take (task, round) tickets, lowest round first, so a task that lags is always resumed at once and no
 * second dispatch round starts a hard task late.  mode: -1 automatic (default; HSR_QUEUE overrides at creation), 0 off, 1 on whenever the env-step
 * has at least two rounds; chunk: substeps per round (0 keeps it; default 20, HSR_QUEUE_CHUNK).  Scheduling only: results are bit-identical. */
int hsr_batch_set_queue(hsr_batch *b, int mode, int chunk);
/* How often the device buffer caps bit since the last call (the counters are cleared): out[0] = (env, substep) pairs that
 * dropped contacts beyond nconmax, out[1] = dropped constraint rows beyond njmax, out[2] = dropped narrowphase work items
 * beyond 64 per env, out[3] = (env, substep) pairs executed.  MuJoCo's own caps are nconmax=100 njmax=500
 * (hsr/models/world.xml:44); the compiled models carry smaller ones. */
int hsr_batch_cap_counts(hsr_batch *b, unsigned long long *out /*[4]*/);
/* of the row-cap events above: how many rows beyond njmax the env would have needed - out[k] counts the events with
 * njmax + 8 k < rows wanted <= njmax + 8 (k + 1) (the last bin is open-ended); cleared by the call.  What the compiled njmax is sized by. */
int hsr_batch_cap_histogram(hsr_batch *b, unsigned long long *out /*[8]*/);
/* Newton iterations every env ran over the last (up to) 100 substeps of its previous env-step launch: the hardness measure
 * hsr_batch_set_schedule packs by (the solver's iteration count MuJoCo reports as mjData.solver_iter, summed). */
int hsr_batch_newton_trips(hsr_batch *b, int32_t *out /*[n_envs]*/);
/* the packing the last persistent launch ran with (k_schedule, csrc/util_kernels.h): out[slot] = env that lane group `slot % (64 / lanes per env)` of task
 * `slot / (64 / lanes per env)` held, -1 = empty; ceil(n_envs / envs per wave) * envs per wave entries.  Contract (tests/test_gpu_hotpath.py): every env exactly
 * once; per chunk of 8192 envs the first lane group of task w holds the env with the w-th most iterations (ties: lower index), the other groups are
 * filled from the easy end.  Results never depend on it.  An env that its wave handed over inside the launch (hsr_batch_set_split) reads -1: the
 * table shows the waves as the launch left them. */
int hsr_batch_packing(hsr_batch *b, int32_t *out /*[ceil(n_envs / epw) * epw]*/);

/* ---- episodes on the device: sampled auto-reset, time limit, episode statistics -------------------------------------------------
 * Opt-in.  hsr_batch_reset / hsr_batch_reset_dev above know nothing of episodes: they neither sample nor touch the books below.
 *
 * Draws come from Philox4x32-10, key = (seed & 0xffffffff, seed >> 32), counter = (gid, episode, stream, block) with
 * gid = env_offset + e, so a shard at env_offset draws what the single batch draws for the same envs.  A 32-bit word x gives
 * u = (x >> 8) 2^-24 and the value min(hi, lo + u (hi - lo)), every operation rounded to float32 on its own; lo == hi gives lo.
 *   stream 0: qpos[i] = word i % 4 of block i / 4 over (qpos_lo[i], qpos_hi[i])
 *   stream 1: the goal point (mocap_pos) = words 0..2 of block 0 over (goal_lo, goal_hi); has_goal == 0: the point is 0
 *   stream 2: the pose of block k = words 0..3 of block k: x, y, z, yaw over (block_lo, block_hi), written to qpos[block_qadr[k] ..+7) as
 *             (x, y, z, cos(yaw/2), 0, 0, sin(yaw/2)) in place of what stream 0 drew there
 *   stream 3: ctrl[a] = word a % 4 of block a / 4 over the actuator's ctrlrange; the second counter word is the caller's action step */
typedef struct hsr_episode_spec {
    uint64_t seed;
    uint32_t env_offset;           /* global id of the batch's env 0 */
    int32_t max_episode_steps;     /* env-steps after which an episode is truncated; 0 = no limit */
    const float *qpos_lo, *qpos_hi; /* [nq]; lo == hi == qpos0 where nothing is sampled */
    int32_t has_goal;
    float goal_lo[3], goal_hi[3];
    int32_t nblock;                /* free bodies placed by stream 2 (0: none) */
    const int32_t *block_qadr;     /* [nblock] qpos address of each one's free joint */
    float block_lo[4], block_hi[4]; /* x, y, z, yaw */
} hsr_episode_spec;
/* uploads the spec, allocates (first call) and zeroes the per-env books: episode index, length and return.  Synchronises.
 * HSR_EINVAL: a NULL spec or table, a bound that is not finite, lo > hi, max_episode_steps < 0, nblock above the model's free bodies, a
 * block_qadr that is not the address of a free joint.  A refused call leaves the batch as it was. */
int hsr_batch_set_episodes(hsr_batch *b, const hsr_episode_spec *spec);
/* the envs with d_mask[e] != 0 (all if NULL) draw episode ep_index[e], restart from it as in hsr_batch_reset_dev (state reset, forward),
 * ep_index[e] += 1, length and return <- 0.  The dev variant is asynchronous; the host-mask twin synchronises. */
int hsr_batch_reset_sampled_dev(hsr_batch *b, const uint8_t *d_mask);
int hsr_batch_reset_sampled(hsr_batch *b, const uint8_t *mask);
/* Closes the env-step hsr_batch_step_dev just ran, asynchronous on hsr_batch_stream().  Per env: return += reward, length += 1;
 * truncated = max_episode_steps > 0 and length >= max_episode_steps; reset kind = done ? 1 : truncated ? 2 : 0.  Envs of kind 1 / 2 publish
 * return and length in d_fin_return / d_fin_length (0 for the others), draw their next episode and restart from it exactly as
 * hsr_batch_reset_dev(mask, ...) would: the other envs keep every bit of their state.  d_final_obs receives d_obs as the step left it;
 * then the d_obs rows of the reset envs become the new episode's first observation, concat(qpos, 0).
 * d_obs / d_reward / d_done are what the step wrote (NULL: obs is not touched; reward = done; done = the flag the step latched);
 * every output may be NULL.  HSR_EINVAL before hsr_batch_set_episodes. */
int hsr_batch_episode_end_dev(hsr_batch *b, float *d_obs, const float *d_reward, const uint8_t *d_done, float *d_final_obs,
                              uint8_t *d_reset_kind, float *d_fin_return, int32_t *d_fin_length);
/* d_ctrl[N,nu] ~ U(ctrlrange) from stream 3 for action step `step`; a side without a limit (not finite, or the compiled models' marker
 * 1e30) counts as -1 / +1.  Asynchronous. */
int hsr_batch_sample_ctrl_dev(hsr_batch *b, uint32_t step, float *d_ctrl);
/* host copies of the books (any may be NULL); synchronises */
int hsr_batch_episode_state(hsr_batch *b, uint32_t *ep_index, int32_t *ep_length, float *ep_return);

/* ---- exact snapshots: save, restore and fork envs on the device, bit for bit -----------------------------------------------------
 * sim.get_state() / sim.set_state() (hsr/env.py:69,150,175; hsr/mujoco_env.py:87-94) in their exact form.  hsr_batch_set_state above voids
 * the collision caches and runs a forward pass: the batch it leaves is a cold start.  A snapshot holds env RECORDS: everything of an env
 * that a later step / forward / getter reads before it writes -
 *   qpos qvel ctrl mocap_pos qacc_warmstart time, the done / bad-state flags and the substep count of the last step;
 *   the collision caches (cached separating axes and margins, the MPR portals of penetrating pairs, their stamps and the env's tick);
 *   the Newton-iteration count that wave packing reads (never changes a result);
 *   the link poses and velocities of the last forward pass (hsr_batch_body_xpos, _obs_openai, _render and the goal terms read them): a load
 *   runs no forward pass;
 *   the episode books (index, length, return): zero in a record saved before hsr_batch_set_episodes, loaded only into a batch that has them;
 *   an env's next episode is drawn with key (gid of the env it was loaded into, restored episode index).
 * A loaded env continues bit for bit as the saved one did, in any slot of any batch of the same model (results never depend on either).
 * NOT in a record: the solver's and the narrowphase's intermediates (for a loaded env hsr_batch_get_field other than HSR_F_XPOS / HSR_F_XMAT
 * describes nothing until the next forward or step), capture slots and frames, goals, settings, cap statistics, and a hindsight replay
 * (below: a ring of past transitions cannot follow a jump; clear it after a load or a copy).
 * Records are copied as 32-bit patterns (NaN payloads and -0 survive).  A snapshot is bound to a model (the 64-bit FNV-1a hash of its blob,
 * computed by hsr_model_load) and a device, not to the batch that made it: it may be loaded into another batch of the same model on the
 * same device.  Its device storage is released by hsr_snapshot_destroy, or by hsr_batch_destroy of the batch that made it, whichever
 * comes first: after the latter the handle is still the caller's to destroy, and every other use of it returns HSR_EINVAL.
 *
 * Host variants take host id arrays, check everything and synchronise; HSR_EINVAL leaves batch and snapshot untouched: a NULL handle, n < 0
 * or above the batch's envs or the capacity, an id out of range, a repeated destination (env for load / copy, slot for save), capacity < 1,
 * a snapshot of another model or device.  The _dev variants take device id arrays and are asynchronous on hsr_batch_stream(); they check
 * what the host can see (handles, n, model, device); ids out of range are skipped (nothing is read or written for them); repeated
 * destinations are the caller's error - which source wins is unspecified.  Between the streams of two batches that use one snapshot
 * through _dev variants, ordering is the caller's job. */
int hsr_batch_snapshot_create(hsr_batch *b, int capacity, hsr_snapshot **out);
void hsr_snapshot_destroy(hsr_snapshot *s);
int hsr_snapshot_capacity(const hsr_snapshot *s);
/* record slot[i] <- env env[i], i < n; a NULL env / slot array stands for 0..n-1 */
int hsr_batch_snapshot_save(hsr_batch *b, hsr_snapshot *s, const int32_t *env, const int32_t *slot, int n);
int hsr_batch_snapshot_save_dev(hsr_batch *b, hsr_snapshot *s, const int32_t *d_env, const int32_t *d_slot, int n);
/* env env[i] <- record slot[i]; a slot may appear any number of times (fan-out) */
int hsr_batch_snapshot_load(hsr_batch *b, const hsr_snapshot *s, const int32_t *slot, const int32_t *env, int n);
int hsr_batch_snapshot_load_dev(hsr_batch *b, const hsr_snapshot *s, const int32_t *d_slot, const int32_t *d_env, int n);
/* env dst[i] <- env src[i] inside one batch; every source is read before any destination is written (an env may be both), through a scratch
 * snapshot of the batch that the first call allocates and a call with a larger n replaces (that call waits for the stream) */
int hsr_batch_copy_envs(hsr_batch *b, const int32_t *src, const int32_t *dst, int n);
int hsr_batch_copy_envs_dev(hsr_batch *b, const int32_t *d_src, const int32_t *d_dst, int n);
/* Host image of a snapshot, for checkpoint files: a 56-byte little-endian header - "HSRSNAP1", u32 format version (1), u32 header bytes,
 * u64 model fingerprint, i64 capacity, i32 nq nv nu nlink npair_sep (= max(npair, 1)), i32 record words - then uint32 [record words][capacity]
 * as stored (record rows in the order above; csrc/snapshot.h).  export: len must be hsr_snapshot_image_bytes().  import / image_check return
 * HSR_EBLOB, and import leaves the snapshot unchanged, for a wrong magic, version, fingerprint or size field, a capacity other than the
 * snapshot's, and a len that is short, long or negative.  export and import wait for the whole device. */
int hsr_snapshot_image_bytes(const hsr_snapshot *s, long long *out);
int hsr_snapshot_export(const hsr_snapshot *s, void *out, long long len);
int hsr_snapshot_import(hsr_snapshot *s, const void *image, long long len);
/* no device work (usable without a GPU): 32-bit words per record; whether `image` is a snapshot image of model m (its capacity in *capacity, may be NULL) */
int hsr_model_snapshot_record_words(const hsr_model *m);
int hsr_model_snapshot_image_check(const hsr_model *m, const void *image, long long len, int *capacity);

/* ---- hindsight replay on the device: an episode-aware transition ring and a relabelling sampler ----------------------------------------
 * Opt-in.  The task is sparse-reward and goal-conditioned: reward = float(goal body within the geofence of the sampled point)
 * (hsr/env.py:124-133,137-147), a new point every episode (hsr/env.py:161-172), observations meant as the pair (observation, goal)
 * (hsr/env.py:275).  A replay replaces the host ring of rl_utils/replay_buffer.py:27-82 (store, sample) for this env and adds what hindsight
 * relabelling needs and only the batch has: the goal body's position after the step and before the auto-reset moves it, mocap_pos, and
 * where an episode ends inside the ring.
 *
 * Ownership as for snapshots: a replay is bound to the batch that made it, reads that batch's arrays and launches on hsr_batch_stream().
 * Its storage goes with hsr_replay_destroy, or with hsr_batch_destroy of its batch, whichever is first: after the latter the handle is
 * still the caller's to destroy, and every other use returns HSR_EINVAL.  A batch that never creates one allocates nothing.  A replay is
 * NOT part of an env record (snapshots above): after hsr_batch_snapshot_load* / hsr_batch_copy_envs* the ring describes a past the envs no
 * longer have - clear it.
 *
 * Storage per env: capacity_steps rows of W = 2 obs_dim + nu + 10 words (padded to a multiple of 4):
 *   obs | act | next_obs | achieved_next[3] | desired[3] | reward | done | ep_id | ep_step
 * Protocol (host state machine EMPTY -> READY -> PENDING; a call out of order returns HSR_EINVAL and launches nothing):
 *   commit(d_obs [N,obs_dim], d_reset [N] or NULL = all): d_obs is what the policy acts on next; d_reset[e] != 0: env e starts a new episode
 *     with this row: ep_id[e] += 1, ep_step[e] = 0; otherwise ep_step[e] += 1 (the replay's own uint32 counters; the batch's episode books
 *     are not read).  From PENDING it also closes the pending transition: pushed += 1.
 *   record(d_ctrl [N,nu], d_next_obs [N,obs_dim], d_reward [N], d_done [N]): only from READY, after hsr_batch_step_dev and BEFORE
 *     hsr_batch_episode_end_dev / any reset.  Writes slot pushed mod T of every env: obs = the committed row, act, next_obs, reward, done
 *     (NULL: the flag the step latched, reward = float(flag), as in hsr_batch_episode_end_dev), ep_id, ep_step, achieved_next =
 *     xpos(goal_body) as hsr_batch_body_xpos gives it for the step just run, desired = the env's mocap_pos.
 *   clear: back to EMPTY, pushed = 0, counters 0; frees nothing.
 * Sampling (the replacement of ReplayBuffer.sample, rl_utils/replay_buffer.py:64-82, with the 'future' relabelling strategy): count =
 * min(pushed, T); the stored steps of an env have ages j = 0 .. count-1, oldest first, slot(j) = (pushed - count + j) mod T.  Sample i of
 * draw `draw` takes the Philox block of key (seed & 0xffffffff, seed >> 32), counter (i, draw, 4, env_offset); mulhi(w, n) = (w n) >> 32:
 *   e = mulhi(word0, N), j = mulhi(word1, count), relabel = (float)(word2 >> 8) 2^-24 < her_ratio (a float32 compare);
 *   j_end = the largest age >= j with the ep_id of age j (ids are monotone per env: the run is contiguous);
 *   j_goal = j + mulhi(word3, j_end - j + 1).
 *   not relabelled: goal = desired[j], reward and done as stored;
 *   relabelled: goal = achieved_next[j_goal], reward = float(norm(achieved_next[j] - goal) < geofence) - the env's own goal test,
 *     hsr/env.py:124-133,137-147 -, done = reward != 0 (success is the only terminal; truncation never is).
 *   obs / act / next_obs / achieved_next are the rows of (e, slot(j)) as stored, moved as 32-bit patterns;
 *   d_index[i] = (e, slot(j), relabelled ? slot(j_goal) : -1, relabelled).
 * Every output may be NULL.  The call is asynchronous and never writes the ring or the batch.  HSR_EINVAL: count == 0, a pending record,
 * batch < 1, her_ratio not in [0, 1]. */
typedef struct hsr_replay_spec {
    uint64_t seed;
    uint32_t env_offset;      /* as in hsr_episode_spec: salts the draws of a shard */
    int32_t  capacity_steps;  /* T: env-steps kept per env (ring) */
    int32_t  obs_dim;         /* floats per observation row the caller will hand over (nq+nv, or 25 for 'openai') */
    int32_t  goal_body;       /* the body whose xpos is the achieved goal; not the mocap body */
    float    geofence;
} hsr_replay_spec;
/* HSR_EINVAL (nothing allocated, the batch as it was): a NULL argument, capacity_steps < 1, obs_dim < 1 or above 2^20, a goal_body out of
 * range or the mocap body, a geofence that is not finite or <= 0, a ring beyond 2^40 bytes, and a batch with extra goal terms
 * (hsr_batch_set_goals with n > 0: a reward of several terms cannot be recomputed from one relabelled point; record refuses likewise when
 * terms were set later).  HSR_EDEVICE: no device memory; what was allocated is freed. */
int  hsr_batch_replay_create(hsr_batch *b, const hsr_replay_spec *spec, hsr_replay **out);
void hsr_replay_destroy(hsr_replay *r);
int  hsr_replay_clear(hsr_replay *r);
int  hsr_replay_commit_dev(hsr_replay *r, const float *d_obs, const uint8_t *d_reset);
int  hsr_replay_record_dev(hsr_replay *r, const float *d_ctrl, const float *d_next_obs, const float *d_reward, const uint8_t *d_done);
int  hsr_replay_state(hsr_replay *r, int32_t *count, int32_t *head_slot, uint32_t *pushed_lo); /* host books, no device work: count, pushed mod T, pushed & 0xffffffff */
int  hsr_replay_sample_dev(hsr_replay *r, uint32_t draw, int batch, float her_ratio,
                           float *d_obs, float *d_act, float *d_next_obs, float *d_goal, float *d_achieved_next,
                           float *d_reward, uint8_t *d_done, int32_t *d_index /*[batch,4]*/);
/* Episode segments and n-step targets (the windows of ReplayBuffer.sample(batch_size, seq_len), rl_utils/replay_buffer.py:59-66, made
 * aware of episodes): the steps after a sampled one, inside its episode, under the same relabelled goal.  L = seq_len.
 *   Draw: sample i takes the Philox block of hsr_replay_sample_dev - stream 4, counter (i, draw, 4, env_offset); e, j, relabel and
 *     j_goal = j + mulhi(word3, j_end - j + 1) are as there; j_end, the last age with the ep_id of age j, is found for every sample.
 *   Window: length = min(L, j_end - j + 1); step k < length is age j + k.  A window never leaves its episode and never passes the
 *     ring's newest step.
 *   Goal: goal = relabel ? achieved_next[j_goal] : desired[j] - one goal for the whole window.
 *   Copied rows: obs, act, next_obs, achieved_next of step k are the rows of (e, slot(j + k)) as stored, moved as 32-bit patterns.
 *   Reward and done of step k: not relabelled: as stored.  Relabelled: reach = norm(achieved_next[j + k] - goal) < geofence, the
 *     expression of hsr_replay_sample_dev; reward = float(reach), done = reach.
 *   Padding: steps k >= length are written as zero words in every per-step output (obs, act, next_obs, achieved_next, reward, done).
 *   n-step: m = the smallest k + 1 with done_k != 0 over k < length, else length.  acc = 0, g = 1; for k = 0 .. m-1: acc = acc + g reward_k,
 *     then g = g gamma - every product and every sum a float32 operation of its own.  nstep = m, nstep_return = acc, nstep_discount = g
 *     (gamma^m), nstep_obs = next_obs[j + m - 1], nstep_done = done_{m-1}.  A window cut by the time limit, by L or by the ring's newest
 *     step ends with nstep_done = 0: record stores the terminal observation as next_obs, so the caller bootstraps from nstep_obs,
 *     target = nstep_return + nstep_discount (1 - nstep_done) V(nstep_obs, goal).
 *   index[i] = (e, slot(j), relabelled ? slot(j_goal) : -1, relabelled), as hsr_replay_sample_dev gives it for the window's first step.
 *   L = 1: the window equals hsr_replay_sample_dev with the same draw, bit for bit; for rewards 0 / 1, nstep_return = reward and
 *     nstep_discount = gamma.
 * Every pointer of `out` may be NULL.  The call is asynchronous on the batch stream, never writes the ring or the batch and allocates
 * nothing.  HSR_EINVAL (nothing launched, outputs untouched): everything hsr_replay_sample_dev refuses; out == NULL; seq_len < 1 or
 * seq_len > capacity_steps; gamma not finite or outside [0, 1]; batch * seq_len >= 2^31. */
typedef struct hsr_replay_seq_out {      /* device pointers, each may be NULL; L = seq_len */
    float *obs;            /* [batch, L, obs_dim] */
    float *act;            /* [batch, L, nu] */
    float *next_obs;       /* [batch, L, obs_dim] */
    float *achieved_next;  /* [batch, L, 3] */
    float *goal;           /* [batch, 3]  one goal per window */
    float *reward;         /* [batch, L] */
    uint8_t *done;         /* [batch, L] */
    int32_t *length;       /* [batch]  valid steps, 1..L */
    int32_t *nstep;        /* [batch]  m, 1..length */
    float *nstep_return;   /* [batch] */
    float *nstep_discount; /* [batch]  gamma^m */
    float *nstep_obs;      /* [batch, obs_dim]  next_obs of step m-1 */
    uint8_t *nstep_done;   /* [batch]  done of step m-1 */
    int32_t *index;        /* [batch, 4]  as hsr_replay_sample_dev, for the window's first step */
} hsr_replay_seq_out;
int  hsr_replay_sample_seq_dev(hsr_replay *r, uint32_t draw, int batch, int seq_len, float her_ratio, float gamma,
                               const hsr_replay_seq_out *out);
/* Prioritised replay (Schaul et al., "Prioritized Experience Replay", ICLR 2016): an opt-in sum tree over the ring's cells, a stratified
 * sampler that draws a cell with probability priority / total, and updates from the learner's TD errors.  A replay that never calls
 * hsr_replay_priority_enable allocates nothing more and behaves as above, bit for bit; hsr_replay_sample_dev and
 * hsr_replay_sample_seq_dev stay the uniform functions on a replay with priorities.
 *   Cells and leaves: a cell is (slot, env); its leaf has index c = slot N + e (env fastest: one record touches one contiguous run of N
 *     leaves) and holds a float32 priority; a cell without a stored transition has leaf 0.
 *   Tree: logically a complete binary tree over 2^h >= T N leaves, absent leaves 0; every inner node is left + right as ONE float64
 *     addition of its children (leaves widened exactly).  The shape is fixed, so every node - and total, the root - is a function of the
 *     leaves alone; there are no floating-point atomics.  (Stored: every sixth level; the levels between are rebuilt where needed.)
 *   Descent for a target u >= 0 (float64): at a node with children (l, r) go left if u < l or r == 0, else u = u - l and go right.  With
 *     total > 0 the leaf reached has a positive priority for every u, u == total included.
 *   Draw: sample i of draw `draw` takes the Philox block of stream 6 - key as above, counter (i, draw, 6, env_offset).
 *     r = ((word0 >> 5) 2^26 + (word1 >> 6)) 2^-53; u = ((double)i + r) / (double)batch, then u = u total (stratified; each operation a
 *     float64 operation of its own).  The leaf reached gives (e, slot); its age is j = (slot - first + T) mod T with first = slot(0).
 *     From there on the sample is hsr_replay_sample_dev's: relabel from word2, j_goal from word3 and j_end, rows moved as 32-bit
 *     patterns, the relabelled reward by the same goal test, d_index with the same meaning.  d_prob[i] = (float)((double)leaf / total).
 *   New transitions: record sets the N leaves of the slot it writes to p_new and re-sums their ancestors.  p_new = p_init at first and
 *     after clear, then the running maximum of p_init and every priority an update has stored.  clear zeroes the tree.
 *   Update (sampled_at, batch, d_index [batch,4], d_priority [batch]): only index[:,0] = e and index[:,1] = slot are read.  The value
 *     stored is d_priority clamped into [p_min, p_max], NaN as p_max.  When several rows name one cell the largest clamped value wins,
 *     whatever the order of the rows.  Ancestors are re-summed from their children.  Skipped silently: a row with e or slot out of range,
 *     a cell that holds no transition, a stale cell.  Staleness: W = pushed + (a record is pending); k_s = the largest k < W with k mod T
 *     == slot; the cell is live for the token iff k_s exists and k_s < sampled_at.  sampled_at is the 64-bit `pushed` at the time of the
 *     sample (hsr_replay_priority_state).
 *   hsr_replay_priority_sample_seq_dev: priority and d_prob are those of the window's first step, everything else is
 *     hsr_replay_sample_seq_dev; with L = 1 it equals hsr_replay_priority_sample_dev bit for bit.
 * All calls but hsr_replay_priority_state are asynchronous on the batch stream; nothing is allocated after enable (max_batch sizes the
 * per-sample scratch the replay owns).  HSR_EINVAL, nothing launched: priorities not enabled; the batch destroyed; for the samplers
 * everything the uniform twin refuses (a pending record, count == 0, batch < 1, ..); batch > max_batch; update: count == 0, batch < 1, a
 * NULL array, sampled_at > pushed; enable: not in the EMPTY state, enabled already, a non-finite value, not 0 < p_min <= p_init <= p_max,
 * max_batch < 1, T N > 2^30. */
typedef struct hsr_priority_spec {
    float   p_init;        /* priority of a new transition until an update stores a larger one */
    float   p_min, p_max;  /* stored priorities are clamped into [p_min, p_max]; p_min > 0 keeps every stored transition reachable */
    int32_t max_batch;     /* largest batch of a prioritised sample or update */
} hsr_priority_spec;
int  hsr_replay_priority_enable(hsr_replay *r, const hsr_priority_spec *spec);
int  hsr_replay_priority_state(hsr_replay *r, uint64_t *pushed, double *total, float *p_new);   /* synchronises the stream; each may be NULL */
int  hsr_replay_priority_sample_dev(hsr_replay *r, uint32_t draw, int batch, float her_ratio,
                                    float *d_obs, float *d_act, float *d_next_obs, float *d_goal, float *d_achieved_next,
                                    float *d_reward, uint8_t *d_done, int32_t *d_index /*[batch,4]*/, float *d_prob /*[batch]*/);
int  hsr_replay_priority_sample_seq_dev(hsr_replay *r, uint32_t draw, int batch, int seq_len, float her_ratio, float gamma,
                                        const hsr_replay_seq_out *out, float *d_prob /*[batch]*/);
int  hsr_replay_priority_update_dev(hsr_replay *r, uint64_t sampled_at, int batch, const int32_t *d_index /*[batch,4]*/, const float *d_priority /*[batch]*/);
int  hsr_replay_priority_read_dev(hsr_replay *r, float *d_leaves /*[T,N]*/);                     /* the leaves, for tests and checkpoints */

/* ---- on-policy rollouts on the device: a rollout store, GAE with the time-limit bootstrap, advantage statistics, shuffled minibatches ----
 * Opt-in; the on-policy twin of the replay above (PPO / A2C on a batch of lock-stepped envs).  Ownership as for the replay: a rollout is
 * bound to the batch that made it and launches on hsr_batch_stream(); its storage goes with hsr_rollout_destroy, or with hsr_batch_destroy
 * of its batch, whichever is first: after the latter the handle is still the caller's to destroy, and every other use returns HSR_EINVAL.
 * A batch that never creates one allocates nothing.  A rollout reads nothing of the batch but N, nu and the stream, and is NOT part of an
 * env record: after hsr_batch_snapshot_load* / hsr_batch_copy_envs* start it again with hsr_rollout_begin_dev.
 *
 * Storage for T = horizon steps of N envs: rows [T][N] of obs | act (obs_dim + nu words, padded to a multiple of 4); planes [T][N], env
 * fastest, of logp, value, reward, kind, v_term, adv, ret; a head row [N][obs_dim]: the observation the policy acts on next.
 * Rows and scalars move as 32-bit patterns (NaN payloads and -0 survive).
 * Protocol (host state machine EMPTY, READY(t), STAGED, DONE; a call out of order returns HSR_EINVAL, launches nothing and leaves books and
 * storage as they were):
 *   begin(d_obs [N,obs_dim])    any state -> READY(0); head = d_obs
 *   stage(d_act [N,nu], d_logp [N], d_value [N])    READY(t < T) -> STAGED; slot t: obs = head, act, logp, value
 *   close(d_reward [N], d_kind [N], d_next_obs [N,obs_dim])    STAGED -> READY(t + 1); slot t: reward, kind, v_term = 0; head = d_next_obs.
 *     d_kind is what hsr_batch_episode_end_dev writes: 0 the episode goes on; 2 it was cut by the time limit: GAE bootstraps from v_term;
 *     any other value: terminal, no bootstrap.
 *   bootstrap(d_value_terminal [N])    READY(t >= 1), state unchanged: v_term of slot t - 1 = d_value_terminal (the critic's value of the
 *     terminal observation; read only where kind == 2); the last call wins.  A truncated step whose bootstrap was never called bootstraps
 *     from 0.
 *   finish(d_last_value [N] = V(head))    READY(T) -> DONE: GAE and the statistics below
 *   next    DONE -> READY(0); the head row stays
 *   minibatch, stats, planes    only in DONE
 * GAE, per env, t = T-1 .. 0, every operation one float32 operation rounded on its own (no fma); gl = (float)gamma * (float)lam in float32:
 *   nv    = kind[t] == 0 ? (t == T-1 ? last_value : value[t+1]) : kind[t] == 2 ? v_term[t] : 0
 *   delta = (reward[t] + gamma nv) - value[t]
 *   carry = (kind[t] == 0 && t < T-1) ? adv[t+1] : 0
 *   adv[t] = delta + gl carry;   ret[t] = adv[t] + value[t]
 * Statistics over all M = T N advantages, in fp64 with a fixed reduction shape (the same inputs give the same bits):
 *   mean = sum(adv) / M;  var = sum((adv - mean)^2) / M (a second pass);  std = sqrt(var);  rstd = 1 / (std + 1e-8)
 * each kept as the float32 rounding of its fp64 value.
 * Shuffle of epoch `epoch`: a stateless bijection of [0, M), a four-round Feistel network with cycle walking.  Round keys k[0..3] = the
 * Philox4x32-10 block of key (seed & 0xffffffff, seed >> 32), counter (epoch, 0, 5, env_offset).  bits = bit length of M - 1,
 * h = max(1, (bits + 1) / 2), mask = 2^h - 1.  perm(i): x = i; repeat { L = x >> h, R = x & mask; for k in k[0..3]: (L, R) = (R, L ^ F(R, k));
 * x = L << h | R } until x < M.  F(v, k) in uint32: v ^= k; v *= 0x9E3779B1; v ^= v >> 15; v *= 0x85EBCA77; v ^= v >> 13; return v & mask.
 * minibatch(epoch, first, count, normalize, outputs): row i < count is element p = perm(first + i), t = p / N, e = p % N, of the store:
 *   d_obs [count,obs_dim], d_act [count,nu], d_logp, d_value, d_ret [count] as stored; d_adv = normalize ? (adv - mean32) rstd32 (two
 *   float32 operations) : adv; d_index [count,2] = (t, e).  Every output may be NULL; nothing is written past row count - 1.
 *   HSR_EINVAL: count < 1, first < 0, first + count > M. */
typedef struct hsr_rollout hsr_rollout;
typedef struct hsr_rollout_spec {
    uint64_t seed;
    uint32_t env_offset;      /* as in hsr_episode_spec: salts the shuffle of a shard */
    int32_t  horizon;         /* T: env-steps per rollout */
    int32_t  obs_dim;         /* floats per observation row the caller will hand over (nq+nv, or 25 for 'openai') */
    float    gamma;
    float    lam;
} hsr_rollout_spec;
/* HSR_EINVAL (nothing allocated): a NULL argument, horizon < 1, obs_dim < 1 or above 2^20, gamma or lam not finite or outside [0, 1],
 * T N >= 2^31, storage beyond 2^40 bytes.  HSR_EDEVICE: no device memory; what was allocated is freed. */
int  hsr_batch_rollout_create(hsr_batch *b, const hsr_rollout_spec *spec, hsr_rollout **out);
void hsr_rollout_destroy(hsr_rollout *r);
int  hsr_rollout_begin_dev(hsr_rollout *r, const float *d_obs);
int  hsr_rollout_stage_dev(hsr_rollout *r, const float *d_act, const float *d_logp, const float *d_value);
int  hsr_rollout_close_dev(hsr_rollout *r, const float *d_reward, const uint8_t *d_kind, const float *d_next_obs);
int  hsr_rollout_bootstrap_dev(hsr_rollout *r, const float *d_value_terminal);
int  hsr_rollout_finish_dev(hsr_rollout *r, const float *d_last_value);
int  hsr_rollout_next(hsr_rollout *r);
int  hsr_rollout_state(hsr_rollout *r, int32_t *state, int32_t *t); /* host books, no device work: 0 EMPTY, 1 READY, 2 STAGED, 3 DONE; steps closed */
int  hsr_rollout_stats(hsr_rollout *r, float *mean, float *std, float *rstd); /* waits for the stream */
int  hsr_rollout_minibatch_dev(hsr_rollout *r, uint32_t epoch, int first, int count, int normalize,
                               float *d_obs, float *d_act, float *d_logp, float *d_value, float *d_adv, float *d_ret, int32_t *d_index /*[count,2]*/);
int  hsr_rollout_planes_dev(hsr_rollout *r, float *d_adv, float *d_ret); /* [T,N] copies of the advantage and return planes */

/* ---- running mean / std normalisation of rows on the device: fp64 moments, float32 publish, clipped apply ----
 * Opt-in; what a learner puts between the env's rows (or a sampled batch) and its networks.  Ownership as for the rollout: a normaliser is
 * bound to the batch that made it and launches on hsr_batch_stream(); its storage goes with hsr_norm_destroy, or with hsr_batch_destroy of
 * its batch, whichever is first: after the latter the handle is still the caller's to destroy, and every other use returns HSR_EINVAL.
 * A batch that never creates one allocates and launches nothing.  A normaliser reads nothing of the batch but the stream, and is NOT part
 * of an env record: hsr_batch_snapshot_load* / hsr_batch_copy_envs* leave it alone (its statistics are the learner's, not the envs').
 *
 * State for dim columns: count (fp64, exact: whole numbers below 2^53), mean[dim] and m2[dim] (fp64), the published float32 mean32[dim]
 * and rstd32[dim], and skipped (uint64).
 * update(rows [n, dim] float32 with a row stride in floats, mask uint8 [n] or NULL): a row is selected if its mask byte is non-zero (no
 *   mask: every row); a selected row counts if all its dim values are finite, else it is left out and adds 1 to skipped (a row the mask
 *   does not select is neither).  Of the m rows that count: mean_b = sum(x) / m, m2_b = sum((x - mean_b)^2) (a second pass), in fp64, then
 *   Chan's rule: delta = mean_b - mean; tot = count + m; mean += delta m / tot; m2 += m2_b + delta^2 count m / tot; count = tot.
 *   m == 0 leaves count, mean, m2 and the published vectors as they were, bit for bit.  Every sum has a shape fixed by (n, dim) alone
 *   (csrc/normalize.h states it); rows left out add +0.0 in place, so the same rows in the same places give the same bits whatever else
 *   the array held.  No atomics.
 * publish, after every update, clear and set_state: std = sqrt(max(m2 / count, eps^2)); mean32 = (float)mean; rstd32 = (float)(1 / std);
 *   count == 0: mean32 = 0, rstd32 = 1.
 * apply: y = clamp((x - mean32) rstd32, -clip, clip): a float32 subtraction and a float32 product, each rounded on its own (no fma), then
 *   y > clip ? clip : y < -clip ? -clip : y, so a NaN stays a NaN.  In place (d_out == d_in with equal strides) or out of place.
 * apply_batch: up to 8 contiguous tensors of rows in place in ONE launch, each with the statistics of `obs` (which == 0) or `goal`
 *   (which == 1).  rows = all rows of the tensor; a tensor of windows has seq_len > 1 rows per window, and with d_length [rows / seq_len]
 *   the rows at and past a window's length are left as they are (padding stays zero).
 * Every *_dev call is asynchronous on the batch's stream, with one exception: an update whose n is larger than that of every update
 * before it (the first one included) waits for the stream and allocates its partial sums anew; updates of a size seen before allocate
 * and wait for nothing.  HSR_EINVAL (nothing launched): dim outside 1..1024; eps <= 0 or not finite;
 * clip <= 0 or not finite; n < 0; a row stride below dim; set_state with a negative or non-finite count or m2 or a non-finite mean; an
 * item with rows < 0, seq_len < 1 or rows no multiple of seq_len, or with which outside {0, 1}. */
typedef struct hsr_norm hsr_norm;
typedef struct hsr_norm_item {
    float   *d_rows;          /* [rows, dim of its normaliser], contiguous, normalised in place */
    int64_t  rows;
    int32_t  seq_len;         /* 1: plain rows; L: windows of L rows, cut by d_length */
    int32_t  which;           /* 0: the obs normaliser, 1: the goal normaliser */
} hsr_norm_item;
int  hsr_batch_norm_create(hsr_batch *b, int dim, float eps, float clip, hsr_norm **out);
void hsr_norm_destroy(hsr_norm *r);
int  hsr_norm_clear(hsr_norm *r);                         /* count = 0, mean = m2 = 0, skipped = 0; publishes the identity */
int  hsr_norm_update_dev(hsr_norm *r, const float *d_rows, int stride, const uint8_t *d_mask, int n);
int  hsr_norm_apply_dev(hsr_norm *r, const float *d_in, int in_stride, float *d_out, int out_stride, int n);
int  hsr_norm_apply_batch_dev(hsr_norm *obs, hsr_norm *goal, const hsr_norm_item *items, int n_items, const int32_t *d_length);
int  hsr_norm_state(hsr_norm *r, double *count, double *mean /*[dim]*/, double *m2 /*[dim]*/, uint64_t *skipped); /* waits for the stream; each may be NULL */
int  hsr_norm_set_state(hsr_norm *r, double count, const double *mean, const double *m2, uint64_t skipped);      /* republishes */
int  hsr_norm_published_dev(hsr_norm *r, float *d_mean32 /*[dim]*/, float *d_rstd32 /*[dim]*/);                    /* either may be NULL */

/* ---- planning on the device: a cross-entropy-method (CEM) controller over forked envs ----
 * Opt-in.  The simulator is the model: fork the current state K times (hsr_batch_snapshot_save_dev / _load_dev above), try K action
 * sequences over H env-steps, keep the good ones, refit, repeat.  A planner works on a PLANNING batch, a second batch of the same model on
 * the same device with N = P K envs: it plans for P acting envs ("groups") with K candidates each, candidate k of group p = env p K + k.
 * The acting batch is never touched by a planner; it is only read, by the caller, through a snapshot.  Ownership as for the replay and the
 * normaliser: a planner is bound to the (planning) batch that made it and launches on hsr_batch_stream(); its storage goes with
 * hsr_plan_destroy, or with hsr_batch_destroy of its batch, whichever is first: after the latter the handle is still the caller's to destroy,
 * and every other use returns HSR_EINVAL.  A batch that never creates one allocates and launches nothing.  Not part of an env record.
 *
 * State: mean, sigma float32 [P][H][nu]; per candidate the cost J and the discount g (float32), alive (u8), reach_step (int32, -1 = the
 * goal was not reached); per group failed (u32: updates that found no finite cost) and the index and cost of the best candidate of the
 * last update.  The actions as sampled are kept, float32 [P][H][nu][K], for the refit.  A new planner is reset and begun.
 * The range of actuator a: (lo, hi) = its ctrlrange, a side without a limit (not finite, or the compiled models' marker 1e30) counts as
 * -1 / +1, the convention of hsr_batch_sample_ctrl_dev; half_range = (hi - lo) 0.5, a float32 difference and a float32 product.
 *   reset(d_mask [P] or NULL = all): mean <- clamp(0, lo, hi), sigma <- init_std half_range (a float32 product), for the masked groups.
 *   shift(d_mask or NULL): mean[h] <- mean[h + 1], the last step repeats; sigma <- its initial value as in reset.
 *   begin: J = 0, g = 1, alive = 1, reach_step = -1 for every candidate; once per iteration, after the candidates were loaded.
 *   sample(call, iter, h, d_ctrl [N][nu]): ctrl = clamp(mean[p][h][a] + sigma[p][h][a] z, lo, hi), a float32 product and a float32 sum each
 *     rounded on its own, clamp(x) = x < lo ? lo : x > hi ? hi : x.  Candidate 0 takes z = 0: the current mean is always a candidate.
 *     Otherwise z is the Irwin-Hall normal of ONE Philox block (no logf / cosf: bit-reproducible): u_i = (w_i >> 8) 2^-24,
 *     z = (((u0 + u1) + (u2 + u3)) - 2) (float)sqrt(3), every operation a float32 operation of its own; |z| <= 2 sqrt(3).
 *     Key (seed & 0xffffffff, seed >> 32), counter (env_offset + p, call 256 + iter, 7, (k H + h) nu + a): stream 7.  iter is in 0..255.
 *   accumulate(h), after hsr_batch_step_dev of step h, for a live candidate, every operation a float32 operation of its own:
 *     d = sqrt((dx dx + dy dy) + dz dz) of xpos(goal_body) - mocap_pos (xpos as hsr_batch_body_xpos gives it; an IEEE square root).  This is
 *     the expression of the env-step's goal test without its contractions and with an exact square root, so the two distances may differ in
 *     the last bit; `done` is the step's own.  If the env is bad (hsr_batch_bad_state): J = +inf, alive = 0.  Else J = J + g d, then
 *     g = g gamma, and if the step latched done: alive = 0, reach_step = h - the rest of the horizon costs nothing.
 *   add_cost(d_extra [N]): J = J + extra for every candidate; the hook for a learned terminal value.
 *   update, one workgroup per group: key = J, a NaN or an infinity of either sign counting as +inf (by the bits).
 *     rank(k) = #{ j : key_j < key_k or (key_j == key_k and j < k) }; E' = min(elites, number of finite costs); k is elite iff rank(k) < E'.
 *     best index = the candidate of rank 0, best cost = its key (candidate 0 and +inf when no cost is finite).
 *     E' == 0: mean and sigma stay bit for bit, failed += 1.  Otherwise per (h, a), over the actions x as sampled, in fp64:
 *       m = (sum over elites of x) / E';  v = (sum over elites of (x - m)^2) / E' (a second pass; the difference and the square each rounded);
 *       mean <- (float)(mean + alpha (m - mean));  sigma <- (float)max(sigma + alpha (sqrt(v) - sigma), min_std half_range[a]), every
 *       operation a double operation of its own (alpha, min_std, half_range, mean, sigma widened exactly).
 *     Both sums run over all K leaves, candidate k at leaf k, a non-elite adding +0.0 in place, in a tree whose shape depends on K only:
 *       lane l of 64 adds the leaves l, l + 64, l + 128, .. serially from 0.0 in this order; then the 64 lane values are added in the tree
 *       v[l] += v[l + off] for off = 32, 16, 8, 4, 2, 1, the sum being lane 0's.  A chain is at most ceil(K / 64) + 6 additions long.
 *   action(d_ctrl [P][nu]): mean[p][0].
 *   readers: costs (J [N], reach_step [N]), state (mean, sigma), best (index [P], cost [P]) copy on the stream, each output may be NULL;
 *     failed copies to the host and waits for the stream.
 * All _dev calls are asynchronous on the planning batch's stream.  No atomics anywhere.  HSR_EINVAL, nothing launched and everything as it
 * was: create with a NULL argument, a model without actuators, samples outside 2..1024, envs != groups samples, horizon outside 1..64,
 * elites outside 1..samples, a goal_body out of range or the mocap body, a batch with extra goal terms (hsr_batch_set_goals with n > 0: a
 * cost of several terms cannot be computed from one goal point; accumulate refuses likewise when terms were set later), gamma outside
 * [0, 1], alpha outside (0, 1], init_std or min_std not finite or <= 0, samples horizon nu >= 2^32; sample with iter outside 0..255, h
 * outside 0..H-1 or a NULL d_ctrl; accumulate with h outside 0..H-1; add_cost, action, failed with a NULL array.
 * geofence is what the caller hands to hsr_batch_step_dev of the planning batch: it is part of the spec for the layers above, the
 * library neither checks nor reads it. */
typedef struct hsr_plan hsr_plan;
typedef struct hsr_plan_spec {
    uint64_t seed;
    uint32_t env_offset;      /* as in hsr_episode_spec: global id of group 0, so a shard draws what the single batch draws for the same envs */
    int32_t  groups;          /* P */
    int32_t  samples;         /* K */
    int32_t  horizon;         /* H */
    int32_t  elites;
    int32_t  goal_body;
    float    geofence;
    float    gamma;
    float    alpha;
    float    init_std;
    float    min_std;
} hsr_plan_spec;
int  hsr_batch_plan_create(hsr_batch *b, const hsr_plan_spec *spec, hsr_plan **out);
void hsr_plan_destroy(hsr_plan *r);
int  hsr_plan_reset_dev(hsr_plan *r, const uint8_t *d_mask);
int  hsr_plan_shift_dev(hsr_plan *r, const uint8_t *d_mask);
int  hsr_plan_begin_dev(hsr_plan *r);
int  hsr_plan_sample_dev(hsr_plan *r, uint32_t call, int iter, int h, float *d_ctrl);
int  hsr_plan_accumulate_dev(hsr_plan *r, int h);
int  hsr_plan_add_cost_dev(hsr_plan *r, const float *d_extra);
int  hsr_plan_update_dev(hsr_plan *r);
int  hsr_plan_action_dev(hsr_plan *r, float *d_ctrl);
int  hsr_plan_costs_dev(hsr_plan *r, float *d_cost /*[N]*/, int32_t *d_reach_step /*[N]*/);
int  hsr_plan_state_dev(hsr_plan *r, float *d_mean /*[P,H,nu]*/, float *d_sigma /*[P,H,nu]*/);
int  hsr_plan_best_dev(hsr_plan *r, int32_t *d_index /*[P]*/, float *d_cost /*[P]*/);
int  hsr_plan_failed(hsr_plan *r, uint32_t *failed /*[P]*/);

/* diagnostics (meaningful only in the -DHSR_PHASE_TIMING build, libhsrsim_timing.so; tools/phase_timing.py,
 * tools/block_times.py): per-phase cycle sums of the last launches, and per-workgroup
 * {start, end (s_memrealtime), HW_ID, XCC_ID, Newton trips, sphere-cull candidates, work items, rows} */
int hsr_batch_phase_cycles(hsr_batch *b, unsigned long long *out /*[32]*/);
int hsr_batch_block_times(hsr_batch *b, unsigned long long *out /*[nblocks,40]: 8 header words + 26 phase cycle sums*/, int nblocks);

#ifdef __cplusplus
}
#endif
#endif /* HSRSIM_H */
