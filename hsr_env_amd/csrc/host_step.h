// Stepping: one substep of the per-substep chain, forward, reset, and the env-step (hsr_batch_step*) on the persistent kernel or the chain.

// one substep of the per-substep chain = 4 launches on the batch stream (the persistent kernel needs none of them)
static void launch_substep(hsr_batch *b, int mode, int goal_body, float geofence, int debug, hipStream_t st, bool timed, int sub = -1) {
    const int N = b->N;
    auto rec = [&](void) { if (timed) { hipEvent_t ev; hipEventCreate(&ev); hipEventRecord(ev, st); b->kev.push_back(ev); } };
    rec();
    hipLaunchKernelGGL(k_kinematics, dim3((N + 63) / 64), dim3(64), (size_t)64 * (b->ds.kstride + 24 * b->dm.nlink + 1) * sizeof(float), st, b->dm, b->ds);
    if (sub >= 0 && b->cap_every > 0 && sub % b->cap_every == 0)
        hipLaunchKernelGGL(k_capture, grid1((size_t)12 * b->dm.nlink * b->cap_n), dim3(256), 0, st, b->ds, b->dm.nlink, (const int *)b->d_cap_env, b->cap_n, b->d_cap,
                           sub / b->cap_every, 1, b->cap_every, (int *)nullptr);
    rec();
    if (b->dm.npair > 0) {
        hipLaunchKernelGGL(k_cull, dim3((N + 63) / 64, (b->dm.npair + b->pairs_per_wave - 1) / b->pairs_per_wave), dim3(64), 0, st, b->dm, b->ds);
        hipLaunchKernelGGL(k_narrow, dim3(b->narrow_blocks), dim3(64), 0, st, b->dm, b->ds);
    }
    rec();
    by_group(b->group, [&](auto g) {       // one wave per 64 / lanes-per-env envs
        hipLaunchKernelGGL(k_solve_mf<decltype(g)::value>, dim3((N * g() + 63) / 64), dim3(64), b->mf_lds_bytes, st, b->dm, b->ds,
                           mode, goal_body, geofence, debug);
    });
    rec();
}

extern "C" int hsr_batch_forward(hsr_batch *b) {
    ENTER_DEV(b);
    hipLaunchKernelGGL(k_clear_done, grid1(b->N), dim3(256), 0, b->stream, b->ds);
    launch_substep(b, 0, -1, 0.f, 1, b->stream, false);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(b->stream));
    return HSR_OK;
}

extern "C" int hsr_batch_reset(hsr_batch *b, const uint8_t *mask, const float *qpos0, const float *mocap) {
    ENTER_DEV(b);
    const size_t N = b->N;
    const int nq = b->dm.nq;
    float *d_q = nullptr, *d_m = nullptr, *d_q0m = b->d_qpos0;
    size_t off = 0;
    if (qpos0) { d_q = b->d_stage + off; off += N * nq; HIPCHK(hipMemcpyAsync(d_q, qpos0, N * nq * sizeof(float), hipMemcpyHostToDevice, b->stream)); }
    if (mocap) { d_m = b->d_stage + off; off += N * 3; HIPCHK(hipMemcpyAsync(d_m, mocap, N * 3 * sizeof(float), hipMemcpyHostToDevice, b->stream)); }
    if (off > b->stage_floats) return fail(HSR_EINVAL, "staging overflow in reset");
    if (mask) HIPCHK(hipMemcpyAsync(b->d_stage_u8, mask, N, hipMemcpyHostToDevice, b->stream));
    hipLaunchKernelGGL(k_reset, grid1(N), dim3(256), 0, b->stream, b->dm, b->ds, mask ? (const uint8_t *)b->d_stage_u8 : (const uint8_t *)nullptr,
                       (const float *)d_q, (const float *)d_q0m, (const float *)d_m, mask ? 1 : 0);
    // the forward pass concerns the reset envs only (MujocoEnv.reset() touches one env, hsr/mujoco_env.py:83-85): with a mask the
    // others stay parked as "done" for that pass, as in hsr_batch_reset_dev
    launch_substep(b, 0, -1, 0.f, 1, b->stream, false);
    hipLaunchKernelGGL(k_clear_done, grid1(N), dim3(256), 0, b->stream, b->ds);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(b->stream));
    return HSR_OK;
}

// the forward pass after a masked reset concerns the reset envs only (the reference's reset() touches one env): the others are
// parked as "done" for that pass by k_reset, so its kernels skip them (whole waves return when none of their envs was reset)
// device-pointer reset: envs with d_mask[e] != 0 (or, when d_mask == NULL, the envs whose done flag was
// latched by the last step) restart from d_qpos0[e] / d_mocap[e]; asynchronous; followed by forward.
extern "C" int hsr_batch_reset_dev(hsr_batch *b, const uint8_t *d_mask, const float *d_qpos0, const float *d_mocap) {
    ENTER_DEV(b);
    const size_t N = b->N;
    // k_reset with park = 1 does all three jobs in one launch: mask = done flags (d_mask == NULL), reset of the masked envs, and the
    // unmasked ones parked as "done" for the forward pass that follows
    hipLaunchKernelGGL(k_reset, grid1(N), dim3(256), 0, b->stream, b->dm, b->ds, d_mask, d_qpos0, (const float *)b->d_qpos0, d_mocap, 1);
    launch_substep(b, 0, -1, 0.f, 0, b->stream, false);
    hipLaunchKernelGGL(k_clear_done, grid1(N), dim3(256), 0, b->stream, b->ds);
    HIPCHK(hipGetLastError());
    return HSR_OK;
}
// the capture buffer of a step with cap_rows rows per slot: grown after the stream has let go of the old one; a new buffer holds NaN
static int grow_capture(hsr_batch *b, int cap_rows) {
    const size_t need = (size_t)cap_rows * 12 * b->dm.nlink * b->cap_n;
    if (need <= b->cap_floats) return HSR_OK;
    HIPCHK(hipStreamSynchronize(b->stream));
    if (b->d_cap) { HIPCHK(hipFree(b->d_cap)); b->d_cap = nullptr; b->cap_floats = 0; }
    HIPCHK(hipMalloc(&b->d_cap, need * sizeof(float)));
    HIPCHK(hipMemsetD32Async((hipDeviceptr_t)b->d_cap, 0x7fc00000, need, b->stream));
    b->cap_floats = need;
    return upload_capture_desc(b, b->cap_every, b->cap_n);
}

// (how one env-step runs on the persistent kernel is decided by plan_launch, launch_plan.h: pure arithmetic that a host program tests)

// the whole env-step in one launch of the persistent kernel: it reads ctrl and writes obs / reward / done / nsteps itself
static int launch_persistent(hsr_batch *b, const StepIO &io, int n_substeps, int goal_body, float geofence) {
    hipStream_t st = b->stream;
    if (b->profiling) { hipEvent_t ev; for (int k = 0; k < 3; k++) { hipEventCreate(&ev); hipEventRecord(ev, st); b->kev.push_back(ev); } }
    if (!b->d_dm) {
        const int rc = upload(b, &b->d_dm, &b->dm, 1);
        if (rc) return rc;
    }
    if (b->schedule)
        hipLaunchKernelGGL(k_schedule, dim3((b->N + SCHED_CHUNK - 1) / SCHED_CHUNK), dim3(1024), 0, st, b->ds, 64 / b->group, b->d_slot_env);
    const PersistLaunch p = plan_launch(b->N, b->group, b->slots, n_substeps, b->queue, b->queue_chunk, b->queue_chunk_set,
                                        b->solo_servers, b->solo_trips, b->kernel_sv != nullptr, b->schedule,
                                        SplitSettings{b->split, b->split_inst, b->split_period, b->split_trips, b->split_min_left, b->split_extra,
                                                      b->split_lone, b->split_lone_trips});
    DevState dsl = b->ds;
    b->handovers_counted = p.rounds > 0 || p.split.on;
    dsl.slot_env = b->schedule ? b->d_slot_env : nullptr;
    dsl.solo_servers = p.solo_servers;
    if (p.solo_servers > 0) { dsl.solo_trips_x4 = p.solo_trips_x4; dsl.solo_min_left = p.solo_min_left; }
    if (p.rounds > 0) {
        dsl.q_chunk = p.chunk;
        hipLaunchKernelGGL(k_queue_init, grid1((size_t)p.rounds * p.tasks), dim3(256), 0, st, dsl, p.tasks, p.rounds);
    }
    if (p.split.on) {
        dsl.split_period = p.split.period; dsl.split_trips_x4 = p.split.trips_x4; dsl.split_min_left = p.split.min_left;
        dsl.split_lone_x4 = p.split.lone_x4;
        hipLaunchKernelGGL(k_split_init, dim3(8), dim3(256), 0, st, dsl);
    }
    hipEvent_t k0 = nullptr, k1 = nullptr;
    if (b->kernel_log) { hipEventCreate(&k0); hipEventCreate(&k1); hipEventRecord(k0, st); }
    const int debug = (b->debug_store ? 1 : 0) | (b->test_hooks & ~32) | (b->mpr_warm ? 0 : 8);
    hipLaunchKernelGGL(p.solo_servers > 0 ? b->kernel_sv : b->kernel, dim3(p.grid), dim3(64), b->persist_lds_bytes, st,
                       (const DevModel *)b->d_dm, dsl, n_substeps, goal_body, geofence, debug, io);
    if ((b->test_hooks & 32) && b->ds.q_err) HIPCHK(hipMemsetD32Async((hipDeviceptr_t)b->ds.q_err, 1, 1, st));      // tests: what q_claim's watchdog does when a ticket is never served
    if (b->kernel_log) { hipEventRecord(k1, st); b->klog.push_back({k0, k1}); }
    if (b->profiling) { hipEvent_t ev; hipEventCreate(&ev); hipEventRecord(ev, st); b->kev.push_back(ev); }   // slots 0,1 empty; slot 2 = the persistent kernel
    return HSR_OK;
}
// the env-step as the per-substep chain, replayed from a captured graph (cached per GraphKey) unless profiling times every launch
static int launch_chain(hsr_batch *b, int n_substeps, int goal_body, float geofence) {
    hipStream_t st = b->stream;
    if (!b->use_graph || b->profiling || n_substeps <= 0) {
        for (int i = 0; i < n_substeps; i++) launch_substep(b, 1, goal_body, geofence, 0, st, b->profiling, i);
        return HSR_OK;
    }
    GraphKey key{n_substeps, goal_body, geofence, b->cap_every, b->cap_n, b->d_cap};
    auto it = b->graphs.find(key);
    if (it == b->graphs.end()) {
        hipGraph_t graph;
        HIPCHK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
        for (int i = 0; i < n_substeps; i++) launch_substep(b, 1, goal_body, geofence, 0, st, false, i);
        HIPCHK(hipStreamEndCapture(st, &graph));
        hipGraphExec_t exec;
        HIPCHK(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
        hipGraphDestroy(graph);
        if (b->graphs.size() >= 8) { for (auto &kv : b->graphs) hipGraphExecDestroy(kv.second); b->graphs.clear(); }
        it = b->graphs.emplace(key, exec).first;
    }
    HIPCHK(hipGraphLaunch(it->second, st));
    return HSR_OK;
}
// hsr_batch_set_profiling(b, 1): wait for the step and sum the event intervals per kernel slot (kinematics, collide, solve)
static int finish_profiling(hsr_batch *b) {
    HIPCHK(hipEventRecord(b->ev1, b->stream));
    HIPCHK(hipEventSynchronize(b->ev1));
    HIPCHK(hipEventElapsedTime(&b->last_total_ms, b->ev0, b->ev1));
    for (int k = 0; k < 3; k++) { b->last_kernel_ms[k] = 0; b->last_launches[k] = 0; }
    for (size_t i = 0; i + 3 < b->kev.size(); i += 4)
        for (int k = 0; k < 3; k++) { float ms = 0; hipEventElapsedTime(&ms, b->kev[i + k], b->kev[i + k + 1]); b->last_kernel_ms[k] += ms; b->last_launches[k]++; }
    return HSR_OK;
}

extern "C" int hsr_batch_step_dev(hsr_batch *b, const float *d_ctrl, int n_substeps, int goal_body, float geofence,
                                  float *d_obs, float *d_reward, uint8_t *d_done, int32_t *d_nsteps) {
    ENTER_DEV(b);
    if (!d_ctrl || n_substeps < 0) return fail(HSR_EINVAL, "bad arguments to hsr_batch_step");
    if (goal_body >= b->dm.nbody) return fail(HSR_EINVAL, "goal body out of range");
    const int N = b->N;
    hipStream_t st = b->stream;
    int rc;
    if (b->profiling) {
        for (hipEvent_t ev : b->kev) hipEventDestroy(ev);
        b->kev.clear();
        HIPCHK(hipEventRecord(b->ev0, st));
    }
    const int cap_rows = b->cap_every > 0 ? (n_substeps > 0 ? (n_substeps - 1) / b->cap_every + 1 : 0) + 1 : 0;
    if (cap_rows > 0 && (rc = grow_capture(b, cap_rows))) return rc;
    if (b->persist && n_substeps > 0) {
        const StepIO io{d_ctrl, d_obs, d_reward, d_done, d_nsteps, b->cap_every > 0 ? b->d_cap_desc : nullptr};
        if ((rc = launch_persistent(b, io, n_substeps, goal_body, geofence))) return rc;
    } else {
        hipLaunchKernelGGL(k_begin_step, grid1(N), dim3(256), 0, st, b->ds, d_ctrl, b->dm.nu);
        if ((rc = launch_chain(b, n_substeps, goal_body, geofence))) return rc;
        if (d_obs) {
            const int nq = b->dm.nq, nv = b->dm.nv;
            hipLaunchKernelGGL(k_soa_to_aos, grid1((size_t)nq * N), dim3(256), 0, st, d_obs, (const float *)b->ds.qpos, nq, N, nq + nv, 0);
            hipLaunchKernelGGL(k_soa_to_aos, grid1((size_t)nv * N), dim3(256), 0, st, d_obs, (const float *)b->ds.qvel, nv, N, nq + nv, nq);
        }
        hipLaunchKernelGGL(k_end_step, grid1(N), dim3(256), 0, st, b->ds, d_reward, d_done, d_nsteps);
    }
    if (cap_rows > 0)       // the final frame (the poses after the step: the reference's 50 closing frames show them, hsr/env.py:128-130) and the counts
        hipLaunchKernelGGL(k_capture, grid1((size_t)12 * b->dm.nlink * b->cap_n), dim3(256), 0, st, b->ds, b->dm.nlink, (const int *)b->d_cap_env, b->cap_n, b->d_cap,
                           cap_rows - 1, 0, b->cap_every, b->d_cap_cnt);
    b->cap_rows = cap_rows;
    HIPCHK(hipGetLastError());
    return b->profiling ? finish_profiling(b) : HSR_OK;
}

extern "C" int hsr_batch_step(hsr_batch *b, const float *ctrl, int n_substeps, int goal_body, float geofence,
                              float *obs, float *reward, uint8_t *done, int32_t *nsteps) {
    ENTER_DEV(b);
    if (!ctrl) return fail(HSR_EINVAL, "bad arguments to hsr_batch_step");
    const size_t N = b->N;
    const int nu = b->dm.nu, no = b->dm.nq + b->dm.nv;
    // staging layout: [ctrl N*nu | obs N*no | reward N]
    if (N * (size_t)(nu + no + 1) > b->stage_floats) return fail(HSR_EINVAL, "staging overflow in step");
    float *d_ctrl = b->d_stage, *d_obs = b->d_stage + N * nu, *d_rew = d_obs + N * no;
    HIPCHK(hipMemcpyAsync(d_ctrl, ctrl, N * nu * sizeof(float), hipMemcpyHostToDevice, b->stream));
    int rc = hsr_batch_step_dev(b, d_ctrl, n_substeps, goal_body, geofence, obs ? d_obs : nullptr, reward ? d_rew : nullptr,
                                done ? b->d_stage_u8 : nullptr, nsteps ? b->d_stage_i32 : nullptr);
    if (rc) return rc;
    if (obs) HIPCHK(hipMemcpyAsync(obs, d_obs, N * no * sizeof(float), hipMemcpyDeviceToHost, b->stream));
    if (reward) HIPCHK(hipMemcpyAsync(reward, d_rew, N * sizeof(float), hipMemcpyDeviceToHost, b->stream));
    if (done) HIPCHK(hipMemcpyAsync(done, b->d_stage_u8, N, hipMemcpyDeviceToHost, b->stream));
    if (nsteps) HIPCHK(hipMemcpyAsync(nsteps, b->d_stage_i32, N * sizeof(int32_t), hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    return queue_error(b);
}
