// Settings, state / field getters and setters, diagnostics: the entry points that neither create, step nor render.

// `count` elements of a device array to the caller once the stream has drained; clear: counters, zeroed on the device after the read
template <typename T>
static int read_drained(hsr_batch *b, T *out, T *src, size_t count, bool clear = false) {
    HIPCHK(hipStreamSynchronize(b->stream));
    HIPCHK(hipMemcpy(out, src, count * sizeof(T), hipMemcpyDeviceToHost));
    if (clear) HIPCHK(hipMemset(src, 0, count * sizeof(T)));
    return HSR_OK;
}
extern "C" int hsr_batch_size(const hsr_batch *b) { ENTER(b); return b->N; }
extern "C" void *hsr_batch_stream(const hsr_batch *b) { return b ? (void *)b->stream : nullptr; }
extern "C" int hsr_batch_sync(hsr_batch *b) { ENTER_DEV(b); HIPCHK(hipStreamSynchronize(b->stream)); return queue_error(b); }
extern "C" int hsr_batch_set_profiling(hsr_batch *b, int on) { ENTER(b); b->profiling = on == 1; b->kernel_log = on == 2; return HSR_OK; }
// durations (ms) of the persistent-kernel launches logged since the last call (hsr_batch_set_profiling(b, 2)); synchronises the stream
extern "C" int hsr_batch_kernel_times(hsr_batch *b, float *out_ms, int cap) {
    ENTER_DEV(b);
    HIPCHK(hipStreamSynchronize(b->stream));
    int n = 0;
    for (auto &pr : b->klog) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess && out_ms && n < cap) out_ms[n] = ms;
        n++;
        hipEventDestroy(pr.first); hipEventDestroy(pr.second);
    }
    b->klog.clear();
    const int qe = queue_error(b);
    return qe ? qe : n;
}
extern "C" int hsr_batch_set_graph(hsr_batch *b, int on) { ENTER(b); b->use_graph = on != 0; return HSR_OK; }
static void clear_margins(hsr_batch *b) {
    hipLaunchKernelGGL(k_clear_margins, grid1((size_t)b->ds.npair_sep * b->N), dim3(256), 0, b->stream, b->ds);
}
extern "C" int hsr_batch_set_persistent(hsr_batch *b, int on) {
    ENTER(b);
    const bool want = on != 0 && b->kernel;
    if (want && !b->persist) { hipSetDevice(b->device); clear_margins(b); }      // the per-substep chain does not maintain the margins
    b->persist = want;
    return b->persist ? 1 : 0;
}
extern "C" int hsr_batch_is_persistent(const hsr_batch *b) {
    ENTER(b);
    if (!b->persist) return 0;
    return 1 | (b->const_row >= 0 ? 2 : 0) | (b->kin3 ? 4 : 0);
}
extern "C" int hsr_batch_set_debug(hsr_batch *b, int on) {
    ENTER(b);
    b->debug_store = (on & 1) != 0;
    b->test_hooks = on & (6 | 16 | 32 | 64 | 128);
    return HSR_OK;
}
extern "C" int hsr_batch_set_schedule(hsr_batch *b, int on) { ENTER(b); b->schedule = on != 0; return HSR_OK; }
extern "C" int hsr_batch_set_mpr_warm(hsr_batch *b, int on) {
    ENTER_DEV(b);
    if ((on != 0) != b->mpr_warm) clear_margins(b);
    b->mpr_warm = on != 0;
    return HSR_OK;
}
extern "C" int hsr_batch_set_solo(hsr_batch *b, int servers, float trips) {
    ENTER(b);
    if (servers < 0 || trips < 0.f) return fail(HSR_EINVAL, "hsr_batch_set_solo: servers >= 0, trips >= 0");
    b->solo_servers = servers;
    if (trips > 0.f) b->solo_trips = trips;
    return b->kernel_sv ? HSR_OK : 1;          // 1: accepted, but this model's kernel instance has no server path (the setting has no effect)
}
extern "C" int hsr_batch_set_split(hsr_batch *b, int on, int period, float trips, int min_left, int extra_helpers) {
    ENTER(b);
    if (period < 0 || period >= SPLIT_MAX_SUBSTEPS || trips > 1000.f || min_left < 0 || extra_helpers < 0 || extra_helpers > SPLIT_MAX_EXTRA)
        return fail(HSR_EINVAL, "hsr_batch_set_split: period 0..2047, trips <= 1000, min_left >= 0, extra_helpers 0..4096");
    b->split = on != 0;
    if (period > 0) b->split_period = period;
    if (trips >= 0.f) b->split_trips = trips;
    if (min_left > 0) b->split_min_left = min_left;
    b->split_extra = extra_helpers;
    return b->kernel && b->split_inst ? HSR_OK : 1;      // 1: accepted, but this batch's kernel instance never splits (the setting has no effect)
}
extern "C" int hsr_batch_set_split_lone(hsr_batch *b, int on, float trips) {
    ENTER(b);
    if (trips > 1000.f) return fail(HSR_EINVAL, "hsr_batch_set_split_lone: trips <= 1000");
    b->split_lone = on != 0;
    if (trips > 0.f) b->split_lone_trips = trips;
    return b->kernel && b->split_inst ? HSR_OK : 1;      // 1: accepted, but this batch's kernel instance never splits (the setting has no effect)
}
extern "C" int hsr_batch_solo_handovers(hsr_batch *b, int *out) {
    ENTER_DEV(b);
    if (!out) return fail(HSR_EINVAL, "null argument");
    const int rc = read_drained(b, out, b->ds.sq_ctl + 1, 1);
    if (!b->handovers_counted) *out = 0;          // (the word is reset only in front of launches that count)
    return rc ? rc : queue_error(b);
}
extern "C" int hsr_batch_set_queue(hsr_batch *b, int mode, int chunk) {
    ENTER(b);
    if (mode < -1 || mode > 1 || chunk < 0) return fail(HSR_EINVAL, "hsr_batch_set_queue: mode -1 / 0 / 1, chunk >= 0");
    b->queue = mode;
    if (chunk > 0) { b->queue_chunk = chunk; b->queue_chunk_set = true; }
    return HSR_OK;
}
extern "C" int hsr_batch_set_goals(hsr_batch *b, int n, const int *body_a, const int *body_b, const float *dist) {
    ENTER_DEV(b);
    if (n < 0 || n > 4 || (n > 0 && (!body_a || !body_b || !dist))) return fail(HSR_EINVAL, "hsr_batch_set_goals: 0..4 terms");
    for (int k = 0; k < n; k++)
        if (body_a[k] < 0 || body_a[k] >= b->dm.nbody || body_b[k] < 0 || body_b[k] >= b->dm.nbody) return fail(HSR_EINVAL, "hsr_batch_set_goals: body id out of range");
    HIPCHK(hipStreamSynchronize(b->stream));
    b->ds.ngoal = n;
    for (int k = 0; k < n; k++) { b->ds.goal_a[k] = body_a[k]; b->ds.goal_b[k] = body_b[k]; b->ds.goal_d[k] = dist[k]; }
    for (auto &kv : b->graphs) hipGraphExecDestroy(kv.second);      // captured launches carry the old terms
    b->graphs.clear();
    return HSR_OK;
}
extern "C" int hsr_batch_cap_counts(hsr_batch *b, unsigned long long *out) {
    ENTER_DEV(b);
    if (!out) return fail(HSR_EINVAL, "null argument");
    const int rc = read_drained(b, out, b->ds.capstat, 4, true);
    return rc ? rc : queue_error(b);
}
extern "C" int hsr_batch_cap_histogram(hsr_batch *b, unsigned long long *out) {
    ENTER_DEV(b);
    if (!out) return fail(HSR_EINVAL, "null argument");
    return read_drained(b, out, b->ds.capstat + 4, 8, true);
}

// per-env Newton iterations over the last (up to) 100 substeps of the previous persistent launch: what k_schedule packs by
extern "C" int hsr_batch_newton_trips(hsr_batch *b, int32_t *out) {
    ENTER_DEV(b);
    if (!out) return fail(HSR_EINVAL, "null argument");
    return read_drained(b, out, b->ds.trips, (size_t)b->N);
}
// the packing the last persistent launch ran with: out[slot] = env of lane group `slot % (64 / group)` of task `slot / (64 / group)`, -1 = empty
extern "C" int hsr_batch_packing(hsr_batch *b, int32_t *out) {
    ENTER_DEV(b);
    if (!out) return fail(HSR_EINVAL, "null argument");
    if (!b->persist || !b->schedule || !b->d_slot_env) return fail(HSR_EINVAL, "hsr_batch_packing: no packed persistent launch on this batch");
    const int epb = 64 / b->group, slots = (b->N + epb - 1) / epb * epb;
    const int rc = read_drained(b, out, b->d_slot_env, (size_t)slots);
    return rc ? rc : queue_error(b);
}
static int to_device_soa(hsr_batch *b, float *dst, const float *host, int rows) {
    const size_t n = (size_t)rows * b->N;
    if (n > b->stage_floats) return fail(HSR_EINVAL, "staging overflow");
    HIPCHK(hipMemcpyAsync(b->d_stage, host, n * sizeof(float), hipMemcpyHostToDevice, b->stream));
    hipLaunchKernelGGL(k_aos_to_soa, grid1(n), dim3(256), 0, b->stream, dst, (const float *)b->d_stage, rows, b->N);
    HIPCHK(hipStreamSynchronize(b->stream));
    return HSR_OK;
}
static int to_host_aos(hsr_batch *b, float *host, const float *src, int rows) {
    const size_t n = (size_t)rows * b->N;
    if (n > b->stage_floats) return fail(HSR_EINVAL, "staging overflow");
    hipLaunchKernelGGL(k_soa_to_aos, grid1(n), dim3(256), 0, b->stream, b->d_stage, src, rows, b->N, rows, 0);
    return stage_to_host(b, host, b->d_stage, n);
}

extern "C" int hsr_batch_get_state(hsr_batch *b, float *time, float *qpos, float *qvel) {
    ENTER_DEV(b);
    int rc;
    if (time && (rc = to_host_aos(b, time, b->ds.time, 1))) return rc;
    if (qpos && (rc = to_host_aos(b, qpos, b->ds.qpos, b->dm.nq))) return rc;
    if (qvel && (rc = to_host_aos(b, qvel, b->ds.qvel, b->dm.nv))) return rc;
    return queue_error(b);
}
extern "C" int hsr_batch_set_state(hsr_batch *b, const float *time, const float *qpos, const float *qvel) {
    ENTER_DEV(b);
    clear_margins(b);                     // positions jump: the separation margins of the convex pairs are void
    int rc;
    if (time && (rc = to_device_soa(b, b->ds.time, time, 1))) return rc;
    if (qpos && (rc = to_device_soa(b, b->ds.qpos, qpos, b->dm.nq))) return rc;
    if (qvel && (rc = to_device_soa(b, b->ds.qvel, qvel, b->dm.nv))) return rc;
    return hsr_batch_forward(b);
}
extern "C" int hsr_batch_set_mocap(hsr_batch *b, const float *mocap) { ENTER_DEV(b); return to_device_soa(b, b->ds.mocap, mocap, 3); }
extern "C" int hsr_batch_set_warmstart(hsr_batch *b, const float *w) { ENTER_DEV(b); return to_device_soa(b, b->ds.warm, w, b->dm.nv); }
extern "C" int hsr_batch_get_warmstart(hsr_batch *b, float *w) { ENTER_DEV(b); return to_host_aos(b, w, b->ds.warm, b->dm.nv); }
extern "C" int hsr_batch_body_xpos(hsr_batch *b, int body_id, float *out) {
    ENTER_DEV(b);
    if (body_id < 0 || body_id >= b->dm.nbody) return fail(HSR_EINVAL, "body id out of range");
    hipLaunchKernelGGL(k_body_xpos, grid1(b->N), dim3(256), 0, b->stream, b->dm, b->ds, body_id, b->d_stage);
    return stage_to_host(b, out, b->d_stage, (size_t)b->N * 3);
}

static int obs_openai_launch(hsr_batch *b, const int *ids, float *d_out) {
    if (!ids) return fail(HSR_EINVAL, "null argument");
    const DevModel &d = b->dm;
    for (int k = 0; k < 3; k++) if (ids[k] < 0 || ids[k] >= d.nbody || b->model->i32("body_mocap")[ids[k]]) return fail(HSR_EINVAL, "obs_openai: bad body id");
    if (ids[3] < 0 || ids[3] >= d.nq || ids[4] < 0 || ids[4] >= d.nq || ids[5] < 0 || ids[5] >= d.nv || ids[6] < 0 || ids[6] >= d.nv)
        return fail(HSR_EINVAL, "obs_openai: bad joint address");
    hipLaunchKernelGGL(k_obs_openai, grid1(b->N), dim3(256), 0, b->stream, b->dm, b->ds, ids[0], ids[1], ids[2], ids[3], ids[4], ids[5], ids[6], d.timestep, d_out);
    HIPCHK(hipGetLastError());
    return HSR_OK;
}
extern "C" int hsr_batch_obs_openai_dev(hsr_batch *b, const int *ids, float *d_out) {
    ENTER_DEV(b);
    return obs_openai_launch(b, ids, d_out);
}
extern "C" int hsr_batch_obs_openai(hsr_batch *b, const int *ids, float *out) {
    ENTER_DEV(b);
    const int rc = obs_openai_launch(b, ids, b->d_stage);
    return rc ? rc : stage_to_host(b, out, b->d_stage, (size_t)b->N * 25);
}

extern "C" int hsr_batch_bad_state(hsr_batch *b, uint8_t *out) {
    ENTER_DEV(b);
    std::vector<int> tmp(b->N);
    const int rc = stage_to_host(b, tmp.data(), b->ds.bad, (size_t)b->N);
    if (rc) return rc;
    int any = 0;
    for (int i = 0; i < b->N; i++) { out[i] = (uint8_t)(tmp[i] != 0); any |= tmp[i]; }
    const int qe = queue_error(b);        // a drained launch outranks a diverged env: its envs stopped mid env-step
    return qe ? qe : (any ? HSR_EBADSTATE : HSR_OK);
}

extern "C" int hsr_batch_get_field(hsr_batch *b, int field, float *out) {
    ENTER_DEV(b);
    const DevModel &d = b->dm;
    const size_t N = b->N;
    switch (field) {
    case HSR_F_XPOS: return to_host_aos(b, out, b->ds.xpos, 3 * d.nlink);
    case HSR_F_XMAT: return to_host_aos(b, out, b->ds.xmat, 9 * d.nlink);
    case HSR_F_QACC: return to_host_aos(b, out, b->ds.qacc, d.nv);
    case HSR_F_QACC_SMOOTH: return to_host_aos(b, out, b->ds.qacc_smooth, d.nv);
    case HSR_F_QFRC_SMOOTH: return to_host_aos(b, out, b->ds.qfrc_smooth, d.nv);
    case HSR_F_QFRC_CONSTRAINT: return to_host_aos(b, out, b->ds.qfrc_constraint, d.nv);
    case HSR_F_M:
        hipLaunchKernelGGL(k_expand_M, grid1(N), dim3(256), 0, b->stream, b->ds, b->d_stage, d.nv);
        return stage_to_host(b, out, b->d_stage, N * d.nv * d.nv);
    case HSR_F_NCON: case HSR_F_NEFC: case HSR_F_NITER: {
        const int *src = field == HSR_F_NCON ? b->ds.ncon : (field == HSR_F_NEFC ? b->ds.nefc : b->ds.niter);
        hipLaunchKernelGGL(k_i32_to_f32, grid1(N), dim3(256), 0, b->stream, b->d_stage, src, N);
        return stage_to_host(b, out, b->d_stage, N); }
    case HSR_F_CONTACT:
        hipLaunchKernelGGL(k_contacts_out, grid1(N), dim3(256), 0, b->stream, b->dm, b->ds, b->d_stage);
        return stage_to_host(b, out, b->d_stage, N * d.nslot * 7);
    default: return fail(HSR_EINVAL, "unknown field");
    }
}

// diagnostic builds (-DHSR_PHASE_TIMING): read and clear the per-phase cycle sums of the timed kernels (solve_g.h: PHASE_*)
extern "C" int hsr_batch_phase_cycles(hsr_batch *b, unsigned long long *out /*[32]*/) {
    ENTER_DEV(b);
    return read_drained(b, out, b->ds.phase_cyc, 32, true);
}

// diagnostic builds: per-workgroup (start, end) s_memrealtime stamps and HW_ID / XCC_ID of the last persistent launch
extern "C" int hsr_batch_block_times(hsr_batch *b, unsigned long long *out, int nblocks) {
    ENTER_DEV(b);
    if (nblocks > 8192) nblocks = 8192;
    // nblocks < 0, lifetime build: the per-env stamps (solve_g.h ENV_STAMP), 2 x 8192 values, cleared by the read
    if (nblocks < 0) return read_drained(b, out, b->ds.phase_cyc + 32 + 40 * 4096, (size_t)2 * 8192, true);
    return read_drained(b, out, b->ds.phase_cyc + 32, (size_t)nblocks * 40);
}

extern "C" int hsr_batch_last_timing(hsr_batch *b, float *total_ms, float *kernel_ms, int *launches) {
    ENTER(b);
    if (total_ms) *total_ms = b->last_total_ms;
    for (int k = 0; k < 3; k++) { if (kernel_ms) kernel_ms[k] = b->last_kernel_ms[k]; if (launches) launches[k] = b->last_launches[k]; }
    return HSR_OK;
}
