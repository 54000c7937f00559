// Hindsight replay: the hsr_replay record, its storage and the launches of replay.h and, for a replay with priorities, replay_prio.h.  What may run when, and with which numbers, is decided
// by the plain functions of replay_logic.h; a refused call launches nothing and leaves the books as they were.  A replay is bound to its
// batch (it reads that batch's pose arrays and launches on its stream) and is not part of an env record (snapshot.h).

struct hsr_replay {
    hsr_batch *owner = nullptr;    // NULL once hsr_batch_destroy released the storage
    int device = 0;
    ReplayBooks books{};
    ReplayDev dev{};
    PrioBooks prio{};              // priorities: off until hsr_replay_priority_enable, and then pdev owns the tree
    PrioDev pdev{};
};

static void replay_free_storage(hsr_replay *r) {
    ReplayDev &D = r->dev;
    for (uint32_t **p : {&D.rows, &D.ep_plane, &D.head, &D.ep_id, &D.ep_step}) { if (*p) hipFree(*p); *p = nullptr; }
    PrioDev &P = r->pdev;
    for (void **p : {(void **)&P.leaf, (void **)&P.node, (void **)&P.p_new, (void **)&P.cell}) { if (*p) hipFree(*p); *p = nullptr; }
    r->prio.enabled = false;
}
// hsr_batch_destroy: as for snapshots, the storage goes with the batch and the handle stays the caller's to destroy
static void replay_release_all(hsr_batch *b) {
    for (hsr_replay *r : b->replays) { replay_free_storage(r); r->owner = nullptr; }
    b->replays.clear();
}
static int replay_live(const hsr_replay *r, const char *who) {
    if (!r) return fail(HSR_EINVAL, "%s: null replay", who);
    if (!r->owner) return fail(HSR_EINVAL, "%s: the replay's batch was destroyed, and its storage with it", who);
    return HSR_OK;
}
static int replay_zero_counters(hsr_replay *r) {
    const size_t n = (size_t)r->books.N * sizeof(uint32_t);
    HIPCHK(hipMemsetAsync(r->dev.ep_id, 0, n, r->owner->stream));
    HIPCHK(hipMemsetAsync(r->dev.ep_step, 0, n, r->owner->stream));
    return HSR_OK;
}

// Priorities (replay_prio.h, replay_prio_logic.h): every launch goes on the batch stream, level by level
static int prio_zero_tree(hsr_replay *r) {
    const PrioDev &P = r->pdev;
    hipStream_t st = r->owner->stream;
    HIPCHK(hipMemsetAsync(P.leaf, 0, (size_t)P.L.n[0] * sizeof(float), st));
    HIPCHK(hipMemsetAsync(P.node, 0, (size_t)P.L.nodes * sizeof(double), st));
    uint32_t bits;
    memcpy(&bits, &r->prio.p_init, sizeof bits);
    HIPCHK(hipMemsetD32Async((hipDeviceptr_t)P.p_new, (int)bits, 1, st));
    return HSR_OK;
}
// re-sum the ancestors of leaves lo .. hi, one launch per stored level
static int prio_resum_span(hsr_replay *r, uint32_t lo, uint32_t hi) {
    const PrioDev &P = r->pdev;
    for (int k = 1; k <= P.L.levels; k++) {
        lo >>= PRIO_RADIX_LOG2; hi >>= PRIO_RADIX_LOG2;
        const uint32_t count = hi - lo + 1;
        hipLaunchKernelGGL(k_prio_resum_range, grid1(count, PRIO_WAVES), dim3(PRIO_BLOCK), 0, r->owner->stream, P, k, lo, count);
    }
    HIPCHK(hipGetLastError());
    return HSR_OK;
}
static int prio_record(hsr_replay *r, int slot) {
    const PrioDev &P = r->pdev;
    const uint32_t N = (uint32_t)r->books.N, lo = (uint32_t)slot * N;
    hipLaunchKernelGGL(k_prio_set_leaves, grid1(N, PRIO_BLOCK), dim3(PRIO_BLOCK), 0, r->owner->stream, P, lo, N);
    return prio_resum_span(r, lo, lo + N - 1);
}

extern "C" int hsr_batch_replay_create(hsr_batch *b, const hsr_replay_spec *spec, hsr_replay **out) {
    ENTER_DEV(b);
    if (!spec || !out) return fail(HSR_EINVAL, "hsr_batch_replay_create: null argument");
    const char *why = replay_spec_error(spec->capacity_steps, spec->obs_dim, spec->goal_body, spec->geofence, b->dm.nbody, b->model->i32("body_mocap"), b->ds.ngoal);
    if (why) return fail(HSR_EINVAL, "hsr_batch_replay_create: %s", why);
    const ReplayLayout L = replay_layout(spec->obs_dim, b->dm.nu);
    const size_t T = (size_t)spec->capacity_steps, N = (size_t)b->N;
    const uint64_t ring = replay_ring_bytes(spec->capacity_steps, b->N, L.stride);
    if (!ring) return fail(HSR_EINVAL, "hsr_batch_replay_create: capacity_steps x envs x row does not fit a device");
    hsr_replay *r = new hsr_replay();
    r->owner = b; r->device = b->device;
    replay_books_init(&r->books, spec->capacity_steps, b->N);
    ReplayDev &D = r->dev;
    D.L = L; D.T = spec->capacity_steps; D.N = b->N;
    D.key0 = (uint32_t)(spec->seed & 0xffffffffu); D.key1 = (uint32_t)(spec->seed >> 32); D.env_offset = spec->env_offset;
    D.goal_body = spec->goal_body; D.geofence = spec->geofence;
    const size_t bytes[5] = {(size_t)ring, T * N * 4, N * (size_t)L.obs_dim * 4, N * 4, N * 4};
    uint32_t **ptr[5] = {&D.rows, &D.ep_plane, &D.head, &D.ep_id, &D.ep_step};
    for (int k = 0; k < 5; k++)
        if (hipMalloc((void **)ptr[k], bytes[k]) != hipSuccess || hipMemset(*ptr[k], 0, bytes[k]) != hipSuccess) {
            replay_free_storage(r);
            delete r;
            hipGetLastError();     // the failed allocation is reported here, not by the batch's next launch
            return fail(HSR_EDEVICE, "replay: no device memory for %s bytes", std::to_string(bytes[k]).c_str());
        }
    b->replays.push_back(r);
    *out = r;
    return HSR_OK;
}
extern "C" void hsr_replay_destroy(hsr_replay *r) {
    if (!r) return;
    if (r->owner) {
        std::vector<hsr_replay *> &v = r->owner->replays;
        v.erase(std::remove(v.begin(), v.end(), r), v.end());
        hipSetDevice(r->device);
        hipStreamSynchronize(r->owner->stream);        // the only stream that uses it
        replay_free_storage(r);
    }
    delete r;
}
extern "C" int hsr_replay_clear(hsr_replay *r) {
    int rc = replay_live(r, "hsr_replay_clear");
    if (rc) return rc;
    HIPCHK(hipSetDevice(r->device));
    if ((rc = replay_zero_counters(r))) return rc;
    if (r->prio.enabled && (rc = prio_zero_tree(r))) return rc;
    replay_clear_done(&r->books);
    return HSR_OK;
}
extern "C" int hsr_replay_state(hsr_replay *r, int32_t *count, int32_t *head_slot, uint32_t *pushed_lo) {
    const int rc = replay_live(r, "hsr_replay_state");
    if (rc) return rc;
    if (count) *count = replay_count(&r->books);
    if (head_slot) *head_slot = replay_head_slot(&r->books);
    if (pushed_lo) *pushed_lo = (uint32_t)(r->books.pushed & 0xffffffffu);
    return HSR_OK;
}

extern "C" int hsr_replay_commit_dev(hsr_replay *r, const float *d_obs, const uint8_t *d_reset) {
    const int rc = replay_live(r, "hsr_replay_commit_dev");
    if (rc) return rc;
    if (!d_obs) return fail(HSR_EINVAL, "hsr_replay_commit_dev: null d_obs");
    const char *why = replay_commit_error(&r->books);
    if (why) return fail(HSR_EINVAL, "hsr_replay_commit_dev: %s", why);
    HIPCHK(hipSetDevice(r->device));
    const ReplayDev &D = r->dev;
    hipLaunchKernelGGL(k_replay_commit, grid1((size_t)D.N * D.L.obs_dim, REPLAY_BLOCK), dim3(REPLAY_BLOCK), 0, r->owner->stream, D, (const uint32_t *)d_obs, d_reset);
    HIPCHK(hipGetLastError());
    replay_commit_done(&r->books);
    return HSR_OK;
}
extern "C" int hsr_replay_record_dev(hsr_replay *r, const float *d_ctrl, const float *d_next_obs, const float *d_reward, const uint8_t *d_done) {
    const int rc = replay_live(r, "hsr_replay_record_dev");
    if (rc) return rc;
    if (!d_ctrl || !d_next_obs) return fail(HSR_EINVAL, "hsr_replay_record_dev: null d_ctrl / d_next_obs");
    const char *why = replay_record_error(&r->books);
    if (why) return fail(HSR_EINVAL, "hsr_replay_record_dev: %s", why);
    hsr_batch *b = r->owner;
    if (b->ds.ngoal > 0) return fail(HSR_EINVAL, "hsr_replay_record_dev: the batch has extra goal terms by now (hsr_batch_set_goals): their reward cannot be relabelled");
    HIPCHK(hipSetDevice(r->device));
    const ReplayDev &D = r->dev;
    hipLaunchKernelGGL(k_replay_record, grid1((size_t)D.N, REPLAY_PER_BLOCK), dim3(REPLAY_BLOCK), 0, b->stream, b->dm, b->ds, D, replay_head_slot(&r->books),
                       (const uint32_t *)d_ctrl, (const uint32_t *)d_next_obs, (const uint32_t *)d_reward, d_done);
    HIPCHK(hipGetLastError());
    if (r->prio.enabled) {
        const int rc2 = prio_record(r, replay_head_slot(&r->books));
        if (rc2) return rc2;
    }
    replay_record_done(&r->books);
    return HSR_OK;
}
extern "C" int hsr_replay_sample_dev(hsr_replay *r, uint32_t draw, int batch, float her_ratio, float *d_obs, float *d_act, float *d_next_obs, float *d_goal,
                                     float *d_achieved_next, float *d_reward, uint8_t *d_done, int32_t *d_index) {
    const int rc = replay_live(r, "hsr_replay_sample_dev");
    if (rc) return rc;
    const char *why = replay_sample_error(&r->books, batch, her_ratio);
    if (why) return fail(HSR_EINVAL, "hsr_replay_sample_dev: %s", why);
    HIPCHK(hipSetDevice(r->device));
    hipLaunchKernelGGL(k_replay_sample, grid1((size_t)batch, REPLAY_PER_BLOCK), dim3(REPLAY_BLOCK), 0, r->owner->stream, r->dev, replay_first_slot(&r->books),
                       replay_count(&r->books), draw, batch, her_ratio, (uint32_t *)d_obs, (uint32_t *)d_act, (uint32_t *)d_next_obs, (uint32_t *)d_goal,
                       (uint32_t *)d_achieved_next, (uint32_t *)d_reward, d_done, d_index);
    HIPCHK(hipGetLastError());
    return HSR_OK;
}
extern "C" int hsr_replay_sample_seq_dev(hsr_replay *r, uint32_t draw, int batch, int seq_len, float her_ratio, float gamma, const hsr_replay_seq_out *out) {
    const int rc = replay_live(r, "hsr_replay_sample_seq_dev");
    if (rc) return rc;
    const char *why = replay_sample_seq_error(&r->books, batch, seq_len, her_ratio, gamma, out != nullptr);
    if (why) return fail(HSR_EINVAL, "hsr_replay_sample_seq_dev: %s", why);
    HIPCHK(hipSetDevice(r->device));
    hipLaunchKernelGGL(k_replay_sample_seq, grid1((size_t)batch * (size_t)seq_len, REPLAY_PER_BLOCK), dim3(REPLAY_BLOCK), 0, r->owner->stream, r->dev,
                       replay_first_slot(&r->books), replay_count(&r->books), draw, batch, seq_len, her_ratio, gamma, *out);
    HIPCHK(hipGetLastError());
    return HSR_OK;
}

// ---- priorities
extern "C" int hsr_replay_priority_enable(hsr_replay *r, const hsr_priority_spec *spec) {
    const int rc = replay_live(r, "hsr_replay_priority_enable");
    if (rc) return rc;
    if (!spec) return fail(HSR_EINVAL, "hsr_replay_priority_enable: null spec");
    const char *why = prio_enable_error(&r->books, &r->prio, spec->p_init, spec->p_min, spec->p_max, spec->max_batch);
    if (why) return fail(HSR_EINVAL, "hsr_replay_priority_enable: %s", why);
    HIPCHK(hipSetDevice(r->device));
    PrioDev &P = r->pdev;
    P.L = prio_levels((uint64_t)r->books.T * (uint64_t)r->books.N);
    P.p_min = spec->p_min; P.p_max = spec->p_max;
    const size_t bytes[4] = {(size_t)P.L.n[0] * sizeof(float), (size_t)P.L.nodes * sizeof(double), sizeof(uint32_t), (size_t)spec->max_batch * sizeof(int32_t)};
    void **ptr[4] = {(void **)&P.leaf, (void **)&P.node, (void **)&P.p_new, (void **)&P.cell};
    for (int k = 0; k < 4; k++)
        if (hipMalloc(ptr[k], bytes[k]) != hipSuccess) {
            for (int c = 0; c < k; c++) { hipFree(*ptr[c]); *ptr[c] = nullptr; }
            *ptr[k] = nullptr;
            hipGetLastError();
            return fail(HSR_EDEVICE, "replay priorities: no device memory for %s bytes", std::to_string(bytes[k]).c_str());
        }
    r->prio.p_init = spec->p_init; r->prio.p_min = spec->p_min; r->prio.p_max = spec->p_max; r->prio.max_batch = spec->max_batch;
    HIPCHK(hipMemsetAsync(P.cell, 0, bytes[3], r->owner->stream));
    const int rz = prio_zero_tree(r);
    if (rz) return rz;
    r->prio.enabled = true;
    return HSR_OK;
}
extern "C" int hsr_replay_priority_state(hsr_replay *r, uint64_t *pushed, double *total, float *p_new) {
    const int rc = replay_live(r, "hsr_replay_priority_state");
    if (rc) return rc;
    if (!r->prio.enabled) return fail(HSR_EINVAL, "hsr_replay_priority_state: priorities are not enabled");
    HIPCHK(hipSetDevice(r->device));
    const PrioDev &P = r->pdev;
    double t = 0.0;
    float p = 0.f;
    HIPCHK(hipMemcpyAsync(&t, P.node + P.L.offset[P.L.levels], sizeof t, hipMemcpyDeviceToHost, r->owner->stream));
    HIPCHK(hipMemcpyAsync(&p, P.p_new, sizeof p, hipMemcpyDeviceToHost, r->owner->stream));
    HIPCHK(hipStreamSynchronize(r->owner->stream));
    if (pushed) *pushed = r->books.pushed;
    if (total) *total = t;
    if (p_new) *p_new = p;
    return HSR_OK;
}
static void prio_launch_descent(hsr_replay *r, uint32_t draw, int batch, float *d_prob) {
    const ReplayDev &D = r->dev;
    hipLaunchKernelGGL(k_prio_descend, grid1((size_t)batch, PRIO_WAVES), dim3(PRIO_BLOCK), 0, r->owner->stream, r->pdev, D.key0, D.key1, D.env_offset, draw, batch, d_prob);
}
extern "C" int hsr_replay_priority_sample_dev(hsr_replay *r, uint32_t draw, int batch, float her_ratio, float *d_obs, float *d_act, float *d_next_obs, float *d_goal,
                                              float *d_achieved_next, float *d_reward, uint8_t *d_done, int32_t *d_index, float *d_prob) {
    const int rc = replay_live(r, "hsr_replay_priority_sample_dev");
    if (rc) return rc;
    const char *why = prio_sample_error(&r->books, &r->prio, batch, her_ratio);
    if (why) return fail(HSR_EINVAL, "hsr_replay_priority_sample_dev: %s", why);
    HIPCHK(hipSetDevice(r->device));
    prio_launch_descent(r, draw, batch, d_prob);
    hipLaunchKernelGGL(k_prio_sample, grid1((size_t)batch, REPLAY_PER_BLOCK), dim3(REPLAY_BLOCK), 0, r->owner->stream, r->dev, (const int32_t *)r->pdev.cell,
                       replay_first_slot(&r->books), replay_count(&r->books), draw, batch, her_ratio, (uint32_t *)d_obs, (uint32_t *)d_act, (uint32_t *)d_next_obs,
                       (uint32_t *)d_goal, (uint32_t *)d_achieved_next, (uint32_t *)d_reward, d_done, d_index);
    HIPCHK(hipGetLastError());
    return HSR_OK;
}
extern "C" int hsr_replay_priority_sample_seq_dev(hsr_replay *r, uint32_t draw, int batch, int seq_len, float her_ratio, float gamma, const hsr_replay_seq_out *out,
                                                  float *d_prob) {
    const int rc = replay_live(r, "hsr_replay_priority_sample_seq_dev");
    if (rc) return rc;
    const char *why = prio_sample_seq_error(&r->books, &r->prio, batch, seq_len, her_ratio, gamma, out != nullptr);
    if (why) return fail(HSR_EINVAL, "hsr_replay_priority_sample_seq_dev: %s", why);
    HIPCHK(hipSetDevice(r->device));
    prio_launch_descent(r, draw, batch, d_prob);
    hipLaunchKernelGGL(k_prio_sample_seq, grid1((size_t)batch * (size_t)seq_len, REPLAY_PER_BLOCK), dim3(REPLAY_BLOCK), 0, r->owner->stream, r->dev,
                       (const int32_t *)r->pdev.cell, replay_first_slot(&r->books), replay_count(&r->books), draw, batch, seq_len, her_ratio, gamma, *out);
    HIPCHK(hipGetLastError());
    return HSR_OK;
}
extern "C" int hsr_replay_priority_update_dev(hsr_replay *r, uint64_t sampled_at, int batch, const int32_t *d_index, const float *d_priority) {
    const int rc = replay_live(r, "hsr_replay_priority_update_dev");
    if (rc) return rc;
    const char *why = prio_update_error(&r->books, &r->prio, sampled_at, batch, d_index && d_priority);
    if (why) return fail(HSR_EINVAL, "hsr_replay_priority_update_dev: %s", why);
    HIPCHK(hipSetDevice(r->device));
    const PrioDev &P = r->pdev;
    hipStream_t st = r->owner->stream;
    hipLaunchKernelGGL(k_prio_update_mark, grid1((size_t)batch, PRIO_BLOCK), dim3(PRIO_BLOCK), 0, st, P, r->books.T, r->books.N, prio_written(&r->books), sampled_at, batch, d_index);
    hipLaunchKernelGGL(k_prio_update_max, grid1((size_t)batch, PRIO_BLOCK), dim3(PRIO_BLOCK), 0, st, P, batch, d_priority);
    // a level with no more nodes than rows is re-summed whole; a larger one only under the rows' leaves
    for (int k = 1; k <= P.L.levels; k++) {
        if (P.L.n[k] <= (uint32_t)batch) hipLaunchKernelGGL(k_prio_resum_range, grid1(P.L.n[k], PRIO_WAVES), dim3(PRIO_BLOCK), 0, st, P, k, 0u, P.L.n[k]);
        else hipLaunchKernelGGL(k_prio_resum_rows, grid1((size_t)batch, PRIO_WAVES), dim3(PRIO_BLOCK), 0, st, P, k, batch);
    }
    HIPCHK(hipGetLastError());
    return HSR_OK;
}
extern "C" int hsr_replay_priority_read_dev(hsr_replay *r, float *d_leaves) {
    const int rc = replay_live(r, "hsr_replay_priority_read_dev");
    if (rc) return rc;
    if (!r->prio.enabled) return fail(HSR_EINVAL, "hsr_replay_priority_read_dev: priorities are not enabled");
    if (!d_leaves) return fail(HSR_EINVAL, "hsr_replay_priority_read_dev: null d_leaves");
    HIPCHK(hipSetDevice(r->device));
    HIPCHK(hipMemcpyAsync(d_leaves, r->pdev.leaf, (size_t)r->pdev.L.n[0] * sizeof(float), hipMemcpyDeviceToDevice, r->owner->stream));
    return HSR_OK;
}
