// On-policy rollouts: the hsr_rollout record, its storage and the launches of rollout.h.  What may run when, and with which numbers, is
// decided by the plain functions of rollout_logic.h; a refused call launches nothing and leaves the books as they were.  A rollout is bound
// to its batch (it launches on that batch's stream) and is not part of an env record (snapshot.h).

struct hsr_rollout {
    hsr_batch *owner = nullptr;    // NULL once hsr_batch_destroy released the storage
    int device = 0;
    RolloutBooks books{};
    RolloutDev dev{};
    int half_bits = 1;             // the shuffle's h (rollout_half_bits of T N)
    int gae_blocks = 1, var_blocks = 1;
};

static void rollout_free_storage(hsr_rollout *r) {
    RolloutDev &D = r->dev;
    for (void **p : {(void **)&D.rows, (void **)&D.head, (void **)&D.logp, (void **)&D.partial, (void **)&D.stats}) { if (*p) hipFree(*p); *p = nullptr; }
}
// hsr_batch_destroy: as for replays, the storage goes with the batch and the handle stays the caller's to destroy
static void rollout_release_all(hsr_batch *b) {
    for (hsr_rollout *r : b->rollouts) { rollout_free_storage(r); r->owner = nullptr; }
    b->rollouts.clear();
}
static int rollout_live(const hsr_rollout *r, const char *who) {
    if (!r) return fail(HSR_EINVAL, "%s: null rollout", who);
    if (!r->owner) return fail(HSR_EINVAL, "%s: the rollout's batch was destroyed, and its storage with it", who);
    return HSR_OK;
}
// the common opening of a protocol call (who: a string literal): the handle, the books' verdict, the device made current
#define ROLLOUT_ENTER(r, who, why_expr) do { \
        const int rc_ = rollout_live((r), who); \
        if (rc_) return rc_; \
        const char *why_ = (why_expr); \
        if (why_) return fail(HSR_EINVAL, who ": %s", why_); \
        HIPCHK(hipSetDevice((r)->device)); \
    } while (0)

extern "C" int hsr_batch_rollout_create(hsr_batch *b, const hsr_rollout_spec *spec, hsr_rollout **out) {
    ENTER_DEV(b);
    if (!spec || !out) return fail(HSR_EINVAL, "hsr_batch_rollout_create: null argument");
    const char *why = rollout_spec_error(spec->horizon, spec->obs_dim, spec->gamma, spec->lam, b->N);
    if (why) return fail(HSR_EINVAL, "hsr_batch_rollout_create: %s", why);
    const RolloutLayout L = rollout_layout(spec->obs_dim, b->dm.nu);
    if (!rollout_storage_bytes(spec->horizon, b->N, L.stride, L.obs_dim)) return fail(HSR_EINVAL, "hsr_batch_rollout_create: horizon x envs x row does not fit a device");
    hsr_rollout *r = new hsr_rollout();
    r->owner = b; r->device = b->device;
    rollout_books_init(&r->books, spec->horizon, b->N);
    const size_t items = (size_t)rollout_items(&r->books), N = (size_t)b->N;
    r->half_bits = rollout_half_bits((int64_t)items);
    r->gae_blocks = (int)((N + ROLLOUT_GAE_BLOCK - 1) / ROLLOUT_GAE_BLOCK);
    r->var_blocks = (int)std::min<size_t>((items + ROLLOUT_BLOCK - 1) / ROLLOUT_BLOCK, ROLLOUT_VAR_BLOCKS);
    RolloutDev &D = r->dev;
    D.L = L; D.T = spec->horizon; D.N = b->N;
    D.key0 = (uint32_t)(spec->seed & 0xffffffffu); D.key1 = (uint32_t)(spec->seed >> 32); D.env_offset = spec->env_offset;
    D.gamma = spec->gamma; D.gl = spec->gamma * spec->lam;
    // five allocations: the rows, the head, the seven planes in one piece, the partial sums with the fp64 mean behind them, the statistics
    const size_t npartial = (size_t)std::max(r->gae_blocks, r->var_blocks);
    const size_t bytes[5] = {items * (size_t)L.stride * 4, N * (size_t)L.obs_dim * 4, items * ROLLOUT_PLANES * 4, (npartial + 1) * sizeof(double), 3 * sizeof(float)};
    void **ptr[5] = {(void **)&D.rows, (void **)&D.head, (void **)&D.logp, (void **)&D.partial, (void **)&D.stats};
    for (int k = 0; k < 5; k++)
        if (hipMalloc(ptr[k], bytes[k]) != hipSuccess || hipMemset(*ptr[k], 0, bytes[k]) != hipSuccess) {
            rollout_free_storage(r);
            delete r;
            hipGetLastError();     // the failed allocation is reported here, not by the batch's next launch
            return fail(HSR_EDEVICE, "rollout: no device memory for %s bytes", std::to_string(bytes[k]).c_str());
        }
    uint32_t **plane[ROLLOUT_PLANES] = {&D.logp, &D.value, &D.reward, &D.kind, &D.v_term, &D.adv, &D.ret};
    for (int k = 1; k < ROLLOUT_PLANES; k++) *plane[k] = D.logp + (size_t)k * items;
    D.mean64 = D.partial + npartial;
    b->rollouts.push_back(r);
    *out = r;
    return HSR_OK;
}
extern "C" void hsr_rollout_destroy(hsr_rollout *r) {
    if (!r) return;
    if (r->owner) {
        std::vector<hsr_rollout *> &v = r->owner->rollouts;
        v.erase(std::remove(v.begin(), v.end(), r), v.end());
        hipSetDevice(r->device);
        hipStreamSynchronize(r->owner->stream);        // the only stream that uses it
        rollout_free_storage(r);
    }
    delete r;
}
extern "C" int hsr_rollout_state(hsr_rollout *r, int32_t *state, int32_t *t) {
    const int rc = rollout_live(r, "hsr_rollout_state");
    if (rc) return rc;
    if (state) *state = r->books.state;
    if (t) *t = r->books.t;
    return HSR_OK;
}

extern "C" int hsr_rollout_begin_dev(hsr_rollout *r, const float *d_obs) {
    ROLLOUT_ENTER(r, "hsr_rollout_begin_dev", !d_obs ? "null d_obs" : rollout_begin_error(&r->books));
    const RolloutDev &D = r->dev;
    hipLaunchKernelGGL(k_rollout_rows, grid1((size_t)D.N * D.L.obs_dim, ROLLOUT_BLOCK), dim3(ROLLOUT_BLOCK), 0, r->owner->stream, D, -1, (const uint32_t *)d_obs);
    HIPCHK(hipGetLastError());
    rollout_begin_done(&r->books);
    return HSR_OK;
}
extern "C" int hsr_rollout_stage_dev(hsr_rollout *r, const float *d_act, const float *d_logp, const float *d_value) {
    ROLLOUT_ENTER(r, "hsr_rollout_stage_dev", !d_act || !d_logp || !d_value ? "null d_act / d_logp / d_value" : rollout_stage_error(&r->books));
    const RolloutDev &D = r->dev;
    hipLaunchKernelGGL(k_rollout_stage, grid1((size_t)D.N, ROLLOUT_PER_BLOCK), dim3(ROLLOUT_BLOCK), 0, r->owner->stream, D, rollout_stage_slot(&r->books),
                       (const uint32_t *)d_act, (const uint32_t *)d_logp, (const uint32_t *)d_value);
    HIPCHK(hipGetLastError());
    rollout_stage_done(&r->books);
    return HSR_OK;
}
extern "C" int hsr_rollout_close_dev(hsr_rollout *r, const float *d_reward, const uint8_t *d_kind, const float *d_next_obs) {
    ROLLOUT_ENTER(r, "hsr_rollout_close_dev", !d_reward || !d_kind || !d_next_obs ? "null d_reward / d_kind / d_next_obs" : rollout_close_error(&r->books));
    const RolloutDev &D = r->dev;
    hipLaunchKernelGGL(k_rollout_close, grid1((size_t)D.N * D.L.obs_dim, ROLLOUT_BLOCK), dim3(ROLLOUT_BLOCK), 0, r->owner->stream, D, rollout_stage_slot(&r->books),
                       (const uint32_t *)d_reward, d_kind, (const uint32_t *)d_next_obs);
    HIPCHK(hipGetLastError());
    rollout_close_done(&r->books);
    return HSR_OK;
}
extern "C" int hsr_rollout_bootstrap_dev(hsr_rollout *r, const float *d_value_terminal) {
    ROLLOUT_ENTER(r, "hsr_rollout_bootstrap_dev", !d_value_terminal ? "null d_value_terminal" : rollout_bootstrap_error(&r->books));
    const RolloutDev &D = r->dev;
    hipLaunchKernelGGL(k_rollout_rows, grid1((size_t)D.N, ROLLOUT_BLOCK), dim3(ROLLOUT_BLOCK), 0, r->owner->stream, D, rollout_bootstrap_slot(&r->books),
                       (const uint32_t *)d_value_terminal);
    HIPCHK(hipGetLastError());
    return HSR_OK;
}
extern "C" int hsr_rollout_finish_dev(hsr_rollout *r, const float *d_last_value) {
    ROLLOUT_ENTER(r, "hsr_rollout_finish_dev", !d_last_value ? "null d_last_value" : rollout_finish_error(&r->books));
    const RolloutDev &D = r->dev;
    const int items = (int)rollout_items(&r->books);
    hipStream_t s = r->owner->stream;
    hipLaunchKernelGGL(k_rollout_gae, dim3(r->gae_blocks), dim3(ROLLOUT_GAE_BLOCK), 0, s, D, d_last_value);
    hipLaunchKernelGGL(k_rollout_moment, dim3(1), dim3(ROLLOUT_BLOCK), 0, s, D, r->gae_blocks, items, 0);
    hipLaunchKernelGGL(k_rollout_var, dim3(r->var_blocks), dim3(ROLLOUT_BLOCK), 0, s, D, items);
    hipLaunchKernelGGL(k_rollout_moment, dim3(1), dim3(ROLLOUT_BLOCK), 0, s, D, r->var_blocks, items, 1);
    HIPCHK(hipGetLastError());
    rollout_finish_done(&r->books);
    return HSR_OK;
}
extern "C" int hsr_rollout_next(hsr_rollout *r) {
    const int rc = rollout_live(r, "hsr_rollout_next");
    if (rc) return rc;
    const char *why = rollout_read_error(&r->books);
    if (why) return fail(HSR_EINVAL, "hsr_rollout_next: %s", why);
    rollout_next_done(&r->books);
    return HSR_OK;
}
extern "C" int hsr_rollout_stats(hsr_rollout *r, float *mean, float *std, float *rstd) {
    ROLLOUT_ENTER(r, "hsr_rollout_stats", rollout_read_error(&r->books));
    float h[3];
    HIPCHK(hipMemcpyAsync(h, r->dev.stats, sizeof h, hipMemcpyDeviceToHost, r->owner->stream));
    HIPCHK(hipStreamSynchronize(r->owner->stream));
    if (mean) *mean = h[0];
    if (std) *std = h[1];
    if (rstd) *rstd = h[2];
    return HSR_OK;
}
extern "C" int hsr_rollout_minibatch_dev(hsr_rollout *r, uint32_t epoch, int first, int count, int normalize, float *d_obs, float *d_act, float *d_logp,
                                         float *d_value, float *d_adv, float *d_ret, int32_t *d_index) {
    ROLLOUT_ENTER(r, "hsr_rollout_minibatch_dev", rollout_minibatch_error(&r->books, first, count));
    hipLaunchKernelGGL(k_rollout_minibatch, grid1((size_t)count, ROLLOUT_PER_BLOCK), dim3(ROLLOUT_BLOCK), 0, r->owner->stream, r->dev, epoch, first, count,
                       normalize, r->half_bits, (uint32_t *)d_obs, (uint32_t *)d_act, (uint32_t *)d_logp, (uint32_t *)d_value, (uint32_t *)d_adv,
                       (uint32_t *)d_ret, d_index);
    HIPCHK(hipGetLastError());
    return HSR_OK;
}
extern "C" int hsr_rollout_planes_dev(hsr_rollout *r, float *d_adv, float *d_ret) {
    ROLLOUT_ENTER(r, "hsr_rollout_planes_dev", rollout_read_error(&r->books));
    const size_t bytes = (size_t)rollout_items(&r->books) * 4;
    if (d_adv) HIPCHK(hipMemcpyAsync(d_adv, r->dev.adv, bytes, hipMemcpyDeviceToDevice, r->owner->stream));
    if (d_ret) HIPCHK(hipMemcpyAsync(d_ret, r->dev.ret, bytes, hipMemcpyDeviceToDevice, r->owner->stream));
    return HSR_OK;
}
