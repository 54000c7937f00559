// The cross-entropy-method planner: the hsr_plan record, its storage and the launches of plan.h.  Which numbers are acceptable is decided by
// the plain functions of plan_logic.h; a refused call launches nothing.  A planner is bound to its (planning) batch: it launches on that
// batch's stream and reads that batch's poses, mocap points and done / bad flags.  It is not part of an env record (snapshot.h).

struct hsr_plan {
    hsr_batch *owner = nullptr;    // NULL once hsr_batch_destroy released the storage
    int device = 0;
    PlanDev dev{};
    std::vector<void *> mem;
};

static void plan_free_storage(hsr_plan *r) {
    for (void *p : r->mem) hipFree(p);
    r->mem.clear();
    r->dev = PlanDev{};
}
// hsr_batch_destroy: as for replays and normalisers, the storage goes with the batch and the handle stays the caller's to destroy
static void plan_release_all(hsr_batch *b) {
    for (hsr_plan *r : b->plans) { plan_free_storage(r); r->owner = nullptr; }
    b->plans.clear();
}
static int plan_live(const hsr_plan *r, const char *who) {
    if (!r) return fail(HSR_EINVAL, "%s: null planner", who);
    if (!r->owner) return fail(HSR_EINVAL, "%s: the planner's batch was destroyed, and its storage with it", who);
    return HSR_OK;
}
// the common opening of a call (who: a string literal): the handle, the checks' verdict, the device made current
#define PLAN_ENTER(r, who, why_expr) do { \
        const int rc_ = plan_live((r), who); \
        if (rc_) return rc_; \
        const char *why_ = (why_expr); \
        if (why_) return fail(HSR_EINVAL, who ": %s", why_); \
        HIPCHK(hipSetDevice((r)->device)); \
    } while (0)
template <typename T>
static bool plan_alloc(hsr_plan *r, T **p, size_t count) {
    void *q = nullptr;
    if (hipMalloc(&q, count * sizeof(T)) != hipSuccess) return false;
    r->mem.push_back(q);
    if (hipMemset(q, 0, count * sizeof(T)) != hipSuccess) return false;
    *p = (T *)q;
    return true;
}
static int plan_launch_reset(hsr_plan *r, const uint8_t *d_mask, int shift) {
    const PlanDev &D = r->dev;
    hipLaunchKernelGGL(k_plan_reset, grid1((size_t)D.P * D.nu, PLAN_BLOCK), dim3(PLAN_BLOCK), 0, r->owner->stream, D, r->owner->dm.act_ctrlrange, d_mask, shift);
    HIPCHK(hipGetLastError());
    return HSR_OK;
}

extern "C" int hsr_batch_plan_create(hsr_batch *b, const hsr_plan_spec *spec, hsr_plan **out) {
    ENTER_DEV(b);
    if (!spec || !out) return fail(HSR_EINVAL, "hsr_batch_plan_create: null argument");
    const char *why = plan_spec_error(b->N, spec->groups, spec->samples, spec->horizon, spec->elites, spec->goal_body, spec->gamma, spec->alpha, spec->init_std,
                                      spec->min_std, b->dm.nu, b->dm.nbody, b->model->i32("body_mocap"), b->ds.ngoal);
    if (why) return fail(HSR_EINVAL, "hsr_batch_plan_create: %s", why);
    hsr_plan *r = new hsr_plan();
    r->owner = b; r->device = b->device;
    PlanDev &D = r->dev;
    D.P = spec->groups; D.K = spec->samples; D.H = spec->horizon; D.nu = b->dm.nu; D.N = b->N; D.elites = spec->elites;
    D.key0 = (uint32_t)(spec->seed & 0xffffffffu); D.key1 = (uint32_t)(spec->seed >> 32); D.env_offset = spec->env_offset;
    D.goal_body = spec->goal_body;
    D.gamma = spec->gamma; D.alpha = spec->alpha; D.init_std = spec->init_std; D.min_std = spec->min_std;
    const size_t P = (size_t)D.P, N = (size_t)D.N, row = (size_t)D.H * D.nu;
    const bool ok = plan_alloc(r, &D.mean, P * row) && plan_alloc(r, &D.sigma, P * row) && plan_alloc(r, &D.act, N * row) && plan_alloc(r, &D.J, N) &&
                    plan_alloc(r, &D.g, N) && plan_alloc(r, &D.alive, N) && plan_alloc(r, &D.reach, N) && plan_alloc(r, &D.failed, P) &&
                    plan_alloc(r, &D.best_index, P) && plan_alloc(r, &D.best_cost, P);
    if (!ok) {
        plan_free_storage(r);
        delete r;
        hipGetLastError();         // the failed allocation is reported here, not by the batch's next launch
        return fail(HSR_EDEVICE, "planner: no device memory");
    }
    // a new planner is a reset one with a begun iteration: every field a reader may ask for is defined
    int rc = plan_launch_reset(r, nullptr, 0);
    if (!rc) {
        hipLaunchKernelGGL(k_plan_begin, grid1(N, PLAN_BLOCK), dim3(PLAN_BLOCK), 0, b->stream, D);
        if (hipGetLastError() != hipSuccess) rc = fail(HSR_EDEVICE, "planner: launch failed");
    }
    if (rc) { hipStreamSynchronize(b->stream); plan_free_storage(r); delete r; return rc; }
    b->plans.push_back(r);
    *out = r;
    return HSR_OK;
}
extern "C" void hsr_plan_destroy(hsr_plan *r) {
    if (!r) return;
    if (r->owner) {
        std::vector<hsr_plan *> &v = r->owner->plans;
        v.erase(std::remove(v.begin(), v.end(), r), v.end());
        hipSetDevice(r->device);
        hipStreamSynchronize(r->owner->stream);        // the only stream that uses it
        plan_free_storage(r);
    }
    delete r;
}

extern "C" int hsr_plan_reset_dev(hsr_plan *r, const uint8_t *d_mask) {
    PLAN_ENTER(r, "hsr_plan_reset_dev", nullptr);
    return plan_launch_reset(r, d_mask, 0);
}
extern "C" int hsr_plan_shift_dev(hsr_plan *r, const uint8_t *d_mask) {
    PLAN_ENTER(r, "hsr_plan_shift_dev", nullptr);
    return plan_launch_reset(r, d_mask, 1);
}
extern "C" int hsr_plan_begin_dev(hsr_plan *r) {
    PLAN_ENTER(r, "hsr_plan_begin_dev", nullptr);
    hipLaunchKernelGGL(k_plan_begin, grid1((size_t)r->dev.N, PLAN_BLOCK), dim3(PLAN_BLOCK), 0, r->owner->stream, r->dev);
    HIPCHK(hipGetLastError());
    return HSR_OK;
}
extern "C" int hsr_plan_sample_dev(hsr_plan *r, uint32_t call, int iter, int h, float *d_ctrl) {
    PLAN_ENTER(r, "hsr_plan_sample_dev", plan_sample_error(iter, h, r->dev.H, d_ctrl));
    const PlanDev &D = r->dev;
    hipLaunchKernelGGL(k_plan_sample, grid1((size_t)D.N * D.nu, PLAN_BLOCK), dim3(PLAN_BLOCK), 0, r->owner->stream, D, r->owner->dm.act_ctrlrange, call, iter, h, d_ctrl);
    HIPCHK(hipGetLastError());
    return HSR_OK;
}
extern "C" int hsr_plan_accumulate_dev(hsr_plan *r, int h) {
    PLAN_ENTER(r, "hsr_plan_accumulate_dev", plan_step_error(h, r->dev.H));
    hsr_batch *b = r->owner;
    if (b->ds.ngoal > 0) return fail(HSR_EINVAL, "hsr_plan_accumulate_dev: the batch has extra goal terms now (hsr_batch_set_goals)");
    hipLaunchKernelGGL(k_plan_accumulate, grid1((size_t)r->dev.N, PLAN_BLOCK), dim3(PLAN_BLOCK), 0, b->stream, b->dm, b->ds, r->dev, h);
    HIPCHK(hipGetLastError());
    return HSR_OK;
}
extern "C" int hsr_plan_add_cost_dev(hsr_plan *r, const float *d_extra) {
    PLAN_ENTER(r, "hsr_plan_add_cost_dev", d_extra ? nullptr : "null d_extra");
    hipLaunchKernelGGL(k_plan_add_cost, grid1((size_t)r->dev.N, PLAN_BLOCK), dim3(PLAN_BLOCK), 0, r->owner->stream, r->dev, d_extra);
    HIPCHK(hipGetLastError());
    return HSR_OK;
}
extern "C" int hsr_plan_update_dev(hsr_plan *r) {
    PLAN_ENTER(r, "hsr_plan_update_dev", nullptr);
    const PlanDev &D = r->dev;
    const int threads = (D.K + PLAN_WAVE - 1) / PLAN_WAVE * PLAN_WAVE;
    hipLaunchKernelGGL(k_plan_update, dim3(D.P), dim3(threads), 0, r->owner->stream, D, r->owner->dm.act_ctrlrange);
    HIPCHK(hipGetLastError());
    return HSR_OK;
}
extern "C" int hsr_plan_action_dev(hsr_plan *r, float *d_ctrl) {
    PLAN_ENTER(r, "hsr_plan_action_dev", d_ctrl ? nullptr : "null d_ctrl");
    const PlanDev &D = r->dev;
    hipLaunchKernelGGL(k_plan_action, grid1((size_t)D.P * D.nu, PLAN_BLOCK), dim3(PLAN_BLOCK), 0, r->owner->stream, D, d_ctrl);
    HIPCHK(hipGetLastError());
    return HSR_OK;
}

// readers: device-to-device copies on the batch's stream; every output may be NULL
static int plan_copy_out(hsr_plan *r, void *dst, const void *src, size_t bytes) {
    if (dst && bytes) HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, r->owner->stream));
    return HSR_OK;
}
extern "C" int hsr_plan_costs_dev(hsr_plan *r, float *d_cost, int32_t *d_reach_step) {
    PLAN_ENTER(r, "hsr_plan_costs_dev", nullptr);
    const size_t N = (size_t)r->dev.N;
    const int rc = plan_copy_out(r, d_cost, r->dev.J, N * sizeof(float));
    return rc ? rc : plan_copy_out(r, d_reach_step, r->dev.reach, N * sizeof(int32_t));
}
extern "C" int hsr_plan_state_dev(hsr_plan *r, float *d_mean, float *d_sigma) {
    PLAN_ENTER(r, "hsr_plan_state_dev", nullptr);
    const size_t bytes = (size_t)r->dev.P * r->dev.H * r->dev.nu * sizeof(float);
    const int rc = plan_copy_out(r, d_mean, r->dev.mean, bytes);
    return rc ? rc : plan_copy_out(r, d_sigma, r->dev.sigma, bytes);
}
extern "C" int hsr_plan_best_dev(hsr_plan *r, int32_t *d_index, float *d_cost) {
    PLAN_ENTER(r, "hsr_plan_best_dev", nullptr);
    const size_t P = (size_t)r->dev.P;
    const int rc = plan_copy_out(r, d_index, r->dev.best_index, P * sizeof(int32_t));
    return rc ? rc : plan_copy_out(r, d_cost, r->dev.best_cost, P * sizeof(float));
}
extern "C" int hsr_plan_failed(hsr_plan *r, uint32_t *failed) {
    PLAN_ENTER(r, "hsr_plan_failed", failed ? nullptr : "null failed");
    HIPCHK(hipMemcpyAsync(failed, r->dev.failed, (size_t)r->dev.P * sizeof(uint32_t), hipMemcpyDeviceToHost, r->owner->stream));
    HIPCHK(hipStreamSynchronize(r->owner->stream));
    return HSR_OK;
}
