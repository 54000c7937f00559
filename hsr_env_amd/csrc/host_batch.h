// The hsr_batch record and what every hsr_batch_* entry point shares: error and entry-guard macros, device allocation, the upload and
// staging helpers, the lanes-per-env dispatch.
static_assert(HSR_GEOM_MESH == GEOM_MESH, "host_model.h restates model.h's GEOM_MESH");

#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail(HSR_EDEVICE, "HIP error: %s", hipGetErrorString(e_)); } while (0)
// Every hsr_batch_* entry point starts with one of the two (hsr_batch_stream and hsr_batch_destroy, which do not return a code, test the
// handle themselves): the handle check, and for a function that touches the device the batch's device made current
#define ENTER(b) do { if (!(b)) return fail(HSR_EINVAL, "null batch"); } while (0)
#define ENTER_DEV(b) do { ENTER(b); HIPCHK(hipSetDevice((b)->device)); } while (0)

typedef void (*persist_fn)(const DevModel *, DevState, int, int, float, int, StepIO);
// the chain's captured graphs hold the capture launches too (period, slots, buffer)
struct GraphKey {
    int nsub, goal_body; float geofence; int cap_every, cap_n; const void *cap;
    bool operator<(const GraphKey &o) const { return std::tie(nsub, goal_body, geofence, cap_every, cap_n, cap) < std::tie(o.nsub, o.goal_body, o.geofence, o.cap_every, o.cap_n, o.cap); }
};

// the environment switches that only the creation of a batch reads (read_switches, host_create.h; the others set hsr_batch fields)
struct CreateSwitches {
    bool no_const = false;         // HSR_NO_CONST: never choose a constant kernel instance
    int nfb_max = 1 << 30;         // HSR_NFB: upper bound on DevModel::nfb
    bool tables_lds = false;       // HSR_TABLES_GLOBAL=0: keep the pair / geom tables of the persistent kernel in LDS
    bool debug = false;            // HSR_DEBUG: print the chosen instance's resources
};

struct hsr_batch {
    const hsr_model *model = nullptr;
    CreateSwitches sw;
    int N = 0, device = 0;
    hipStream_t stream = nullptr;
    DevModel dm{};
    DevModel *d_dm = nullptr;       // device copy for kernels that take the model by pointer
    DevState ds{};
    std::vector<void *> allocs;
    float *d_qpos0 = nullptr;      // model qpos0 on the device
    float *d_stage = nullptr;      // staging for host-pointer API: max(N*(nq+nv), ...) floats
    size_t stage_floats = 0;
    uint8_t *d_stage_u8 = nullptr;
    int32_t *d_stage_i32 = nullptr;
    int narrow_blocks = 2048;      // persistent-style grid of k_narrow (HSR_NARROW_BLOCKS overrides)
    int pairs_per_wave = 4;        // k_collide: pairs walked by one wave (HSR_PPW overrides)
    int group = 16;                // lanes per env of the cooperative solver
    size_t mf_lds_bytes = 0;
    bool persist = false;          // whole env-step in one persistent kernel (k_env_step_mf); hsr_batch_set_persistent(b, 0) disables
    bool use_graph = true, profiling = false, debug_store = false;
    // the persistent-kernel instance, chosen once at creation (plan_persist) and read by every later use
    int const_row = -1;            // row of kCfgConsts (cfg_consts.h) whose constant instance serves the model, -1 = a generic instance
    bool kin3 = false;             // ... and that instance knows the model's kinematic tree at compile time (kin3.h)
    bool persist_tg = false;       // the instance reads its pair / geom tables from global memory (LDS budget)
    persist_fn kernel = nullptr;   // the instance; NULL: the model does not fit the persistent kernel (lane maps, LDS, kinematic structure)
    persist_fn kernel_sv = nullptr;     // its twin with the solo-server path, NULL if there is none
    size_t persist_lds_bytes = 0;
    bool mpr_warm = true;          // penetrating convex pairs start MPR from the portal of their previous substep (HSR_MPR_WARM=0 / hsr_batch_set_mpr_warm turn it off)
    int test_hooks = 0;            // hsr_batch_set_debug bits 1.. : force rarely taken solver branches (tests only)
    bool schedule = true;          // re-pack the envs over the waves of the persistent kernel before every launch (HSR_SCHEDULE=0 / hsr_batch_set_schedule turn it off)
    int *d_slot_env = nullptr;
    std::map<GraphKey, hipGraphExec_t> graphs;
    float last_total_ms = 0, last_kernel_ms[3] = {0, 0, 0};
    int last_launches[3] = {0, 0, 0};
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::vector<hipEvent_t> kev;
    int slots = 0;                 // workgroups of the persistent kernel the GPU holds at once (occupancy x compute units)
    int queue = -1;                // work queue of the persistent kernel: -1 = automatic (on when there are more tasks than slots), 0 / 1 forced (HSR_QUEUE)
    int queue_chunk = 20;          // substeps per round of the work queue (HSR_QUEUE_CHUNK)
    bool queue_chunk_set = false;  // ... chosen by the caller (environment / hsr_batch_set_queue): no automatic choice then
    int solo_servers = 0;          // workgroups of a queued launch that run hard envs alone (persist.h; hsr_batch_set_solo / HSR_SOLO); 0 = off
    float solo_trips = 3.5f;       // hand-over threshold: Newton iterations per substep over a round
    // hard envs handed over inside a launch without the queue (persist.h, split_logic.h; hsr_batch_set_split / HSR_SPLIT*)
    bool handovers_counted = false;     // the last persistent launch counted hand-overs in sq_ctl (queued or splitting); else hsr_batch_solo_handovers says 0
    bool split_inst = false;       // the kernel instance is one whose launches may split (host_create.h: kPersistInstances)
    bool split = true;             // on by default: measured on the headline; HSR_SPLIT=0 / hsr_batch_set_split(b, 0, ...) turn it off
    int split_period = 8;          // substeps between two check points of a wave (swept: 8 / 16 / 32)
    float split_trips = 2.0f;      // an env is hard at this many Newton iterations per substep over the window (swept: 1.5 / 2.0 / 2.5 / 3.5 / 4.5)
    int split_min_left = 40;       // no hand-over with fewer substeps ahead
    int split_extra = 0;           // tests: workgroups without a task that start as helpers
    bool split_lone = true;        // the lone rule (split_decide_lone), on by default: measured on the headline; HSR_SPLIT_LONE=0 / hsr_batch_set_split_lone(b, 0, ...) turn it off
    float split_lone_trips = 4.5f; // a wave's hardest env leaves easier neighbours at this many Newton iterations per substep over the window (swept: 2.5 / 3.5 / 4.5)
    bool kernel_log = false;       // hsr_batch_set_profiling(b, 2): an event pair around every launch of the persistent kernel, no synchronisation
    std::vector<std::pair<hipEvent_t, hipEvent_t>> klog;
    // ray caster (hsr_batch_render*): its own tables and buffers, built on first use; it never touches the simulation state
    float4 *d_planes = nullptr;    // hull face planes of every mesh geom
    int2 *d_prange = nullptr;      // [ngeom] (offset, count) into d_planes
    float4 *d_rgba = nullptr;      // [ngeom] colours of the next render
    std::vector<float> rgba_host;  // what d_rgba holds
    void *d_rimg = nullptr;        // staging of the host variant: rgb | depth | segid
    size_t rimg_bytes = 0;
    // in-step frame capture (hsr_batch_set_capture): every cap_every substeps, the poses of the envs in the cap_n slots (model.h: StepIO::cap)
    int cap_every = 0, cap_n = 0;  // cap_every = 0: off
    CaptureDesc *d_cap_desc = nullptr;     // what the persistent kernel reads (model.h)
    int *d_cap_slot = nullptr;     // [N] slot of every env, -1: none
    int *d_cap_env = nullptr;      // [HSR_CAPTURE_MAX] env of every slot
    int *d_cap_cnt = nullptr;      // [HSR_CAPTURE_MAX] frames of every slot in the last step
    float *d_cap = nullptr;        // [rows][12 nlink][cap_n]: the frames of the last step, its final poses in the last row
    size_t cap_floats = 0;
    int cap_rows = 0;              // rows of the last step (frames of its longest possible run + the final one); 0: none since the last set_capture
    // episodes on the device (hsr_batch_set_episodes, host_episode.h): the spec's tables and the per-env books, allocated by the first call
    EpisodeDev ep{};
    bool ep_set = false;           // hsr_batch_set_episodes succeeded at least once: the episode entry points may run
    float *d_ep_range = nullptr;   // [2 nq]: qpos_lo | qpos_hi
    int *d_ep_block_qadr = nullptr;     // [free bodies of the model]
    // snapshots (host_snapshot.h): the ones this batch made and nobody destroyed yet - hsr_batch_destroy releases their storage -, and the
    // scratch one hsr_batch_copy_envs* goes through, made by its first call (one of `snapshots`, so its storage goes the same way);
    // the record's descriptor table (snapshot.h), built by the first launch that needs it
    std::vector<hsr_snapshot *> snapshots;
    hsr_snapshot *fork_scratch = nullptr;
    SnapTable snap_tab{};
    bool snap_tab_built = false;   // snap_table checks the episode books' pointers in it against the batch's on every use
    // hindsight replays (host_replay.h) this batch made and nobody destroyed yet: hsr_batch_destroy releases their storage
    std::vector<hsr_replay *> replays;
    // on-policy rollouts (host_rollout.h), likewise
    std::vector<hsr_rollout *> rollouts;
    // running-moments normalisers (host_normalize.h), likewise
    std::vector<hsr_norm *> norms;
    // cross-entropy-method planners (host_plan.h), likewise
    std::vector<hsr_plan *> plans;
};
static void snap_release_all(hsr_batch *b);     // host_snapshot.h
static void replay_release_all(hsr_batch *b);   // host_replay.h
static void rollout_release_all(hsr_batch *b);  // host_rollout.h
static void norm_release_all(hsr_batch *b);     // host_normalize.h
static void plan_release_all(hsr_batch *b);     // host_plan.h
template <typename T>
static int dalloc(hsr_batch *b, T **p, size_t count) {
    void *q = nullptr;
    HIPCHK(hipMalloc(&q, (count ? count : 1) * sizeof(T)));
    HIPCHK(hipMemset(q, 0, (count ? count : 1) * sizeof(T)));
    b->allocs.push_back(q);
    *p = (T *)q;
    return HSR_OK;
}
// a host array on the device: allocated (hsr_batch_destroy frees it) with `pad` zeroed elements behind it, copied, the pointer stored
template <typename D, typename T>
static int upload(hsr_batch *b, D *dst, const T *src, size_t count, size_t pad = 0) {
    T *d;
    const int rc = dalloc(b, &d, count + pad);
    if (rc) return rc;
    if (count) HIPCHK(hipMemcpy(d, src, count * sizeof(T), hipMemcpyHostToDevice));
    *dst = (D)d;
    return HSR_OK;
}
template <typename D, typename T>
static int upload(hsr_batch *b, D *dst, const std::vector<T> &v, size_t pad = 0) { return upload(b, dst, v.data(), v.size(), pad); }
// `count` elements of a device buffer (the staging area, as a rule) to the caller's array; waits for the stream
template <typename T>
static int stage_to_host(hsr_batch *b, T *host, const T *d_src, size_t count) {
    HIPCHK(hipMemcpyAsync(host, d_src, count * sizeof(T), hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    return HSR_OK;
}
// f(lanes per env as a compile-time constant): the cooperative solver and the persistent kernel's layout exist for 16 and 32 lanes
template <typename F>
static auto by_group(int group, F f) { return group == 16 ? f(std::integral_constant<int, 16>()) : f(std::integral_constant<int, 32>()); }
// what the persistent kernel reads of the capture settings (model.h: CaptureDesc), after d_cap, the period or the slots changed
static int upload_capture_desc(hsr_batch *b, int every, int n) {
    const CaptureDesc cd{b->d_cap, b->d_cap_slot, every, n};
    HIPCHK(hipMemcpy(b->d_cap_desc, &cd, sizeof cd, hipMemcpyHostToDevice));
    return HSR_OK;
}
static int require_captured_step(const hsr_batch *b, const char *who) {
    if (b->cap_every <= 0 || b->cap_rows <= 0) return fail(HSR_EINVAL, "%s: no captured step (hsr_batch_set_capture, then a step)", who);
    return HSR_OK;
}
static inline dim3 grid1(size_t n, int t = 256) { return dim3((unsigned)((n + t - 1) / t)); }
// the work queue's watchdog (persist.h: q_claim) tripped in some launch since the last check: the flag is sticky on the device (no launch
// clears it) and only this function resets it, after reading it - every synchronising entry point ends with it
static int queue_error(hsr_batch *b) {
    int err = 0;
    if (b->ds.q_err && hipMemcpy(&err, b->ds.q_err, sizeof err, hipMemcpyDeviceToHost) == hipSuccess && err) {
        hipMemset(b->ds.q_err, 0, sizeof err);
        return fail(HSR_EDEVICE, "persistent kernel: a work-queue ticket was never served (launch drained by its watchdog)");
    }
    return HSR_OK;
}
