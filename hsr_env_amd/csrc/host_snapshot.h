// Snapshots: env records kept on the device (snapshot.h), saved from / loaded into a batch, copied env to env inside one, and their host
// image for checkpoint files.  Nothing here runs a forward pass or touches an array outside the record (snapshot.h lists it).

struct hsr_snapshot {
    hsr_batch *owner = nullptr;    // the batch that made it (its hsr_batch_destroy releases the storage); NULL once that batch is gone
    int device = 0;
    uint64_t fingerprint = 0;      // of the model blob (hsr_model_load): a snapshot is bound to a model layout and a device, not to a batch
    int dims[SNAP_NDIM] = {0, 0, 0, 0, 0};
    int words = 0, capacity = 0;
    uint32_t *d = nullptr;         // [words][capacity]
};

static void snap_model_dims(const hsr_model *m, int dims[SNAP_NDIM]) {
    dims[0] = m->sizes[HSR_NQ]; dims[1] = m->sizes[HSR_NV]; dims[2] = m->sizes[HSR_NU]; dims[3] = m->sizes[HSR_NLINK];
    dims[4] = std::max(m->sizes[HSR_NPAIR], 1);
}
// the batch's arrays behind the record's fields: built by the first launch that needs it and kept in the batch.  The DevState arrays live
// as long as the batch; the episode books appear with hsr_batch_set_episodes, so the three pointers kept for them are compared with the
// batch's on every use and the table is built again when they differ (today: once, when the books are allocated)
static const SnapTable &snap_table(hsr_batch *b) {
    const DevState &s = b->ds;
    const EpisodeDev &E = b->ep;
    void *books[3] = {b->ep_set ? E.ep_index : nullptr, b->ep_set ? E.ep_length : nullptr, b->ep_set ? E.ep_return : nullptr};
    const SnapField *f = b->snap_tab.f;
    if (b->snap_tab_built && f[SNAP_EP_INDEX].base == books[0] && f[SNAP_EP_LENGTH].base == books[1] && f[SNAP_EP_RETURN].base == books[2]) return b->snap_tab;
    void *base[SNAP_NFIELD] = {s.qpos, s.qvel, s.ctrl, s.mocap, s.warm, s.time, s.done, s.bad, s.nsteps, s.tick, s.sepax, s.septick, s.trips,
                               s.xpos, s.xmat, s.lvel, books[0], books[1], books[2]};
    int dims[SNAP_NDIM], rows[SNAP_NFIELD];
    snap_model_dims(b->model, dims);
    SnapTable &t = b->snap_tab;
    t.words = snap_field_rows(dims, rows);
    t.N = b->N;
    for (int k = 0, row = 0; k < SNAP_NFIELD; row += rows[k], k++) t.f[k] = SnapField{(uint32_t *)base[k], row, rows[k]};
    b->snap_tab_built = true;
    return t;
}
static int snap_alloc(hsr_batch *b, int capacity, hsr_snapshot **out) {
    hsr_snapshot *s = new hsr_snapshot();
    s->owner = b; s->device = b->device; s->fingerprint = b->model->fingerprint; s->capacity = capacity;
    snap_model_dims(b->model, s->dims);
    int rows[SNAP_NFIELD];
    s->words = snap_field_rows(s->dims, rows);
    const size_t bytes = (size_t)s->words * capacity * sizeof(uint32_t);
    if (hipMalloc((void **)&s->d, bytes) != hipSuccess || hipMemset(s->d, 0, bytes) != hipSuccess) {
        if (s->d) hipFree(s->d);
        delete s;
        return fail(HSR_EDEVICE, "snapshot: no device memory for %s bytes", std::to_string(bytes).c_str());
    }
    b->snapshots.push_back(s);
    *out = s;
    return HSR_OK;
}
// hsr_batch_destroy: the storage of every snapshot the batch made goes with it; a handle the caller still holds stays valid for
// hsr_snapshot_destroy (and refuses everything else).  The scratch snapshot of hsr_batch_copy_envs* is one of them; nobody else holds its
// handle, so that goes too.
static void snap_release_all(hsr_batch *b) {
    for (hsr_snapshot *s : b->snapshots) { hipFree(s->d); s->d = nullptr; s->owner = nullptr; }
    b->snapshots.clear();
    delete b->fork_scratch;
    b->fork_scratch = nullptr;
}
// what the host can see of a (batch, snapshot, n) triple: handles, the storage still there, same model layout, same device, n
static int snap_check(const hsr_batch *b, const hsr_snapshot *s, int n, const char *who) {
    if (!s) return fail(HSR_EINVAL, "%s: null snapshot", who);
    if (!s->d) return fail(HSR_EINVAL, "%s: the batch that made the snapshot was destroyed, and its storage with it", who);
    int dims[SNAP_NDIM];
    snap_model_dims(b->model, dims);
    if (s->fingerprint != b->model->fingerprint || memcmp(s->dims, dims, sizeof dims) != 0) return fail(HSR_EINVAL, "%s: the snapshot belongs to another model", who);
    if (s->device != b->device) return fail(HSR_EINVAL, "%s: the snapshot lives on another device", who);
    if (n < 0 || n > b->N || n > s->capacity) return fail(HSR_EINVAL, "%s: n outside 0 .. min(envs, capacity)", who);
    return HSR_OK;
}
// ids[0..n) inside 0..range (NULL: the identity), and - for the side that is written - no id twice
static int snap_check_ids(const int32_t *ids, int n, int range, bool distinct, const char *who) {
    if (!ids) return HSR_OK;                   // 0..n-1, and n <= range was checked
    std::vector<char> seen(distinct ? range : 0, 0);
    for (int i = 0; i < n; i++) {
        if (ids[i] < 0 || ids[i] >= range) return fail(HSR_EINVAL, "%s: an id is out of range", who);
        if (distinct && seen[ids[i]]++) return fail(HSR_EINVAL, "%s: a destination appears twice", who);
    }
    return HSR_OK;
}
static int snap_launch(hsr_batch *b, uint32_t *store, int capacity, const int32_t *d_env, const int32_t *d_slot, int n, int to_batch) {
    if (n == 0) return HSR_OK;
    const SnapTable &t = snap_table(b);
    if (t.words > 65535) return fail(HSR_EINVAL, "snapshot: a record of %s words exceeds the 65535 rows one launch covers", std::to_string(t.words).c_str());
    hipLaunchKernelGGL(k_snapshot_copy, dim3((unsigned)((n + 255) / 256), (unsigned)t.words), dim3(256), 0, b->stream, t, store, capacity, d_env, d_slot, n, to_batch);
    HIPCHK(hipGetLastError());
    return HSR_OK;
}
// two host id arrays (either may be NULL) into the batch's staging area, as device pointers
static int snap_stage_ids(hsr_batch *b, const int32_t *a, const int32_t *c, int n, const int32_t **d_a, const int32_t **d_c) {
    int32_t *st = (int32_t *)b->d_stage;       // stage_floats > 2 N (alloc_staging_and_reset)
    *d_a = *d_c = nullptr;
    if (a && n) { HIPCHK(hipMemcpyAsync(st, a, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, b->stream)); *d_a = st; }
    if (c && n) { HIPCHK(hipMemcpyAsync(st + n, c, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, b->stream)); *d_c = st + n; }
    return HSR_OK;
}

extern "C" int hsr_batch_snapshot_create(hsr_batch *b, int capacity, hsr_snapshot **out) {
    ENTER_DEV(b);
    if (!out) return fail(HSR_EINVAL, "hsr_batch_snapshot_create: null argument");
    if (capacity < 1) return fail(HSR_EINVAL, "hsr_batch_snapshot_create: capacity < 1");
    return snap_alloc(b, capacity, out);
}
extern "C" void hsr_snapshot_destroy(hsr_snapshot *s) {
    if (!s) return;
    if (s->owner) {
        std::vector<hsr_snapshot *> &v = s->owner->snapshots;
        v.erase(std::remove(v.begin(), v.end(), s), v.end());
        hipSetDevice(s->device);
        hipDeviceSynchronize();                // whichever batch's stream used it last
        hipFree(s->d);
    }
    delete s;
}
extern "C" int hsr_snapshot_capacity(const hsr_snapshot *s) { return s ? s->capacity : fail(HSR_EINVAL, "null snapshot"); }

extern "C" int hsr_batch_snapshot_save_dev(hsr_batch *b, hsr_snapshot *s, const int32_t *d_env, const int32_t *d_slot, int n) {
    ENTER_DEV(b);
    const int rc = snap_check(b, s, n, "hsr_batch_snapshot_save_dev");
    return rc ? rc : snap_launch(b, s->d, s->capacity, d_env, d_slot, n, 0);
}
extern "C" int hsr_batch_snapshot_load_dev(hsr_batch *b, const hsr_snapshot *s, const int32_t *d_slot, const int32_t *d_env, int n) {
    ENTER_DEV(b);
    const int rc = snap_check(b, s, n, "hsr_batch_snapshot_load_dev");
    return rc ? rc : snap_launch(b, s->d, s->capacity, d_env, d_slot, n, 1);
}
static int snap_host(hsr_batch *b, const hsr_snapshot *s, const int32_t *env, const int32_t *slot, int n, int to_batch, const char *who) {
    int rc;
    if ((rc = snap_check(b, s, n, who))) return rc;
    if ((rc = snap_check_ids(env, n, b->N, to_batch != 0, who)) || (rc = snap_check_ids(slot, n, s->capacity, to_batch == 0, who))) return rc;
    const int32_t *d_env, *d_slot;
    if ((rc = snap_stage_ids(b, env, slot, n, &d_env, &d_slot)) || (rc = snap_launch(b, s->d, s->capacity, d_env, d_slot, n, to_batch))) {
        hipStreamSynchronize(b->stream);       // a copy of the caller's ids may be pending: they are the caller's again on return
        return rc;
    }
    HIPCHK(hipStreamSynchronize(b->stream));
    return queue_error(b);
}
extern "C" int hsr_batch_snapshot_save(hsr_batch *b, hsr_snapshot *s, const int32_t *env, const int32_t *slot, int n) {
    ENTER_DEV(b);
    return snap_host(b, s, env, slot, n, 0, "hsr_batch_snapshot_save");
}
extern "C" int hsr_batch_snapshot_load(hsr_batch *b, const hsr_snapshot *s, const int32_t *slot, const int32_t *env, int n) {
    ENTER_DEV(b);
    return snap_host(b, s, env, slot, n, 1, "hsr_batch_snapshot_load");
}

// dst[i] <- src[i] with every source read before any destination is written: through the batch's scratch snapshot (made by the first
// call, replaced by a larger one - after the stream has drained - when n exceeds it), record i in slot i.  Two launches on the stream.
static int snap_fork(hsr_batch *b, const int32_t *d_src, const int32_t *d_dst, int n) {
    if (n == 0) return HSR_OK;
    if (!b->fork_scratch || b->fork_scratch->capacity < n) {
        HIPCHK(hipStreamSynchronize(b->stream));
        if (b->fork_scratch) { hsr_snapshot *old = b->fork_scratch; b->fork_scratch = nullptr; hsr_snapshot_destroy(old); }
        const int rc = snap_alloc(b, n, &b->fork_scratch);     // stays in b->snapshots: snap_release_all frees its storage with the others
        if (rc) return rc;
    }
    hsr_snapshot *s = b->fork_scratch;
    const int rc = snap_launch(b, s->d, s->capacity, d_src, nullptr, n, 0);
    return rc ? rc : snap_launch(b, s->d, s->capacity, d_dst, nullptr, n, 1);
}
extern "C" int hsr_batch_copy_envs_dev(hsr_batch *b, const int32_t *d_src, const int32_t *d_dst, int n) {
    ENTER_DEV(b);
    if (n < 0 || n > b->N) return fail(HSR_EINVAL, "hsr_batch_copy_envs_dev: n outside 0 .. envs");
    return snap_fork(b, d_src, d_dst, n);
}
extern "C" int hsr_batch_copy_envs(hsr_batch *b, const int32_t *src, const int32_t *dst, int n) {
    ENTER_DEV(b);
    const char *who = "hsr_batch_copy_envs";
    if (n < 0 || n > b->N) return fail(HSR_EINVAL, "%s: n outside 0 .. envs", who);
    int rc;
    if ((rc = snap_check_ids(src, n, b->N, false, who)) || (rc = snap_check_ids(dst, n, b->N, true, who))) return rc;
    const int32_t *d_src, *d_dst;
    if ((rc = snap_stage_ids(b, src, dst, n, &d_src, &d_dst)) || (rc = snap_fork(b, d_src, d_dst, n))) {
        hipStreamSynchronize(b->stream);       // as in snap_host
        return rc;
    }
    HIPCHK(hipStreamSynchronize(b->stream));
    return queue_error(b);
}

// ---- host image: SnapImageHeader (little-endian, 56 bytes), then the words [words][capacity] exactly as stored
struct SnapImageHeader {
    char magic[8];                 // "HSRSNAP1"
    uint32_t version, header_bytes;
    uint64_t fingerprint;
    int64_t capacity;
    int32_t dims[SNAP_NDIM], words;
};
static_assert(sizeof(SnapImageHeader) == 56, "the image header is packed by construction");
static const char kSnapMagic[9] = "HSRSNAP1";
enum { SNAP_IMAGE_VERSION = 1 };

static long long snap_image_bytes(int words, int capacity) { return (long long)sizeof(SnapImageHeader) + 4LL * words * capacity; }
// an image of `len` bytes against a model layout: HSR_EBLOB unless every header field is the expected one and len is exactly the size the
// header implies (computed by division: a capacity whose byte count does not fit 63 bits never reaches a multiplication)
static int snap_image_check(uint64_t fingerprint, const int dims[SNAP_NDIM], const void *image, long long len, int *capacity) {
    int rows[SNAP_NFIELD];
    const int words = snap_field_rows(dims, rows);
    SnapImageHeader h;
    if (len < (long long)sizeof h) return fail(HSR_EBLOB, "snapshot image: shorter than its header");
    memcpy(&h, image, sizeof h);
    if (memcmp(h.magic, kSnapMagic, 8) != 0) return fail(HSR_EBLOB, "snapshot image: wrong magic");
    if (h.version != SNAP_IMAGE_VERSION || h.header_bytes != sizeof h) return fail(HSR_EBLOB, "snapshot image: unknown format version");
    if (h.fingerprint != fingerprint) return fail(HSR_EBLOB, "snapshot image: written for another model");
    if (memcmp(h.dims, dims, sizeof h.dims) != 0 || h.words != words) return fail(HSR_EBLOB, "snapshot image: record layout differs from the model's");
    const long long body = len - (long long)sizeof h, per_slot = 4LL * words;
    if (h.capacity < 1 || h.capacity > 0x7fffffffLL || body % per_slot != 0 || body / per_slot != h.capacity)
        return fail(HSR_EBLOB, "snapshot image: length does not match its capacity");
    if (capacity) *capacity = (int)h.capacity;
    return HSR_OK;
}
extern "C" int hsr_model_snapshot_record_words(const hsr_model *m) {
    if (!m) return fail(HSR_EINVAL, "null model");
    int dims[SNAP_NDIM], rows[SNAP_NFIELD];
    snap_model_dims(m, dims);
    return snap_field_rows(dims, rows);
}
extern "C" int hsr_model_snapshot_image_check(const hsr_model *m, const void *image, long long len, int *capacity) {
    if (!m || !image) return fail(HSR_EINVAL, "hsr_model_snapshot_image_check: null argument");
    int dims[SNAP_NDIM];
    snap_model_dims(m, dims);
    return snap_image_check(m->fingerprint, dims, image, len, capacity);
}
extern "C" int hsr_snapshot_image_bytes(const hsr_snapshot *s, long long *out) {
    if (!s || !out) return fail(HSR_EINVAL, "hsr_snapshot_image_bytes: null argument");
    *out = snap_image_bytes(s->words, s->capacity);
    return HSR_OK;
}
// export / import are host calls on the whole device: they wait for every stream of it first, so no launch that uses the snapshot is in flight
extern "C" int hsr_snapshot_export(const hsr_snapshot *s, void *out, long long len) {
    if (!s || !out) return fail(HSR_EINVAL, "hsr_snapshot_export: null argument");
    if (!s->d) return fail(HSR_EINVAL, "hsr_snapshot_export: the batch that made the snapshot was destroyed, and its storage with it");
    if (len != snap_image_bytes(s->words, s->capacity)) return fail(HSR_EINVAL, "hsr_snapshot_export: len is not hsr_snapshot_image_bytes()");
    SnapImageHeader h{};
    memcpy(h.magic, kSnapMagic, 8);
    h.version = SNAP_IMAGE_VERSION; h.header_bytes = sizeof h; h.fingerprint = s->fingerprint; h.capacity = s->capacity;
    memcpy(h.dims, s->dims, sizeof h.dims); h.words = s->words;
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy((char *)out + sizeof h, s->d, (size_t)(len - (long long)sizeof h), hipMemcpyDeviceToHost));
    memcpy(out, &h, sizeof h);
    return HSR_OK;
}
extern "C" int hsr_snapshot_import(hsr_snapshot *s, const void *image, long long len) {
    if (!s || !image) return fail(HSR_EINVAL, "hsr_snapshot_import: null argument");
    if (!s->d) return fail(HSR_EINVAL, "hsr_snapshot_import: the batch that made the snapshot was destroyed, and its storage with it");
    int capacity = 0;
    const int rc = snap_image_check(s->fingerprint, s->dims, image, len, &capacity);
    if (rc) return rc;
    if (capacity != s->capacity) return fail(HSR_EBLOB, "snapshot image: its capacity is not the snapshot's");
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(s->d, (const char *)image + sizeof(SnapImageHeader), (size_t)(len - (long long)sizeof(SnapImageHeader)), hipMemcpyHostToDevice));
    return HSR_OK;
}
