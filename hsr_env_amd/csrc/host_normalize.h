// Running-moments normalisers: the hsr_norm record, its storage and the launches of normalize.h.  Which numbers are acceptable is decided by
// the plain functions of normalize_logic.h; a refused call launches nothing.  A normaliser is bound to its batch (it launches on that
// batch's stream) and is not part of an env record (snapshot.h): its statistics are the learner's, not the envs'.

struct hsr_norm {
    hsr_batch *owner = nullptr;    // NULL once hsr_batch_destroy released the storage
    int device = 0;
    NormDev dev{};
    int64_t partial_doubles = 0;   // what dev.partial holds; it grows with the largest update seen
    std::vector<double> upload;    // set_state's host image: count | mean | m2 | skipped bits
};

static void norm_free_storage(hsr_norm *r) {
    NormDev &D = r->dev;
    for (void **p : {(void **)&D.state, (void **)&D.mean32, (void **)&D.partial}) { if (*p) hipFree(*p); *p = nullptr; }
    D.skipped = nullptr; D.rstd32 = nullptr;
    r->partial_doubles = 0;
}
// hsr_batch_destroy: as for replays and rollouts, the storage goes with the batch and the handle stays the caller's to destroy
static void norm_release_all(hsr_batch *b) {
    for (hsr_norm *r : b->norms) { norm_free_storage(r); r->owner = nullptr; }
    b->norms.clear();
}
static int norm_live(const hsr_norm *r, const char *who) {
    if (!r) return fail(HSR_EINVAL, "%s: null normaliser", who);
    if (!r->owner) return fail(HSR_EINVAL, "%s: the normaliser's batch was destroyed, and its storage with it", who);
    return HSR_OK;
}
// the common opening of a call (who: a string literal): the handle, the checks' verdict, the device made current
#define NORM_ENTER(r, who, why_expr) do { \
        const int rc_ = norm_live((r), who); \
        if (rc_) return rc_; \
        const char *why_ = (why_expr); \
        if (why_) return fail(HSR_EINVAL, who ": %s", why_); \
        HIPCHK(hipSetDevice((r)->device)); \
    } while (0)
static inline size_t norm_state_bytes(int dim) { return (size_t)(2 * dim + 2) * sizeof(double); }      // count | mean | m2 | skipped
static_assert(NORM_BATCH_ITEMS == 8, "norm_batch_error's message names the number");
static inline dim3 norm_grid(size_t elements) { return dim3((unsigned)std::min<size_t>((elements + NORM_BLOCK - 1) / NORM_BLOCK, 1u << 16)); }

static int norm_zero_and_publish(hsr_norm *r) {
    const NormDev &D = r->dev;
    HIPCHK(hipMemsetAsync(D.state, 0, norm_state_bytes(D.dim), r->owner->stream));
    hipLaunchKernelGGL(k_norm_publish, grid1((size_t)D.dim, NORM_BLOCK), dim3(NORM_BLOCK), 0, r->owner->stream, D);
    HIPCHK(hipGetLastError());
    return HSR_OK;
}

extern "C" int hsr_batch_norm_create(hsr_batch *b, int dim, float eps, float clip, hsr_norm **out) {
    ENTER_DEV(b);
    if (!out) return fail(HSR_EINVAL, "hsr_batch_norm_create: null argument");
    const char *why = norm_create_error(dim, eps, clip);
    if (why) return fail(HSR_EINVAL, "hsr_batch_norm_create: %s", why);
    hsr_norm *r = new hsr_norm();
    r->owner = b; r->device = b->device;
    NormDev &D = r->dev;
    D.dim = dim; D.eps = (double)eps; D.clip = clip;
    // two allocations now (the fp64 state with the skipped count behind it, the two published vectors); the partials come with the first update
    if (hipMalloc((void **)&D.state, norm_state_bytes(dim)) != hipSuccess || hipMalloc((void **)&D.mean32, (size_t)2 * dim * sizeof(float)) != hipSuccess) {
        norm_free_storage(r);
        delete r;
        hipGetLastError();
        return fail(HSR_EDEVICE, "normaliser: no device memory");
    }
    D.skipped = (unsigned long long *)(D.state + 1 + 2 * dim);
    D.rstd32 = D.mean32 + dim;
    const int rc = norm_zero_and_publish(r);
    if (rc) { norm_free_storage(r); delete r; return rc; }
    b->norms.push_back(r);
    *out = r;
    return HSR_OK;
}
extern "C" void hsr_norm_destroy(hsr_norm *r) {
    if (!r) return;
    if (r->owner) {
        std::vector<hsr_norm *> &v = r->owner->norms;
        v.erase(std::remove(v.begin(), v.end(), r), v.end());
        hipSetDevice(r->device);
        hipStreamSynchronize(r->owner->stream);        // the only stream that uses it
        norm_free_storage(r);
    }
    delete r;
}
extern "C" int hsr_norm_clear(hsr_norm *r) {
    NORM_ENTER(r, "hsr_norm_clear", nullptr);
    return norm_zero_and_publish(r);
}

extern "C" int hsr_norm_update_dev(hsr_norm *r, const float *d_rows, int stride, const uint8_t *d_mask, int n) {
    NORM_ENTER(r, "hsr_norm_update_dev", norm_update_error(r->dev.dim, n, stride, d_rows));
    if (n == 0) return HSR_OK;
    NormDev &D = r->dev;
    hipStream_t s = r->owner->stream;
    const int64_t need = norm_partial_doubles(n, D.dim);
    if (need > r->partial_doubles) {
        HIPCHK(hipStreamSynchronize(s));               // an update in flight still reads the old partials
        if (D.partial) hipFree(D.partial);
        D.partial = nullptr; r->partial_doubles = 0;
        HIPCHK(hipMalloc((void **)&D.partial, (size_t)need * sizeof(double)));
        r->partial_doubles = need;
    }
    const int tiles = (int)norm_tiles(n);
    hipLaunchKernelGGL(k_norm_pass<0>, dim3(tiles), dim3(NORM_BLOCK), 0, s, D, d_rows, (size_t)stride, d_mask, n, tiles);
    hipLaunchKernelGGL(k_norm_pass<1>, dim3(tiles), dim3(NORM_BLOCK), 0, s, D, d_rows, (size_t)stride, d_mask, n, tiles);
    hipLaunchKernelGGL(k_norm_finish, dim3(1), dim3(NORM_BLOCK), 0, s, D, tiles);
    HIPCHK(hipGetLastError());
    return HSR_OK;
}
extern "C" int hsr_norm_apply_dev(hsr_norm *r, const float *d_in, int in_stride, float *d_out, int out_stride, int n) {
    NORM_ENTER(r, "hsr_norm_apply_dev", norm_apply_error(r->dev.dim, n, in_stride, out_stride, d_in, d_out));
    if (n == 0) return HSR_OK;
    hipLaunchKernelGGL(k_norm_apply, norm_grid((size_t)n * r->dev.dim), dim3(NORM_BLOCK), 0, r->owner->stream, r->dev, d_in, (size_t)in_stride, d_out,
                       (size_t)out_stride, n);
    HIPCHK(hipGetLastError());
    return HSR_OK;
}
extern "C" int hsr_norm_apply_batch_dev(hsr_norm *obs, hsr_norm *goal, const hsr_norm_item *items, int n_items, const int32_t *d_length) {
    const char *why = norm_batch_error(items, n_items);
    if (why) return fail(HSR_EINVAL, "hsr_norm_apply_batch_dev: %s", why);
    NormBatch B{};
    B.length = d_length;
    hsr_norm *first = nullptr;
    size_t most = 0;
    for (int k = 0; k < n_items; k++) {
        const hsr_norm_item &it = items[k];
        if ((why = norm_item_error(it.rows, it.seq_len, it.which, it.d_rows))) return fail(HSR_EINVAL, "hsr_norm_apply_batch_dev: %s", why);
        hsr_norm *r = it.which ? goal : obs;
        const int rc = norm_live(r, "hsr_norm_apply_batch_dev");
        if (rc) return rc;
        if (!first) first = r;
        if ((why = norm_owner_error(r->owner, first->owner))) return fail(HSR_EINVAL, "hsr_norm_apply_batch_dev: %s", why);
        B.item[k] = NormBatchItem{it.d_rows, r->dev.mean32, r->dev.rstd32, (int)it.rows, r->dev.dim, it.seq_len, r->dev.clip};
        most = std::max(most, (size_t)it.rows * (size_t)r->dev.dim);
    }
    if (!most) return HSR_OK;
    HIPCHK(hipSetDevice(first->device));
    hipLaunchKernelGGL(k_norm_apply_batch, dim3(norm_grid(most).x, n_items), dim3(NORM_BLOCK), 0, first->owner->stream, B);
    HIPCHK(hipGetLastError());
    return HSR_OK;
}

extern "C" int hsr_norm_state(hsr_norm *r, double *count, double *mean, double *m2, uint64_t *skipped) {
    NORM_ENTER(r, "hsr_norm_state", nullptr);
    const int dim = r->dev.dim;
    std::vector<double> h(2 * dim + 2);
    HIPCHK(hipMemcpyAsync(h.data(), r->dev.state, norm_state_bytes(dim), hipMemcpyDeviceToHost, r->owner->stream));
    HIPCHK(hipStreamSynchronize(r->owner->stream));
    if (count) *count = h[0];
    if (mean) memcpy(mean, h.data() + 1, (size_t)dim * sizeof(double));
    if (m2) memcpy(m2, h.data() + 1 + dim, (size_t)dim * sizeof(double));
    if (skipped) memcpy(skipped, h.data() + 1 + 2 * dim, sizeof(uint64_t));
    return HSR_OK;
}
extern "C" int hsr_norm_set_state(hsr_norm *r, double count, const double *mean, const double *m2, uint64_t skipped) {
    NORM_ENTER(r, "hsr_norm_set_state", !mean || !m2 ? "null mean / m2" : norm_state_error(r->dev.dim, count, mean, m2));
    const int dim = r->dev.dim;
    std::vector<double> &h = r->upload;
    HIPCHK(hipStreamSynchronize(r->owner->stream));    // an earlier set_state's copy may still read the image
    h.assign(2 * dim + 2, 0.0);
    h[0] = count;
    memcpy(h.data() + 1, mean, (size_t)dim * sizeof(double));
    memcpy(h.data() + 1 + dim, m2, (size_t)dim * sizeof(double));
    memcpy(h.data() + 1 + 2 * dim, &skipped, sizeof(uint64_t));
    HIPCHK(hipMemcpyAsync(r->dev.state, h.data(), norm_state_bytes(dim), hipMemcpyHostToDevice, r->owner->stream));
    hipLaunchKernelGGL(k_norm_publish, grid1((size_t)dim, NORM_BLOCK), dim3(NORM_BLOCK), 0, r->owner->stream, r->dev);
    HIPCHK(hipGetLastError());
    return HSR_OK;
}
extern "C" int hsr_norm_published_dev(hsr_norm *r, float *d_mean32, float *d_rstd32) {
    NORM_ENTER(r, "hsr_norm_published_dev", nullptr);
    const size_t bytes = (size_t)r->dev.dim * sizeof(float);
    if (d_mean32) HIPCHK(hipMemcpyAsync(d_mean32, r->dev.mean32, bytes, hipMemcpyDeviceToDevice, r->owner->stream));
    if (d_rstd32) HIPCHK(hipMemcpyAsync(d_rstd32, r->dev.rstd32, bytes, hipMemcpyDeviceToDevice, r->owner->stream));
    return HSR_OK;
}
