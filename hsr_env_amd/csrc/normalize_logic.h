// The arithmetic and the argument checks of the running-moments normaliser (include/hsrsim.h: hsr_norm) in plain C++ without a HIP call or
// header: the finite test of a row, Chan's merge, the publish rule, the float32 apply, the shape of the sums and every HSR_EINVAL condition.
// normalize.h's kernels and host_normalize.h compile these very functions, and so does a stand-alone program under a sanitizer
// (tests/normalize_logic_main.cpp).  A refused call launches nothing.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#ifdef __HIPCC__
#define NORM_HD __host__ __device__
#else
#define NORM_HD
#endif

// The shape of the sums (normalize.h has the kernels): a workgroup takes a tile of NORM_ROWS rows and NORM_COLS columns at a time
enum { NORM_ROWS = 128, NORM_COLS = 64, NORM_LDS_STRIDE = NORM_COLS + 1, NORM_DIM_MAX = 1024, NORM_BATCH_ITEMS = 8 };

NORM_HD static inline int64_t norm_tiles(int64_t n) { return (n + NORM_ROWS - 1) / NORM_ROWS; }
NORM_HD static inline int norm_chunks(int dim) { return (dim + NORM_COLS - 1) / NORM_COLS; }
// doubles per tile of the first pass (a sum per column, the rows counted, the rows skipped) and of the second (a sum per column)
NORM_HD static inline int norm_pass1_width(int dim) { return dim + 2; }
static inline int64_t norm_partial_doubles(int64_t n, int dim) { return norm_tiles(n) * (int64_t)(norm_pass1_width(dim) + dim); }

// NULL when the numbers are acceptable, else what is wrong with them
static inline const char *norm_create_error(int dim, float eps, float clip) {
    if (dim < 1 || dim > NORM_DIM_MAX) return "dim outside 1..1024";
    if (!(eps > 0.f) || !isfinite(eps)) return "eps must be positive and finite";
    if (!(clip > 0.f) || !isfinite(clip)) return "clip must be positive and finite";
    return nullptr;
}
// rows / in / out: the caller's pointers, which may be NULL only when n == 0
static inline const char *norm_update_error(int dim, int64_t n, int64_t stride, const void *rows) {
    if (n < 0) return "n < 0";
    if (n > 0x7fffffff) return "n beyond 2^31 - 1";
    if (stride < dim) return "row stride below dim";
    if (n > 0 && !rows) return "null d_rows";
    return nullptr;
}
static inline const char *norm_apply_error(int dim, int64_t n, int64_t in_stride, int64_t out_stride, const void *in, const void *out) {
    if (n < 0) return "n < 0";
    if (n > 0x7fffffff) return "n beyond 2^31 - 1";
    if (in_stride < dim || out_stride < dim) return "row stride below dim";
    if (n > 0 && (!in || !out)) return "null d_in / d_out";
    return nullptr;
}
// apply to a sampled batch: the item array, then every item - `rows` rows of its normaliser's dim, windows of seq_len rows each, `which`
// naming the normaliser (0 obs, 1 goal), whose handle `norm` must be there and must belong to the batch `owner` of the first item's
static inline const char *norm_batch_error(const void *items, int n_items) {
    if (!items) return "null items";
    if (n_items < 1 || n_items > NORM_BATCH_ITEMS) return "not 1..8 items";
    return nullptr;
}
static inline const char *norm_item_error(int64_t rows, int seq_len, int which, const void *d_rows) {
    if (which != 0 && which != 1) return "item.which must be 0 (obs) or 1 (goal)";
    if (rows < 0) return "rows < 0";
    if (rows > 0x7fffffff) return "rows beyond 2^31 - 1";
    if (seq_len < 1) return "seq_len < 1";
    if (rows % seq_len) return "rows is no multiple of seq_len";
    if (rows > 0 && !d_rows) return "null d_rows";
    return nullptr;
}
static inline const char *norm_owner_error(const void *owner, const void *first_owner) {
    if (owner != first_owner) return "the two normalisers belong to different batches";
    return nullptr;
}
static inline const char *norm_state_error(int dim, double count, const double *mean, const double *m2) {
    if (!isfinite(count) || count < 0.0) return "count negative or not finite";
    for (int c = 0; c < dim; c++) {
        if (mean && !isfinite(mean[c])) return "mean not finite";
        if (m2 && (!isfinite(m2[c]) || m2[c] < 0.0)) return "m2 negative or not finite";
    }
    return nullptr;
}

// finite by the bits: no library call, the same answer under every compiler flag
NORM_HD static inline bool norm_finite32(float x) {
    uint32_t u;
    memcpy(&u, &x, sizeof u);
    return (u & 0x7f800000u) != 0x7f800000u;
}
NORM_HD static inline bool norm_row_finite(const float *row, int dim) {
    bool ok = true;
    for (int c = 0; c < dim; c++) ok = ok && norm_finite32(row[c]);
    return ok;
}

// Chan's rule for one column: m rows of mean mean_b and m2_b = sum (x - mean_b)^2 join `count` rows.  m == 0 writes nothing.  The caller
// moves count (to count + m) after the last column.
NORM_HD static inline void norm_merge(double count, double m, double mean_b, double m2_b, double *mean, double *m2) {
    if (!(m > 0.0)) return;
    const double delta = mean_b - *mean, tot = count + m;
    const double step = delta * m / tot;
    const double cross = delta * delta * count * m / tot;
    *mean = *mean + step;
    *m2 = *m2 + (m2_b + cross);
}

// what apply reads: std = sqrt(max(m2 / count, eps^2)); nothing counted yet -> the identity
NORM_HD static inline void norm_publish(double count, double mean, double m2, double eps, float *mean32, float *rstd32) {
    if (!(count > 0.0)) { *mean32 = 0.f; *rstd32 = 1.f; return; }
    const double var = m2 / count, floor2 = eps * eps;
    const double sd = sqrt(var > floor2 ? var : floor2);
    *mean32 = (float)mean;
    *rstd32 = (float)(1.0 / sd);
}

// y = clamp((x - mean32) rstd32, -clip, clip): two float32 operations, each rounded on its own; the clamp is two comparisons, which a NaN fails
NORM_HD static inline float norm_apply(float x, float mean32, float rstd32, float clip) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const float centred = x - mean32;
    float y = centred * rstd32;
    if (y > clip) y = clip;
    if (y < -clip) y = -clip;
    return y;
}
