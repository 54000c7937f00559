// Running mean / std normalisation of observation and goal rows on the device (include/hsrsim.h: hsr_norm): fp64 moments updated from
// float32 rows by Chan's rule, published as float32 mean and 1 / std, and the clipped float32 apply.  The arithmetic of a column - merge,
// publish, apply - is normalize_logic.h's; this file moves rows and adds them up.  Nothing here reads or writes the simulation state.
//
// An update is two passes over the rows and three launches:
//   k_norm_pass<0>   per tile of NORM_ROWS rows: sum x per column, rows counted, rows skipped   -> pass-1 partials [tiles][dim + 2]
//   k_norm_pass<1>   per tile: sum (x - mean_b)^2 per column, mean_b = (sum of the pass-1 partials) / m, which every workgroup adds up for
//                    itself (the same additions in the same order give every workgroup the same bits)   -> pass-2 partials [tiles][dim]
//   k_norm_finish    one workgroup: both sums of the partials, Chan's merge, publish
//
// A workgroup stages its tile in LDS, NORM_COLS columns at a time, with loads that run along the rows in memory (one contiguous piece when the
// row stride equals dim <= NORM_COLS), and marks each row kept or left out: kept = inside n, mask byte non-zero (or no mask), all dim values
// finite.  Then wave w takes the columns c = w (mod 4): lane = row.  The LDS row stride is NORM_COLS + 1 words, odd, so the 64 lanes of a
// column read 64 different banks, as do the lanes that test their row.
//
// THE SHAPE OF EVERY SUM depends on (n, dim) only, never on the data or the mask; a row that is left out, or lies past n, adds +0.0 in
// the place where its value would have been added:
//   1. per lane, serially: the tile's rows lane and lane + 64, in this order;
//   2. the 64 lanes in wave_sum_fixed's shuffle tree (rollout.h)   -> the tile's partial;
//   3. the partials of a column: lane l adds those of tiles l, l + 64, l + 128, .. serially in this order, then the same shuffle tree.
// No atomics, and no sum is shared between columns; a column's sums do not depend on which wave computes them.
#pragma once
#include "normalize_logic.h"

enum { NORM_BLOCK = 256, NORM_WAVES = NORM_BLOCK / 64 };
static_assert(NORM_ROWS == 2 * 64, "step 1 of the shape: two rows per lane");
static_assert(NORM_LDS_STRIDE % 2 == 1, "an odd LDS row stride keeps a column's lanes on different banks");

struct NormDev {
    double *state;                 // count | mean[dim] | m2[dim]
    unsigned long long *skipped;   // [1]
    float *mean32, *rstd32;        // [dim] each: what apply reads
    double *partial;               // pass-1 partials [tiles][dim + 2], then pass-2 partials [tiles][dim]
    int dim;
    double eps;                    // (double) of the float the caller gave
    float clip;
};
__device__ __forceinline__ double *norm_mean(const NormDev &R) { return R.state + 1; }
__device__ __forceinline__ double *norm_m2(const NormDev &R) { return R.state + 1 + R.dim; }

// step 3 of the shape, by one whole wave: column `col` of `tiles` partial rows of `width` doubles; every lane returns the sum
__device__ __forceinline__ double norm_sum_partials(const double *partial, int tiles, int width, int col, int lane) {
    double v = 0.0;
    for (int t = lane; t < tiles; t += 64) v += partial[(size_t)t * width + col];
    v = wave_sum_fixed(v);
    return __shfl(v, 0, 64);
}

// PASS 0: sums of x, the rows counted (pseudo-column dim) and skipped (dim + 1).  PASS 1: sums of (x - mean_b)^2.
template <int PASS>
__global__ void __launch_bounds__(NORM_BLOCK) k_norm_pass(NormDev R, const float *rows, size_t stride, const uint8_t *mask, int n, int tiles) {
    __shared__ float tile[NORM_ROWS * NORM_LDS_STRIDE];
    __shared__ uint8_t keep[NORM_ROWS], skip[NORM_ROWS];
    __shared__ double mean_b[PASS == 1 ? NORM_DIM_MAX : 1];
    const int dim = R.dim, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r0 = blockIdx.x * NORM_ROWS, nrows = min(NORM_ROWS, n - r0), nch = norm_chunks(dim), w1 = norm_pass1_width(dim);
    const double *p1 = R.partial;
    double *out = PASS == 0 ? R.partial + (size_t)blockIdx.x * w1 : R.partial + (size_t)tiles * w1 + (size_t)blockIdx.x * dim;

    if (PASS == 1) {
        const double m = norm_sum_partials(p1, tiles, w1, dim, lane);
        for (int c = wave; c < dim; c += NORM_WAVES) {
            const double s = norm_sum_partials(p1, tiles, w1, c, lane);
            if (lane == 0) mean_b[c] = s / m;          // m == 0: never used, every row is left out
        }
    }
    // rows of the tile that the mask selects; the finite test below may still leave them out
    if (tid < NORM_ROWS) keep[tid] = tid < nrows && (!mask || mask[r0 + tid] != 0);
    auto stage = [&](int c0, int cw) {
        for (int i = tid; i < NORM_ROWS * cw; i += NORM_BLOCK) {
            const int r = i / cw, c = i - r * cw;
            tile[r * NORM_LDS_STRIDE + c] = r < nrows ? rows[(size_t)(r0 + r) * stride + c0 + c] : 0.f;
        }
    };
    // first walk over the columns: which rows are finite throughout
    bool finite = true;
    for (int ch = 0; ch < nch; ch++) {
        const int c0 = ch * NORM_COLS, cw = min(NORM_COLS, dim - c0);
        if (ch) __syncthreads();
        stage(c0, cw);
        __syncthreads();
        if (tid < NORM_ROWS) finite = finite && norm_row_finite(tile + tid * NORM_LDS_STRIDE, cw);
    }
    if (tid < NORM_ROWS) {
        skip[tid] = keep[tid] && !finite;
        keep[tid] = keep[tid] && finite;
    }
    __syncthreads();
    // second walk: the sums.  With one chunk the tile is still staged
    for (int ch = 0; ch < nch; ch++) {
        const int c0 = ch * NORM_COLS, cw = min(NORM_COLS, dim - c0);
        if (nch > 1) {
            __syncthreads();
            stage(c0, cw);
            __syncthreads();
        }
        for (int c = wave; c < cw; c += NORM_WAVES) {
            double v = 0.0;
#pragma unroll
            for (int h = 0; h < NORM_ROWS / 64; h++) {
                const int r = lane + 64 * h;
                const double x = (double)tile[r * NORM_LDS_STRIDE + c];
                double term = x;
                if (PASS == 1) { const double d = x - mean_b[c0 + c]; term = d * d; }
                v += keep[r] ? term : 0.0;
            }
            v = wave_sum_fixed(v);
            if (lane == 0) out[c0 + c] = v;
        }
    }
    if (PASS == 0 && wave < 2) {           // the two pseudo-columns, in the same shape
        const uint8_t *flag = wave == 0 ? keep : skip;
        double v = 0.0;
#pragma unroll
        for (int h = 0; h < NORM_ROWS / 64; h++) v += flag[lane + 64 * h] ? 1.0 : 0.0;
        v = wave_sum_fixed(v);
        if (lane == 0) out[dim + wave] = v;
    }
}

// one workgroup: the sums of both kinds of partials, merge, publish.  Every column is written by lane 0 of its wave; count and skipped by
// thread 0, after every column has read the old count
__global__ void __launch_bounds__(NORM_BLOCK) k_norm_finish(NormDev R, int tiles) {
    const int dim = R.dim, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, w1 = norm_pass1_width(dim);
    const double *p1 = R.partial, *p2 = R.partial + (size_t)tiles * w1;
    const double count = R.state[0];
    const double m = norm_sum_partials(p1, tiles, w1, dim, lane);
    const double tot = count + m;
    for (int c = wave; c < dim; c += NORM_WAVES) {
        const double s = norm_sum_partials(p1, tiles, w1, c, lane), q = norm_sum_partials(p2, tiles, dim, c, lane);
        if (lane == 0 && m > 0.0) {
            double mean = norm_mean(R)[c], m2 = norm_m2(R)[c];
            norm_merge(count, m, s / m, q, &mean, &m2);
            norm_mean(R)[c] = mean; norm_m2(R)[c] = m2;
            norm_publish(tot, mean, m2, R.eps, R.mean32 + c, R.rstd32 + c);
        }
    }
    const double sk = norm_sum_partials(p1, tiles, w1, dim + 1, lane);
    __syncthreads();
    if (threadIdx.x == 0) {
        if (m > 0.0) R.state[0] = tot;
        *R.skipped += (unsigned long long)sk;
    }
}

// publish alone: after create, clear and set_state
__global__ void __launch_bounds__(NORM_BLOCK) k_norm_publish(NormDev R) {
    const int c = blockIdx.x * NORM_BLOCK + threadIdx.x;
    if (c < R.dim) norm_publish(R.state[0], norm_mean(R)[c], norm_m2(R)[c], R.eps, R.mean32 + c, R.rstd32 + c);
}

// apply: element i of the n x dim rows to thread i mod (grid x block); in place when out == in
__global__ void __launch_bounds__(NORM_BLOCK) k_norm_apply(NormDev R, const float *in, size_t in_stride, float *out, size_t out_stride, int n) {
    const size_t dim = (size_t)R.dim, total = (size_t)n * dim;
    for (size_t i = (size_t)blockIdx.x * NORM_BLOCK + threadIdx.x; i < total; i += (size_t)gridDim.x * NORM_BLOCK) {
        const size_t r = i / dim, c = i - r * dim;
        out[r * out_stride + c] = norm_apply(in[r * in_stride + c], R.mean32[c], R.rstd32[c], R.clip);
    }
}

// apply to a sampled batch, every tensor in one launch: blockIdx.y = the tensor.  Tensors are contiguous rows of their norm's dim, in place.
// A tensor of windows (seq_len > 1) leaves the rows at and past its window's length alone: they are padding and stay zero.
struct NormBatchItem {
    float *rows;
    const float *mean32, *rstd32;
    int n, dim, seq_len;
    float clip;
};
struct NormBatch {
    NormBatchItem item[NORM_BATCH_ITEMS];
    const int32_t *length;         // [windows] or NULL
};
__global__ void __launch_bounds__(NORM_BLOCK) k_norm_apply_batch(NormBatch B) {
    const NormBatchItem &I = B.item[blockIdx.y];
    const size_t dim = (size_t)I.dim, total = (size_t)I.n * dim;
    for (size_t i = (size_t)blockIdx.x * NORM_BLOCK + threadIdx.x; i < total; i += (size_t)gridDim.x * NORM_BLOCK) {
        const size_t r = i / dim, c = i - r * dim;
        if (I.seq_len > 1 && B.length) {
            const size_t w = r / (size_t)I.seq_len;
            if ((int)(r - w * I.seq_len) >= B.length[w]) continue;
        }
        I.rows[i] = norm_apply(I.rows[i], I.mean32[c], I.rstd32[c], I.clip);
    }
}
