// Env records: what a snapshot holds of one env, and the one kernel that moves records between a batch and a snapshot.
//
// A record is everything of an env that a later step / forward / getter READS BEFORE IT WRITES (persist.h: the loads at the head of
// k_env_step_mf and its convex-pair section; solve_mf.h, collide.h: the chain; util_kernels.h, render.h: the getters):
//   simulation state   qpos qvel ctrl mocap warm time done bad nsteps
//   collision caches   tick, sepax (separating axis + margin, or the portal vertex ids of a penetrating pair), septick - all three or
//                      none: a stamp counts only against its env's tick
//   packing input      trips (never changes a result; copied so that a restored batch launches with the packing it would have had)
//   last forward pass  xpos xmat lvel (hsr_batch_body_xpos, obs_openai, render and the goal points read them without recomputing; copied,
//                      so that a load needs no forward pass)
//   episode books      ep_index ep_length ep_return (zero in a record saved from a batch without hsr_batch_set_episodes; loaded only into
//                      a batch that has them; the draw key stays (gid of the destination env, restored episode index))
// NOT in a record: what every substep rewrites before reading it (con, ncon_pair, kin_aos, the pair lists, M, qacc*, qfrc*, ncon / nefc /
// niter: for a loaded env hsr_batch_get_field other than HSR_F_XPOS / HSR_F_XMAT describes nothing until the next forward or step), the
// capture slots, goals, settings, queue and solo-server control words, cap statistics.
//
// Every field is an array of 4-byte words laid out [row][N], env fastest (model.h); a record is the concatenation of its fields' rows in
// the order of the enum below, and a snapshot stores records the same way, [record row][capacity].  Words are copied as uint32_t bit
// patterns, never through float arithmetic: NaN payloads, -0 and the vertex ids kept in sepax rows survive.
#pragma once
#include <stdint.h>

enum SnapFieldId { SNAP_QPOS = 0, SNAP_QVEL, SNAP_CTRL, SNAP_MOCAP, SNAP_WARM, SNAP_TIME, SNAP_DONE, SNAP_BAD, SNAP_NSTEPS, SNAP_TICK, SNAP_SEPAX,
                   SNAP_SEPTICK, SNAP_TRIPS, SNAP_XPOS, SNAP_XMAT, SNAP_LVEL, SNAP_EP_INDEX, SNAP_EP_LENGTH, SNAP_EP_RETURN, SNAP_NFIELD };
enum { SNAP_NDIM = 5 };            // the model sizes a record's layout depends on: nq nv nu nlink npair_sep (= max(npair, 1), model.h)

// rows of every field, from the sizes alone (no batch, no device): the one statement of the record's layout.  Returns the record's words.
static inline int snap_field_rows(const int dims[SNAP_NDIM], int rows[SNAP_NFIELD]) {
    const int nq = dims[0], nv = dims[1], nu = dims[2], nlink = dims[3], npair_sep = dims[4];
    rows[SNAP_QPOS] = nq; rows[SNAP_QVEL] = nv; rows[SNAP_CTRL] = nu; rows[SNAP_MOCAP] = 3; rows[SNAP_WARM] = nv;
    rows[SNAP_TIME] = rows[SNAP_DONE] = rows[SNAP_BAD] = rows[SNAP_NSTEPS] = rows[SNAP_TICK] = 1;
    rows[SNAP_SEPAX] = 4 * npair_sep; rows[SNAP_SEPTICK] = npair_sep; rows[SNAP_TRIPS] = 1;
    rows[SNAP_XPOS] = 3 * nlink; rows[SNAP_XMAT] = 9 * nlink; rows[SNAP_LVEL] = 6 * nlink;
    rows[SNAP_EP_INDEX] = rows[SNAP_EP_LENGTH] = rows[SNAP_EP_RETURN] = 1;
    int words = 0;
    for (int k = 0; k < SNAP_NFIELD; k++) words += rows[k];
    return words;
}

// the record of one batch: field k holds the record rows [row0, row0 + rows) at base[(row - row0) * N + env]; base == NULL (the episode
// books of a batch without episodes): the rows are saved as zero and not loaded
struct SnapField { uint32_t *base; int row0, rows; };
struct SnapTable { SnapField f[SNAP_NFIELD]; int words, N; };

// n records between a batch and a snapshot: to_batch == 0: store[.][slot[i]] <- env env[i]; else env env[i] <- store[.][slot[i]] (NULL index
// array = identity).  grid.y = record row, lane = i: with contiguous indices both sides are read and written coalesced.  An index outside
// its range makes the thread skip the record: whatever the caller passes, nothing is read or written outside the N envs / the capacity.
__global__ void __launch_bounds__(256) k_snapshot_copy(SnapTable t, uint32_t *store, int capacity, const int32_t *env, const int32_t *slot, int n, int to_batch) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, row = blockIdx.y;
    if (i >= n || row >= t.words) return;
    const int e = env ? env[i] : i, sl = slot ? slot[i] : i;
    if (e < 0 || e >= t.N || sl < 0 || sl >= capacity) return;
    int k = 0;
    while (k < SNAP_NFIELD - 1 && row >= t.f[k].row0 + t.f[k].rows) k++;
    uint32_t *field = t.f[k].base, *rec = store + (size_t)row * capacity + sl;
    if (field) field += (size_t)(row - t.f[k].row0) * t.N + e;
    if (to_batch) { if (field) *field = *rec; }
    else *rec = field ? *field : 0u;
}
