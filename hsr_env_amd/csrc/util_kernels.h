// The small kernels of the host layer: table building, layout / IO, reset, observation, introspection, margin clearing, frame capture,
// and the work-queue set-up and wave scheduler of the persistent kernel.  (The simulation kernels are in kin2.h .. persist.h.)
// global copies of the two constant LDS tables of the persistent kernel (same packing: kin2.h)
__global__ void k_build_tables(DevModel m, DevState s) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m.ngeom) { geom_consts_store(m.geom_rec + 32 * i, s.geom_c + 8 * i); if (m.nldsv > 0 && m.geom_ldsv[i] >= 0) hull_lds_patch(s.geom_c + 8 * i, m.geom_ldsv[i]); }
    if (i < ((m.npair_pad + 7) & ~7)) {
        unsigned pk = 0;
        if (i < m.npair) {
            const float4 a = reinterpret_cast<const float4 *>(m.pair_geo)[2 * i], b = reinterpret_cast<const float4 *>(m.pair_geo)[2 * i + 1];
            const int code = (int)a.x;
            pk = pair_pack(code & 255, (int)a.y, (int)b.x, (code >> 8) ? a.w : a.z + a.w);
        }
        s.pair_pack[i] = pk;
    }
}
// ------------------------------------------------------------------ small layout / IO kernels
__global__ void k_aos_to_soa(float *dst, const float *src, int rows, int N) {   // src [N,rows] -> dst [rows][N]
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)rows * N) return;
    int r = (int)(i / N), e = (int)(i % N);
    dst[i] = src[(size_t)e * rows + r];
}
__global__ void k_soa_to_aos(float *dst, const float *src, int rows, int N, int dst_stride, int dst_off) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)rows * N) return;
    int r = (int)(i / N), e = (int)(i % N);
    dst[(size_t)e * dst_stride + dst_off + r] = src[i];
}
__global__ void k_begin_step(DevState s, const float *ctrl_in, int nu) {
    int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= s.N) return;
    for (int a = 0; a < nu; a++) s.ctrl[(size_t)a * s.N + e] = ctrl_in[(size_t)e * nu + a];
    s.done[e] = 0;
    s.nsteps[e] = 0;
}
__global__ void k_end_step(DevState s, float *reward, uint8_t *done, int32_t *nsteps) {
    int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= s.N) return;
    if (reward) reward[e] = s.done[e] ? 1.f : 0.f;
    if (done) done[e] = (uint8_t)(s.done[e] != 0);
    if (nsteps) nsteps[e] = s.nsteps[e];
}
__global__ void k_clear_done(DevState s) {
    int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < s.N) s.done[e] = 0;
}
// park: mask == NULL means "the envs whose done flag is set", and the envs that are not reset are left parked (done = 1) for the
// forward pass of the reset ones (hsr_batch_reset_dev clears the flags after it)
__global__ void k_reset(DevModel m, DevState s, const uint8_t *mask, const float *qpos0_env, const float *qpos0_model, const float *mocap, int park) {
    int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= s.N) return;
    const bool sel = mask ? mask[e] != 0 : (park ? s.done[e] != 0 : true);
    s.done[e] = (park && !sel) ? 1 : 0;
    if (!sel) return;
    const int N = s.N;
    for (int i = 0; i < m.nq; i++) s.qpos[(size_t)i * N + e] = qpos0_env ? qpos0_env[(size_t)e * m.nq + i] : qpos0_model[i];
    for (int i = 0; i < m.nv; i++) { s.qvel[(size_t)i * N + e] = 0; s.warm[(size_t)i * N + e] = 0; s.qacc[(size_t)i * N + e] = 0; }
    for (int i = 0; i < m.nu; i++) s.ctrl[(size_t)i * N + e] = 0;
    for (int k = 0; k < 3; k++) s.mocap[(size_t)k * N + e] = mocap ? mocap[(size_t)e * 3 + k] : 0.f;
    s.time[e] = 0; s.bad[e] = 0; s.nsteps[e] = 0;
    for (int p = 0; p < m.npair; p++) {      // the geoms jumped: no separation margin is left, and no portal of the previous substep (margin row -1: rows 0-2 hold its vertex ids)
        float *mg = s.sepax + (size_t)(4 * p + 3) * N + e;
        if (*mg < 0.f) { mg[-(ptrdiff_t)N] = 0.f; mg[-2 * (ptrdiff_t)N] = 0.f; mg[-3 * (ptrdiff_t)N] = 0.f; }
        *mg = 0.f;
    }
}
__global__ void k_body_xpos(DevModel m, DevState s, int body, float *out) {
    int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= s.N) return;
    const int N = s.N;
    v3 p;
    if (m.body_mocap[body]) p = mk3(s.mocap[e], s.mocap[N + e], s.mocap[2 * N + e]);
    else {
        const int l = m.body_link[body];
        View xpos{s.xpos + e, N}, xmat{s.xmat + e, N};
        p = xpos.get3(l) + mulmv(xmat.getm(l), ld3(m.body_pos, body));
    }
    out[3 * e] = p.x; out[3 * e + 1] = p.y; out[3 * e + 2] = p.z;
}
// The reference's 'openai' observation (hsr/env.py:72-110, after gym's FetchEnv) with its evident intent restored
// (SURVEY.md 8a-5 lists the defects): 25 floats per env =
//   grip_pos 3 | object_pos 3 | object_rel_pos 3 | gripper_state 2 (finger joint qpos) | object_rot 3 (mat2euler) |
//   object_velp 3 ((v_obj - v_grip) dt) | object_velr 3 (w_obj dt) | grip_velp 3 (v_grip dt) | gripper_vel 2 (dt/2 finger qvel)
// body positions / velocities are those of the last forward pass (sim.data.xpos / cvel after mj_step), joint values the
// current ones, dt = nsubsteps * timestep with nsubsteps = 1.
__device__ __forceinline__ void body_pose_vel(const DevModel &m, const DevState &s, int body, int e, v3 &p, v3 &v, v3 &w, m3 &R) {
    const int N = s.N, l = m.body_link[body], nl = m.nlink;
    const View xpos{s.xpos + e, N}, xmat{s.xmat + e, N};
    const m3 Rl = xmat.getm(l);
    const v3 off = mulmv(Rl, ld3(m.body_pos, body));
    p = xpos.get3(l) + off;
    R = mulmm(Rl, ldm(m.body_mat, body));
    w = mk3(s.lvel[(size_t)(3 * l) * N + e], s.lvel[(size_t)(3 * l + 1) * N + e], s.lvel[(size_t)(3 * l + 2) * N + e]);
    const v3 vo = mk3(s.lvel[(size_t)(3 * nl + 3 * l) * N + e], s.lvel[(size_t)(3 * nl + 3 * l + 1) * N + e], s.lvel[(size_t)(3 * nl + 3 * l + 2) * N + e]);
    v = vo + cross(w, off);
}
__global__ void k_obs_openai(DevModel m, DevState s, int body_l, int body_r, int body_obj, int qadr_l, int qadr_r, int dadr_l, int dadr_r,
                             float dt, float *out) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= s.N) return;
    const int N = s.N;
    v3 pl, vl, wl, pr, vr, wr, po, vo, wo;
    m3 Rl, Rr, Ro;
    body_pose_vel(m, s, body_l, e, pl, vl, wl, Rl);
    body_pose_vel(m, s, body_r, e, pr, vr, wr, Rr);
    body_pose_vel(m, s, body_obj, e, po, vo, wo, Ro);
    const v3 grip = (pl + pr) * 0.5f, gvel = (vl + vr) * (0.5f * dt);
    const v3 rel = po - grip, ovel = vo * dt - gvel, orot = wo * dt;
    // mat2euler (hsr/env.py:256-272)
    const float cy = sqrtf(Ro.a[8] * Ro.a[8] + Ro.a[5] * Ro.a[5]);
    const bool cond = cy > 4.f * 2.220446049250313e-16f;
    const float ez = cond ? -atan2f(Ro.a[1], Ro.a[0]) : -atan2f(-Ro.a[3], Ro.a[4]);
    const float ey = -atan2f(-Ro.a[2], cy);
    const float ex = cond ? -atan2f(Ro.a[5], Ro.a[8]) : 0.f;
    float *o = out + (size_t)25 * e;
    o[0] = grip.x; o[1] = grip.y; o[2] = grip.z; o[3] = po.x; o[4] = po.y; o[5] = po.z; o[6] = rel.x; o[7] = rel.y; o[8] = rel.z;
    o[9] = s.qpos[(size_t)qadr_l * N + e]; o[10] = s.qpos[(size_t)qadr_r * N + e];
    o[11] = ex; o[12] = ey; o[13] = ez;
    o[14] = ovel.x; o[15] = ovel.y; o[16] = ovel.z; o[17] = orot.x; o[18] = orot.y; o[19] = orot.z;
    o[20] = gvel.x; o[21] = gvel.y; o[22] = gvel.z;
    o[23] = 0.5f * dt * s.qvel[(size_t)dadr_l * N + e]; o[24] = 0.5f * dt * s.qvel[(size_t)dadr_r * N + e];
}
__global__ void k_i32_to_f32(float *dst, const int *src, size_t n) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = (float)src[i];
}
__global__ void k_contacts_out(DevModel m, DevState s, float *out) {   // [N, nslot, 7]; empty slot: dist = +1
    int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= s.N) return;
    const int N = s.N;
    for (int p = 0; p < m.npair; p++) {
        const int cnt = s.ncon_pair[(size_t)e * m.npair_pad + p];
        for (int slot = m.pair_slot[p]; slot < m.pair_slot[p + 1]; slot++) {
            float *o = out + ((size_t)e * m.nslot + slot) * 7;
            const bool used = slot - m.pair_slot[p] < cnt;
            for (int k = 0; k < 7; k++) o[k] = used ? s.con[((size_t)e * m.nslot + slot) * 8 + k] : (k == 6 ? 1.f : 0.f);
        }
    }
}
__global__ void k_expand_M(DevState s, float *out, int nv) {   // packed [nM][N] -> [N,nv,nv]
    int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= s.N) return;
    for (int i = 0; i < nv; i++) for (int j = 0; j <= i; j++) {
        const float v = s.M[(size_t)(i * (i + 1) / 2 + j) * s.N + e];
        out[((size_t)e * nv + i) * nv + j] = v; out[((size_t)e * nv + j) * nv + i] = v;
    }
}
__global__ void k_clear_margins(DevState s) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (size_t)s.npair_sep * s.N) {
        float *mg = s.sepax + (4 * (i / s.N) + 3) * s.N + i % s.N;
        if (*mg < 0.f) { mg[-(ptrdiff_t)s.N] = 0.f; mg[-2 * (ptrdiff_t)s.N] = 0.f; mg[-3 * (ptrdiff_t)s.N] = 0.f; }      // portal vertex ids, not a direction
        *mg = 0.f;
    }
}
// Frame capture outside the persistent kernel (hsr_batch_set_capture): lane = (pose row, slot); frame `frame` of every slot gets its env's
// xpos / xmat - on the chain's capture substeps right after k_kinematics, for the envs still live (not done: k_kinematics has just written
// their poses), and at the end of every step as the slot's final frame, with the slot's frame count (from nsteps: the substeps it ran)
__global__ void k_capture(DevState s, int nlink, const int *cap_env, int R, float *cap, int frame, int live_only, int every, int *cnt) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 12 * nlink * R) return;
    const int row = i / R, r = i % R, e = cap_env[r];
    if (live_only && s.done[e]) return;
    cap[(size_t)frame * 12 * nlink * R + i] = row < 3 * nlink ? s.xpos[(size_t)row * s.N + e] : s.xmat[(size_t)(row - 3 * nlink) * s.N + e];
    if (cnt && row == 0) { const int n = s.nsteps[e]; cnt[r] = n == 0 ? 0 : (n - 1) / every + 1; }
}
// Wave packing of the persistent kernel (on by default; HSR_SCHEDULE=0 or hsr_batch_set_schedule(b, 0) keeps the identity packing).
// A launch ends with the wave that holds the hardest env (the one that needs the most Newton iterations per substep), and a wave
// advances at the pace of its hardest env while the others idle: so every one of the hardest envs gets a wave of its own, filled up
// with the easiest envs (which leave the Newton loop after one iteration), hardest waves dispatched first.  Hardness = the
// iterations an env ran in the last 100 substeps of its previous launch (DevState::trips).  Measured (r2, 8192 envs, the bench's
// freshly sampled ctrl per env-step - the worst case for a predictor: corr 0.3 from one env-step to the next,
// tools/exp_predict.py): cfg3 +0.5..1 % (one round of 2048 workgroups: only the packing counts), cfg4 +6 % (4096 workgroups over
// 1792 slots: the dispatch order counts too); with the packing computed from the state the env-step starts from it would be 15 %,
// and a policy whose actions are correlated from one env-step to the next comes closer to that.  Splitting the env-step into
// re-packed launches costs more than it gains (every launch then waits for its own slowest wave: +10 %).
// One workgroup sorts up to 8192 envs (bitonic, keys in LDS); larger batches are packed chunk by chunk.
// Results do not depend on the packing: no value of an env is ever combined with another env's.
enum { SCHED_CHUNK = 8192 };
// round 0 of the work queue holds every task in packing order (hard ones first); the other rounds are empty
__global__ void k_queue_init(DevState s, int T, int R) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < R) { s.q_head[i] = 0; s.q_wpos[i] = i == 0 ? T : 0; }
    if (i < 4) s.sq_ctl[i] = i == 2 ? s.solo_servers : 0;          // tickets taken, items reserved, free servers, finished tasks
    if (s.solo_servers > 0) for (int k = i; k < s.sq_cap; k += gridDim.x * blockDim.x) s.sq_items[k] = -1;
    // q_err is NOT cleared here: a trip stays on record until the host has read it (queue_error), however many launches were enqueued since
    if (i < R * T) s.q_items[i] = i < T ? i : -1;
}
// a splitting launch (persist.h): control words zeroed, no ticket filled.  q_err is NOT cleared, as above
__global__ void k_split_init(DevState s) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < SPLIT_CTL_WORDS) s.sq_ctl[i] = 0;
    for (int k = i; k < s.sq_cap; k += gridDim.x * blockDim.x) s.sq_items[k] = -1;
}
// The bitonic network with eight consecutive keys per thread in registers: exchanges at distance 1, 2, 4 stay inside the thread, 8 .. 256 inside
// the wave (one shuffle per key), and only 512 .. 4096 cross waves through LDS - 10 of the 91 stages need a barrier (round 3: all 91, 124 us of
// every env-step; the packing it computes saves 280 us of the cfg3 launch)
template <int J> __device__ __forceinline__ void sched_local_stage(unsigned (&v)[8], int tid, int k) {
    unsigned w[8];
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const int i = 8 * tid + r;
        const unsigned a = v[r], c = v[r ^ J];
        w[r] = (((i & J) == 0) == ((i & k) == 0)) ? (a > c ? a : c) : (a < c ? a : c);     // the lower index of a descending pair keeps the larger key
    }
#pragma unroll
    for (int r = 0; r < 8; r++) v[r] = w[r];
}
__global__ void __launch_bounds__(1024) k_schedule(DevState s, int epb, int *slot_env) {
    __shared__ unsigned key[SCHED_CHUNK];
    const int tid = threadIdx.x;
    const int e0 = blockIdx.x * SCHED_CHUNK, n = min(SCHED_CHUNK, s.N - e0);
    unsigned v[8];
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const int i = 8 * tid + r;
        const int t = i < n ? min(s.trips[e0 + i], 0x1fffe) : 0;
        v[r] = i < n ? ((unsigned)(t + 1) << 13) | (unsigned)(SCHED_CHUNK - 1 - i) : 0u;       // descending: more iterations first, then lower index
    }
    for (int k = 2; k <= SCHED_CHUNK; k <<= 1) {
        for (int j = k >> 1; j >= 512; j >>= 1) {              // partner in another wave: keys laid out [register][thread], no bank conflicts
#pragma unroll
            for (int r = 0; r < 8; r++) key[1024 * r + tid] = v[r];
            __syncthreads();
#pragma unroll
            for (int r = 0; r < 8; r++) {
                const int i = 8 * tid + r;
                const unsigned a = v[r], c = key[1024 * r + (tid ^ (j >> 3))];
                v[r] = (((i & j) == 0) == ((i & k) == 0)) ? (a > c ? a : c) : (a < c ? a : c);
            }
            __syncthreads();
        }
        for (int j = (k >> 1) < 256 ? (k >> 1) : 256; j >= 8; j >>= 1) {      // partner in the same wave
#pragma unroll
            for (int r = 0; r < 8; r++) {
                const int i = 8 * tid + r;
                const unsigned a = v[r], c = (unsigned)__shfl_xor((int)v[r], j >> 3, 64);
                v[r] = (((i & j) == 0) == ((i & k) == 0)) ? (a > c ? a : c) : (a < c ? a : c);
            }
        }
        if (k >= 8) sched_local_stage<4>(v, tid, k);
        if (k >= 4) sched_local_stage<2>(v, tid, k);
        sched_local_stage<1>(v, tid, k);
    }
#pragma unroll
    for (int r = 0; r < 8; r++) key[8 * tid + r] = v[r];
    __syncthreads();
    const int nw = (n + epb - 1) / epb;
    for (int sl = threadIdx.x; sl < nw * epb; sl += blockDim.x) {
        const int w = sl / epb, j = sl % epb;
        int idx;                                                   // position in the sorted list
        if (j == 0) idx = w;
        else { const int r = (j - 1) * nw + w; idx = r < n - nw ? n - 1 - r : -1; }
        slot_env[(size_t)e0 / epb * epb + sl] = (idx >= 0 && idx < n) ? e0 + (SCHED_CHUNK - 1 - (int)(key[idx] & (SCHED_CHUNK - 1))) : -1;
    }
}
