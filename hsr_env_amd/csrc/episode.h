// Episodes on the device (hsr_batch_set_episodes .. hsr_batch_sample_ctrl_dev): a counter-based sampler of reset states, goal points and
// actions, and the bookkeeping that closes an env-step - return, length, time limit, who is reset.  The reset itself stays k_reset.
//
// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11) in plain C++.  A draw is a pure function of
// (seed, global env id, episode or action step, stream, block): a shard at env_offset draws what the single batch draws for the same envs.
//   key     = (seed & 0xffffffff, seed >> 32)
//   counter = (gid, episode, stream, block), gid = env_offset + e
//   stream 0: qpos[i] = word i % 4 of block i / 4, over the per-dof range table
//   stream 1: goal point = words 0..2 of block 0
//   stream 2: pose of block b = words 0..3 of block b: x, y, z, yaw -> free-joint slot (x, y, z, cos(yaw/2), 0, 0, sin(yaw/2))
//   stream 3: ctrl[a] = word a % 4 of block a / 4; the second counter word is the caller's action-step counter
//   value   = min(hi, lo + u (hi - lo)), u = (word >> 8) 2^-24, every operation rounded to fp32 on its own (no contraction)
enum { EP_STREAM_QPOS = 0, EP_STREAM_GOAL = 1, EP_STREAM_BLOCK = 2, EP_STREAM_CTRL = 3 };

struct Philox4 { uint32_t x, y, z, w; };
__device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return Philox4{c0, c1, c2, c3};
}
__device__ __forceinline__ uint32_t philox_word(const Philox4 &p, int k) { return k == 0 ? p.x : k == 1 ? p.y : k == 2 ? p.z : p.w; }
// The product and the sum must round separately.  __fmul_rn / __fadd_rn do not see to that here: hipcc's headers define them as plain
// `x * y` and `x + y`, which the default -ffp-contract=fast-honor-pragmas fuses into one v_fmac_f32 once they are inlined (seen in the
// disassembly; the fused value differs from the stated one in the last bit for some words).  The pragma is what keeps them apart.
__device__ __forceinline__ float ep_uniform(uint32_t word, float lo, float hi) {
#pragma clang fp contract(off)
    const float u = (float)(word >> 8) * 5.9604644775390625e-8f;        // 24 bits: exact
    const float span = hi - lo;
    const float scaled = u * span;
    return fminf(hi, lo + scaled);
}

// what the episode kernels read and keep: the spec's tables and the per-env books, all owned by the batch
struct EpisodeDev {
    uint32_t key0, key1, env_offset;
    int max_steps;                 // 0: no time limit
    const float *qlo, *qhi;        // [nq]; lo == hi == qpos0 outside the sampled joints
    int has_goal;
    float glo[3], ghi[3];
    int nblock;
    const int *block_qadr;         // [nblock] free-joint qpos addresses
    float blo[4], bhi[4];          // x, y, z, yaw
    uint32_t *ep_index;            // [N] episodes begun by every env
    int32_t *ep_length;            // [N] env-steps of the running episode
    float *ep_return;              // [N] its reward sum
    float *qpos0, *mocap;          // [N, nq], [N, 3]: the last sample of every env (what k_reset reads)
    uint8_t *mask;                 // [N] reset kind of the last episode end / sampled reset
};

// episode `ep` of env e: start state and goal point into the sample buffers
__device__ __forceinline__ void ep_sample_start(const EpisodeDev &E, int nq, int e, uint32_t ep) {
    const uint32_t gid = E.env_offset + (uint32_t)e;
    float *q = E.qpos0 + (size_t)e * nq;
    for (int blk = 0; 4 * blk < nq; blk++) {
        const Philox4 p = philox4x32_10(gid, ep, EP_STREAM_QPOS, (uint32_t)blk, E.key0, E.key1);
        for (int k = 0; k < 4 && 4 * blk + k < nq; k++) q[4 * blk + k] = ep_uniform(philox_word(p, k), E.qlo[4 * blk + k], E.qhi[4 * blk + k]);
    }
    for (int b = 0; b < E.nblock; b++) {
        const Philox4 p = philox4x32_10(gid, ep, EP_STREAM_BLOCK, (uint32_t)b, E.key0, E.key1);
        const float half = __fmul_rn(ep_uniform(p.w, E.blo[3], E.bhi[3]), 0.5f);
        float *o = q + E.block_qadr[b];
        o[0] = ep_uniform(p.x, E.blo[0], E.bhi[0]); o[1] = ep_uniform(p.y, E.blo[1], E.bhi[1]); o[2] = ep_uniform(p.z, E.blo[2], E.bhi[2]);
        o[3] = cosf(half); o[4] = 0.f; o[5] = 0.f; o[6] = sinf(half);
    }
    float *g = E.mocap + (size_t)e * 3;
    if (E.has_goal) {
        const Philox4 p = philox4x32_10(gid, ep, EP_STREAM_GOAL, 0u, E.key0, E.key1);
        g[0] = ep_uniform(p.x, E.glo[0], E.ghi[0]); g[1] = ep_uniform(p.y, E.glo[1], E.ghi[1]); g[2] = ep_uniform(p.z, E.glo[2], E.ghi[2]);
    } else { g[0] = 0.f; g[1] = 0.f; g[2] = 0.f; }
}

// hsr_batch_reset_sampled*: the masked envs (all when sel == NULL) draw their next episode and start their books again
__global__ void k_episode_begin(EpisodeDev E, int N, int nq, const uint8_t *sel) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N) return;
    const bool on = sel ? sel[e] != 0 : true;
    E.mask[e] = on ? 1 : 0;
    if (!on) return;
    ep_sample_start(E, nq, e, E.ep_index[e]);
    E.ep_index[e] += 1;
    E.ep_length[e] = 0;
    E.ep_return[e] = 0.f;
}

// After an env-step (lane = env): books, time limit, who is reset (mask: 0 goes on, 1 done, 2 truncated), the samples of those envs, and their
// rows of obs replaced by the first observation of the new episode, concat(qpos0, 0).  final_obs, when asked for, gets every row of obs as the
// step left it: a workgroup copies the rows of its own 256 envs (contiguous), then overwrites among them.
__global__ void __launch_bounds__(256) k_episode_end(EpisodeDev E, int N, int nq, int nv, const int *done_latched, float *obs, const float *reward,
                                                     const uint8_t *done, float *final_obs, uint8_t *reset_kind, float *fin_return, int32_t *fin_length) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    const int no = nq + nv;
    if (final_obs) {
        const size_t base = (size_t)blockIdx.x * blockDim.x * no;
        const int rows = min((int)blockDim.x, N - (int)(blockIdx.x * blockDim.x));
        for (int i = threadIdx.x; i < rows * no; i += blockDim.x) final_obs[base + i] = obs[base + i];
        __syncthreads();
    }
    if (e >= N) return;
    const bool d = done ? done[e] != 0 : done_latched[e] != 0;
    const float ret = __fadd_rn(E.ep_return[e], reward ? reward[e] : (d ? 1.f : 0.f));
    const int len = E.ep_length[e] + 1;
    const bool over = E.max_steps > 0 && len >= E.max_steps;
    const int sel = d ? 1 : (over ? 2 : 0);
    E.mask[e] = (uint8_t)sel;
    if (reset_kind) reset_kind[e] = (uint8_t)sel;
    if (fin_return) fin_return[e] = sel ? ret : 0.f;
    if (fin_length) fin_length[e] = sel ? len : 0;
    E.ep_return[e] = sel ? 0.f : ret;
    E.ep_length[e] = sel ? 0 : len;
    if (!sel) return;
    ep_sample_start(E, nq, e, E.ep_index[e]);
    E.ep_index[e] += 1;
    if (obs) {
        float *o = obs + (size_t)e * no;
        const float *q = E.qpos0 + (size_t)e * nq;
        for (int i = 0; i < nq; i++) o[i] = q[i];
        for (int i = 0; i < nv; i++) o[nq + i] = 0.f;
    }
}

// ctrl[N, nu] ~ U(ctrlrange) for action step `step`; a side without a limit (not finite, or the model's marker 1e30) is -1 / +1
__global__ void k_sample_ctrl(EpisodeDev E, int N, int nu, const float *ctrlrange, uint32_t step, float *ctrl) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N) return;
    const uint32_t gid = E.env_offset + (uint32_t)e;
    for (int blk = 0; 4 * blk < nu; blk++) {
        const Philox4 p = philox4x32_10(gid, step, EP_STREAM_CTRL, (uint32_t)blk, E.key0, E.key1);
        for (int k = 0; k < 4 && 4 * blk + k < nu; k++) {
            const int a = 4 * blk + k;
            float lo = ctrlrange[2 * a], hi = ctrlrange[2 * a + 1];
            if (!(fabsf(lo) < 1e30f)) lo = -1.f;
            if (!(fabsf(hi) < 1e30f)) hi = 1.f;
            ctrl[(size_t)e * nu + a] = ep_uniform(philox_word(p, k), lo, hi);
        }
    }
}
