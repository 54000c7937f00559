// Episodes on the device: hsr_batch_set_episodes uploads the spec and allocates the books; the sampled reset, the episode end and the action
// sampler launch the kernels of episode.h and hand the reset itself to hsr_batch_reset_dev (k_reset, forward, k_clear_done), unchanged.

static bool ep_bounds_ok(const float *lo, const float *hi, int n) {
    for (int i = 0; i < n; i++) if (!std::isfinite(lo[i]) || !std::isfinite(hi[i]) || lo[i] > hi[i]) return false;
    return true;
}
static int require_episodes(const hsr_batch *b, const char *who) {
    if (!b->ep_set) return fail(HSR_EINVAL, "%s: no episode spec (hsr_batch_set_episodes first)", who);
    return HSR_OK;
}

extern "C" int hsr_batch_set_episodes(hsr_batch *b, const hsr_episode_spec *spec) {
    ENTER_DEV(b);
    if (!spec) return fail(HSR_EINVAL, "hsr_batch_set_episodes: null spec");
    const int nq = b->dm.nq, nl = b->dm.nlink;
    const size_t N = (size_t)b->N;
    if (!spec->qpos_lo || !spec->qpos_hi) return fail(HSR_EINVAL, "hsr_batch_set_episodes: qpos_lo / qpos_hi missing");
    if (spec->max_episode_steps < 0) return fail(HSR_EINVAL, "hsr_batch_set_episodes: max_episode_steps < 0");
    if (!ep_bounds_ok(spec->qpos_lo, spec->qpos_hi, nq)) return fail(HSR_EINVAL, "hsr_batch_set_episodes: a qpos bound is not finite, or lo > hi");
    if (spec->has_goal && !ep_bounds_ok(spec->goal_lo, spec->goal_hi, 3)) return fail(HSR_EINVAL, "hsr_batch_set_episodes: a goal bound is not finite, or lo > hi");
    const int *lf = b->model->i32("link_free"), *lqa = b->model->i32("link_qposadr");
    int nfree = 0;
    for (int l = 1; l < nl; l++) nfree += lf[l] ? 1 : 0;
    if (spec->nblock < 0 || spec->nblock > nfree) return fail(HSR_EINVAL, "hsr_batch_set_episodes: nblock outside 0..%s (the model's free bodies)", std::to_string(nfree).c_str());
    if (spec->nblock > 0) {
        if (!spec->block_qadr) return fail(HSR_EINVAL, "hsr_batch_set_episodes: block_qadr missing");
        if (!ep_bounds_ok(spec->block_lo, spec->block_hi, 4)) return fail(HSR_EINVAL, "hsr_batch_set_episodes: a block bound is not finite, or lo > hi");
        for (int k = 0; k < spec->nblock; k++) {
            bool ok = false;
            for (int l = 1; l < nl; l++) ok = ok || (lf[l] && lqa[l] == spec->block_qadr[k]);
            if (!ok) return fail(HSR_EINVAL, "hsr_batch_set_episodes: block_qadr holds %s, which is not the address of a free joint", std::to_string(spec->block_qadr[k]).c_str());
        }
    }
    HIPCHK(hipStreamSynchronize(b->stream));       // no launch in flight reads the tables that change below
    EpisodeDev &E = b->ep;
    int rc = 0;
    if (!E.ep_index) {
        if ((rc = dalloc(b, &b->d_ep_range, (size_t)2 * nq)) || (rc = dalloc(b, &b->d_ep_block_qadr, (size_t)nfree))) return rc;
        if ((rc = dalloc(b, &E.ep_index, N)) || (rc = dalloc(b, &E.ep_length, N)) || (rc = dalloc(b, &E.ep_return, N))) return rc;
        if ((rc = dalloc(b, &E.qpos0, N * nq)) || (rc = dalloc(b, &E.mocap, N * 3)) || (rc = dalloc(b, &E.mask, N))) return rc;
        E.qlo = b->d_ep_range; E.qhi = b->d_ep_range + nq; E.block_qadr = b->d_ep_block_qadr;
    }
    HIPCHK(hipMemcpy(b->d_ep_range, spec->qpos_lo, nq * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(b->d_ep_range + nq, spec->qpos_hi, nq * sizeof(float), hipMemcpyHostToDevice));
    if (spec->nblock > 0) HIPCHK(hipMemcpy(b->d_ep_block_qadr, spec->block_qadr, spec->nblock * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemset(E.ep_index, 0, N * sizeof(uint32_t)));
    HIPCHK(hipMemset(E.ep_length, 0, N * sizeof(int32_t)));
    HIPCHK(hipMemset(E.ep_return, 0, N * sizeof(float)));
    HIPCHK(hipMemset(E.qpos0, 0, N * nq * sizeof(float)));
    HIPCHK(hipMemset(E.mocap, 0, N * 3 * sizeof(float)));
    HIPCHK(hipMemset(E.mask, 0, N));
    E.key0 = (uint32_t)(spec->seed & 0xffffffffu); E.key1 = (uint32_t)(spec->seed >> 32);
    E.env_offset = spec->env_offset;
    E.max_steps = spec->max_episode_steps;
    E.has_goal = spec->has_goal != 0;
    for (int k = 0; k < 3; k++) { E.glo[k] = E.has_goal ? spec->goal_lo[k] : 0.f; E.ghi[k] = E.has_goal ? spec->goal_hi[k] : 0.f; }
    E.nblock = spec->nblock;
    for (int k = 0; k < 4; k++) { E.blo[k] = E.nblock ? spec->block_lo[k] : 0.f; E.bhi[k] = E.nblock ? spec->block_hi[k] : 0.f; }
    b->ep_set = true;
    return HSR_OK;
}

extern "C" int hsr_batch_reset_sampled_dev(hsr_batch *b, const uint8_t *d_mask) {
    ENTER_DEV(b);
    int rc = require_episodes(b, "hsr_batch_reset_sampled");
    if (rc) return rc;
    hipLaunchKernelGGL(k_episode_begin, grid1(b->N), dim3(256), 0, b->stream, b->ep, b->N, b->dm.nq, d_mask);
    return hsr_batch_reset_dev(b, b->ep.mask, b->ep.qpos0, b->ep.mocap);
}
extern "C" int hsr_batch_reset_sampled(hsr_batch *b, const uint8_t *mask) {
    ENTER_DEV(b);
    int rc = require_episodes(b, "hsr_batch_reset_sampled");
    if (rc) return rc;
    if (mask) HIPCHK(hipMemcpyAsync(b->d_stage_u8, mask, (size_t)b->N, hipMemcpyHostToDevice, b->stream));
    if ((rc = hsr_batch_reset_sampled_dev(b, mask ? b->d_stage_u8 : nullptr))) return rc;
    HIPCHK(hipStreamSynchronize(b->stream));
    return HSR_OK;
}

extern "C" int hsr_batch_episode_end_dev(hsr_batch *b, float *d_obs, const float *d_reward, const uint8_t *d_done, float *d_final_obs,
                                         uint8_t *d_reset_kind, float *d_fin_return, int32_t *d_fin_length) {
    ENTER_DEV(b);
    const int rc = require_episodes(b, "hsr_batch_episode_end_dev");
    if (rc) return rc;
    if (d_final_obs && !d_obs) return fail(HSR_EINVAL, "hsr_batch_episode_end_dev: d_final_obs without d_obs");
    hipLaunchKernelGGL(k_episode_end, grid1(b->N), dim3(256), 0, b->stream, b->ep, b->N, b->dm.nq, b->dm.nv, (const int *)b->ds.done, d_obs, d_reward, d_done,
                       d_final_obs, d_reset_kind, d_fin_return, d_fin_length);
    return hsr_batch_reset_dev(b, b->ep.mask, b->ep.qpos0, b->ep.mocap);
}

extern "C" int hsr_batch_sample_ctrl_dev(hsr_batch *b, uint32_t step, float *d_ctrl) {
    ENTER_DEV(b);
    const int rc = require_episodes(b, "hsr_batch_sample_ctrl_dev");
    if (rc) return rc;
    if (!d_ctrl) return fail(HSR_EINVAL, "hsr_batch_sample_ctrl_dev: null d_ctrl");
    hipLaunchKernelGGL(k_sample_ctrl, grid1(b->N), dim3(256), 0, b->stream, b->ep, b->N, b->dm.nu, b->dm.act_ctrlrange, step, d_ctrl);
    HIPCHK(hipGetLastError());
    return HSR_OK;
}

extern "C" int hsr_batch_episode_state(hsr_batch *b, uint32_t *ep_index, int32_t *ep_length, float *ep_return) {
    ENTER_DEV(b);
    const int rc = require_episodes(b, "hsr_batch_episode_state");
    if (rc) return rc;
    const size_t N = (size_t)b->N;
    HIPCHK(hipStreamSynchronize(b->stream));
    if (ep_index) HIPCHK(hipMemcpy(ep_index, b->ep.ep_index, N * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (ep_length) HIPCHK(hipMemcpy(ep_length, b->ep.ep_length, N * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (ep_return) HIPCHK(hipMemcpy(ep_return, b->ep.ep_return, N * sizeof(float), hipMemcpyDeviceToHost));
    return queue_error(b);
}
