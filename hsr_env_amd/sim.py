"""ctypes binding of libhsrsim.so (include/hsrsim.h) - the batched, GPU-resident stand-in for the
slice of ``mujoco_py`` the reference touches (hsr/mujoco_env.py:33-34,84,87-94,101-103;
hsr/env.py:116,123,144,153,169,175-176,180,184,209).

There is no CPU fallback: if the shared library is missing or no GPU is visible, construction
raises (``DependencyNotInstalled`` mirrors hsr/mujoco_env.py:12-15).
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np

from .model import Model

_HERE = Path(__file__).parent
import os
LIB_PATH = Path(os.environ.get("HSR_LIB", _HERE / "libhsrsim.so"))


class DependencyNotInstalled(ImportError):
    """Raised when libhsrsim.so (or a GPU) is unavailable - reference: gym.error.DependencyNotInstalled
    raised by hsr/mujoco_env.py:12-15 when mujoco_py is missing."""


class MujocoException(RuntimeError):
    """Some env reached a non-finite state (reference: mujoco_py.MujocoException on MuJoCo warnings)."""


def raise_if_diverged(sim):
    """MujocoException when the last step left some env of `sim` non-finite (a handle without bad_state is not asked)."""
    bad_state = getattr(sim, "bad_state", None)
    if bad_state is not None:
        bad, any_bad = bad_state()
        if any_bad:                                                     # mujoco_py.MujocoException on MuJoCo's divergence warnings
            raise MujocoException(f"simulation diverged in env(s) {np.flatnonzero(bad)[:8].tolist()} (non-finite or |q| > 1e10)")


_vp, _fp_t, _u8p, _i32p = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.POINTER(C.c_int32)
_ip, _ullp = C.POINTER(C.c_int), C.POINTER(C.c_ulonglong)
_int, _float = C.c_int, C.c_float
_dp = C.POINTER(C.c_double)
_RENDER = [_vp, _fp_t, _int, _int, _int, _fp_t]          # batch, camera, track_body, width, height, geom_rgba; then rgb, depth, segid
# the ABI as this module uses it: name -> (restype, argtypes); include/hsrsim.h declares it (tests/test_abi.py holds the two together)
PROTOTYPES = {
    "hsr_last_error": (C.c_char_p, []),
    "hsr_model_load": (_int, [C.c_char_p, C.c_size_t, C.POINTER(_vp)]),
    "hsr_model_destroy": (None, [_vp]),
    "hsr_model_size": (_int, [_vp, _int]),
    "hsr_model_timestep": (C.c_double, [_vp]),
    "hsr_model_ctrlrange": (_int, [_vp, _fp_t]),
    "hsr_model_qpos0": (_int, [_vp, _fp_t]),
    "hsr_model_body_id": (_int, [_vp, C.c_char_p]),
    "hsr_model_joint_qpos_addr": (_int, [_vp, C.c_char_p, _ip, _ip]),
    "hsr_model_hull_planes": (_int, [_vp, _int, _fp_t, _int]),
    "hsr_batch_create": (_int, [_vp, _int, _int, C.POINTER(_vp)]),
    "hsr_batch_destroy": (None, [_vp]),
    "hsr_batch_size": (_int, [_vp]),
    "hsr_batch_stream": (_vp, [_vp]),
    "hsr_batch_sync": (_int, [_vp]),
    "hsr_batch_reset": (_int, [_vp, _u8p, _fp_t, _fp_t]),
    "hsr_batch_reset_dev": (_int, [_vp, _vp, _vp, _vp]),
    "hsr_batch_get_state": (_int, [_vp, _fp_t, _fp_t, _fp_t]),
    "hsr_batch_set_state": (_int, [_vp, _fp_t, _fp_t, _fp_t]),
    "hsr_batch_set_mocap": (_int, [_vp, _fp_t]),
    "hsr_batch_set_warmstart": (_int, [_vp, _fp_t]),
    "hsr_batch_get_warmstart": (_int, [_vp, _fp_t]),
    "hsr_batch_forward": (_int, [_vp]),
    "hsr_batch_step": (_int, [_vp, _fp_t, _int, _int, _float, _fp_t, _fp_t, _u8p, _i32p]),
    "hsr_batch_step_dev": (_int, [_vp, _vp, _int, _int, _float, _vp, _vp, _vp, _vp]),
    "hsr_batch_set_goals": (_int, [_vp, _int, _ip, _ip, _fp_t]),
    "hsr_batch_body_xpos": (_int, [_vp, _int, _fp_t]),
    "hsr_batch_obs_openai": (_int, [_vp, _ip, _fp_t]),
    "hsr_batch_obs_openai_dev": (_int, [_vp, _ip, _vp]),
    "hsr_batch_render": (_int, _RENDER + [_u8p, _fp_t, _i32p]),
    "hsr_batch_render_dev": (_int, _RENDER + [_vp, _vp, _vp]),
    "hsr_batch_set_capture": (_int, [_vp, _int, _int, _i32p]),
    "hsr_batch_capture_counts": (_int, [_vp, _i32p]),
    "hsr_batch_capture_poses": (_int, [_vp, _fp_t, _fp_t]),
    "hsr_batch_render_frames": (_int, _RENDER + [_u8p, _fp_t, _i32p]),
    "hsr_batch_render_frames_dev": (_int, _RENDER + [_vp, _vp, _vp]),
    "hsr_batch_bad_state": (_int, [_vp, _u8p]),
    "hsr_batch_get_field": (_int, [_vp, _int, _fp_t]),
    "hsr_batch_set_profiling": (_int, [_vp, _int]),
    "hsr_batch_last_timing": (_int, [_vp, _fp_t, _fp_t, _ip]),
    "hsr_batch_kernel_times": (_int, [_vp, _fp_t, _int]),
    "hsr_batch_set_graph": (_int, [_vp, _int]),
    "hsr_batch_set_persistent": (_int, [_vp, _int]),
    "hsr_batch_is_persistent": (_int, [_vp]),
    "hsr_batch_set_debug": (_int, [_vp, _int]),
    "hsr_batch_set_solo": (_int, [_vp, _int, _float]),
    "hsr_batch_solo_handovers": (_int, [_vp, _ip]),
    "hsr_batch_set_split": (_int, [_vp, _int, _int, _float, _int, _int]),
    "hsr_batch_set_split_lone": (_int, [_vp, _int, _float]),
    "hsr_batch_set_schedule": (_int, [_vp, _int]),
    "hsr_batch_set_mpr_warm": (_int, [_vp, _int]),
    "hsr_batch_set_queue": (_int, [_vp, _int, _int]),
    "hsr_batch_cap_counts": (_int, [_vp, _ullp]),
    "hsr_batch_cap_histogram": (_int, [_vp, _ullp]),
    "hsr_batch_newton_trips": (_int, [_vp, _i32p]),
    "hsr_batch_packing": (_int, [_vp, _i32p]),
    "hsr_batch_set_episodes": (_int, [_vp, _vp]),
    "hsr_batch_reset_sampled_dev": (_int, [_vp, _vp]),
    "hsr_batch_reset_sampled": (_int, [_vp, _u8p]),
    "hsr_batch_episode_end_dev": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "hsr_batch_sample_ctrl_dev": (_int, [_vp, C.c_uint32, _vp]),
    "hsr_batch_episode_state": (_int, [_vp, C.POINTER(C.c_uint32), _i32p, _fp_t]),
    "hsr_batch_phase_cycles": (_int, [_vp, _ullp]),
    "hsr_batch_block_times": (_int, [_vp, _ullp, _int]),
    "hsr_batch_snapshot_create": (_int, [_vp, _int, C.POINTER(_vp)]),
    "hsr_snapshot_destroy": (None, [_vp]),
    "hsr_snapshot_capacity": (_int, [_vp]),
    "hsr_batch_snapshot_save": (_int, [_vp, _vp, _i32p, _i32p, _int]),
    "hsr_batch_snapshot_save_dev": (_int, [_vp, _vp, _vp, _vp, _int]),
    "hsr_batch_snapshot_load": (_int, [_vp, _vp, _i32p, _i32p, _int]),
    "hsr_batch_snapshot_load_dev": (_int, [_vp, _vp, _vp, _vp, _int]),
    "hsr_batch_copy_envs": (_int, [_vp, _i32p, _i32p, _int]),
    "hsr_batch_copy_envs_dev": (_int, [_vp, _vp, _vp, _int]),
    "hsr_snapshot_image_bytes": (_int, [_vp, C.POINTER(C.c_longlong)]),
    "hsr_snapshot_export": (_int, [_vp, _vp, C.c_longlong]),
    "hsr_snapshot_import": (_int, [_vp, C.c_char_p, C.c_longlong]),
    "hsr_model_snapshot_record_words": (_int, [_vp]),
    "hsr_model_snapshot_image_check": (_int, [_vp, C.c_char_p, C.c_longlong, _ip]),
    "hsr_batch_replay_create": (_int, [_vp, _vp, C.POINTER(_vp)]),
    "hsr_replay_destroy": (None, [_vp]),
    "hsr_replay_clear": (_int, [_vp]),
    "hsr_replay_commit_dev": (_int, [_vp, _vp, _vp]),
    "hsr_replay_record_dev": (_int, [_vp, _vp, _vp, _vp, _vp]),
    "hsr_replay_state": (_int, [_vp, _i32p, _i32p, C.POINTER(C.c_uint32)]),
    "hsr_replay_sample_dev": (_int, [_vp, C.c_uint32, _int, _float, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "hsr_replay_sample_seq_dev": (_int, [_vp, C.c_uint32, _int, _int, _float, _float, _vp]),
    "hsr_replay_priority_enable": (_int, [_vp, _vp]),
    "hsr_replay_priority_state": (_int, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_double), C.POINTER(C.c_float)]),
    "hsr_replay_priority_sample_dev": (_int, [_vp, C.c_uint32, _int, _float, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "hsr_replay_priority_sample_seq_dev": (_int, [_vp, C.c_uint32, _int, _int, _float, _float, _vp, _vp]),
    "hsr_replay_priority_update_dev": (_int, [_vp, C.c_uint64, _int, _vp, _vp]),
    "hsr_replay_priority_read_dev": (_int, [_vp, _vp]),
    "hsr_batch_rollout_create": (_int, [_vp, _vp, C.POINTER(_vp)]),
    "hsr_rollout_destroy": (None, [_vp]),
    "hsr_rollout_begin_dev": (_int, [_vp, _vp]),
    "hsr_rollout_stage_dev": (_int, [_vp, _vp, _vp, _vp]),
    "hsr_rollout_close_dev": (_int, [_vp, _vp, _vp, _vp]),
    "hsr_rollout_bootstrap_dev": (_int, [_vp, _vp]),
    "hsr_rollout_finish_dev": (_int, [_vp, _vp]),
    "hsr_rollout_next": (_int, [_vp]),
    "hsr_rollout_state": (_int, [_vp, _i32p, _i32p]),
    "hsr_rollout_stats": (_int, [_vp, _fp_t, _fp_t, _fp_t]),
    "hsr_rollout_minibatch_dev": (_int, [_vp, C.c_uint32, _int, _int, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "hsr_rollout_planes_dev": (_int, [_vp, _vp, _vp]),
    "hsr_batch_norm_create": (_int, [_vp, _int, _float, _float, C.POINTER(_vp)]),
    "hsr_norm_destroy": (None, [_vp]),
    "hsr_norm_clear": (_int, [_vp]),
    "hsr_norm_update_dev": (_int, [_vp, _vp, _int, _vp, _int]),
    "hsr_norm_apply_dev": (_int, [_vp, _vp, _int, _vp, _int, _int]),
    "hsr_norm_apply_batch_dev": (_int, [_vp, _vp, _vp, _int, _vp]),
    "hsr_norm_state": (_int, [_vp, _dp, _dp, _dp, C.POINTER(C.c_uint64)]),
    "hsr_norm_set_state": (_int, [_vp, C.c_double, _dp, _dp, C.c_uint64]),
    "hsr_norm_published_dev": (_int, [_vp, _vp, _vp]),
    "hsr_batch_plan_create": (_int, [_vp, _vp, C.POINTER(_vp)]),
    "hsr_plan_destroy": (None, [_vp]),
    "hsr_plan_reset_dev": (_int, [_vp, _vp]),
    "hsr_plan_shift_dev": (_int, [_vp, _vp]),
    "hsr_plan_begin_dev": (_int, [_vp]),
    "hsr_plan_sample_dev": (_int, [_vp, C.c_uint32, _int, _int, _vp]),
    "hsr_plan_accumulate_dev": (_int, [_vp, _int]),
    "hsr_plan_add_cost_dev": (_int, [_vp, _vp]),
    "hsr_plan_update_dev": (_int, [_vp]),
    "hsr_plan_action_dev": (_int, [_vp, _vp]),
    "hsr_plan_costs_dev": (_int, [_vp, _vp, _vp]),
    "hsr_plan_state_dev": (_int, [_vp, _vp, _vp]),
    "hsr_plan_best_dev": (_int, [_vp, _vp, _vp]),
    "hsr_plan_failed": (_int, [_vp, C.POINTER(C.c_uint32)]),
}
EXPORTS = list(PROTOTYPES)

CAPTURE_MAX = 1024          # include/hsrsim.h: HSR_CAPTURE_MAX

F_XPOS, F_XMAT, F_M, F_QACC, F_QACC_SMOOTH, F_QFRC_SMOOTH, F_QFRC_CONSTRAINT, F_NCON, F_NEFC, F_CONTACT, F_NITER = range(11)

_lib = None


def load_library():
    """dlopen libhsrsim.so and declare prototypes; raises DependencyNotInstalled if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise DependencyNotInstalled(
            f"{LIB_PATH} not built. Run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950); there is no CPU fallback for the product path.")
    L = C.CDLL(str(LIB_PATH))
    for name, (restype, argtypes) in PROTOTYPES.items():
        f = getattr(L, name)
        f.restype, f.argtypes = restype, argtypes
    _lib = L
    return L


def _fp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))


def _f32(a, shape=None):
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=np.float32)
    if shape is not None:
        assert a.shape == tuple(shape), f"expected shape {tuple(shape)}, got {a.shape}"
    return a


def _check(L, rc):
    if rc == 0:
        return
    msg = L.hsr_last_error().decode()
    if rc == -3:
        raise DependencyNotInstalled(f"libhsrsim: {msg}")
    if rc == -2:
        raise IOError(f"libhsrsim: {msg}")
    if rc == -5:
        raise MujocoException(f"libhsrsim: {msg}")
    if rc == -4:
        raise KeyError(msg)
    raise AssertionError(f"libhsrsim: {msg}")


class BatchSim:
    """N independent simulations advanced in lockstep on one GPU.

    Mirrors, per env, ``mujoco_py.MjSim``: ``step/forward/reset/get_state/set_state`` and the
    ``sim.data`` fields the reference reads or writes (ctrl, qpos, qvel, mocap_pos, body xpos)."""

    def __init__(self, model: Model, n_envs: int, device: int = 0):
        self.model = model
        self.n = int(n_envs)
        self._L = L = load_library()
        raw = model.to_bytes()
        self._m = C.c_void_p()
        _check(L, L.hsr_model_load(raw, len(raw), C.byref(self._m)))
        self._b = C.c_void_p()
        _check(L, L.hsr_batch_create(self._m, self.n, int(device), C.byref(self._b)))
        self.nq, self.nv, self.nu = model.nq, model.nv, model.nu
        self.device = device

    def close(self):
        if getattr(self, "_b", None):
            self._L.hsr_batch_destroy(self._b); self._b = None
        if getattr(self, "_m", None):
            self._L.hsr_model_destroy(self._m); self._m = None

    __del__ = close

    # -- sim.reset() (+ the qpos/mocap writes of reset_model) then forward
    def reset(self, mask=None, qpos0=None, mocap=None):
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        q = _f32(qpos0, (self.n, self.nq)); mc = _f32(mocap, (self.n, 3))
        _check(self._L, self._L.hsr_batch_reset(self._b, None if m is None else m.ctypes.data_as(C.POINTER(C.c_uint8)), _fp(q), _fp(mc)))

    def reset_dev(self, d_mask, d_qpos0, d_mocap):
        """Device-pointer masked reset (d_mask None/0 -> envs whose done flag was latched); async."""
        _check(self._L, self._L.hsr_batch_reset_dev(self._b, d_mask, d_qpos0, d_mocap))

    def forward(self):
        _check(self._L, self._L.hsr_batch_forward(self._b))

    # -- episodes on the device (include/hsrsim.h: hsr_batch_set_episodes ..; episodes.EpisodeSpec builds the spec)
    def set_episodes(self, spec):
        """Upload the sampler's tables and zero the per-env books (episode index, length, return); synchronises."""
        c, keep = spec.to_c()
        _check(self._L, self._L.hsr_batch_set_episodes(self._b, C.byref(c)))
        del keep

    def reset_sampled(self, mask=None):
        """The masked envs (all if None) draw their next episode on the device and restart from it; synchronises."""
        m = None if mask is None else np.ascontiguousarray(np.asarray(mask).reshape(self.n) != 0, dtype=np.uint8)
        _check(self._L, self._L.hsr_batch_reset_sampled(self._b, None if m is None else m.ctypes.data_as(_u8p)))

    def reset_sampled_dev(self, d_mask=None):
        """reset_sampled with a device mask (uint8 [N] pointer; None: all envs); asynchronous on the batch stream."""
        _check(self._L, self._L.hsr_batch_reset_sampled_dev(self._b, d_mask))

    def episode_end_dev(self, d_obs, d_reward, d_done, d_final_obs=None, d_reset_kind=None, d_fin_return=None, d_fin_length=None):
        """Close the env-step step_dev just ran: books, time limit, sampled reset of the envs that are done or truncated (device
        pointers: float32 [N,nq+nv], float32 [N], uint8 [N]; outputs float32 [N,nq+nv], uint8 [N] (0 / 1 done / 2 truncated),
        float32 [N], int32 [N], any None); asynchronous on the batch stream."""
        _check(self._L, self._L.hsr_batch_episode_end_dev(self._b, d_obs, d_reward, d_done, d_final_obs, d_reset_kind, d_fin_return, d_fin_length))

    def sample_ctrl_dev(self, step: int, d_ctrl):
        """d_ctrl float32 [N,nu] ~ U(ctrlrange) for action step `step` (0 .. 2**32 - 1); asynchronous on the batch stream."""
        _check(self._L, self._L.hsr_batch_sample_ctrl_dev(self._b, int(step) & 0xffffffff, d_ctrl))

    def episode_state(self):
        """(episode index uint32 [N], length int32 [N], return float32 [N]) of every env; synchronises."""
        i = np.empty(self.n, np.uint32); l = np.empty(self.n, np.int32); r = np.empty(self.n, np.float32)
        _check(self._L, self._L.hsr_batch_episode_state(self._b, i.ctypes.data_as(C.POINTER(C.c_uint32)), l.ctypes.data_as(_i32p), _fp(r)))
        return i, l, r

    # -- exact snapshots (include/hsrsim.h: hsr_batch_snapshot_create ..; the class Snapshot below)
    def snapshot(self, capacity=None) -> "Snapshot":
        """Device storage for `capacity` env records (default: one per env), bound to this batch's model and device."""
        return Snapshot(self, self.n if capacity is None else capacity)

    # -- hindsight replay (include/hsrsim.h: hsr_batch_replay_create ..; the class Replay below, replay.HindsightReplay on top of it)
    def replay(self, spec: "ReplaySpec") -> "Replay":
        """An episode-aware transition ring on the device with a relabelling sampler, bound to this batch."""
        return Replay(self, spec)

    # -- on-policy rollouts (include/hsrsim.h: hsr_batch_rollout_create ..; the class Rollout below, rollout.OnPolicyRollout on top of it)
    def rollout(self, spec: "RolloutSpec") -> "Rollout":
        """A store of `horizon` env-steps on the device with GAE, advantage statistics and shuffled minibatches, bound to this batch."""
        return Rollout(self, spec)

    # -- running-moments normalisers (include/hsrsim.h: hsr_batch_norm_create ..; the class Norm below, normalize.RunningNorm on top of it)
    def norm(self, dim: int, eps: float = 0.01, clip: float = 5.0) -> "Norm":
        """Running fp64 moments of `dim` columns on the device with their float32 publish and clipped apply, bound to this batch."""
        return Norm(self, dim, eps, clip)

    # -- cross-entropy-method planners (include/hsrsim.h: hsr_batch_plan_create ..; the class Plan below, planner.CEMPlanner on top of it)
    def plan(self, spec: "PlanSpec") -> "Plan":
        """A CEM planner whose candidates are this batch's envs (groups x samples of them), bound to this batch."""
        return Plan(self, spec)

    def copy_envs(self, src, dst):
        """env dst[i] <- env src[i] on the device, every source read before any destination is written; the destinations then continue
        bit for bit as their sources do.  int32 numpy arrays / sequences (checked, synchronises) or torch int32 tensors on the batch's
        device (asynchronous on the batch stream; ids out of range are skipped, a repeated destination is the caller's error)."""
        dev, a, b, n, keep = _id_pair(self, src, dst)
        fn = self._L.hsr_batch_copy_envs_dev if dev else self._L.hsr_batch_copy_envs
        _check(self._L, fn(self._b, a, b, n))
        del keep

    def get_state(self):
        t = np.empty(self.n, np.float32); q = np.empty((self.n, self.nq), np.float32); v = np.empty((self.n, self.nv), np.float32)
        _check(self._L, self._L.hsr_batch_get_state(self._b, _fp(t), _fp(q), _fp(v)))
        return t, q, v

    def set_state(self, time=None, qpos=None, qvel=None):
        t = _f32(time, (self.n,)); q = _f32(qpos, (self.n, self.nq)); v = _f32(qvel, (self.n, self.nv))
        _check(self._L, self._L.hsr_batch_set_state(self._b, _fp(t), _fp(q), _fp(v)))

    def set_mocap(self, mocap):
        _check(self._L, self._L.hsr_batch_set_mocap(self._b, _fp(_f32(mocap, (self.n, 3)))))

    def set_warmstart(self, w):
        _check(self._L, self._L.hsr_batch_set_warmstart(self._b, _fp(_f32(w, (self.n, self.nv)))))

    def get_warmstart(self):
        w = np.empty((self.n, self.nv), np.float32)
        _check(self._L, self._L.hsr_batch_get_warmstart(self._b, _fp(w)))
        return w

    def step(self, ctrl, n_substeps, goal_body=-1, geofence=0.0):
        """HSREnv.step for all envs -> (obs[N,nq+nv], reward[N], done[N] bool, nsteps[N])."""
        c = _f32(ctrl, (self.n, self.nu))
        obs = np.empty((self.n, self.nq + self.nv), np.float32); rew = np.empty(self.n, np.float32)
        done = np.empty(self.n, np.uint8); ns = np.empty(self.n, np.int32)
        _check(self._L, self._L.hsr_batch_step(self._b, _fp(c), int(n_substeps), int(goal_body), float(geofence), _fp(obs), _fp(rew),
                                               done.ctypes.data_as(C.POINTER(C.c_uint8)), ns.ctypes.data_as(C.POINTER(C.c_int32))))
        return obs, rew, done.astype(bool), ns

    def step_dev(self, d_ctrl, n_substeps, goal_body, geofence, d_obs=None, d_reward=None, d_done=None, d_nsteps=None):
        """Device-pointer variant (ints from tensor.data_ptr()); asynchronous on the batch stream."""
        _check(self._L, self._L.hsr_batch_step_dev(self._b, d_ctrl, int(n_substeps), int(goal_body), float(geofence),
                                                   d_obs, d_reward, d_done, d_nsteps))

    def sync(self):
        _check(self._L, self._L.hsr_batch_sync(self._b))

    def stream_ptr(self) -> int:
        """hipStream_t of the batch (wrap with torch.cuda.ExternalStream to order torch ops after steps)."""
        return int(self._L.hsr_batch_stream(self._b))

    def body_xpos(self, body_id: int):
        out = np.empty((self.n, 3), np.float32)
        _check(self._L, self._L.hsr_batch_body_xpos(self._b, int(body_id), _fp(out)))
        return out

    def openai_ids(self, finger_bodies=("hand_l_distal_link", "hand_r_distal_link"), object_body=None,
                   finger_joints=("hand_l_proximal_joint", "hand_r_proximal_joint")):
        """Body ids / joint addresses the fused 'openai' observation needs (names of hsr/env.py:58-59,90-97)."""
        m = self.model
        jn, qa, da = m.names["joint"], m.meta["joint_qposadr"], m.meta["joint_dofadr"]
        ids = [m.body_id(finger_bodies[0]), m.body_id(finger_bodies[1]), m.body_id(object_body or m.block_body())]
        ids += [qa[jn.index(j)][0] for j in finger_joints] + [da[jn.index(j)] for j in finger_joints]
        return (C.c_int * 7)(*ids)

    def obs_openai(self, ids=None):
        """[N, 25] 'openai' observation (include/hsrsim.h: hsr_batch_obs_openai)."""
        out = np.empty((self.n, 25), np.float32)
        _check(self._L, self._L.hsr_batch_obs_openai(self._b, ids or self.openai_ids(), _fp(out)))
        return out

    def obs_openai_dev(self, d_out, ids=None):
        _check(self._L, self._L.hsr_batch_obs_openai_dev(self._b, ids or self.openai_ids(), C.c_void_p(int(d_out))))

    def _render_args(self, camera, geom_rgba):
        from .render import default_camera
        cam = camera if camera is not None else default_camera(self.model)
        pal = None if geom_rgba is None else _f32(geom_rgba, (self.model.ngeom, 4))
        return cam.as_array(), int(cam.track_body), pal

    def _render_host(self, fn, lead, fill, width, height, camera, rgb, depth, segmentation, geom_rgba):
        """render / render_frames: outputs of shape lead + (H, W[, 3]); before the call they hold `fill` (rgb, depth, segmentation; None: anything)."""
        cam, track, pal = self._render_args(camera, geom_rgba)
        w, h = int(width), int(height)
        ok = 1 <= w <= 4096 and 1 <= h <= 4096
        new = lambda shape, dt, v: np.empty(shape, dt) if v is None else np.full(shape, v, dt)
        o_rgb = new(lead + (h, w, 3), np.uint8, fill[0]) if rgb and ok else None
        o_dep = new(lead + (h, w), np.float32, fill[1]) if depth and ok else None
        o_seg = new(lead + (h, w), np.int32, fill[2]) if segmentation and ok else None
        _check(self._L, fn(self._b, _fp(cam), track, w, h, _fp(pal), None if o_rgb is None else o_rgb.ctypes.data_as(C.POINTER(C.c_uint8)),
                           _fp(o_dep), None if o_seg is None else o_seg.ctypes.data_as(C.POINTER(C.c_int32))))
        outs = [o for o, want in ((o_rgb, rgb), (o_dep, depth), (o_seg, segmentation)) if want]
        return outs[0] if len(outs) == 1 else tuple(outs)

    def _render_dev(self, who, fn, lead, width, height, camera, rgb, depth, segmentation, geom_rgba):
        """render_dev / render_frames_dev: check the caller's tensors (shape lead + (H, W[, 3])) and launch on the batch stream."""
        cam, track, pal = self._render_args(camera, geom_rgba)
        w, h = int(width), int(height)
        for t, shape, dt in ((rgb, lead + (h, w, 3), "torch.uint8"), (depth, lead + (h, w), "torch.float32"),
                             (segmentation, lead + (h, w), "torch.int32")):
            if t is not None:
                if tuple(t.shape) != shape or str(t.dtype) != dt or not t.is_contiguous() or t.device.type != "cuda":
                    raise AssertionError(f"{who}: expected a contiguous {dt} tensor of shape {shape} on the GPU")
                if t.device.index != self.device:
                    raise AssertionError(f"{who}: tensor on cuda:{t.device.index}, the batch is on cuda:{self.device}")
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        _check(self._L, fn(self._b, _fp(cam), track, w, h, _fp(pal), ptr(rgb), ptr(depth), ptr(segmentation)))

    def render(self, width, height, camera=None, rgb=True, depth=False, segmentation=False, geom_rgba=None):
        """Images of every env from one camera (include/hsrsim.h: hsr_batch_render) -> the requested ones of
        rgb uint8 [N,H,W,3], depth float32 [N,H,W] (distance along the camera axis; zfar on background), segmentation int32 [N,H,W]
        (geom id, -1 on background), in that order; a single array when one is requested.  camera: render.Camera (None: the
        model's default_camera); geom_rgba: [ngeom,4] colours (None: render.default_palette).  Poses of the last reset / forward / step."""
        fn = self._L.hsr_batch_render
        return self._render_host(fn, (self.n,), (None, None, None), width, height, camera, rgb, depth, segmentation, geom_rgba)

    def render_dev(self, width, height, camera=None, rgb=None, depth=None, segmentation=None, geom_rgba=None):
        """render() into caller-provided torch tensors on the batch's device (uint8 [N,H,W,3], float32 [N,H,W], int32 [N,H,W];
        None skips an output); asynchronous on the batch stream (stream_ptr)."""
        self._render_dev("render_dev", self._L.hsr_batch_render_dev, (self.n,), width, height, camera, rgb, depth, segmentation, geom_rgba)

    # -- in-step frame capture (include/hsrsim.h: hsr_batch_set_capture; the recorder of hsr/env.py:118-131)
    def set_capture(self, env_ids, every):
        """Capture the link poses of the envs `env_ids` (slot r = env_ids[r]) every `every` substeps of each later step, before the
        substep's dynamics, while the env is live; plus one final frame per slot with the poses after the step.  every = 0: off."""
        ids = np.ascontiguousarray(np.atleast_1d(np.asarray(env_ids if every else [], dtype=np.int32)))
        self._cap_n = len(ids) if every else 0
        _check(self._L, self._L.hsr_batch_set_capture(self._b, int(every), len(ids), ids.ctypes.data_as(C.POINTER(C.c_int32)) if len(ids) else None))

    def capture_counts(self):
        """Frames of every slot in the last step (the final frame not counted): int32 [n]."""
        out = np.empty(max(getattr(self, "_cap_n", 0), 1), np.int32)
        rc = self._L.hsr_batch_capture_counts(self._b, out.ctypes.data_as(C.POINTER(C.c_int32)))
        if rc < 0:
            _check(self._L, rc)
        return out[:self._cap_n]

    def capture_rows(self):
        """Rows per slot of the last step: the frames of its longest possible run, then the final frame."""
        rc = self._L.hsr_batch_capture_counts(self._b, None)
        if rc < 0:
            _check(self._L, rc)
        return rc

    def capture_poses(self):
        """(xpos float32 [n, rows, nlink, 3], xmat [n, rows, nlink, 3, 3]) of the last step; row k < count: frame k, last row: the final frame."""
        rows, nl = self.capture_rows(), self.model.nlink
        xpos = np.empty((self._cap_n, rows, nl, 3), np.float32); xmat = np.empty((self._cap_n, rows, nl, 3, 3), np.float32)
        _check(self._L, self._L.hsr_batch_capture_poses(self._b, _fp(xpos), _fp(xmat)))
        return xpos, xmat

    def render_frames(self, width, height, camera=None, rgb=True, depth=False, segmentation=False, geom_rgba=None):
        """render() of the captured frames of the last step: rgb uint8 [n, rows, H, W, 3], depth float32 [n, rows, H, W], segmentation
        int32 [n, rows, H, W] (the requested ones, in that order; a single array when one is requested); row k < capture_counts()[slot]
        is frame k, the last row the final frame, the rows in between are zero (depth: NaN, segmentation: -2)."""
        fn, lead = self._L.hsr_batch_render_frames, (self._cap_n, self.capture_rows())
        return self._render_host(fn, lead, (0, np.nan, -2), width, height, camera, rgb, depth, segmentation, geom_rgba)

    def render_frames_dev(self, width, height, camera=None, rgb=None, depth=None, segmentation=None, geom_rgba=None):
        """render_frames() into caller-provided torch tensors on the batch's device (uint8 [n,rows,H,W,3], float32 [n,rows,H,W], int32
        [n,rows,H,W]; None skips an output); the rows past a slot's count are left as they are.  Asynchronous on the batch stream."""
        fn, lead = self._L.hsr_batch_render_frames_dev, (self._cap_n, self.capture_rows())
        self._render_dev("render_frames_dev", fn, lead, width, height, camera, rgb, depth, segmentation, geom_rgba)

    def bad_state(self):
        out = np.empty(self.n, np.uint8)
        rc = self._L.hsr_batch_bad_state(self._b, out.ctypes.data_as(C.POINTER(C.c_uint8)))
        if rc not in (0, -5):
            _check(self._L, rc)
        return out.astype(bool), rc == -5

    def get_field(self, field: int):
        m = self.model
        shapes = {F_XPOS: (self.n, m.nlink, 3), F_XMAT: (self.n, m.nlink, 3, 3), F_M: (self.n, m.nv, m.nv),
                  F_QACC: (self.n, m.nv), F_QACC_SMOOTH: (self.n, m.nv), F_QFRC_SMOOTH: (self.n, m.nv),
                  F_QFRC_CONSTRAINT: (self.n, m.nv), F_NCON: (self.n,), F_NEFC: (self.n,), F_NITER: (self.n,),
                  F_CONTACT: (self.n, m.nslot, 7)}
        out = np.empty(shapes[field], np.float32)
        _check(self._L, self._L.hsr_batch_get_field(self._b, field, _fp(out)))
        return out

    def set_profiling(self, on):
        """True / 1: time the next step (synchronises); 2: log every launch of the persistent kernel (no synchronisation)."""
        _check(self._L, self._L.hsr_batch_set_profiling(self._b, int(on)))

    def set_mpr_warm(self, on: bool):
        """Portal warm start of the convex-pair narrowphase (include/hsrsim.h: hsr_batch_set_mpr_warm)."""
        _check(self._L, self._L.hsr_batch_set_mpr_warm(self._b, int(on)))

    def set_queue(self, mode: int, chunk: int = 0):
        """Work queue of the persistent kernel: mode -1 automatic, 0 off, 1 on; chunk = substeps per round (0 keeps the current one)."""
        _check(self._L, self._L.hsr_batch_set_queue(self._b, int(mode), int(chunk)))

    def kernel_times(self, cap: int = 4096):
        """Durations (ms) of the persistent-kernel launches logged since the last call (set_profiling(2)); synchronises."""
        buf = (C.c_float * cap)()
        n = self._L.hsr_batch_kernel_times(self._b, buf, cap)
        if n < 0:
            _check(self._L, n)
        if n > cap:
            raise ValueError(f"{n} launches were logged, the buffer holds {cap}: pass cap >= the number of launches since the last call")
        return np.array(buf[:n], dtype=np.float64)

    def set_graph(self, on: bool):
        _check(self._L, self._L.hsr_batch_set_graph(self._b, int(on)))

    def set_persistent(self, on: bool) -> bool:
        return bool(self._L.hsr_batch_set_persistent(self._b, int(on)))

    def is_persistent(self) -> bool:
        return bool(self._L.hsr_batch_is_persistent(self._b))

    def kernel_flags(self) -> int:
        """hsr_batch_is_persistent's bit mask: 1 = whole env-step in the persistent kernel, 2 = the instance carries the model's scalars as
        compile-time constants, 4 = and its kinematic tree (csrc/kin3.h)."""
        return int(self._L.hsr_batch_is_persistent(self._b))

    def set_debug(self, on):
        """Also store the contact counts / solver counters of each env's last substep during step() (persistent kernel).
        `on` may be a bit mask: 1 = store, 2 / 4 = test hooks (J v per contact / PSD-majorant Newton steps), include/hsrsim.h."""
        _check(self._L, self._L.hsr_batch_set_debug(self._b, int(on)))

    def set_goals(self, terms):
        """Further goal terms [(body_a, body_b, distance), ...] AND-ed with the main term of step() (include/hsrsim.h)."""
        n = len(terms)
        a = (C.c_int * max(n, 1))(*[int(t[0]) for t in terms]); b = (C.c_int * max(n, 1))(*[int(t[1]) for t in terms])
        d = (C.c_float * max(n, 1))(*[float(t[2]) for t in terms])
        _check(self._L, self._L.hsr_batch_set_goals(self._b, n, a, b, d))

    def set_solo(self, servers: int, trips: float = 0.0) -> bool:
        """Solo servers of the persistent kernel (include/hsrsim.h): `servers` workgroups run hard envs alone; 0 = off.  Results then
        depend on the hand-over at rounding level (another summation order of the contact terms), not bit for bit.  False when the model's kernel instance has no server path."""
        rc = self._L.hsr_batch_set_solo(self._b, int(servers), float(trips))
        if rc < 0:
            _check(self._L, rc)
        return rc == 0

    def solo_handovers(self) -> int:
        """Envs handed over to solo servers by the last step() (persistent kernel); synchronises."""
        out = C.c_int(0)
        _check(self._L, self._L.hsr_batch_solo_handovers(self._b, C.byref(out)))
        return int(out.value)

    def set_split(self, on: bool, period: int = 0, trips: float = -1.0, min_left: int = 0, extra_helpers: int = 0) -> bool:
        """Hand-over of hard envs inside a launch (include/hsrsim.h): a wave that finds two or more hard envs among its own gives all but
        the hardest to workgroups that have finished; never changes a result.  period / trips / min_left: 0 / negative / 0 keep the current
        value; trips = 0 counts every live env as hard and extra_helpers adds workgroups without a task (both for tests).  solo_handovers()
        counts the hand-overs of the last step.  False when the batch's kernel instance never splits."""
        rc = self._L.hsr_batch_set_split(self._b, int(on), int(period), float(trips), int(min_left), int(extra_helpers))
        if rc < 0:
            _check(self._L, rc)
        return rc == 0

    def set_split_lone(self, on: bool, trips: float = -1.0) -> bool:
        """The lone rule of the hand-over inside a launch (include/hsrsim.h): a wave whose hardest env ran `trips` Newton iterations per
        substep or more, next to a live env that ran fewer, gives that env to a finished workgroup too and goes on with the easier ones;
        never changes a result.  Needs set_split on; trips <= 0 keeps the current threshold.  False when the batch's kernel instance
        never splits."""
        rc = self._L.hsr_batch_set_split_lone(self._b, int(on), float(trips))
        if rc < 0:
            _check(self._L, rc)
        return rc == 0

    def set_schedule(self, on: bool):
        """Wave packing of the persistent kernel by env hardness (default on); never changes a result."""
        _check(self._L, self._L.hsr_batch_set_schedule(self._b, int(on)))

    def cap_counts(self):
        """(contact-cap hits, row-cap hits, item-cap hits, env-substeps executed) since the last call."""
        out = (C.c_ulonglong * 4)()
        _check(self._L, self._L.hsr_batch_cap_counts(self._b, out))
        return tuple(int(x) for x in out)

    def cap_histogram(self):
        """Row-cap events by how many rows beyond njmax the env wanted (bins of 8 rows, last bin open); cleared by the call."""
        out = (C.c_ulonglong * 8)()
        _check(self._L, self._L.hsr_batch_cap_histogram(self._b, out))
        return [int(x) for x in out]

    def newton_trips(self):
        """Newton iterations of every env over the last (up to) 100 substeps of the previous step() (persistent kernel)."""
        out = np.empty(self.n, np.int32)
        _check(self._L, self._L.hsr_batch_newton_trips(self._b, out.ctypes.data_as(C.POINTER(C.c_int32))))
        return out

    def packing(self, envs_per_wave: int):
        """env held by every lane group of every task of the last persistent launch (-1: empty), [tasks, envs_per_wave]."""
        if envs_per_wave not in (2, 4):
            raise ValueError("envs_per_wave is 4 (16 lanes per env) or 2 (32 lanes per env)")
        # the library writes ceil(N / epw) * epw entries with ITS envs-per-wave: the buffer covers either value whatever the caller passed
        out = np.full(self.n + 64, -1, np.int32)
        _check(self._L, self._L.hsr_batch_packing(self._b, out.ctypes.data_as(C.POINTER(C.c_int32))))
        slots = (self.n + envs_per_wave - 1) // envs_per_wave * envs_per_wave
        return out[:slots].reshape(-1, envs_per_wave)

    def last_timing(self):
        tot = C.c_float(0); k = (C.c_float * 3)(); n = (C.c_int * 3)()
        _check(self._L, self._L.hsr_batch_last_timing(self._b, C.byref(tot), k, n))
        return float(tot.value), [float(x) for x in k], [int(x) for x in n]


def _id_pair(sim, a, b):
    """Two id arrays of one length (either may be None = 0..n-1; both None: every env) -> (device variant?, pointer a, pointer b, n, what
    keeps the pointers alive).  numpy arrays / sequences: int32 host pointers; torch tensors (int32, contiguous, on the batch's device):
    their data_ptr()."""
    dev = [x is not None and hasattr(x, "data_ptr") for x in (a, b)]
    if any(dev):
        for x in (a, b):
            if x is None:
                continue
            if not hasattr(x, "data_ptr"):
                raise AssertionError("ids: device tensors and host arrays cannot be mixed in one call")
            if str(x.dtype) != "torch.int32" or x.dim() != 1 or not x.is_contiguous() or x.device.type != "cuda" or x.device.index != sim.device:
                raise AssertionError(f"ids: expected a contiguous 1-d torch.int32 tensor on cuda:{sim.device}")
        ptr = lambda x: None if x is None else C.c_void_p(x.data_ptr())
        keep = (a, b)
    else:
        a, b = [None if x is None else np.ascontiguousarray(np.atleast_1d(x), dtype=np.int32) for x in (a, b)]
        for x in (a, b):
            if x is not None and x.ndim != 1:
                raise AssertionError("ids: expected 1-d arrays")
        ptr = lambda x: None if x is None else x.ctypes.data_as(_i32p)
        keep = (a, b)
    lens = {int(x.shape[0]) for x in keep if x is not None}
    if len(lens) > 1:
        raise AssertionError("ids: the two arrays differ in length")
    return any(dev), ptr(keep[0]), ptr(keep[1]), (lens.pop() if lens else sim.n), keep


class Snapshot:
    """Env records on the device (include/hsrsim.h: hsr_snapshot): everything of an env that a later step, forward or getter reads -
    state, warm start, collision caches, last poses, episode books - so that a loaded env continues bit for bit.  Bound to
    the model and the device of the batch that made it, not to the batch: ``load(into=other)`` restores into another BatchSim of the
    same model.  Its storage is released by close() or by close() of the batch that made it, whichever comes first."""

    def __init__(self, sim: BatchSim, capacity: int):
        self.sim = sim
        self._s = C.c_void_p()
        _check(sim._L, sim._L.hsr_batch_snapshot_create(sim._b, int(capacity), C.byref(self._s)))
        self.capacity = int(capacity)

    def close(self):
        if getattr(self, "_s", None):
            self.sim._L.hsr_snapshot_destroy(self._s); self._s = None

    __del__ = close

    def save(self, envs=None, slots=None):
        """record slots[i] <- env envs[i] (None: 0..n-1; both None: every env, capacity permitting).  Host ids are checked and the call
        synchronises; torch int32 tensors on the batch's device launch asynchronously on the batch stream."""
        dev, e, s, n, keep = _id_pair(self.sim, envs, slots)
        L = self.sim._L
        _check(L, (L.hsr_batch_snapshot_save_dev if dev else L.hsr_batch_snapshot_save)(self.sim._b, self._s, e, s, n))
        del keep

    def load(self, slots=None, envs=None, into: BatchSim = None):
        """env envs[i] <- record slots[i] of `into` (default: the batch that made the snapshot; None: 0..n-1; both None: every env, capacity
        permitting, as in save()); a slot may feed any number of envs.  No forward pass runs: the loaded envs hold the poses the record was
        saved with."""
        sim = into if into is not None else self.sim
        dev, s, e, n, keep = _id_pair(sim, slots, envs)
        L = sim._L
        _check(L, (L.hsr_batch_snapshot_load_dev if dev else L.hsr_batch_snapshot_load)(sim._b, self._s, s, e, n))
        del keep

    def to_bytes(self) -> bytes:
        """The host image (header + records): what a checkpoint file holds."""
        L = self.sim._L
        size = C.c_longlong(0)
        _check(L, L.hsr_snapshot_image_bytes(self._s, C.byref(size)))
        buf = C.create_string_buffer(size.value)
        _check(L, L.hsr_snapshot_export(self._s, buf, size.value))
        return buf.raw

    def _from_image(self, data: bytes):
        """Replace the records by those of an image of the same model and capacity (IOError otherwise; the records then stay as they were)."""
        L = self.sim._L
        _check(L, L.hsr_snapshot_import(self._s, bytes(data), len(data)))
        return self

    @classmethod
    def from_bytes(cls, sim: BatchSim, data: bytes) -> "Snapshot":
        """A snapshot of `sim`'s model holding the records of an image written by to_bytes() (IOError: not an image of this model)."""
        L = sim._L
        cap = C.c_int(0)
        _check(L, L.hsr_model_snapshot_image_check(sim._m, bytes(data), len(data), C.byref(cap)))
        return cls(sim, cap.value)._from_image(data)


class ReplaySpec(C.Structure):
    """include/hsrsim.h: hsr_replay_spec."""
    _fields_ = [("seed", C.c_uint64), ("env_offset", C.c_uint32), ("capacity_steps", C.c_int32), ("obs_dim", C.c_int32),
                ("goal_body", C.c_int32), ("geofence", C.c_float)]


class PrioritySpec(C.Structure):
    """include/hsrsim.h: hsr_priority_spec."""
    _fields_ = [("p_init", C.c_float), ("p_min", C.c_float), ("p_max", C.c_float), ("max_batch", C.c_int32)]


class ReplaySeqOut(C.Structure):
    """include/hsrsim.h: hsr_replay_seq_out - device addresses, each may be None."""
    _fields_ = [(name, C.c_void_p) for name in ("obs", "act", "next_obs", "achieved_next", "goal", "reward", "done", "length", "nstep", "nstep_return",
                                                "nstep_discount", "nstep_obs", "nstep_done", "index")]


class Replay:
    """The transition ring of a batch (include/hsrsim.h: hsr_replay) as the library exposes it: device pointers in, asynchronous on the
    batch stream.  Its storage is released by close() or by close() of its batch, whichever comes first."""

    def __init__(self, sim: BatchSim, spec: ReplaySpec):
        self.sim, self.spec = sim, spec
        self._r = C.c_void_p()
        _check(sim._L, sim._L.hsr_batch_replay_create(sim._b, C.byref(spec), C.byref(self._r)))

    def close(self):
        if getattr(self, "_r", None):
            self.sim._L.hsr_replay_destroy(self._r); self._r = None

    __del__ = close

    def clear(self):
        _check(self.sim._L, self.sim._L.hsr_replay_clear(self._r))

    def commit_dev(self, d_obs, d_reset=None):
        """d_obs float32 [N, obs_dim]: what the policy acts on next; d_reset uint8 [N]: the envs that start an episode with it (None: all)."""
        _check(self.sim._L, self.sim._L.hsr_replay_commit_dev(self._r, d_obs, d_reset))

    def record_dev(self, d_ctrl, d_next_obs, d_reward=None, d_done=None):
        """After step_dev and before episode_end_dev: the transition of every env into the ring's head slot."""
        _check(self.sim._L, self.sim._L.hsr_replay_record_dev(self._r, d_ctrl, d_next_obs, d_reward, d_done))

    def state(self):
        """(count, head slot, pushed & 0xffffffff): the host books, no device work."""
        c, h, p = C.c_int32(0), C.c_int32(0), C.c_uint32(0)
        _check(self.sim._L, self.sim._L.hsr_replay_state(self._r, C.byref(c), C.byref(h), C.byref(p)))
        return int(c.value), int(h.value), int(p.value)

    def sample_dev(self, draw, batch, her_ratio, d_obs=None, d_act=None, d_next_obs=None, d_goal=None, d_achieved_next=None, d_reward=None,
                   d_done=None, d_index=None):
        """Minibatch `draw` of `batch` samples into device arrays (any None); include/hsrsim.h states the function."""
        _check(self.sim._L, self.sim._L.hsr_replay_sample_dev(self._r, int(draw) & 0xffffffff, int(batch), float(her_ratio), d_obs, d_act, d_next_obs,
                                                              d_goal, d_achieved_next, d_reward, d_done, d_index))

    def sample_seq_dev(self, draw, batch, seq_len, her_ratio, gamma, out: "ReplaySeqOut"):
        """Windows of up to `seq_len` steps and their n-step targets for minibatch `draw` into the device arrays of `out` (any None);
        include/hsrsim.h states the function."""
        _check(self.sim._L, self.sim._L.hsr_replay_sample_seq_dev(self._r, int(draw) & 0xffffffff, int(batch), int(seq_len), float(her_ratio), float(gamma),
                                                                  None if out is None else C.byref(out)))

    # -- priorities (include/hsrsim.h: hsr_replay_priority_*)
    def priority_enable(self, spec: "PrioritySpec"):
        """Only on an empty replay: a sum tree over the ring's cells; new transitions enter with the largest priority stored so far."""
        _check(self.sim._L, self.sim._L.hsr_replay_priority_enable(self._r, C.byref(spec)))

    def priority_state(self):
        """(pushed, total, p_new) after a synchronisation of the batch stream; pushed is the sampled_at token of a sample taken now."""
        n, t, p = C.c_uint64(0), C.c_double(0), C.c_float(0)
        _check(self.sim._L, self.sim._L.hsr_replay_priority_state(self._r, C.byref(n), C.byref(t), C.byref(p)))
        return int(n.value), float(t.value), float(p.value)

    def priority_sample_dev(self, draw, batch, her_ratio, d_obs=None, d_act=None, d_next_obs=None, d_goal=None, d_achieved_next=None, d_reward=None,
                            d_done=None, d_index=None, d_prob=None):
        _check(self.sim._L, self.sim._L.hsr_replay_priority_sample_dev(self._r, int(draw) & 0xffffffff, int(batch), float(her_ratio), d_obs, d_act,
                                                                       d_next_obs, d_goal, d_achieved_next, d_reward, d_done, d_index, d_prob))

    def priority_sample_seq_dev(self, draw, batch, seq_len, her_ratio, gamma, out: "ReplaySeqOut", d_prob=None):
        _check(self.sim._L, self.sim._L.hsr_replay_priority_sample_seq_dev(self._r, int(draw) & 0xffffffff, int(batch), int(seq_len), float(her_ratio),
                                                                           float(gamma), None if out is None else C.byref(out), d_prob))

    def priority_update_dev(self, sampled_at, batch, d_index, d_priority):
        """d_index int32 [batch, 4] as a sample wrote it (env and slot are read), d_priority float32 [batch]; rows of cells overwritten
        since `sampled_at` are skipped."""
        _check(self.sim._L, self.sim._L.hsr_replay_priority_update_dev(self._r, int(sampled_at), int(batch), d_index, d_priority))

    def priority_read_dev(self, d_leaves):
        """The leaves, float32 [T, N], into a device array."""
        _check(self.sim._L, self.sim._L.hsr_replay_priority_read_dev(self._r, d_leaves))


class RolloutSpec(C.Structure):
    """include/hsrsim.h: hsr_rollout_spec."""
    _fields_ = [("seed", C.c_uint64), ("env_offset", C.c_uint32), ("horizon", C.c_int32), ("obs_dim", C.c_int32), ("gamma", C.c_float),
                ("lam", C.c_float)]


ROLLOUT_EMPTY, ROLLOUT_READY, ROLLOUT_STAGED, ROLLOUT_DONE = range(4)


class Rollout:
    """The on-policy rollout store of a batch (include/hsrsim.h: hsr_rollout) as the library exposes it: device pointers in, asynchronous
    on the batch stream.  Its storage is released by close() or by close() of its batch, whichever comes first."""

    def __init__(self, sim: BatchSim, spec: RolloutSpec):
        self.sim, self.spec = sim, spec
        self._r = C.c_void_p()
        _check(sim._L, sim._L.hsr_batch_rollout_create(sim._b, C.byref(spec), C.byref(self._r)))

    def close(self):
        if getattr(self, "_r", None):
            self.sim._L.hsr_rollout_destroy(self._r); self._r = None

    __del__ = close

    def begin_dev(self, d_obs):
        """d_obs float32 [N, obs_dim]: what the policy acts on first; from any state to READY(0)."""
        _check(self.sim._L, self.sim._L.hsr_rollout_begin_dev(self._r, d_obs))

    def stage_dev(self, d_act, d_logp, d_value):
        """Slot t: the head observation, d_act float32 [N, nu], d_logp and d_value float32 [N]."""
        _check(self.sim._L, self.sim._L.hsr_rollout_stage_dev(self._r, d_act, d_logp, d_value))

    def close_dev(self, d_reward, d_kind, d_next_obs):
        """Slot t: d_reward float32 [N], d_kind uint8 [N] (episode_end_dev's reset kind); d_next_obs [N, obs_dim] becomes the head."""
        _check(self.sim._L, self.sim._L.hsr_rollout_close_dev(self._r, d_reward, d_kind, d_next_obs))

    def bootstrap_dev(self, d_value_terminal):
        """float32 [N]: the critic's value of the terminal observation of the step closed last (read where kind == 2)."""
        _check(self.sim._L, self.sim._L.hsr_rollout_bootstrap_dev(self._r, d_value_terminal))

    def finish_dev(self, d_last_value):
        """float32 [N]: V(head) after the last step; runs GAE and the statistics."""
        _check(self.sim._L, self.sim._L.hsr_rollout_finish_dev(self._r, d_last_value))

    def next(self):
        _check(self.sim._L, self.sim._L.hsr_rollout_next(self._r))

    def state(self):
        """(state, steps closed): the host books, no device work."""
        s, t = C.c_int32(0), C.c_int32(0)
        _check(self.sim._L, self.sim._L.hsr_rollout_state(self._r, C.byref(s), C.byref(t)))
        return int(s.value), int(t.value)

    def stats(self):
        """(mean, std, rstd) of the advantages as the device keeps them (float32); synchronises."""
        m, s, r = C.c_float(0), C.c_float(0), C.c_float(0)
        _check(self.sim._L, self.sim._L.hsr_rollout_stats(self._r, C.byref(m), C.byref(s), C.byref(r)))
        return np.float32(m.value), np.float32(s.value), np.float32(r.value)

    def minibatch_dev(self, epoch, first, count, normalize, d_obs=None, d_act=None, d_logp=None, d_value=None, d_adv=None, d_ret=None, d_index=None):
        """Rows first .. first + count - 1 of the shuffle of `epoch` into device arrays (any None); include/hsrsim.h states the function."""
        _check(self.sim._L, self.sim._L.hsr_rollout_minibatch_dev(self._r, int(epoch) & 0xffffffff, int(first), int(count), int(bool(normalize)), d_obs, d_act,
                                                                  d_logp, d_value, d_adv, d_ret, d_index))

    def planes_dev(self, d_adv=None, d_ret=None):
        """The advantage and return planes, float32 [T, N] each (either None)."""
        _check(self.sim._L, self.sim._L.hsr_rollout_planes_dev(self._r, d_adv, d_ret))


class NormItem(C.Structure):
    """include/hsrsim.h: hsr_norm_item."""
    _fields_ = [("d_rows", C.c_void_p), ("rows", C.c_int64), ("seq_len", C.c_int32), ("which", C.c_int32)]


class Norm:
    """A running-moments normaliser of a batch (include/hsrsim.h: hsr_norm) as the library exposes it: device pointers in, asynchronous on
    the batch stream.  Its storage is released by close() or by close() of its batch, whichever comes first."""

    def __init__(self, sim: BatchSim, dim: int, eps: float, clip: float):
        self.sim, self.dim = sim, int(dim)
        self._r = C.c_void_p()
        _check(sim._L, sim._L.hsr_batch_norm_create(sim._b, int(dim), float(eps), float(clip), C.byref(self._r)))

    def close(self):
        if getattr(self, "_r", None):
            self.sim._L.hsr_norm_destroy(self._r); self._r = None

    __del__ = close

    def clear(self):
        _check(self.sim._L, self.sim._L.hsr_norm_clear(self._r))

    def update_dev(self, d_rows, stride, d_mask, n):
        """d_rows float32 [n, dim] with `stride` floats between rows; d_mask uint8 [n] or None."""
        _check(self.sim._L, self.sim._L.hsr_norm_update_dev(self._r, d_rows, int(stride), d_mask, int(n)))

    def apply_dev(self, d_in, in_stride, d_out, out_stride, n):
        _check(self.sim._L, self.sim._L.hsr_norm_apply_dev(self._r, d_in, int(in_stride), d_out, int(out_stride), int(n)))

    def state(self):
        """(count, mean [dim], m2 [dim], skipped) as the device keeps them (fp64; skipped an int); synchronises."""
        count, skipped = C.c_double(0), C.c_uint64(0)
        mean, m2 = np.empty(self.dim, np.float64), np.empty(self.dim, np.float64)
        _check(self.sim._L, self.sim._L.hsr_norm_state(self._r, C.byref(count), mean.ctypes.data_as(_dp), m2.ctypes.data_as(_dp), C.byref(skipped)))
        return float(count.value), mean, m2, int(skipped.value)

    def set_state(self, count, mean, m2, skipped=0):
        mean, m2 = (np.ascontiguousarray(a, dtype=np.float64).reshape(self.dim) for a in (mean, m2))
        _check(self.sim._L, self.sim._L.hsr_norm_set_state(self._r, float(count), mean.ctypes.data_as(_dp), m2.ctypes.data_as(_dp), int(skipped)))

    def published_dev(self, d_mean32=None, d_rstd32=None):
        """The published float32 vectors, [dim] each, into device arrays (either None)."""
        _check(self.sim._L, self.sim._L.hsr_norm_published_dev(self._r, d_mean32, d_rstd32))


class PlanSpec(C.Structure):
    """include/hsrsim.h: hsr_plan_spec."""
    _fields_ = [("seed", C.c_uint64), ("env_offset", C.c_uint32), ("groups", C.c_int32), ("samples", C.c_int32), ("horizon", C.c_int32),
                ("elites", C.c_int32), ("goal_body", C.c_int32), ("geofence", C.c_float), ("gamma", C.c_float), ("alpha", C.c_float),
                ("init_std", C.c_float), ("min_std", C.c_float)]


class Plan:
    """The CEM planner of a planning batch (include/hsrsim.h: hsr_plan) as the library exposes it: device pointers in, asynchronous on the
    batch stream.  Its storage is released by close() or by close() of its batch, whichever comes first."""

    def __init__(self, sim: BatchSim, spec: PlanSpec):
        self.sim, self.spec = sim, spec
        self._r = C.c_void_p()
        _check(sim._L, sim._L.hsr_batch_plan_create(sim._b, C.byref(spec), C.byref(self._r)))

    def close(self):
        if getattr(self, "_r", None):
            self.sim._L.hsr_plan_destroy(self._r); self._r = None

    __del__ = close

    def reset_dev(self, d_mask=None):
        """The groups with d_mask[p] != 0 (uint8 [P]; None: all): mean <- 0 clamped into the ctrl range, sigma <- init_std half_range."""
        _check(self.sim._L, self.sim._L.hsr_plan_reset_dev(self._r, d_mask))

    def shift_dev(self, d_mask=None):
        """The masked groups: mean[h] <- mean[h + 1], the last step repeats; sigma back to its initial value."""
        _check(self.sim._L, self.sim._L.hsr_plan_shift_dev(self._r, d_mask))

    def begin_dev(self):
        _check(self.sim._L, self.sim._L.hsr_plan_begin_dev(self._r))

    def sample_dev(self, call, iteration, h, d_ctrl):
        """d_ctrl float32 [N, nu]: the candidates' actions of step h, iteration `iteration` (0..255) of plan call `call`."""
        _check(self.sim._L, self.sim._L.hsr_plan_sample_dev(self._r, int(call) & 0xffffffff, int(iteration), int(h), d_ctrl))

    def accumulate_dev(self, h):
        """After step_dev of step h: the candidates' costs take the step's distance to the goal."""
        _check(self.sim._L, self.sim._L.hsr_plan_accumulate_dev(self._r, int(h)))

    def add_cost_dev(self, d_extra):
        _check(self.sim._L, self.sim._L.hsr_plan_add_cost_dev(self._r, d_extra))

    def update_dev(self):
        _check(self.sim._L, self.sim._L.hsr_plan_update_dev(self._r))

    def action_dev(self, d_ctrl):
        """d_ctrl float32 [P, nu] <- mean[p][0]."""
        _check(self.sim._L, self.sim._L.hsr_plan_action_dev(self._r, d_ctrl))

    def costs_dev(self, d_cost=None, d_reach_step=None):
        """J float32 [N] and reach_step int32 [N] into device arrays (either None)."""
        _check(self.sim._L, self.sim._L.hsr_plan_costs_dev(self._r, d_cost, d_reach_step))

    def state_dev(self, d_mean=None, d_sigma=None):
        """mean and sigma, float32 [P, H, nu] each, into device arrays (either None)."""
        _check(self.sim._L, self.sim._L.hsr_plan_state_dev(self._r, d_mean, d_sigma))

    def best_dev(self, d_index=None, d_cost=None):
        """Index int32 [P] and cost float32 [P] of every group's best candidate of the last update (either None)."""
        _check(self.sim._L, self.sim._L.hsr_plan_best_dev(self._r, d_index, d_cost))

    def failed(self):
        """Updates of every group that found no finite cost, uint32 [P]; synchronises."""
        out = np.empty(self.spec.groups, np.uint32)
        _check(self.sim._L, self.sim._L.hsr_plan_failed(self._r, out.ctypes.data_as(C.POINTER(C.c_uint32))))
        return out


def norm_apply_batch_dev(obs: Norm, goal: Norm, items, d_length=None):
    """items: (device pointer, rows, seq_len, which: 0 obs / 1 goal) of up to 8 contiguous tensors, normalised in place in one launch."""
    arr = (NormItem * len(items))(*[NormItem(int(p), int(rows), int(seq), int(which)) for p, rows, seq, which in items])
    L = (obs or goal).sim._L
    _check(L, L.hsr_norm_apply_batch_dev(obs._r if obs is not None else None, goal._r if goal is not None else None, arr, len(items), d_length))
