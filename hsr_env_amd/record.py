"""Video recording of chosen envs (the reference's ``record=True``: hsr/env.py:50-66,118-131 with gym's VideoRecorder), with numpy alone.

The frames come from the device: every ``record_freq`` substeps of an env-step the persistent kernel copies the recorded envs' link
poses into a capture buffer (include/hsrsim.h: hsr_batch_set_capture), and after the step one launch of the ray caster renders all of
them (hsr_batch_render_frames).  ``EnvRecorder`` turns those frames into one video per recorded env: the frames of every step in order,
then - after a step that ended in ``done`` - 50 copies of the env's final frame, as the reference's loop does (hsr/env.py:128-130).

Videos are YUV4MPEG2 (``.y4m``): uncompressed 4:4:4, BT.601 full range, 30 frames per second (gym's VideoRecorder default when
``metadata`` names no fps).  gym writes mp4 through ffmpeg; ``ffmpeg -i env0.y4m env0.mp4`` converts.  Next to each video a
``.meta.json`` lists, for every frame, its env-step index, substep, episode index and whether it is one of the trailing frames.
"""
from __future__ import annotations

import json
from pathlib import Path

import numpy as np

FPS = 30
TAIL_FRAMES = 50                          # hsr/env.py:129

# BT.601, full range (JFIF): rows Y, Cb, Cr; offsets 0, 128, 128
_RGB2YUV = np.array([[0.299, 0.587, 0.114],
                     [-0.168736, -0.331264, 0.5],
                     [0.5, -0.418688, -0.081312]])
_YUV2RGB = np.array([[1.0, 0.0, 1.402],
                     [1.0, -0.344136, -0.714136],
                     [1.0, 1.772, 0.0]])


def rgb_to_yuv(rgb: np.ndarray) -> np.ndarray:
    """uint8 [..., 3] RGB -> uint8 [..., 3] Y Cb Cr (BT.601 full range, rounded)."""
    yuv = np.asarray(rgb, np.float64) @ _RGB2YUV.T
    yuv[..., 1:] += 128.0
    return np.clip(np.rint(yuv), 0, 255).astype(np.uint8)


def yuv_to_rgb(yuv: np.ndarray) -> np.ndarray:
    """Inverse of rgb_to_yuv, up to rounding (within 2 levels per channel)."""
    y = np.asarray(yuv, np.float64).copy()
    y[..., 1:] -= 128.0
    return np.clip(np.rint(y @ _YUV2RGB.T), 0, 255).astype(np.uint8)


class VideoRecorder:
    """One YUV4MPEG2 file: ``capture_frame(rgb uint8 [H, W, 3], meta)`` appends a frame, ``close()`` finishes it and writes
    ``<path minus .y4m>.meta.json`` with the frames' meta entries (the role of gym's VideoRecorder, hsr/env.py:61-65)."""

    def __init__(self, path, width: int, height: int, fps: int = FPS):
        self.path = Path(path)
        self.meta_path = self.path.with_suffix(".meta.json")
        self.width, self.height, self.fps = int(width), int(height), int(fps)
        self._f, self.closed = None, False          # the file is created with the first frame (or by close)
        self.frames = []

    def _open(self):
        if self._f is None:
            self.path.parent.mkdir(parents=True, exist_ok=True)
            self._f = open(self.path, "wb")
            self._f.write(f"YUV4MPEG2 W{self.width} H{self.height} F{self.fps}:1 Ip A1:1 C444 XCOLORRANGE=FULL\n".encode())

    def capture_frame(self, rgb: np.ndarray, meta: dict = None):
        rgb = np.asarray(rgb)
        if rgb.shape != (self.height, self.width, 3) or rgb.dtype != np.uint8:
            raise ValueError(f"expected a uint8 frame of shape {(self.height, self.width, 3)}, got {rgb.dtype} {rgb.shape}")
        if self.closed:
            raise ValueError("capture_frame on a closed recorder")
        self._open()
        yuv = rgb_to_yuv(rgb)
        self._f.write(b"FRAME\n")
        self._f.write(np.ascontiguousarray(np.moveaxis(yuv, -1, 0)).tobytes())      # planar: Y, then Cb, then Cr
        self.frames.append(dict(meta or {}))

    def close(self):
        if self.closed:
            return
        self._open()
        self._f.close()
        self._f, self.closed = None, True
        self.meta_path.write_text(json.dumps({"width": self.width, "height": self.height, "fps": self.fps, "colorspace": "C444",
                                              "range": "full", "frames": self.frames}))


def read_y4m(path):
    """(header fields, uint8 [frames, H, W, 3] Y Cb Cr) of a file written by VideoRecorder."""
    data = Path(path).read_bytes()
    nl = data.index(b"\n")
    fields = data[:nl].decode().split()
    if fields[0] != "YUV4MPEG2":
        raise ValueError("not a YUV4MPEG2 file")
    hdr = {f[0]: f[1:] for f in fields[1:]}
    w, h = int(hdr["W"]), int(hdr["H"])
    if hdr.get("C", "420jpeg") != "444":
        raise ValueError("only C444 files are read")
    size = 3 * w * h
    frames, pos = [], nl + 1
    while pos < len(data):
        end = data.index(b"\n", pos)
        if not data[pos:end].startswith(b"FRAME"):
            raise ValueError("corrupt frame header")
        pos = end + 1
        frames.append(np.frombuffer(data[pos:pos + size], np.uint8).reshape(3, h, w).transpose(1, 2, 0))
        pos += size
    return hdr, (np.stack(frames) if frames else np.zeros((0, h, w, 3), np.uint8))


class EnvRecorder:
    """The recording side of VecHSREnv: one VideoRecorder per recorded env (global id `gid`, local index `local`, capture slot = its
    position in `local_ids`).  After every env-step, ``after_step`` renders the captured frames and appends them; ``on_reset`` counts
    episodes.  ``sim`` needs set_capture / capture_counts / render_frames (BatchSim)."""

    def __init__(self, sim, path, global_ids, local_ids, freq: int, size, camera):
        self.sim, self.freq, self.camera = sim, int(freq), camera
        self.width, self.height = (int(size), int(size)) if np.isscalar(size) else (int(size[0]), int(size[1]))
        self.global_ids, self.local_ids = list(global_ids), list(local_ids)
        self.path = path = Path(path)
        self.recorders = [VideoRecorder(path / f"env{g}.y4m", self.width, self.height) for g in self.global_ids]
        self.episode = np.zeros(len(self.local_ids), np.int64)
        self.step_index = 0
        if self.local_ids:
            sim.set_capture(self.local_ids, self.freq)

    def on_reset(self, reset_mask, stepped):
        """Envs that are reset after having stepped since their last reset start a new episode."""
        for r, e in enumerate(self.local_ids):
            if reset_mask[e] and stepped[e]:
                self.episode[r] += 1

    def after_step(self, done, nsteps):
        if self.local_ids:
            counts = self.sim.capture_counts()
            frames = self.sim.render_frames(self.width, self.height, self.camera)       # [slots, rows, H, W, 3]
            for r, e in enumerate(self.local_ids):
                meta = {"step": self.step_index, "episode": int(self.episode[r])}
                for k in range(int(counts[r])):
                    self.recorders[r].capture_frame(frames[r, k], dict(meta, substep=k * self.freq, tail=False))
                if done[e]:
                    for _ in range(TAIL_FRAMES):
                        self.recorders[r].capture_frame(frames[r, -1], dict(meta, substep=int(nsteps[e]), tail=True))
        self.step_index += 1

    def close(self):
        for rec in self.recorders:
            rec.close()


def expected_frames(nsteps: int, every: int, done: bool) -> int:
    """Frames one env-step adds to a recorded env's video."""
    n = 0 if nsteps <= 0 else (nsteps - 1) // every + 1
    return n + (TAIL_FRAMES if done else 0)
