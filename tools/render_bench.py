"""Time hsr_batch_render_dev (RGB + depth, default camera) with device events after warm-up and print one JSON line.

    python tools/render_bench.py [--config cfg3] [--envs 8192] [--sizes 64 128] [--min-seconds 0.5]

Per size: renders are timed in a window of at least --min-seconds of GPU work (events on the batch stream); reported are ms per render,
Mrays/s (one ray per pixel) and the bytes one render writes (3 B of RGB + 4 B of depth per pixel).  The state rendered is that of a
reset plus two env-steps of random actions.
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg3")
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--min-seconds", type=float, default=0.5)
    a = ap.parse_args()
    import torch
    from hsr_env_amd.compiler import load_config
    from hsr_env_amd.sim import BatchSim
    m = load_config(a.config)
    n = a.envs
    sim = BatchSim(m, n)
    rng = np.random.default_rng(0)
    sim.reset()
    for _ in range(2):
        sim.step(rng.uniform(m.act_ctrlrange[:, 0], m.act_ctrlrange[:, 1], (n, m.nu)), 20)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.ExternalStream(sim.stream_ptr(), device=dev)
    res = {"config": a.config, "envs": n, "sizes": {}}
    for sz in a.sizes:
        rgb = torch.empty((n, sz, sz, 3), dtype=torch.uint8, device=dev)
        depth = torch.empty((n, sz, sz), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        for _ in range(3):                                          # warm-up: code object, plane tables, palette
            sim.render_dev(sz, sz, None, rgb=rgb, depth=depth)
        sim.sync()
        reps, ms = 1, 0.0
        while True:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(reps):
                sim.render_dev(sz, sz, None, rgb=rgb, depth=depth)
            e1.record(stream)
            e1.synchronize()
            ms = e0.elapsed_time(e1)
            if ms >= 1e3 * a.min_seconds:
                break
            reps = max(reps * 2, int(reps * 1.2e3 * a.min_seconds / max(ms, 1e-3)))
        per = ms / reps
        rays = n * sz * sz
        res["sizes"][str(sz)] = {"ms_per_render": round(per, 4), "renders_timed": reps, "window_ms": round(ms, 1),
                                 "mrays_per_s": round(rays / per / 1e3, 1), "bytes_written": rays * 7,
                                 "write_GBps": round(rays * 7 / per / 1e6, 1)}
        assert torch.isfinite(depth).all()
    sim.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
