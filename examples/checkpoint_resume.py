"""Checkpoint a training run's environment side and resume it: FleetVecNormalize.save / .load hold the normaliser's statistics,
FleetVecEnv.save_state / .load_state the env state on the device -- running episodes, aged batteries (state of health, rainflow
and SEI state persist across episodes), start-time overrides.  The resumed pair continues exactly where the saved one stood.
    python examples/checkpoint_resume.py [--envs 256] [--evs 8]
Needs an MI355X (there is no CPU fallback)."""
import argparse
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--evs", type=int, default=8)
    args = ap.parse_args()
    from bench import bench_config
    from fleetrl_amd import FleetVecEnv, FleetVecNormalize
    from fleetrl_amd.synth import synth_tables

    E, N = args.envs, args.evs
    cfg, tables = bench_config(E, N, "ct"), synth_tables("ct", N)
    cfg["episode_length"] = 24
    rng = np.random.default_rng(0)
    acts = rng.uniform(-1, 1, size=(160, E, N)).astype(np.float32)

    vn = FleetVecNormalize(FleetVecEnv(cfg, E, tables=tables))
    vn.reset()
    for a in acts[:96]:  # one whole episode: every env has just been reset, so the discounted returns start at zero on both sides
        vn.step(a)
    with tempfile.TemporaryDirectory() as d:
        vn.save(os.path.join(d, "vecnormalize.npz"))
        vn.venv.save_state(os.path.join(d, "env_state.npz"))
        want = [vn.step(a) for a in acts[96:]]
        # ---- "another process": fresh objects from the same config ----
        env = FleetVecEnv(cfg, E, tables=tables)
        env.load_state(os.path.join(d, "env_state.npz"))
        vn2 = FleetVecNormalize.load(os.path.join(d, "vecnormalize.npz"), env)
        got = [vn2.step(a) for a in acts[96:]]
    same = all(np.array_equal(w[0], g[0]) and np.array_equal(w[1], g[1]) and np.array_equal(w[2], g[2]) for w, g in zip(want, got))
    print(f"resumed run equals the uninterrupted one over {len(want)} steps of {E} envs x {N} EVs: {same}")
    vn.close()
    vn2.close()
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
