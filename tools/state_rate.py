"""Cost of saving, loading and forking env state on the device (fleet_state.hip) at the bench workloads; prints one JSON line per
config and writes it to profiles/state_rate_<config>.json with --write.

Per config (c3; c5 = its first fleet group): medians of repeated HIP-event timings on the handle's stream of
  save_dev / load_dev   fleet_state_save_dev / fleet_state_load_dev, with the blob's bytes; beside them ONE hipMemcpyAsync device to
                        device of the same byte count in the same process (torch's copy_): the yardstick.  load_dev reads the header
                        back and synchronises, so its figure is wall time around the call.
  fork_*                fleet_fork_envs, one source broadcast to E - 1 envs and an E/2 -> E/2 map: time, the bytes the kernel moves
                        (dense records + the live part of every rainflow row, from the sources' stack depths read beforehand), the
                        bytes whole rows would be, and the device-to-device copy of the moved byte count as the yardstick
  save_host             fleet_state_save_host into a NumPy array (wall time)
  fleet_create_ms, hash_ms   FleetBatch construction from ready tables (fleet_create, median of 5) and the table hash it contains
                        (fleet_state_table_hash, host only, median of 9); create_ms: the bench group as a whole, tables and tape
                        included
  --fork-only N         nothing timed here: N forks of each kind at c3, for a `rocprofv3 --kernel-trace --stats` run around this
                        tool, which gives fleet_fork_kernel's own duration
    python tools/state_rate.py [--configs c3,c5] [--reps 9] [--write]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def event_ms(torch, stream, fn, reps):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out)), [round(v, 4) for v in out]


def wall_ms(fn, sync, reps):
    out = []
    for _ in range(reps):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out)), [round(v, 4) for v in out]


def run(torch, name, reps):
    from bench import CONFIGS, Group
    from fleetrl_amd import _capi
    from fleetrl_amd.distributed import shard_range

    spec = CONFIGS[name]
    dev = torch.device("cuda", 0)
    lo, hi = shard_range(spec["envs"], len(spec["groups"]), 0)
    E, N = hi - lo, spec["evs"]
    t0 = time.perf_counter()
    g = Group(torch, dev, spec["groups"][0], E, N, spec, 0, 0, 16, 1)
    create_ms = (time.perf_counter() - t0) * 1e3  # (tables, tape and buffers included: an upper bound of fleet_create)
    from fleetrl_amd.batch import FleetBatch

    creates = []
    for _ in range(5):  # fleet_create alone (tables already built), hash included
        t0 = time.perf_counter()
        twin = FleetBatch(g.params, g.tables, g.tf, device=dev.index)
        creates.append((time.perf_counter() - t0) * 1e3)
        twin.close()
    fleet_create_ms = float(np.median(creates))
    tc, keep = _capi.pack_tables(g.tables, g.tf)
    h = C.c_uint64()
    hashes = []
    for _ in range(9):
        t0 = time.perf_counter()
        g.batch.lib.fleet_state_table_hash(C.byref(g.params), C.byref(tc), C.byref(h))
        hashes.append((time.perf_counter() - t0) * 1e3)
    hash_ms = float(np.median(hashes))
    b = g.batch
    b.use_torch_stream(dev)
    stream = torch.cuda.current_stream(dev)
    b.reset_dev(g.obs.data_ptr())
    for i in range(120):  # past the first episode end: stacks of every depth
        b.step_dev(g.tape[i % g.L].data_ptr(), g.obs.data_ptr(), g.reward.data_ptr(), g.done.data_ptr())
    nbytes = b.state_bytes()
    blob, other = torch.empty(nbytes, dtype=torch.uint8, device=dev), torch.empty(nbytes, dtype=torch.uint8, device=dev)
    res = {"config": name, "envs": E, "evs": N, "state_bytes": nbytes, "create_ms": create_ms, "fleet_create_ms": fleet_create_ms, "hash_ms": hash_ms, "hash_share_of_create": hash_ms / fleet_create_ms, "fleet_create_runs": [round(v, 2) for v in creates],
           "hash_runs": [round(v, 3) for v in hashes], "reps": reps}
    for _ in range(3):
        b.save_state(blob)
        other.copy_(blob)
    res["save_dev_ms"], res["save_dev_runs"] = event_ms(torch, stream, lambda: b.save_state(blob), reps)
    res["memcpy_same_bytes_ms"], res["memcpy_same_bytes_runs"] = event_ms(torch, stream, lambda: other.copy_(blob), reps)
    res["load_dev_wall_ms"], res["load_dev_runs"] = wall_ms(lambda: b.load_state(blob), b.synchronize, reps)
    host = np.empty(nbytes, dtype=np.uint8)
    res["save_host_wall_ms"], res["save_host_runs"] = wall_ms(lambda: b.save_state(host), b.synchronize, max(3, reps // 3))
    hdr = _capi.state_header(host)
    res["sections"] = {n: int(hdr.sec[s].bytes) for s, n in enumerate(_capi.STATE_SECTION_NAMES) if hdr.sec[s].bytes}
    # ---- fork ----
    stack = b.get("rf_stack").astype(np.int64) if spec["deg"] == "rainflow" else np.zeros((E, N), np.int64)
    stride = int(hdr.fp.rf_row_stride)
    dense = N * (16 + 16 + 8 + 8 + 32) + 64 + 4 + 4

    def fork_bytes(src):
        live = (48 + 16 * ((np.maximum(stack[src] - 1, 0) + 1) // 2)).sum() if stride else 0
        return int(len(src) * dense + live), int(len(src) * (dense + N * stride * 8))

    for label, src, dst in (("fork_broadcast", np.zeros(E - 1, np.int32), np.arange(1, E, dtype=np.int32)),
                            ("fork_half_to_half", np.arange(E // 2, dtype=np.int32), np.arange(E // 2, 2 * (E // 2), dtype=np.int32))):
        moved, whole = fork_bytes(src)
        for _ in range(3):
            b.fork_envs(src, dst)
        # (the call reads the handle's error word back, then enqueues the index upload and the kernel: the span between the events
        # holds that 4-byte copy, the host's time between the calls, the upload and the kernel -- an upper bound of the kernel)
        ms, runs = event_ms(torch, stream, lambda: b.fork_envs(src, dst), reps)
        a, c = torch.empty(moved, dtype=torch.uint8, device=dev), torch.empty(moved, dtype=torch.uint8, device=dev)
        c.copy_(a)
        cp, _ = event_ms(torch, stream, lambda: c.copy_(a), reps)
        res[label] = {"pairs": int(len(src)), "ms": ms, "runs": runs, "bytes_moved": moved, "bytes_whole_rows": whole,
                      "live_part_saving": round(whole / moved, 2), "memcpy_moved_bytes_ms": cp}
        b.load_state(blob)
    b.close()
    return res


def fork_only(torch, n):
    """c3, stepped past an episode end, then n broadcasts and n half-to-half forks (for a kernel trace)."""
    from bench import CONFIGS, Group

    spec = CONFIGS["c3"]
    dev = torch.device("cuda", 0)
    E, N = spec["envs"], spec["evs"]
    g = Group(torch, dev, spec["groups"][0], E, N, spec, 0, 0, 16, 1)
    b = g.batch
    b.reset_dev(g.obs.data_ptr())
    for i in range(120):
        b.step_dev(g.tape[i % g.L].data_ptr(), g.obs.data_ptr(), g.reward.data_ptr(), g.done.data_ptr())
    blob = torch.empty(b.state_bytes(), dtype=torch.uint8, device=dev)
    b.save_state(blob)
    for src, dst in ((np.zeros(E - 1, np.int32), np.arange(1, E, dtype=np.int32)),
                     (np.arange(E // 2, dtype=np.int32), np.arange(E // 2, 2 * (E // 2), dtype=np.int32))):
        for _ in range(n):
            b.fork_envs(src, dst)
        b.load_state(blob)
    b.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c3,c5")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--write", action="store_true")
    ap.add_argument("--fork-only", type=int, default=0)
    args = ap.parse_args()
    import torch

    if args.fork_only:
        fork_only(torch, args.fork_only)
        return

    for name in args.configs.split(","):
        res = run(torch, name, args.reps)
        print(json.dumps(res))
        if args.write:
            os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
            with open(os.path.join(ROOT, "profiles", f"state_rate_{name}.json"), "w") as fh:
                json.dump(res, fh, indent=1)
                fh.write("\n")


if __name__ == "__main__":
    main()
