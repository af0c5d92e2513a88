"""Env state (include/fleet_hip.h "env state") without a device: the blob layout, the fingerprint check, the .npz round trip of a
state dict and the ctypes mirrors of the two public structures."""
import ctypes
import io
import os
import subprocess

import numpy as np
import pytest

import bench
from fleetrl_amd import _capi
from fleetrl_amd.config import resolve_config
from fleetrl_amd.params import make_params, time_features
from fleetrl_amd.synth import synth_tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_TABLES = {}


def _tables(uc, n):
    if (uc, n) not in _TABLES:
        _TABLES[(uc, n)] = synth_tables(uc, n, seed=7)
    return _TABLES[(uc, n)]


def _params(uc, n_evs, envs, deg, log=False, log_capacity=None, episode_length=48):
    cfg = bench.bench_config(envs, n_evs, uc, deg=deg)
    cfg["log_data"] = log
    cfg["episode_length"] = episode_length
    tb = _tables(uc, n_evs)
    p = make_params(resolve_config(cfg), tb, envs, seed=0)
    if log_capacity is not None:
        p.log_capacity = log_capacity
    return p, tb


def _align(x):
    return (x + 255) // 256 * 256


def _expected_sections(p, obs_dim):
    """Section sizes from fleet_device.h's record sizes: Hot 16, SegRec 16, f64, f64, SeiRec 32, EnvRec 64, i32, i32, rainflow rows of
    6 header words + (episode_steps + 3) stack words rounded up to 16 words; the log ring's rows."""
    E, N, S = p.num_envs, p.num_cars, p.episode_steps
    EN = E * N
    secs = [EN * 16, EN * 16, EN * 8, EN * 8, EN * 32, E * 64, E * 4, E * 4]
    stride = (6 + S + 3 + 15) // 16 * 16
    secs.append(EN * stride * 8 if p.deg_mode == _capi.DEG_RAINFLOW else 0)
    cap = (p.log_capacity if p.log_capacity > 0 else 2 * (S + 1)) if p.log_data else 0
    secs += [E * 4 if cap else 0, cap * E * 4, cap * E * 4 * 8, cap * E * 4 * N * 8, cap * E * obs_dim * 4]
    return secs, stride, cap


SHAPES = [("lmd", 5, 256, "linear"), ("ct", 50, 4096, "rainflow"), ("ut", 50, 2048, "rainflow"), ("lmd", 200, 2731, "rainflow"),
          ("ct", 1, 3, "rainflow"), ("ct", 64, 5, "rainflow"), ("ct", 65, 5, "none"), ("ut", 257, 2, "rainflow")]


@pytest.mark.parametrize("uc,n_evs,envs,deg", SHAPES)
@pytest.mark.parametrize("log", [False, True])
def test_layout_sections_are_aligned_ordered_and_sum_to_the_record_sizes(uc, n_evs, envs, deg, log):
    p, _ = _params(uc, n_evs, envs, deg, log=log, log_capacity=37 if log and n_evs == 50 else None)
    L = _capi.state_layout(p)
    lib = _capi.load_library()
    obs_dim = lib.fleet_obs_dim(ctypes.byref(p))
    want, stride, cap = _expected_sections(p, obs_dim)
    assert L.alignment == 256 and L.struct_bytes == ctypes.sizeof(_capi.FleetStateLayout)
    assert L.header_bytes == _align(ctypes.sizeof(_capi.FleetStateHeader))
    assert (L.num_envs, L.num_cars, L.obs_dim, L.log_cap) == (envs, n_evs, obs_dim, cap)
    end = L.header_bytes
    for s, nbytes in enumerate(want):
        assert L.sec[s].bytes == nbytes, (s, _capi.STATE_SECTION_NAMES[s])
        if nbytes:
            assert L.sec[s].offset % 256 == 0
            assert L.sec[s].offset == end, "sections in order, each at the first aligned offset after the one before"
            end = _align(L.sec[s].offset + nbytes)
    for s in range(len(want), _capi.STATE_SECTIONS):
        assert L.sec[s].bytes == 0  # (the start schedule belongs to a handle, not to the parameters)
    assert L.total_bytes == end == L.header_bytes + sum(_align(b) for b in want)
    if deg == "rainflow":
        assert L.rf_row_stride == stride and L.stack_cap == p.episode_steps + 3 and L.sec[8].bytes > 0
    else:
        assert L.sec[8].bytes == 0 and L.rf_row_stride == 0, "no rainflow section without rainflow degradation"
    if not log:
        assert all(L.sec[s].bytes == 0 for s in range(9, 14)), "no log sections without the log"


def test_layout_rejects_bad_arguments():
    p, _ = _params("ct", 5, 4, "rainflow")
    lib = _capi.load_library()
    assert lib.fleet_state_layout(None, ctypes.byref(_capi.FleetStateLayout())) == _capi.ERR_INVALID
    assert lib.fleet_state_layout(ctypes.byref(p), None) == _capi.ERR_INVALID
    p.num_cars = 0
    assert lib.fleet_state_layout(ctypes.byref(p), ctypes.byref(_capi.FleetStateLayout())) == _capi.ERR_INVALID


def _header_for(p, table_hash):
    """The header a handle created from `p` writes (no start schedule), built here from the public structures."""
    L = _capi.state_layout(p)
    h = _capi.FleetStateHeader()
    h.magic = _capi.STATE_MAGIC
    h.abi_version = _capi.ABI_VERSION
    h.header_bytes = ctypes.sizeof(h)
    f = h.fp
    for name in ("num_cars", "table_rows", "episode_steps", "deg_mode", "price_lookahead", "bl_pv_lookahead", "picker_mode"):
        setattr(f, name, getattr(p, name))
    for name in ("real_time", "include_building", "include_pv", "aux", "normalize"):
        setattr(f, name, 1 if getattr(p, name) else 0)
    f.stack_cap, f.rf_row_stride, f.log_cap = L.stack_cap, L.rf_row_stride, L.log_cap
    f.seed, f.dt, f.table_hash = p.seed, p.dt, table_hash
    h.num_envs, h.env_id_offset, h.obs_dim = p.num_envs, p.env_id_offset, L.obs_dim
    h.night_hour = -1
    h.total_bytes = L.total_bytes
    for s in range(_capi.STATE_SECTIONS):
        h.sec[s].offset, h.sec[s].bytes = L.sec[s].offset, L.sec[s].bytes
    return h, L


def _blob(h, nbytes=None):
    b = np.zeros(int(h.total_bytes if nbytes is None else nbytes), dtype=np.uint8)
    raw = np.frombuffer(bytes(h), dtype=np.uint8)
    b[:min(raw.size, b.size)] = raw[:b.size]
    return b


def test_table_hash_tells_tables_apart_and_is_stable():
    p, tb = _params("ct", 5, 4, "rainflow")
    tf = time_features(tb)
    h0 = _capi.state_table_hash(p, tb, tf)
    assert h0 == _capi.state_table_hash(p, tb, tf) and h0 != 0
    p2, tb2 = _params("ut", 5, 4, "rainflow")
    assert _capi.state_table_hash(p2, tb2, time_features(tb2)) != h0
    import copy

    tb3 = copy.copy(tb)
    tb3.soc_on_return = np.array(tb.soc_on_return, copy=True)
    flat = tb3.soc_on_return.reshape(-1)
    flat[-1] = np.nextafter(flat[-1], 2.0)  # one bit of the last word
    assert _capi.state_table_hash(p, tb3, tf) != h0


def test_check_accepts_its_own_header_and_names_what_differs():
    p, tb = _params("ct", 5, 4, "rainflow")
    th = _capi.state_table_hash(p, tb, time_features(tb))
    h, L = _header_for(p, th)
    _capi.state_check(p, th, _blob(h))
    _capi.state_check(p, th, _blob(h, ctypes.sizeof(h)) if L.total_bytes <= ctypes.sizeof(h) else _blob(h))

    def rejected(params=p, table_hash=th, blob=None, match=""):
        with pytest.raises(_capi.FleetHipError) as ei:
            _capi.state_check(params, table_hash, _blob(h) if blob is None else blob)
        assert ei.value.status == _capi.ERR_INVALID
        assert match in str(ei.value), str(ei.value)

    def changed(**kw):
        q = _capi.FleetParams.from_buffer_copy(bytes(p))
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    rejected(params=changed(num_cars=6), match="num_cars")
    rejected(params=changed(table_rows=p.table_rows - 1), match="table_rows")
    rejected(params=changed(deg_mode=_capi.DEG_LINEAR), match="deg_mode")
    rejected(params=changed(episode_steps=p.episode_steps + 4), match="episode_steps")
    rejected(params=changed(num_envs=5), match="num_envs")
    rejected(table_hash=th ^ 1, match="table_hash")
    rejected(blob=_blob(h)[:int(h.total_bytes) - 1], match="shorter")
    rejected(blob=_blob(h)[:100], match="shorter")
    for field, value, match in (("abi_version", _capi.ABI_VERSION - 1, "abi_version"), ("magic", _capi.STATE_MAGIC ^ 0xFF, "magic")):
        keep = getattr(h, field)
        setattr(h, field, value)
        rejected(match=match)
        setattr(h, field, keep)
    _capi.state_check(p, th, _blob(h))  # (restored: still accepted)


def test_state_dict_npz_round_trip_is_byte_exact_and_refuses_pickles(tmp_path):
    p, tb = _params("ct", 5, 4, "rainflow", log=True, log_capacity=9)
    h, L = _header_for(p, 1234)
    blob = _blob(h)
    rng = np.random.default_rng(0)
    body = rng.integers(0, 256, size=blob.size, dtype=np.uint8)
    for s in range(_capi.STATE_SECTIONS):  # synthetic section contents; the gaps stay zero
        off, n = int(L.sec[s].offset), int(L.sec[s].bytes)
        blob[off:off + n] = body[off:off + n]
    views = _capi.state_views(blob)
    assert set(views) == {"header", "hot", "run", "soh", "soc_deg", "sei", "env", "night_start", "last_len", "rf_rows", "log_pos",
                          "log_row", "log_env", "log_ev", "log_obs"}
    assert views["hot"].shape == (4, 5) and views["rf_rows"].shape == (4, 5, L.rf_row_stride) and views["env"].shape == (4,)
    assert views["log_ev"].shape == (9, 4, 4, 5) and views["log_obs"].shape == (9, 4, L.obs_dim)
    path = tmp_path / "state.npz"
    np.savez(path, **views)
    with np.load(path, allow_pickle=False) as z:
        back = _capi.state_from_views({k: z[k] for k in z.files})
    assert back.tobytes() == blob.tobytes()
    # a file with a pickled object in it is refused by the loader the env classes use (allow_pickle=False)
    bad = tmp_path / "bad.npz"
    np.savez(bad, **{**views, "soh": np.array([{"a": 1}], dtype=object)})
    with np.load(bad, allow_pickle=False) as z:
        with pytest.raises(ValueError):
            _capi.state_from_views({k: z[k] for k in z.files})
    # ... and a section of the wrong shape or dtype by the rebuild
    with pytest.raises(_capi.FleetHipError):
        _capi.state_from_views({**views, "soh": np.zeros((4, 6))})
    with pytest.raises(_capi.FleetHipError):
        _capi.state_from_views({k: v for k, v in views.items() if k != "sei"})


def test_state_structs_match_the_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fleet_hip.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu", '
                   'sizeof(FleetStateLayout), offsetof(FleetStateLayout, total_bytes), offsetof(FleetStateLayout, log_cap), '
                   'offsetof(FleetStateLayout, sec), sizeof(FleetStateHeader), offsetof(FleetStateHeader, fp), '
                   'offsetof(FleetStateHeader, num_envs), offsetof(FleetStateHeader, total_bytes), offsetof(FleetStateHeader, sec), '
                   'sizeof(FleetStateFingerprint), offsetof(FleetStateFingerprint, table_hash));return 0;}')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    L, H, F = _capi.FleetStateLayout, _capi.FleetStateHeader, _capi.FleetStateFingerprint
    assert got == [ctypes.sizeof(L), L.total_bytes.offset, L.log_cap.offset, L.sec.offset, ctypes.sizeof(H), H.fp.offset,
                   H.num_envs.offset, H.total_bytes.offset, H.sec.offset, ctypes.sizeof(F), F.table_hash.offset]
    hdr = open(os.path.join(ROOT, "include", "fleet_hip.h")).read()
    assert f"#define FLEET_ABI_VERSION {_capi.ABI_VERSION}\n" in hdr and _capi.ABI_VERSION == 11
    assert f"0x{_capi.STATE_MAGIC:x}ull" in hdr.lower()


# ---- the fork tests' inputs, checked here before they go to the GPU ------------------------------------------------------------------
def _residue_depth(series):
    """Entries left on a rainflow stack after `series`: turning points fed through the three-point rule (a range at least as large
    as the one before it closes that one; at the start of the stack only its first point goes).  A model of the kernels' count, good
    to an entry or so: the checks below keep a margin of one."""
    rev, last = [series[0]], 0.0
    for a, b in zip(series[:-1], series[1:]):
        d = b - a
        if d == 0:
            continue
        if last * d < 0:
            rev.append(a)
        last = d
    rev.append(series[-1])
    st = []
    for x in rev:
        st.append(x)
        while len(st) >= 3 and abs(st[-1] - st[-2]) >= abs(st[-2] - st[-3]):
            if len(st) == 3:
                st.pop(0)
            else:
                top = st.pop()
                st.pop()
                st.pop()
                st.append(top)
    return len(st)


@pytest.mark.parametrize("kind", ["within-broadcast", "within-many", "across-equal", "across-one-to-many"])
def test_fork_inputs_meet_the_fork_tests_conditions_on_the_oracle(kind):
    """tests/test_state_gpu.py asserts from the device's own fields, before it forks, that the fork has something to do.  The same
    conditions on the CPU oracle, run on the same start rows and tapes up to the fork step (the oracle has no stack-size field: the
    sizes come from _residue_depth of its SOC samples, with a margin of one entry)."""
    import test_state_gpu as G
    from oracle.fleet_oracle import OracleBatch

    sc = G.fork_inputs(kind)
    tb = sc["tb"]
    deg = (np.asarray(tb.hour) == 14) & (np.asarray(tb.minute) == 45)
    side = {}
    for which in ("s", "d"):
        E = sc["E" + which]
        cpu = OracleBatch(*G._make("ct", G.FORK_N, E, "rainflow", seed=3))
        cpu.set_start_schedule(sc["starts_" + which])
        cpu.reset()
        series = [cpu.get("soc_deg").copy()]
        for k in range(G.FORK_AT):
            cpu.step(sc["tape_" + which][k])
            series.append(cpu.get("soc_deg").copy())
        series = np.array(series)
        depth = np.array([[_residue_depth(list(series[:, e, n])) for n in range(G.FORK_N)] for e in range(E)])
        side[which] = dict(depth=depth, t=cpu.get("time_idx"), start=cpu.get("start_idx"), soc=cpu.get("soc"), done=cpu.get("episodes"))
        cpu.close()
    src, dst = np.array(sc["src_idx"]), np.array(sc["dst_idx"])
    S, D = side["s"], side["d"]
    assert not S["done"].any() and not D["done"].any(), "the fork step lies inside the first episode"
    for e in np.unique(src):
        assert deg[S["start"][e]:S["t"][e]].any(), "the fork point lies after the episode's first degradation row"
    assert (S["depth"][src] >= 4).mean() >= 0.5, "at least half of the forked EVs have a stack of >= 3 entries (margin: 4)"
    for s, d in zip(src, dst):
        assert not np.array_equal(S["soc"][s], D["soc"][d]) and S["t"][s] != D["t"][d]
        assert (np.abs(S["depth"][s] - D["depth"][d]) >= 2).any(), "the two stacks differ (margin: by two entries somewhere)"
    assert (D["depth"][dst] >= S["depth"][src] + 2).any(), "a destination stack deeper than its source's"
    assert (D["depth"][dst] + 2 <= S["depth"][src]).any(), "a destination stack shallower than its source's"
