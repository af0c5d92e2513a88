"""The step kernel's instance matrix: which instances of `fleet_step_kernel` the launch planner can select (the reachable set, swept
through the library's own planner: `fleet_step_instance`, no GPU needed) and the list of test cases that covers every one of them in
every way it can be used.  tests/test_step_instances_cpu.py asserts that the list is complete, tests/test_step_instances_gpu.py runs
each case against the CPU oracle.

A case is (instance, uses): a single-step instance has one use; an instance of the K-step kernel is asked for different things by
different launches -- an action tape with K = 1 or K > 1, each built-in policy, the event-skipping loop of real_time -- and a fault in
the code of one use does not show in another.  A use is named after the launch that asks for it (`use_of`).

Adding an instance to `plan_step_gd` (fleet_step_plan.h, the host half of fleet_kernels.hip): give it a case here (a width N that selects it in `GROUP_WIDTHS` if it is a
new lane group; `cases()` derives the rest), or the CPU test fails and names it."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from fleetrl_amd import _capi

K_BLOCK = 256  # threads per workgroup (fleet_kernels.hip kBlock); the CPU test checks it against the grids the planner returns
DEGS = ("none", "linear", "rainflow")  # index = FLEET_DEG_*
POLICIES = {"uncontrolled": _capi.POLICY_UNCONTROLLED, "distributed": _capi.POLICY_DISTRIBUTED, "night": _capi.POLICY_NIGHT}
K_TAPE = 61  # steps per launch of the K > 1 uses: episode ends (96 rows) and degradation rows fall inside launches


@dataclass(frozen=True)
class Launch:
    """One launch as the planner sees it: the handle's configuration (n_evs, deg, real_time, log_data) and the call."""
    n_evs: int
    deg: int
    real_time: bool
    log_data: bool
    act_mode: int
    K: int
    has_done_count: bool

    def instance(self, num_envs: int = 7) -> tuple[str, int]:
        return _capi.step_instance(num_envs, self.n_evs, self.deg, self.real_time, self.log_data, self.act_mode, self.K,
                                   self.has_done_count)


def abi_accepts(real_time: bool, act_mode: int, K: int, has_done_count: bool) -> bool:
    """Which (configuration, call) combinations an entry point of the C ABI lets through to the planner, on a handle with auto_reset = 1
    (fleet_capi.hip, fleet_hostpath.hip, fleet_tape.hip): fleet_step_dev / fleet_step_host / the tape replays launch K = 1 without a done_count buffer, with any
    configuration; fleet_step_many_dev (an action dtype, K >= 1, done_count or not) and fleet_rollout_policy_dev (a policy, K >= 1,
    done_count or not) refuse real_time = 1.  (Both also need auto_reset = 1, which the planner does not read.)"""
    if real_time:
        return act_mode in (_capi.ACT_F32, _capi.ACT_F64) and K == 1 and not has_done_count
    return True


def use_of(launch: Launch) -> str:
    """What a launch asks of the instance it gets."""
    if launch.real_time:
        return "rt"
    for name, pol in POLICIES.items():
        if launch.act_mode == pol:
            return name
    if launch.K > 1:
        return "tape"
    if launch.has_done_count:
        return "tape1"
    return "f64" if launch.act_mode == _capi.ACT_F64 else "f32"


def reachable() -> dict[str, set[str]]:
    """instance name -> the uses it can be asked for: every combination the C ABI accepts, over all widths up to past the point where
    the planner stops distinguishing them."""
    out: dict[str, set[str]] = {}
    n_max = 2 * int(_capi.load_library().fleet_max_evs_per_lane_group()) + 1
    for n in range(1, n_max + 1):
        for deg in range(3):
            for rt in (False, True):
                for log in (False, True):
                    for act_mode in (_capi.ACT_F32, _capi.ACT_F64, *POLICIES.values()):
                        for K in (1, 2):
                            for hdc in (False, True):
                                if not abi_accepts(rt, act_mode, K, hdc):
                                    continue
                                ln = Launch(n, deg, rt, log, act_mode, K, hdc)
                                out.setdefault(ln.instance()[0], set()).add(use_of(ln))
    return out


@dataclass(frozen=True)
class Case:
    instance: str          # the instance every launch of `uses` must take
    uses: tuple            # use names (`use_of`); several only for the data-log instances, whose checks share one log
    lanes: int             # lanes per env of the instance (its G); envs per workgroup = K_BLOCK / lanes
    n_evs: int
    num_envs: int
    uc: str                # "lmd" | "ct" | "ut"
    deg: str
    real_time: bool
    log_data: bool
    norm: bool
    aux: bool
    building: bool
    pv: bool
    f64: bool              # dtype of the action buffers where the use does not fix it (tape, tape1, rt)
    seed: int

    @property
    def id(self) -> str:
        sw = "".join(c for c, on in zip("nabpd", (self.norm, self.aux, self.building, self.pv, self.f64)) if on)
        return f"{self.instance}-{'+'.join(self.uses)}-N{self.n_evs}xE{self.num_envs}-{self.uc}-{sw or '0'}"

    def policy_chunks(self) -> tuple:
        """Steps per launch of a policy rollout: the per-env window state of the night rule has to survive launch boundaries and
        episode resets.  (A data-log case runs all three policies and everything else on one handle: shorter.)"""
        return (1, 40) if self.log_data else (1, 100, 7, 150)

    def launches(self) -> list[Launch]:
        """The launches the GPU test issues for this case's uses (the hand-over single steps after a tape are another instance's)."""
        deg = DEGS.index(self.deg)
        dt = _capi.ACT_F64 if self.f64 else _capi.ACT_F32
        out = []
        for use in self.uses:
            if use == "rt":
                out.append(Launch(self.n_evs, deg, True, self.log_data, dt, 1, False))
            elif use in POLICIES:  # chunks of K = 1 and K > 1, always with a done_count buffer
                out += [Launch(self.n_evs, deg, False, self.log_data, POLICIES[use], K, True) for K in self.policy_chunks()]
            elif use == "tape":
                out.append(Launch(self.n_evs, deg, False, self.log_data, dt, K_TAPE, True))
            elif use == "tape1":
                out.append(Launch(self.n_evs, deg, False, self.log_data, dt, 1, True))
            else:
                out.append(Launch(self.n_evs, deg, False, self.log_data, _capi.ACT_F64 if use == "f64" else _capi.ACT_F32, 1, False))
        return out


# Widths per lane group: first one that leaves surplus lanes where the group allows it (N = 1 and N = 2 fill theirs), then -- for the
# groups of one wavefront and more -- the exact power of two.  "64w": one wavefront whose lanes walk several EVs each; 70 EVs get there
# only with real_time or the data log (and then still carry their schedule records for a single-step launch to follow).
GROUP_WIDTHS = {"1": (1,), "2": (2,), "4": (3,), "8": (7,), "16": (13,), "32": (31,), "64": (50, 64), "128": (100, 128),
                "256": (130, 256), "64w": (257, 70)}
# big tables are slow to draw: one fleet type per width from 100 EVs on
_UC_OF_BIG = {70: "lmd", 100: "ct", 128: "lmd", 130: "ct", 256: "ut", 257: "ct"}


def _group_of(instance: str) -> str:
    return instance.split(".")[0][1:]


def cases() -> list[Case]:
    """Deterministic: every (instance, use) the planner can reach at the widths of GROUP_WIDTHS, the run-time switches (normalisation,
    auxiliary observations, building load, PV, action dtype, fleet type) rotated over the cases with a fixed seed.  The one combination
    the reference crashes in (normalise + PV without building load) is left out."""
    rng = np.random.default_rng(20260)
    out: list[Case] = []
    seen = set()
    for group, widths in GROUP_WIDTHS.items():
        lanes = int(group.rstrip("w"))
        epb = K_BLOCK // lanes
        for n in widths:
            for deg in range(3):
                found: dict[tuple, list] = {}  # (instance, real_time, log_data) -> uses, in sweep order
                for rt in (False, True):
                    for log in (False, True):
                        for act_mode in (_capi.ACT_F32, _capi.ACT_F64, *POLICIES.values()):
                            for K in (1, 2):
                                for hdc in (False, True):
                                    if not abi_accepts(rt, act_mode, K, hdc):
                                        continue
                                    ln = Launch(n, deg, rt, log, act_mode, K, hdc)
                                    name = ln.instance()[0]
                                    if _group_of(name) != group:
                                        continue  # (70 EVs without real_time / log: the G = 128 instances, which have their widths)
                                    uses = found.setdefault((name, rt, log), [])
                                    if use_of(ln) not in uses:
                                        uses.append(use_of(ln))
                for (name, rt, log), uses in found.items():
                    # the data log is one ring per handle: its uses share a case (one log to check); everything else one use a case
                    for us in ([tuple(uses)] if log else [(u,) for u in uses]):
                        if (name, us, n) in seen:
                            continue
                        seen.add((name, us, n))
                        while True:
                            norm, aux, building, pv = (bool(rng.integers(2)) for _ in range(4))
                            if not (norm and pv and not building):
                                break
                        f64 = bool(rng.integers(2))
                        uc = _UC_OF_BIG.get(n) or ("lmd", "ct", "ut")[int(rng.integers(3))]
                        # whole workgroups and a partly filled last one (where one workgroup holds several envs)
                        k = 2 + int(rng.integers(2))
                        E = epb * k + 1 + int(rng.integers(epb - 1)) if epb > 1 else 3 + int(rng.integers(3))
                        out.append(Case(name, us, lanes, n, E, uc, DEGS[deg], rt, log, norm, aux, building, pv, f64,
                                        seed=len(out)))
    return out


def config_of(case: Case) -> dict:
    """The reference-style config dict of a case (24 h episodes, random start picker), as tests/test_hip_shapes.py writes them."""
    return {
        "data_path": "<synthetic>", "use_case": case.uc, "building_name": None, "price_name": None, "tariff_name": None,
        "schedule_name": None, "pv_name": None, "seed": 0, "include_building": case.building, "include_pv": case.pv,
        "include_price": True, "time_picker": "random", "max_batt_cap_in_all_use_cases": 60, "init_soh": 1.0,
        "log_data": case.log_data, "deg_emp": case.deg == "linear", "calculate_degradation": case.deg != "none", "verbose": 0,
        "normalize_in_env": case.norm, "aux": case.aux, "ignore_price_reward": False, "ignore_overloading_penalty": False,
        "ignore_invalid_penalty": False, "ignore_overcharging_penalty": False, "gen_schedule": False,
        "gen_start_date": None, "gen_end_date": None, "gen_name": None, "gen_n_evs": 1, "spot_markup": None,
        "spot_mul": None, "feed_in_ded": None, "real_time": case.real_time, "episode_length": 24, "target_soc": 0.85,
    }
