"""The device policy without a GPU: the C ABI's declarations and bindings, the refusals fleet_policy_create makes before it touches
the device, the state-dict loaders and the archive reader, the weight fixture, the float64 model of tests/policy_model.py against
torch-CPU float32, and the episode bookkeeping of evaluate_policy against SB3's loop on a scripted env."""
import ctypes as C
import os
import re
import subprocess
import zipfile

import numpy as np
import pytest

import policy_model as pm

ROOT = pm.ROOT
ENTRIES = ("fleet_policy_create", "fleet_policy_destroy", "fleet_policy_last_error", "fleet_policy_set_stream", "fleet_policy_load_host",
           "fleet_policy_load_dev", "fleet_policy_forward_dev", "fleet_policy_describe")


def tile_rows() -> int:
    src = open(os.path.join(ROOT, "fleetrl_amd", "csrc", "fleet_policy.h")).read()
    return int(re.search(r"constexpr int kPolicyRows = (\d+);", src).group(1))


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_header_section_is_placed_after_the_replay_section_and_every_entry_is_bound():
    from fleetrl_amd import _capi

    hdr = open(os.path.join(ROOT, "include", "fleet_hip.h")).read()
    assert re.search(r"^#define FLEET_ABI_VERSION 11$", hdr, flags=re.M) and _capi.ABI_VERSION == 11
    declared = set(re.findall(r"^(?:int|const char\*)\s+(fleet_policy_\w+)\s*\(", hdr, flags=re.M))
    assert declared == set(ENTRIES) == set(_capi.POLICY_SYMBOLS)
    assert hdr.index("replay buffer on the device") < hdr.index("MLP policy on the device")
    section = hdr[hdr.index("MLP policy on the device"):]
    assert "entries added under FLEET_ABI_VERSION 11: nothing that existed before changes, so the number stays" in section[:400]
    assert "} FleetPolicyParams;" in section and "} FleetPolicyHead;" in section
    assert "typedef struct FleetPolicy* fleet_policy_handle;" in section
    lib = _capi.load_library()
    for name in ENTRIES:
        fn = getattr(lib, name)
        assert fn.argtypes is not None, name
        assert fn.restype is (C.c_char_p if name == "fleet_policy_last_error" else C.c_int), name
    assert set(ENTRIES) <= set(_capi.EXPORTED_SYMBOLS)
    for name, value in (("MAX_HEADS", _capi.POLICY_MAX_HEADS), ("MAX_LAYERS", _capi.POLICY_MAX_LAYERS), ("MAX_WIDTH", _capi.POLICY_MAX_WIDTH),
                        ("MAX_OBS_DIM", _capi.POLICY_MAX_OBS_DIM), ("ACT_TANH", _capi.POLICY_ACT_TANH), ("ACT_RELU", _capi.POLICY_ACT_RELU),
                        ("OUT_NONE", _capi.POLICY_OUT_NONE), ("OUT_CLIP", _capi.POLICY_OUT_CLIP), ("OUT_TANH", _capi.POLICY_OUT_TANH)):
        assert re.search(rf"^#define FLEET_POLICY_{name} {value}$", hdr, flags=re.M), name
    assert (_capi.POLICY_MAX_LAYERS, _capi.POLICY_MAX_WIDTH, _capi.POLICY_MAX_OBS_DIM) == (4, 512, 8192)


def test_struct_sizes_and_offsets_match_the_header(tmp_path):
    from fleetrl_amd import _capi

    exprs, want = [], []
    for cname, cls in (("FleetPolicyHead", _capi.FleetPolicyHead), ("FleetPolicyParams", _capi.FleetPolicyParams)):
        exprs.append(f"sizeof({cname})")
        want.append(C.sizeof(cls))
        for n, _ in cls._fields_:
            exprs.append(f"offsetof({cname}, {n})")
            want.append(getattr(cls, n).offset)
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fleet_hip.h"\nint main(){' +
                   "".join(f'printf("%zu ", (size_t){e});' for e in exprs) + "return 0;}")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == want
    assert [n for n, _ in _capi.FleetPolicyParams._fields_] == ["struct_bytes", "obs_dim", "n_heads", "tile_rows", "head"]


def _params(obs_dim=5, heads=((7, 2),), **over):
    from fleetrl_amd import _capi

    p = _capi.FleetPolicyParams()
    p.struct_bytes, p.obs_dim, p.n_heads = C.sizeof(_capi.FleetPolicyParams), obs_dim, len(heads)
    for h, widths in enumerate(heads[:2]):
        p.head[h].n_layers = len(widths)
        for l, w in enumerate(widths[:4]):
            p.head[h].width[l] = w
        p.head[h].output = _capi.POLICY_OUT_CLIP
        p.head[h].lo, p.head[h].hi = -1.0, 1.0
    for k, v in over.items():
        if k.startswith("head0_"):
            setattr(p.head[0], k[6:], v)
        else:
            setattr(p, k, v)
    return p


@pytest.mark.parametrize("bad,word", [(dict(obs_dim=0), "obs_dim"), (dict(obs_dim=8193), "obs_dim"), (dict(heads=((513, 2),)), "width"),
                                      (dict(heads=((7, 0),)), "width"), (dict(head0_n_layers=5), "n_layers"),
                                      (dict(head0_n_layers=0), "n_layers"), (dict(n_heads=3), "n_heads"), (dict(n_heads=0), "n_heads"),
                                      (dict(struct_bytes=8), "struct_bytes"), (dict(head0_activation=2), "activation"),
                                      (dict(head0_output=3), "output"), (dict(head0_lo=2.0), "lo <= hi"),
                                      (dict(head0_hi=float("nan")), "lo <= hi")])
def test_create_refuses_bad_parameters_before_it_touches_the_device(bad, word):
    from fleetrl_amd import _capi

    lib = _capi.load_library()
    weights = np.zeros(1 << 16, np.float32)
    h = C.c_void_p(0xdead)
    assert lib.fleet_policy_create(0, C.byref(_params(**bad)), weights.ctypes.data, C.byref(h)) == _capi.ERR_INVALID
    assert h.value is None
    assert word in lib.fleet_policy_last_error(None).decode()


def test_create_refuses_null_pointers_and_weights_that_are_not_finite():
    from fleetrl_amd import _capi

    lib = _capi.load_library()
    h = C.c_void_p()
    weights = np.zeros(5 * 7 + 7 + 7 * 2 + 2, np.float32)
    assert lib.fleet_policy_create(0, None, weights.ctypes.data, C.byref(h)) == _capi.ERR_INVALID
    assert "null" in lib.fleet_policy_last_error(None).decode()
    assert lib.fleet_policy_create(0, C.byref(_params()), None, C.byref(h)) == _capi.ERR_INVALID
    assert "null" in lib.fleet_policy_last_error(None).decode()
    assert lib.fleet_policy_create(0, C.byref(_params()), weights.ctypes.data, None) == _capi.ERR_INVALID
    for at, what in ((3, "head 0, layer 0: weight 3"), (5 * 7 + 6, "head 0, layer 0: bias 6"), (5 * 7 + 7 + 13, "head 0, layer 1: weight 13")):
        for bad in (np.nan, np.inf, -np.inf):
            w = weights.copy()
            w[at] = bad
            assert lib.fleet_policy_create(0, C.byref(_params()), w.ctypes.data, C.byref(h)) == _capi.ERR_INVALID
            assert what in lib.fleet_policy_last_error(None).decode() and h.value is None
    assert lib.fleet_policy_destroy(None) == _capi.OK and lib.fleet_policy_forward_dev(None, None, 1, None, None, None) == _capi.ERR_INVALID


def test_python_class_refuses_what_the_library_refuses_and_malformed_layers():
    from fleetrl_amd import DevicePolicy, FleetHipError, _capi

    rng = np.random.default_rng(0)
    with pytest.raises(FleetHipError) as ei:
        DevicePolicy(pm.random_layers(rng, (5, 513, 2)))
    assert ei.value.status == _capi.ERR_INVALID and "width" in str(ei.value) and "513" in str(ei.value)
    with pytest.raises(FleetHipError) as ei:
        DevicePolicy(pm.random_layers(rng, (5, 4, 4, 4, 4, 2)))
    assert ei.value.status == _capi.ERR_INVALID and "n_layers" in str(ei.value)
    layers = pm.random_layers(rng, (5, 4, 2))
    layers[1][0][1, 2] = np.nan
    with pytest.raises(FleetHipError) as ei:
        DevicePolicy(layers)
    assert ei.value.status == _capi.ERR_INVALID and "not finite" in str(ei.value)
    with pytest.raises(ValueError):
        DevicePolicy(pm.random_layers(rng, (5, 4)) + pm.random_layers(rng, (3, 2)))  # the chain does not fit
    with pytest.raises(ValueError):
        DevicePolicy(pm.random_layers(rng, (5, 4)), activation="gelu")
    with pytest.raises(ValueError):
        DevicePolicy(pm.random_layers(rng, (5, 4)), output="softmax")


# ---- the loaders -----------------------------------------------------------------------------------------------------------------
def _same(layers, want):
    return len(layers) == len(want) and all(np.array_equal(np.asarray(w), ww) and np.array_equal(np.asarray(b), wb)
                                            for (w, b), (ww, wb) in zip(layers, want))


def test_state_dicts_of_the_three_families_are_recognised():
    from fleetrl_amd.policy import parse_state_dict

    rng = np.random.default_rng(1)
    actor, critic, qf = pm.random_layers(rng, (9, 6, 7, 3)), pm.random_layers(rng, (9, 5, 4, 1)), pm.random_layers(rng, (12, 8, 1))
    got = parse_state_dict(pm.ppo_state_dict(actor, critic))
    assert _same(got["layers"], actor) and _same(got["critic_layers"], critic) and (got["activation"], got["output"]) == ("tanh", "clip")
    assert parse_state_dict(pm.ppo_state_dict(actor, critic), "relu")["activation"] == "relu"
    got = parse_state_dict(pm.td3_state_dict(actor, qf))
    assert _same(got["layers"], actor) and got["critic_layers"] is None and (got["activation"], got["output"]) == ("relu", "tanh")
    got = parse_state_dict(pm.sac_state_dict(actor, qf))
    assert _same(got["layers"], actor) and got["critic_layers"] is None and (got["activation"], got["output"]) == ("relu", "tanh")
    # torch tensors as well as arrays
    import torch

    got = parse_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in pm.td3_state_dict(actor, qf).items()})
    assert [tuple(w.shape) for w, _ in got["layers"]] == [(6, 9), (7, 6), (3, 7)]


@pytest.mark.parametrize("key,shape", [("mlp_extractor.shared_net.0.weight", (4, 9)), ("features_extractor.cnn.0.weight", (8, 3, 3, 3)),
                                       ("pi_features_extractor.extractors.vec.1.weight", (4, 9)), ("log_std", (6, 3)),
                                       ("actor.features_extractor.linear.0.weight", (4, 9)), ("lstm_actor.weight_ih_l0", (8, 9)),
                                       ("q_net.q_net.0.weight", (4, 9))])
def test_everything_else_is_refused_with_the_offending_key(key, shape):
    from fleetrl_amd.policy import parse_state_dict

    rng = np.random.default_rng(2)
    sd = pm.ppo_state_dict(pm.random_layers(rng, (9, 6, 3)), pm.random_layers(rng, (9, 5, 1)))
    if key.startswith(("actor.", "q_net.")):
        sd = pm.td3_state_dict(pm.random_layers(rng, (9, 6, 3)), pm.random_layers(rng, (12, 8, 1))) if key.startswith("actor.") else {}
    sd[key] = np.zeros(shape, np.float32)
    with pytest.raises(ValueError) as ei:
        parse_state_dict(sd)
    assert repr(key) in str(ei.value)


def test_export_and_archive_reader_round_trip_on_a_zip_written_here(tmp_path):
    import sys

    import torch

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import export_sb3_policy

    from fleetrl_amd.policy import parse_state_dict, read_sb3_state_dict

    rng = np.random.default_rng(3)
    actor, critic = pm.random_layers(rng, (11, 6, 7, 2)), pm.random_layers(rng, (11, 5, 4, 1))
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in pm.ppo_state_dict(actor, critic).items()}
    pth = tmp_path / "policy.pth"
    torch.save(sd, pth)
    path = tmp_path / "model.zip"
    with zipfile.ZipFile(path, "w") as zf:
        zf.write(pth, "policy.pth")
        zf.writestr("data", "{}")
        zf.writestr("_stable_baselines3_version", "2.3.2")
    got = read_sb3_state_dict(path)
    assert list(got) == list(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    out = tmp_path / "weights.npz"
    export_sb3_policy.export(path, out)
    with np.load(out) as z:
        assert sorted(z.files) == sorted(sd) and all(z[k].dtype == np.float32 and np.array_equal(z[k], sd[k].numpy()) for k in sd)
        parsed = parse_state_dict({k: z[k] for k in z.files})
    assert _same(parsed["layers"], actor) and _same(parsed["critic_layers"], critic)
    with zipfile.ZipFile(tmp_path / "empty.zip", "w") as zf:
        zf.writestr("data", "{}")
    with pytest.raises(ValueError):
        read_sb3_state_dict(tmp_path / "empty.zip")


def test_fixture_holds_the_shipped_agents_weights_and_nothing_else():
    from fleetrl_amd.policy import parse_state_dict

    z = pm.fixture_arrays()
    assert os.path.getsize(pm.FIXTURE) < 100 * 1024
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in z.values())
    got = parse_state_dict(z)
    assert [w.shape for w, _ in got["layers"]] == [(64, 45), (64, 64), (1, 64)]
    assert [w.shape for w, _ in got["critic_layers"]] == [(64, 45), (64, 64), (1, 64)]
    assert (got["activation"], got["output"]) == ("tanh", "clip") and z["log_std"].shape == (1,)


# ---- the model -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(pm.NETWORKS))
def test_model_agrees_with_torch_cpu_float32_on_every_gpu_case(name):
    """The float64 model against the arithmetic SB3 would run.  Bound 1e-4: two orders above the float32 chain's measured distance
    (2e-7 .. 2e-6, printed), one below the worst-case n * u bound (1e-3 and up at these widths), three below what a misplaced
    weight does (1e-1)."""
    worst = 0.0
    for E in pm.batch_sizes(tile_rows()):
        for y64, eps_ref in pm.reference(name, E):
            assert y64.shape[0] == E and np.isfinite(y64).all()
            worst = max(worst, eps_ref)
    print(f"{name}: eps_ref {worst:.3g}")
    assert worst <= 1e-4
    sizes, _, output = pm.NETWORKS[name]
    assert pm.reference(name, 1)[0][0].shape == (1, sizes[-1])
    if output in ("clip", "tanh"):
        assert np.abs(pm.reference(name, 16 * tile_rows() + 1)[0][0]).max() <= 1.0


def test_model_known_answers():
    x = np.array([[1.0, -2.0]], np.float32)
    layers = [(np.array([[0.5, 0.25], [1.0, 1.0]], np.float32), np.array([0.0, 0.5], np.float32)), (np.array([[2.0, -4.0]], np.float32), np.array([0.25], np.float32))]
    assert pm.forward64(layers, x, "relu", "none").tolist() == [[0.25]]  # hidden (0, -0.5) -> (0, 0)
    assert pm.forward64(layers[:1], x, "relu", "clip", -0.25, 0.25).tolist() == [[0.0, -0.25]]
    assert np.allclose(pm.forward64(layers, x, "tanh", "tanh"), np.tanh(2 * np.tanh(0.0) - 4 * np.tanh(-0.5) + 0.25))
    # the normaliser's expression: mean 1, var 4 - eps, clip 1.5
    got = pm.norm_obs32(np.array([5.0, 2.0, -9.0], np.float32), 1.0, 4.0 - 1e-8, 1.5, 1e-8)
    assert got.dtype == np.float32 and got.tolist() == [1.5, 0.5, -1.5]
    assert pm.batch_sizes(16) == [1, 2, 15, 16, 17, 63, 64, 65, 257]


# ---- evaluate_policy's bookkeeping ----------------------------------------------------------------------------------------------
class ScriptedEnv:
    """E envs whose episode lengths and rewards follow a script: env i ends its j-th episode after lengths[i][j % len] steps; the
    reward of env i at its global step t is a float64 that float32 cannot hold.  The same script behind SB3's host protocol and
    behind the torch protocol evaluate_policy drives (on CPU tensors)."""
    device = "cpu"

    def __init__(self, lengths, episode_steps):
        self.lengths, self.num_envs, self.episode_steps = lengths, len(lengths), episode_steps
        self.steps = 0

    def _reset(self):
        self.t = np.zeros(self.num_envs, dtype=int)
        self.k = np.zeros(self.num_envs, dtype=int)
        self.n = 0
        return np.zeros((self.num_envs, 2), np.float32)

    def _step(self, actions):
        assert np.array_equal(np.asarray(actions), np.full((self.num_envs, 1), 0.5, np.float32))
        self.n += 1
        self.steps += 1
        self.t += 1
        rew = (np.arange(self.num_envs) + 1) / 3.0 + self.n / 7.0
        done = np.array([self.t[i] == self.lengths[i][self.k[i] % len(self.lengths[i])] for i in range(self.num_envs)])
        self.k += done
        self.t[done] = 0
        return np.full((self.num_envs, 2), self.n, np.float32), rew, done

    def reset(self):
        return self._reset()

    def step(self, actions):
        obs, rew, done = self._step(actions)
        return obs, rew, done, [{} for _ in range(self.num_envs)]

    def reset_torch(self, obs_out):
        import torch

        obs_out.copy_(torch.from_numpy(self._reset()))

    def step_torch(self, actions, obs_out, reward_out, done_out):
        import torch

        obs, rew, done = self._step(actions.numpy())
        obs_out.copy_(torch.from_numpy(obs)), reward_out.copy_(torch.from_numpy(rew)), done_out.copy_(torch.from_numpy(done.astype(np.uint8)))


class ConstantPolicy:
    obs_dim, act_dim = 2, 1

    def predict(self, observation, state=None, episode_start=None, deterministic=True):
        return np.full((len(observation), 1), 0.5, np.float32), None

    def act(self, obs, out=None):
        out.fill_(0.5)
        return out


@pytest.mark.parametrize("lengths,block,n_eval", [
    ([[4], [4], [4]], 4, 3), ([[4], [4], [4]], 4, 7), ([[4], [4], [4]], 4, 2),          # even, ragged quotas, fewer episodes than envs
    ([[3, 5], [2], [7, 1, 1], [4]], 4, 9), ([[3, 5], [2], [7, 1, 1], [4]], 6, 1),         # episodes that end anywhere in a block
    ([[1]], 5, 4), ([[6], [5]], 3, 5)])
def test_evaluate_policy_keeps_sb3s_books(lengths, block, n_eval):
    from fleetrl_amd.policy import evaluate_policy

    host, dev = ScriptedEnv(lengths, block), ScriptedEnv(lengths, block)
    want_r, want_l = pm.sb3_evaluate_policy(ConstantPolicy(), host, n_eval_episodes=n_eval, return_episode_rewards=True)
    got_r, got_l = evaluate_policy(ConstantPolicy(), dev, n_eval_episodes=n_eval, return_episode_rewards=True)
    assert len(want_r) == n_eval
    assert got_l == [int(v) for v in want_l]
    assert np.array_equal(np.array(got_r).view(np.uint64), np.array(want_r, dtype=np.float64).view(np.uint64))  # count, order, bits
    assert host.steps <= dev.steps < host.steps + block and dev.steps % block == 0
    if all(len(set(ls)) == 1 and ls[0] == block for ls in lengths):
        assert dev.steps == host.steps  # episodes that end on the block's boundary: the loop ends where SB3's does
    mean, std = evaluate_policy(ConstantPolicy(), ScriptedEnv(lengths, block), n_eval_episodes=n_eval)
    assert (mean, std) == (float(np.mean(want_r)), float(np.std(want_r)))
    with pytest.raises(NotImplementedError):
        evaluate_policy(ConstantPolicy(), ScriptedEnv(lengths, block), deterministic=False)
