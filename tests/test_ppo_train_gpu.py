"""PPO's whole update on the device (fleet_train.hip): the shuffle against tests/train_model.py bit for bit, the one call against the
existing pieces run step by step (model indices, DeviceRolloutBuffer.gather, the model's normalisation, DevicePPOGrad.grad,
DeviceAdam.step) bit for bit, the statistics block, what a result may not depend on, and the refusals that need handles."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import policy_bits as pb
import train_model as tm

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F32 = np.float32
CLIP, VF, ENT, LR, EPS, MAXN = 0.2, 0.5, 0.01, 3e-3, 1e-5, 0.5
SEED = 0x1234567890ABCDEF  # (both key words in use)


def dev():
    return torch.device("cuda", 0)


def on_device(a):
    return torch.from_numpy(np.array(a)).to(dev())


def host(t):
    return t.detach().cpu().numpy().copy()


def same64(a, b) -> bool:
    """Bit equality of float64 values (the statistics block)."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


# name -> (D, hidden widths, A, E, K, activation)
SHAPES = {
    "5-8-8-3": (5, (8, 8), 3, 3, 5, "tanh"),
    "5-8-8-3-relu": (5, (8, 8), 3, 3, 5, "relu"),
    "8-8-8-4": (8, (8, 8), 4, 5, 13, "tanh"),  # D and A multiples of 4: rows move as 16-byte words
    "5-8-3-long": (5, (8,), 3, 3, 700, "tanh"),  # n = 2100: minibatches above 256 lanes and above the 2048 cached rows
}


def weights(shape):
    D, hidden, A, _, _, _ = SHAPES[shape]
    rng = np.random.default_rng(len(shape) + D)
    nets = []
    for out in (A, 1):
        sizes, net = (D, *hidden, out), []
        for i, o in zip(sizes[:-1], sizes[1:]):
            net.append(((rng.standard_normal((o, i)) / np.sqrt(i)).astype(F32), (0.1 * rng.standard_normal(o)).astype(F32)))
        nets.append(net)
    return nets[0], nets[1], (-0.5 + 0.1 * rng.standard_normal(A)).astype(F32)


class Rig:
    """A policy, its torch parameters, a full rollout buffer and the three handles on them, identically initialised per shape."""

    def __init__(self, shape, max_batch, train=True):
        from fleetrl_amd import DeviceAdam, DevicePolicy, DevicePPOGrad, DevicePPOTrain, DeviceRolloutBuffer

        D, _, A, E, K, act = SHAPES[shape]
        actor, critic, log_std = weights(shape)
        self.shape, self.n, self.E, self.K, self.D, self.A = shape, E * K, E, K, D, A
        self.pol = DevicePolicy(actor, critic_layers=critic, activation=act, output="clip")
        self.params = [torch.nn.Parameter(on_device(t)) for net in (actor, critic) for w, b in net for t in (w, b)] + [torch.nn.Parameter(on_device(log_std))]
        self.buf = DeviceRolloutBuffer(E, K, D, A)
        rng = np.random.default_rng(E * K)
        self.buf.observations.copy_(on_device(rng.standard_normal((K, E, D)).astype(F32)))
        for t in range(K):  # actions, values and log-probabilities as a rollout under these weights leaves them
            row = self.buf.slot(t)
            self.pol.sample(row.obs, self.params[-1], seed=5, step=t, actions_out=row.actions, log_prob_out=row.log_prob, values_out=row.value)
        adv = (rng.standard_normal((K, E)) * 2.0 + 0.3).astype(F32)
        self.buf.advantages.copy_(on_device(adv))
        self.buf.returns.copy_(self.buf.values + on_device(adv))
        self.buf.pos, self.buf.full = K, True
        self.grad = DevicePPOGrad(self.pol, max_batch)
        self.adam = DeviceAdam(self.pol, self.params, lr=LR, eps=EPS, max_grad_norm=MAXN)
        self.train = DevicePPOTrain(self.buf, self.grad, self.adam) if train else None
        torch.cuda.synchronize()

    def state(self, stats=None):
        """Everything an update leaves, as host arrays."""
        sd = self.adam.state_dict()["state"]
        out = {"params": [host(p) for p in self.params], "image": [host(t) for t in self.adam.export_image()],
               "exp_avg": [host(sd[i]["exp_avg"]) for i in range(len(sd))], "exp_avg_sq": [host(sd[i]["exp_avg_sq"]) for i in range(len(sd))],
               "step": self.adam.describe()["step"]}
        if stats is not None:
            out["stats"] = host(stats)
        return out

    def one_call(self, *, n_epochs=2, batch_size=4, normalize=True, first_epoch=0, lr=LR):
        stats = self.train.train(self.params, n_epochs=n_epochs, batch_size=batch_size, clip_range=CLIP, vf_coef=VF, ent_coef=ENT, lr=lr,
                                 normalize_advantage=normalize, seed=SEED, first_epoch=first_epoch)
        return self.state(stats)

    def step_by_step(self, *, n_epochs=2, batch_size=4, normalize=True, first_epoch=0):
        """The existing pieces, one minibatch at a time; the statistics block from the model's means of their stats."""
        per = []
        for e in range(n_epochs):
            idx = tm.indices(self.n, SEED, first_epoch + e)
            for start, B in tm.minibatches(self.n, batch_size):
                b = self.buf.gather(on_device(idx[start:start + B]))
                adv = on_device(tm.normalise(host(b.advantages), normalize))
                s = self.grad.grad(b, self.params[-1], CLIP, VF, ENT, into=self.params, advantages=adv)
                self.adam.step(lr=LR)
                per.append(host(s))
        out = self.state()
        out["stats"] = tm.stats_block(per, tm.explained_variance(host(self.buf.returns), host(self.buf.values)),
                                      tm.mean_std(out["params"][-1]))
        return out

    def close(self):
        for h in (self.train, self.adam, self.grad, self.buf, self.pol):
            if h is not None:
                h.close()


def same(a, b, stats=9):
    """Every parameter, the image, Adam's moments and step count, and the first `stats` statistics: bit for bit."""
    return a["step"] == b["step"] and all(pb.same_bits(x, y) for k in ("params", "image", "exp_avg", "exp_avg_sq") for x, y in zip(a[k], b[k])) and \
        all(len(a[k]) == len(b[k]) for k in ("params", "image", "exp_avg", "exp_avg_sq")) and same64(a["stats"][:stats], b["stats"][:stats])


def staging_views(rig):
    """The staging arrays behind describe()["staging"], laid out as the header says: each at the next multiple of 256 bytes."""
    from fleetrl_amd._handle import _DeviceArray

    d = rig.train.describe()
    mb, off, out = d["max_batch"], 0, {}
    for name, cols in (("obs", rig.D), ("actions", rig.A), ("old_log_prob", 1), ("advantages", 1), ("normalised", 1), ("returns", 1)):
        out[name] = torch.as_tensor(_DeviceArray(d["staging"] + off, (mb, cols), "<f4", rig.train), device=dev())
        off = (off + mb * cols * 4 + 255) // 256 * 256
    assert off == d["staging_bytes"]
    return out


# ---- the shuffle ---------------------------------------------------------------------------------------------------------------------
def test_indices_equal_the_model_bit_for_bit():
    rig = Rig("5-8-8-3", 16)
    d = rig.train.describe()
    assert (d["rounds"], d["min_half_bits"], d["tile_rows"], d["max_batch"], d["n_tensors"]) == (tm.ROUNDS, tm.MIN_HALF_BITS, 4, 16, 13)
    assert (d["num_envs"], d["n_steps"], d["obs_dim"], d["act_dim"]) == (3, 5, 5, 3)
    for n in (1, 5, 17, 65, 4097):
        for seed, epoch in ((SEED, 0), (3, 2 ** 33 + 1)):
            got = host(rig.train.indices(n, seed, epoch))
            assert got.dtype == np.int32 and np.array_equal(got, tm.indices(n, seed, epoch)), (n, seed, epoch)
    assert np.array_equal(host(rig.train.indices(4097, 9, 1, 4000, 97)), tm.indices(4097, 9, 1, 4000, 97))
    assert rig.train.indices(10, 1, 0, 10, 0).numel() == 0
    rig.close()


@pytest.mark.parametrize("shape,max_batch", [("5-8-8-3", 16), ("8-8-8-4", 80)])
def test_one_epoch_of_minibatch_launches_gathers_every_row_exactly_once(shape, max_batch):
    """Observed through the staging block that describe() names, after one-epoch calls with lr = 0 on a buffer whose returns[t, e] and
    obs[t, e, 0] hold the flat index e * K + t (old values are not staged): a minibatch of n rows stages the whole epoch in the
    model's order; with batch_size 4 the staging block holds the last minibatch, the model's positions behind the last multiple of 4."""
    rig = Rig(shape, max_batch)
    n, E, K = rig.n, rig.E, rig.K
    flat = (np.arange(E)[None, :] * K + np.arange(K)[:, None]).astype(F32)  # [K, E]
    rig.buf.returns.copy_(on_device(flat))
    rig.buf.observations[:, :, 0].copy_(on_device(flat))
    rig.buf.actions[:, :, -1].copy_(on_device(-flat))
    before = rig.state()
    got = rig.one_call(n_epochs=1, batch_size=n, lr=0.0, first_epoch=6)
    st = staging_views(rig)
    rows = host(st["returns"])[:n, 0]
    assert np.array_equal(np.sort(rows), np.arange(n)) and np.array_equal(rows, tm.indices(n, SEED, 6))
    assert np.array_equal(host(st["obs"])[:n, 0], rows) and np.array_equal(host(st["actions"])[:n, -1], -rows)
    e, t = rows.astype(int) // K, rows.astype(int) % K
    assert pb.same_bits(host(st["obs"])[:n], host(rig.buf.observations)[t, e]) and pb.same_bits(host(st["actions"])[:n], host(rig.buf.actions)[t, e])
    assert pb.same_bits(host(st["old_log_prob"])[:n, 0], host(rig.buf.log_probs)[t, e])
    assert pb.same_bits(host(st["advantages"])[:n, 0], host(rig.buf.advantages)[t, e])
    assert pb.same_bits(host(st["normalised"])[:n, 0], tm.normalise(host(rig.buf.advantages)[t, e]))
    assert all(pb.same_bits(a, b) for a, b in zip(got["params"], before["params"])) and got["step"] == 1 and got["stats"][6] == 1.0
    rig.one_call(n_epochs=1, batch_size=4, lr=0.0, first_epoch=7)
    tail = n - (n - 1) // 4 * 4
    assert np.array_equal(host(staging_views(rig)["returns"])[:tail, 0], tm.indices(n, SEED, 7)[n - tail:])
    rig.buf.check_errors()
    rig.close()


# ---- the equivalence test ------------------------------------------------------------------------------------------------------------
EQUIVALENCE = {
    "base": ("5-8-8-3", 8, dict(batch_size=4)),  # four minibatches per epoch, the last of 3 rows
    "words-16": ("8-8-8-4", 32, dict(batch_size=16)),
    "words-17": ("8-8-8-4", 32, dict(batch_size=17)),
    "batch-n": ("5-8-8-3", 16, dict(batch_size=15)),
    "batch-above-n": ("5-8-8-3", 16, dict(batch_size=64)),
    "batch-1": ("5-8-8-3", 8, dict(batch_size=1, n_epochs=1)),  # no normalisation: SB3's exception for one row
    "normalisation-off": ("5-8-8-3", 8, dict(batch_size=4, normalize=False)),
    "relu": ("5-8-8-3-relu", 8, dict(batch_size=4)),
    "above-the-lanes": ("5-8-3-long", 304, dict(batch_size=300, n_epochs=1)),  # seven minibatches of 300 rows: two passes of the lanes
    "above-the-cache": ("5-8-3-long", 2100, dict(batch_size=2100)),  # rows behind position 2048 are evaluated where they are needed
}


@pytest.mark.parametrize("case", sorted(EQUIVALENCE))
def test_the_one_call_equals_the_existing_pieces_step_by_step_bit_for_bit(case):
    shape, max_batch, kw = EQUIVALENCE[case]
    a, b = Rig(shape, max_batch), Rig(shape, max_batch, train=False)
    start = a.state()
    assert all(pb.same_bits(x, y) for x, y in zip(start["params"], b.state()["params"]))
    got, want = a.one_call(**kw), b.step_by_step(**kw)
    count = len(tm.minibatches(a.n, kw["batch_size"])) * kw.get("n_epochs", 2)
    print(case, "minibatches", count, "statistics", dict(zip(tm.STATS, got["stats"][:9])), "model", want["stats"][:9].tolist())
    assert got["step"] == want["step"] == count and got["stats"][6] == count
    for k in ("params", "image", "exp_avg", "exp_avg_sq"):
        assert len(got[k]) == len(want[k])
        for i, (x, y) in enumerate(zip(got[k], want[k])):
            assert pb.same_bits(x, y), (case, k, i, float(np.abs(x - y).max()))
    assert all(pb.same_bits(p, i) for p, i in zip(got["params"][:-1], got["image"]))  # the image moved with the parameters
    assert not all(pb.same_bits(x, y) for x, y in zip(got["params"], start["params"]))  # and both did move
    assert same64(got["stats"][:8], want["stats"][:8]), (got["stats"][:8].tolist(), want["stats"][:8].tolist())
    assert np.isfinite(got["stats"]).all() and not got["stats"][9:].any()
    std = np.exp(got["params"][-1].astype(np.float64)).mean()
    assert abs(got["stats"][8] - std) <= 8 * 2.0 ** -24 * std
    a.buf.check_errors()
    a.close()
    b.close()


# ---- explained_variance and the mean std ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["5-8-8-3", "5-8-3-long"])
def test_explained_variance_and_the_mean_std_stay_within_the_projects_bound(shape):
    """|device - ref64| <= 8 max(eps_ref, 2^-24 |ref64|): ref64 NumPy float64 on the same buffer, eps_ref the error of SB3's own float32
    evaluation (its explained_variance helper on float32 arrays; exp(log_std).mean() in float32)."""
    rig = Rig(shape, 16)
    got = rig.one_call(n_epochs=1, batch_size=16)
    y, v = host(rig.buf.returns).reshape(-1), host(rig.buf.values).reshape(-1)
    ref = 1.0 - np.var(y.astype(np.float64) - v.astype(np.float64)) / np.var(y.astype(np.float64))
    eps_ref = abs(float(1 - np.var(y - v) / np.var(y)) - ref)
    err, bound = abs(got["stats"][7] - ref), 8 * max(eps_ref, 2.0 ** -24 * abs(ref))
    print(f"{shape}: explained_variance {got['stats'][7]!r} ref {ref!r} eps_ref {eps_ref:.3g} err {err:.3g} bound {bound:.3g}")
    assert err <= bound and same64(got["stats"][7:8], np.array([tm.explained_variance(y, v)]))
    ls = got["params"][-1]
    sref = float(np.exp(ls.astype(np.float64)).mean())
    seps = abs(float(np.exp(ls).mean()) - sref)
    serr, sbound = abs(got["stats"][8] - sref), 8 * max(seps, 2.0 ** -24 * sref)
    print(f"{shape}: std {got['stats'][8]!r} ref {sref!r} eps_ref {seps:.3g} err {serr:.3g} bound {sbound:.3g}")
    assert serr <= sbound
    rig.buf.returns.fill_(2.5)  # constant returns: var(returns) is 0
    assert np.isnan(rig.one_call(n_epochs=1, batch_size=16, first_epoch=1)["stats"][7])
    rig.close()


# ---- determinism ---------------------------------------------------------------------------------------------------------------------
def test_a_result_depends_on_the_state_the_seed_and_the_epoch_and_on_nothing_else():
    shape, kw = "8-8-8-4", dict(batch_size=17, n_epochs=2, first_epoch=3)
    rig = Rig(shape, 32)
    ref = rig.one_call(**kw)
    rig.close()
    assert np.isfinite(ref["stats"]).all() and all(np.isfinite(p).all() for p in ref["params"])

    again = Rig(shape, 32)
    assert same(again.one_call(**kw), ref)  # two calls from identical states
    again.close()

    other = Rig(shape, 32)
    s = torch.cuda.Stream(device=dev())
    torch.cuda.synchronize()
    with torch.cuda.stream(s):  # another stream: the policy's and the buffer's move with torch's current one
        got = other.one_call(**kw)
    torch.cuda.synchronize()
    assert same(got, ref)
    other.close()

    big = Rig(shape, 4 * 32 + 5)  # a larger max_batch: other staging strides, another scratch
    assert big.train.describe()["staging_bytes"] > 32 * (8 + 4 + 4) * 4 and same(big.one_call(**kw), ref)
    big.close()

    nan = Rig(shape, 48)  # NaN behind (and, before the call, in) the staging rows in use
    for t in staging_views(nan).values():
        t.fill_(float("nan"))
    assert same(nan.one_call(**kw), ref)
    assert np.isnan(host(staging_views(nan)["obs"])[17:]).all()  # rows at and past B are never written
    nan.close()

    moved = Rig(shape, 32)
    got = moved.one_call(**dict(kw, first_epoch=4))
    assert not all(pb.same_bits(x, y) for x, y in zip(got["params"], ref["params"])) and got["step"] == ref["step"]
    moved.close()


# ---- the refusals that need handles --------------------------------------------------------------------------------------------------
def test_refusals_that_need_the_handles():
    from fleetrl_amd import DeviceAdam, DevicePPOGrad, DevicePPOTrain, DeviceRolloutBuffer, FleetHipError, _capi

    rig = Rig("5-8-8-3", 4)
    before = rig.state()
    a = _capi.FleetTrainPpoArgs()
    a.n_epochs, a.batch_size, a.normalize_advantage, a.clip_range, a.vf_coef, a.lr, a.beta1, a.beta2, a.eps = 1, 4, 1, CLIP, VF, LR, 0.9, 0.999, EPS
    stats = torch.zeros(16, device=dev(), dtype=torch.float64)
    a.stats = stats.data_ptr()
    for p in rig.params:
        p.grad = torch.zeros_like(p)
    P = (C.c_void_p * 13)(*[p.data_ptr() for p in rig.params])
    G = (C.c_void_p * 13)(*[p.grad.data_ptr() for p in rig.params])
    rig.train.use_torch_stream()
    with pytest.raises(FleetHipError, match=r"fleet_train_ppo_dev: expected 13 gradient tensors \(W, b per layer, then log_std\), got 12"):
        rig.train.train_dev(a, P, G, 12)
    a.batch_size = 5
    with pytest.raises(FleetHipError, match="fleet_train_ppo_dev: a minibatch of 5 rows: B must be at most max_batch = 4, got 5"):
        rig.train.train_dev(a, P, G, 13)
    a.batch_size = 4
    s = torch.cuda.Stream(device=dev())
    rig.buf.set_stream(s.cuda_stream)
    with pytest.raises(FleetHipError, match="fleet_train_ppo_dev: the rollout buffer launches on another stream than the policy"):
        rig.train.train_dev(a, P, G, 13)
    rig.buf.set_stream(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    after = rig.state()
    assert after["step"] == 0 and all(pb.same_bits(x, y) for x, y in zip(after["params"], before["params"]))  # nothing was launched
    rig.train.train_dev(a, P, G, 13)  # and the same arguments pass once the streams agree
    assert rig.adam.describe()["step"] == 4 and np.isfinite(host(stats)).all()
    with pytest.raises(FleetHipError, match="needs a full rollout buffer"):
        rig.buf.reset()
        rig.one_call()
    rig.buf.pos, rig.buf.full = rig.K, True

    # create: handles on different policies, a buffer of other shapes, an optimiser without log_std
    other = Rig("5-8-8-3", 4, train=False)
    with pytest.raises(FleetHipError, match="fleet_train_create: the gradient handle and the optimiser lie on different policies"):
        DevicePPOTrain(rig.buf, rig.grad, other.adam)
    wide = DeviceRolloutBuffer(3, 5, 6, 3)
    with pytest.raises(FleetHipError, match="fleet_train_create: the rollout buffer's obs_dim is 6, the policy's 5"):
        DevicePPOTrain(wide, rig.grad, rig.adam)
    short = DeviceRolloutBuffer(3, 5, 5, 2)
    with pytest.raises(FleetHipError, match="fleet_train_create: the rollout buffer's act_dim is 2, the policy's 3"):
        DevicePPOTrain(short, rig.grad, rig.adam)
    bare = DeviceAdam(rig.pol, rig.params[:-1], lr=LR)
    with pytest.raises(FleetHipError, match="fleet_train_create: the optimiser's span must be both heads of the policy and one extra of length 3"):
        DevicePPOTrain(rig.buf, rig.grad, bare)
    actor_only = DeviceAdam(rig.pol, rig.params[:6] + rig.params[-1:], nets="actor", lr=LR)
    with pytest.raises(FleetHipError, match="the optimiser's span must be both heads"):
        DevicePPOTrain(rig.buf, rig.grad, actor_only)
    assert isinstance(DevicePPOGrad, type)
    for h in (bare, actor_only, wide, short):
        h.close()
    other.close()
    rig.close()


# ---- the example ---------------------------------------------------------------------------------------------------------------------
def test_the_example_runs_at_its_default_sizes_and_prints_finite_statistics():
    """examples/ppo_device_train.py as a child process under a time limit of its own: exit 0, SB3's train/* names, finite numbers."""
    cmd = ["timeout", "-k", "10", "240", sys.executable, os.path.join(tm.ROOT, "examples", "ppo_device_train.py")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) >= 2
    for d in lines:
        for k in ("train/policy_gradient_loss", "train/value_loss", "train/entropy_loss", "train/approx_kl", "train/clip_fraction", "train/loss",
                  "train/n_updates", "train/explained_variance", "train/std"):
            assert np.isfinite(d[k]), (k, d)
    assert lines[-1]["train/n_updates"] > lines[0]["train/n_updates"] > 0
