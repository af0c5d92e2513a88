"""PPO's whole update with value-function clipping (fleet_train_ppo_vclip_dev): the one call against the pieces run step by step (model
indices, DeviceRolloutBuffer.gather, the model's normalisation, DevicePPOGrad.grad(clip_range_vf=...), DeviceAdam.step) bit for bit, the
staged old values, the unclipped call unchanged, and the example with its new flags."""
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
CV = 0.2
SEED = 0x1234567890ABCDEF  # (both key words in use)


def dev():
    return torch.device("cuda", 0)


def on_device(a):
    return torch.from_numpy(np.array(a)).to(dev())


def host(t):
    return t.detach().cpu().numpy().copy()


def same64(a, b) -> bool:
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


# name -> (D, hidden widths, A, E, K)
SHAPES = {
    "5-8-8-3": (5, (8, 8), 3, 3, 5),
    "8-8-8-4": (8, (8, 8), 4, 5, 13),  # D and A multiples of 4: rows move as 16-byte words
    "5-8-3-long": (5, (8,), 3, 3, 700),  # n = 2100: rows behind the 2048 cached positions
}


def weights(shape):
    D, hidden, A, _, _ = SHAPES[shape]
    rng = np.random.default_rng(len(shape) + D)
    nets = []
    for out in (A, 1):
        sizes, net = (D, *hidden, out), []
        for i, o in zip(sizes[:-1], sizes[1:]):
            net.append(((rng.standard_normal((o, i)) / np.sqrt(i)).astype(F32), (0.1 * rng.standard_normal(o)).astype(F32)))
        nets.append(net)
    return nets[0], nets[1], (-0.5 + 0.1 * rng.standard_normal(A)).astype(F32)


class Rig:
    """A policy, its torch parameters, a full rollout buffer and the three handles on them, identically initialised per shape.  The
    buffer's values lie within +-0.45 of what the critic gives under these weights: a clip range of 0.2 takes about half the rows."""

    def __init__(self, shape, max_batch, train=True):
        from fleetrl_amd import DeviceAdam, DevicePolicy, DevicePPOGrad, DevicePPOTrain, DeviceRolloutBuffer

        D, _, A, E, K = SHAPES[shape]
        actor, critic, log_std = weights(shape)
        self.shape, self.n, self.E, self.K, self.D, self.A = shape, E * K, E, K, D, A
        self.pol = DevicePolicy(actor, critic_layers=critic, activation="tanh", output="clip")
        self.params = [torch.nn.Parameter(on_device(t)) for net in (actor, critic) for w, b in net for t in (w, b)] + [torch.nn.Parameter(on_device(log_std))]
        self.buf = DeviceRolloutBuffer(E, K, D, A)
        rng = np.random.default_rng(E * K)
        self.buf.observations.copy_(on_device(rng.standard_normal((K, E, D)).astype(F32)))
        for t in range(K):
            row = self.buf.slot(t)
            self.pol.sample(row.obs, self.params[-1], seed=5, step=t, actions_out=row.actions, log_prob_out=row.log_prob, values_out=row.value)
        adv = (rng.standard_normal((K, E)) * 2.0 + 0.3).astype(F32)
        self.buf.values.add_(on_device(rng.uniform(-0.45, 0.45, (K, E)).astype(F32)))
        self.buf.advantages.copy_(on_device(adv))
        self.buf.returns.copy_(self.buf.values + on_device((0.5 * rng.standard_normal((K, E))).astype(F32)))
        self.buf.pos, self.buf.full = K, True
        self.grad = DevicePPOGrad(self.pol, max_batch)
        self.adam = DeviceAdam(self.pol, self.params, lr=LR, eps=EPS, max_grad_norm=MAXN)
        self.train = DevicePPOTrain(self.buf, self.grad, self.adam) if train else None
        torch.cuda.synchronize()

    def state(self, stats=None):
        sd = self.adam.state_dict()["state"]
        out = {"params": [host(p) for p in self.params], "image": [host(t) for t in self.adam.export_image()],
               "exp_avg": [host(sd[i]["exp_avg"]) for i in range(len(sd))], "exp_avg_sq": [host(sd[i]["exp_avg_sq"]) for i in range(len(sd))],
               "step": self.adam.describe()["step"]}
        if stats is not None:
            out["stats"] = host(stats)
        return out

    def one_call(self, *, cv=CV, n_epochs=2, batch_size=4, normalize=True, first_epoch=0, lr=LR):
        stats = self.train.train(self.params, n_epochs=n_epochs, batch_size=batch_size, clip_range=CLIP, vf_coef=VF, ent_coef=ENT, lr=lr,
                                 normalize_advantage=normalize, seed=SEED, first_epoch=first_epoch, clip_range_vf=cv)
        return self.state(stats)

    def step_by_step(self, *, cv=CV, n_epochs=2, batch_size=4, normalize=True, first_epoch=0):
        """The pieces, one minibatch at a time; the statistics block from the model's means of their stats."""
        per = []
        for e in range(n_epochs):
            idx = tm.indices(self.n, SEED, first_epoch + e)
            for start, B in tm.minibatches(self.n, batch_size):
                b = self.buf.gather(on_device(idx[start:start + B]))
                adv = on_device(tm.normalise(host(b.advantages), normalize))
                s = self.grad.grad(b, self.params[-1], CLIP, VF, ENT, into=self.params, advantages=adv, clip_range_vf=cv)
                self.adam.step(lr=LR)
                per.append(host(s))
        out = self.state()
        out["stats"] = tm.stats_block(per, tm.explained_variance(host(self.buf.returns), host(self.buf.values)), tm.mean_std(out["params"][-1]))
        return out

    def staged_old_values(self):
        from fleetrl_amd._handle import _DeviceArray

        d = self.train.describe()
        assert d["old_values_offset"] >= d["staging_bytes"] + 512 and d["old_values_offset"] % 256 == 0  # behind the stats and the sums
        return torch.as_tensor(_DeviceArray(d["staging"] + d["old_values_offset"], (d["max_batch"],), "<f4", self.train), device=dev())

    def close(self):
        for h in (self.train, self.adam, self.grad, self.buf, self.pol):
            if h is not None:
                h.close()


def same(a, b, stats=8):
    return a["step"] == b["step"] and all(pb.same_bits(x, y) for k in ("params", "image", "exp_avg", "exp_avg_sq") for x, y in zip(a[k], b[k])) and \
        all(len(a[k]) == len(b[k]) for k in ("params", "image", "exp_avg", "exp_avg_sq")) and same64(a["stats"][:stats], b["stats"][:stats])


# ---- the equivalence test ------------------------------------------------------------------------------------------------------------
EQUIVALENCE = {
    "base": ("5-8-8-3", 8, dict(batch_size=4)),  # four minibatches per epoch, the last of 3 rows
    "normalisation-off": ("5-8-8-3", 8, dict(batch_size=4, normalize=False)),
    "words-17": ("8-8-8-4", 32, dict(batch_size=17)),
    "batch-1": ("5-8-8-3", 8, dict(batch_size=1)),
    "above-the-cache": ("5-8-3-long", 2100, dict(batch_size=2100)),  # rows behind position 2048 are evaluated where they are needed
}


@pytest.mark.parametrize("case", sorted(EQUIVALENCE))
def test_the_one_call_equals_the_pieces_step_by_step_bit_for_bit(case):
    shape, max_batch, kw = EQUIVALENCE[case]
    a, b, plain = Rig(shape, max_batch), Rig(shape, max_batch, train=False), Rig(shape, max_batch)
    start = a.state()
    got, want = a.one_call(**kw), b.step_by_step(**kw)
    count = len(tm.minibatches(a.n, kw["batch_size"])) * 2
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
    # the clip bites on this buffer: the unclipped update ends elsewhere, with another value loss
    un = plain.one_call(cv=None, **kw)
    assert un["step"] == count and un["stats"][1] != got["stats"][1]
    assert not all(pb.same_bits(x, y) for x, y in zip(un["params"], got["params"]))
    a.buf.check_errors()
    for r in (a, b, plain):
        r.close()


# ---- the staged old values -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,max_batch", [("5-8-8-3", 16), ("8-8-8-4", 80)])
def test_a_one_epoch_call_stages_the_buffers_values_at_the_models_indices(shape, max_batch):
    rig = Rig(shape, max_batch)
    n, K = rig.n, rig.K
    staged = rig.staged_old_values()
    staged.fill_(float("nan"))
    before = rig.state()
    got = rig.one_call(n_epochs=1, batch_size=n, lr=0.0, first_epoch=6)
    rows = tm.indices(n, SEED, 6).astype(int)
    e, t = rows // K, rows % K
    vals = host(staged)
    assert pb.same_bits(vals[:n], host(rig.buf.values)[t, e]) and np.isnan(vals[n:]).all()  # rows at and past B are never written
    assert all(pb.same_bits(x, y) for x, y in zip(got["params"], before["params"])) and got["step"] == 1
    staged.fill_(float("nan"))
    rig.one_call(cv=None, n_epochs=1, batch_size=n, lr=0.0, first_epoch=7)  # the unclipped update does not stage them
    assert np.isnan(host(staged)).all()
    rig.close()


# ---- the unclipped call is today's ---------------------------------------------------------------------------------------------------
def test_clip_range_vf_none_is_the_existing_update_bit_for_bit():
    """train(clip_range_vf=None) against the existing entry through train_dev on a FleetTrainPpoArgs, and against the unclipped pieces."""
    from fleetrl_amd import _capi

    shape, kw = "8-8-8-4", dict(batch_size=17)
    a, b, c = Rig(shape, 32), Rig(shape, 32), Rig(shape, 32, train=False)
    got = a.one_call(cv=None, **kw)
    x = _capi.FleetTrainPpoArgs()
    x.n_epochs, x.batch_size, x.normalize_advantage, x.clip_range, x.vf_coef, x.ent_coef, x.lr = 2, 17, 1, CLIP, VF, ENT, LR
    x.beta1, x.beta2, x.eps, x.max_grad_norm, x.seed, x.first_epoch = 0.9, 0.999, EPS, MAXN, SEED, 0
    stats = torch.zeros(16, device=dev(), dtype=torch.float64)
    x.stats = stats.data_ptr()
    b.train.use_torch_stream()
    grads = b.train._grad_pointers("train", b.params, b.train._shapes, "the actor's then the critic's, then log_std")
    b.train.train_dev(x, b.train._param_pointers(b.params), grads, len(b.params))
    assert same(got, b.state(stats), stats=16)
    assert same(got, c.step_by_step(cv=None, **kw))
    for r in (a, b, c):
        r.close()


# ---- refusals that need the handle ---------------------------------------------------------------------------------------------------
def test_refusals_that_need_the_handle_and_pythons():
    from fleetrl_amd import FleetHipError

    rig = Rig("5-8-8-3", 4)
    before = rig.state()
    with pytest.raises(FleetHipError, match="fleet_train_ppo_vclip_dev: a minibatch of 5 rows: B must be at most max_batch = 4, got 5"):
        rig.one_call(batch_size=5)
    for bad in (0.0, -0.2, float("nan")):
        with pytest.raises(ValueError, match="`clip_range_vf` must be positive, pass `None` to deactivate vf clipping"):
            rig.one_call(cv=bad)
    after = rig.state()
    assert after["step"] == 0 and all(pb.same_bits(x, y) for x, y in zip(after["params"], before["params"]))  # nothing was launched
    assert rig.one_call(batch_size=4)["step"] == 8
    rig.close()


# ---- the example ---------------------------------------------------------------------------------------------------------------------
def test_the_example_runs_with_value_clipping_and_without_normalisation_and_prints_finite_statistics():
    """examples/ppo_device_train.py as a child process under a time limit of its own: exit 0, SB3's train/* names, finite numbers."""
    cmd = ["timeout", "-k", "10", "240", sys.executable, os.path.join(tm.ROOT, "examples", "ppo_device_train.py"), "--clip-range-vf", "0.2",
           "--no-normalize-advantage", "--iterations", "2"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 2
    for d in lines:
        for k in ("train/policy_gradient_loss", "train/value_loss", "train/entropy_loss", "train/approx_kl", "train/clip_fraction", "train/loss",
                  "train/n_updates", "train/explained_variance", "train/std"):
            assert np.isfinite(d[k]), (k, d)
    assert lines[-1]["train/n_updates"] > lines[0]["train/n_updates"] > 0
