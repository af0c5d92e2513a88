"""PPO's update with early stopping on approx_kl (fleet_train_ppo_kl_dev): the one gated call against the pieces run step by step from
Python with the decision made on the host -- after each DevicePPOGrad.grad read stats[4] and break, before DeviceAdam.step, when
float64(stats[4]) > 1.5 * target_kl -- bit for bit in parameters, image, both moments, the optimiser's step count and all 16 slots of
the statistics block (tests/ppo_kl_model.py); the settlement of the step count; target_kl=None unchanged; the pieces' wrappers; the
example with its new flag.

Every target_kl comes from a dry step-by-step run without a stop: 1.5 * target_kl lies halfway between a running-maximum record of the
approx_kl sequence and the largest value before it, so the stop index is known in advance and no value sits near the threshold."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import policy_bits as pb
import ppo_kl_model as klm
import train_model as tm

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F32, F64 = np.float32, np.float64
CLIP, VF, ENT, LR, EPS, MAXN = 0.2, 0.5, 0.01, 3e-3, 1e-5, 0.5
CV = 0.2
EPOCHS = 3
SEED = 0x1234567890ABCDEF  # (both key words in use)
NEVER = 1e6  # a target_kl above every approx_kl


def dev():
    return torch.device("cuda", 0)


def on_device(a):
    return torch.from_numpy(np.array(a)).to(dev())


def host(t):
    return t.detach().cpu().numpy().copy()


def same64(a, b) -> bool:
    a, b = np.ascontiguousarray(a, F64), np.ascontiguousarray(b, F64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


# name -> (D, hidden widths, A, E, K)
SHAPES = {
    "5-8-8-3": (5, (8, 8), 3, 3, 5),
    "8-8-8-4": (8, (8, 8), 4, 5, 13),  # D and A multiples of 4: rows move as 16-byte words
    "5-8-3-long": (5, (8,), 3, 3, 700),  # n = 2100: rows behind the 2048 cached positions
}
# name -> (shape, max_batch, batch_size): minibatches per epoch 4 (the last of 3 rows), 4 (the last of 14), 17 (the last of 1), 1, 1
CONFIGS = {
    "small-4": ("5-8-8-3", 8, 4),
    "words-17": ("8-8-8-4", 32, 17),
    "words-4": ("8-8-8-4", 32, 4),
    "small-17": ("5-8-8-3", 16, 17),  # batch_size above n: one minibatch of 15 rows per epoch
    "long": ("5-8-3-long", 2100, 2100),
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

    def __init__(self, config):
        from fleetrl_amd import DeviceAdam, DevicePolicy, DevicePPOGrad, DevicePPOTrain, DeviceRolloutBuffer

        shape, max_batch, self.batch_size = CONFIGS[config]
        D, _, A, E, K = SHAPES[shape]
        actor, critic, log_std = weights(shape)
        self.shape, self.n, self.E, self.K, self.D, self.A = shape, E * K, E, K, D, A
        self.per_epoch = len(tm.minibatches(self.n, self.batch_size))
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
        self.train = DevicePPOTrain(self.buf, self.grad, self.adam)
        torch.cuda.synchronize()

    def state(self, stats=None):
        sd = self.adam.state_dict()["state"]
        out = {"params": [host(p) for p in self.params], "image": [host(t) for t in self.adam.export_image()],
               "exp_avg": [host(sd[i]["exp_avg"]) for i in range(len(sd))], "exp_avg_sq": [host(sd[i]["exp_avg_sq"]) for i in range(len(sd))],
               "grads": [None if p.grad is None else host(p.grad) for p in self.params], "step": self.adam.describe()["step"]}
        if stats is not None:
            out["stats"] = host(stats)
        return out

    def one_call(self, *, target_kl, cv=None, n_epochs=EPOCHS, first_epoch=0, lr=LR, batch_size=None):
        stats = self.train.train(self.params, n_epochs=n_epochs, batch_size=batch_size or self.batch_size, clip_range=CLIP, vf_coef=VF, ent_coef=ENT,
                                 lr=lr, seed=SEED, first_epoch=first_epoch, clip_range_vf=cv, target_kl=target_kl)
        return self.state(stats)

    def pieces(self, *, target_kl=None, cv=None, n_epochs=EPOCHS, first_epoch=0):
        """The pieces, one minibatch at a time, the decision on the host: the stats f32[8] of every minibatch that ran."""
        thr = None if target_kl is None else klm.threshold(target_kl)
        per = []
        for e in range(n_epochs):
            idx = tm.indices(self.n, SEED, first_epoch + e)
            for start, B in tm.minibatches(self.n, self.batch_size):
                b = self.buf.gather(on_device(idx[start:start + B]))
                adv = on_device(tm.normalise(host(b.advantages), True))
                s = self.grad.grad(b, self.params[-1], CLIP, VF, ENT, into=self.params, advantages=adv, clip_range_vf=cv)
                per.append(host(s))
                if thr is not None and F64(per[-1][4]) > thr:
                    return per
                self.adam.step(lr=LR)
        return per

    def block(self, per, target_kl):
        """(stop, the statistics block the model gives for the minibatches `per`): explained variance from the model, the mean
        standard deviation from the existing closing launch on the same log_std bits (device_std)."""
        thr = np.inf if target_kl is None else klm.threshold(target_kl)
        ev = tm.explained_variance(host(self.buf.returns), host(self.buf.values))
        return klm.stats_block(per, self.per_epoch, thr, ev, device_std(self.shape, host(self.params[-1])))

    def close(self):
        for h in (self.train, self.adam, self.grad, self.buf, self.pol):
            h.close()


# ---- what is computed once -----------------------------------------------------------------------------------------------------------
_PROBES, _DRY = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _close_the_probes():
    yield
    for rig in _PROBES.values():
        rig.close()
    _PROBES.clear()


def device_std(shape, log_std) -> F64:
    """Slot [8] as the EXISTING closing launch forms it from these log_std bits: an ungated update with lr = 0 on a rig kept for it."""
    config = {"5-8-8-3": "small-17", "8-8-8-4": "words-17", "5-8-3-long": "long"}[shape]
    rig = _PROBES.get(shape) or _PROBES.setdefault(shape, Rig(config))
    with torch.no_grad():
        rig.params[-1].copy_(on_device(np.asarray(log_std, dtype=F32)))
    got = rig.one_call(target_kl=None, n_epochs=1, lr=0.0)
    assert pb.same_bits(got["params"][-1], np.asarray(log_std, dtype=F32))
    return F64(got["stats"][8])


def dry(config, cv=None):
    """The approx_kl sequence (and every stats row) of a step-by-step run of EPOCHS epochs without a stop, once per (config, cv)."""
    key = (config, cv)
    if key not in _DRY:
        rig = Rig(config)
        per = rig.pieces(cv=cv)
        rig.close()
        seq = [float(F64(r[4])) for r in per]
        rec = klm.records(seq)
        print(f"{config} cv={cv}: approx_kl {['%.3g' % x for x in seq]} records {rec}")
        # the preconditions: enough records to place a threshold, one of them behind the first epoch
        assert len(per) == EPOCHS * len(tm.minibatches(rig.n, rig.batch_size)) and np.isfinite(seq).all()
        assert len(rec) >= 3 and rec[0] == 0 and seq[0] >= 0.0, (config, seq)
        assert any(r >= rig.per_epoch for r in rec), (config, seq)
        _DRY[key] = (per, seq, rec)
    return _DRY[key]


def compare(case, got, want, block, grads=True):
    keys = ("params", "image", "exp_avg", "exp_avg_sq") + (("grads",) if grads else ())
    for k in keys:
        assert len(got[k]) == len(want[k])
        for i, (x, y) in enumerate(zip(got[k], want[k])):
            assert pb.same_bits(x, y), (case, k, i, float(np.abs(x - y).max()))
    assert all(pb.same_bits(p, i) for p, i in zip(got["params"][:-1], got["image"]))  # the image moved with the parameters
    assert got["step"] == want["step"], (case, got["step"], want["step"])
    print(case, "statistics", got["stats"].tolist(), "model", block.tolist())
    assert same64(got["stats"], block), (case, got["stats"].tolist(), block.tolist())


def check_stop(case, config, record, cv=None, n_epochs=EPOCHS):
    """A gated call whose threshold lies below the record `record` of the dry sequence, against the pieces under the same target_kl."""
    per_dry, seq, rec = dry(config, cv)
    assert record in rec[1:]
    # no value near the threshold: the record clears everything before it by far more than the comparison's rounding (none: exact)
    assert seq[record] > 1.0001 * max(seq[:record]) and seq[record] > 1e-12, (config, record, seq)
    target = klm.target_for(seq, record)
    a, b = Rig(config), Rig(config)
    got = a.one_call(target_kl=target, cv=cv, n_epochs=n_epochs)
    per = b.pieces(target_kl=target, cv=cv, n_epochs=n_epochs)
    stop, block = b.block(per, target)
    assert stop == record == len(per) - 1 and all(pb.same_bits(x, y) for x, y in zip(per, per_dry[:record + 1]))
    compare(case, got, b.state(), block)
    s = got["stats"]
    assert s[6] == record + 1 and s[9] == record == got["step"] and s[10] == record // a.per_epoch + 1 and s[11] == 1.0
    assert s[12] == F64(F32(seq[record])) and s[12] > klm.threshold(target) and not s[14:].any()
    a.buf.check_errors()
    a.close(), b.close()
    return s


# ---- 1: a target_kl that never triggers ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config,cv", [("small-4", None), ("words-17", None), ("long", None), ("words-17", CV)])
def test_a_target_kl_that_never_triggers_is_the_ungated_update_bit_for_bit(config, cv):
    per, seq, _ = dry(config, cv)
    a, b = Rig(config), Rig(config)
    got, want = a.one_call(target_kl=NEVER, cv=cv), b.one_call(target_kl=None, cv=cv)
    count = EPOCHS * a.per_epoch
    for k in ("params", "image", "exp_avg", "exp_avg_sq", "grads"):
        assert all(pb.same_bits(x, y) for x, y in zip(got[k], want[k])) and len(got[k]) == len(want[k]), k
    assert got["step"] == want["step"] == count and same64(got["stats"][:9], want["stats"][:9]) and not want["stats"][9:].any()
    s = got["stats"]
    assert s[6] == s[9] == count and s[10] == EPOCHS and s[11] == 0.0 and not s[14:].any()
    stop, block = a.block(per, NEVER)
    assert stop is None
    compare(config, got, want, block)  # [12] the last approx_kl, [13] the last epoch's mean: the model's, from the dry run's rows
    assert s[12] == F64(F32(seq[-1]))
    a.close(), b.close()


# ---- 2: the first record, inside epoch 0 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", ["small-4", "words-17", "words-4"])
def test_a_stop_at_the_first_record_inside_epoch_0(config):
    rec = dry(config)[2]
    per_epoch = len(tm.minibatches(np.prod(SHAPES[CONFIGS[config][0]][3:]), CONFIGS[config][2]))
    assert 1 <= rec[1] < per_epoch, (config, rec)
    s = check_stop(config, config, rec[1])
    assert s[10] == 1.0


# ---- 3: a record in a later epoch ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", ["small-4", "words-17", "words-4", "long"])
def test_a_stop_at_a_record_in_a_later_epoch(config):
    per, seq, rec = dry(config)
    per_epoch = len(per) // EPOCHS
    later = [r for r in rec if r >= per_epoch]
    assert later, (config, rec)
    r = later[-1] if later[-1] < len(per) - 1 or len(later) == 1 else later[-2]  # (not the call's last minibatch when there is a choice)
    s = check_stop(config, config, r)
    e0 = r // per_epoch * per_epoch
    assert s[10] == r // per_epoch + 1 >= 2
    # [13]: the mean over the last epoch entered alone; [3] averages over every minibatch that ran
    want13 = F64(0.0)
    for x in seq[e0:r + 1]:
        want13 = want13 + F64(F32(x))
    assert same64(s[13], want13 / F64(r + 1 - e0)) and s[13] != s[3]


# ---- 4: the last minibatch of the call -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", ["small-17", "long"])
def test_a_stop_on_the_last_minibatch_of_the_call_is_folded_by_the_closing_launch(config):
    """One minibatch per epoch: a call of r + 1 epochs ends on the record r, and no minibatch launch comes behind it."""
    per, _, rec = dry(config)
    assert len(per) == EPOCHS
    r = rec[-1]
    assert r >= 1
    s = check_stop(config, config, r, n_epochs=r + 1)
    assert s[6] == r + 1 and s[9] == r and s[10] == r + 1 and s[11] == 1.0


# ---- 5: minibatch 0 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", ["small-4", "words-17"])
def test_a_stop_at_minibatch_0_takes_no_step(config):
    a, b = Rig(config), Rig(config)
    a.one_call(target_kl=None, n_epochs=1)  # an ungated update first: the weights have moved off the buffer's policy
    b.one_call(target_kl=None, n_epochs=1)
    before = a.state()
    assert before["step"] == a.per_epoch
    per = b.pieces(target_kl=1e-30, n_epochs=1, first_epoch=1)  # (stops at once: minibatch 0's approx_kl under the moved weights)
    kl0 = float(F64(per[0][4]))
    assert len(per) == 1 and kl0 > 1e-9, kl0
    target = (0.5 * kl0) / 1.5
    got = a.one_call(target_kl=target, first_epoch=1)
    stop, block = b.block(per, target)
    assert stop == 0
    compare(config, got, b.state(), block)
    for k in ("params", "image", "exp_avg", "exp_avg_sq"):
        assert all(pb.same_bits(x, y) for x, y in zip(got[k], before[k])), k  # nothing moved
    s = got["stats"]
    assert got["step"] == before["step"] and s[6] == 1.0 and s[9] == 0.0 and s[10] == 1.0 and s[11] == 1.0 and s[12] == F64(per[0][4])
    assert s[13] == s[12] == s[3]
    a.close(), b.close()


# ---- 6: value clipping and target_kl together ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", ["small-4", "words-17"])
def test_value_clipping_and_target_kl_together(config):
    per, _, rec = dry(config, CV)
    plain = dry(config)[0]
    assert any(not pb.same_bits(x[:4], y[:4]) for x, y in zip(per, plain))  # the clip bites: another value loss
    later = [r for r in rec if r >= len(per) // EPOCHS]
    check_stop(f"{config}+vclip", config, later[0] if later else rec[-1], cv=CV)


# ---- 7: the settlement ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", ["small-4", "words-17"])
def test_the_step_count_is_settled_and_the_next_calls_start_from_it(config):
    per_dry, seq, rec = dry(config)
    r = rec[1]
    target = klm.target_for(seq, r)
    a, b = Rig(config), Rig(config)
    # a stopped call, then the count asked for right away: the base plus the steps taken, not the steps scheduled
    a.train.train(a.params, n_epochs=EPOCHS, batch_size=a.batch_size, clip_range=CLIP, vf_coef=VF, ent_coef=ENT, lr=LR, seed=SEED, first_epoch=0,
                  target_kl=target)
    assert a.adam.describe()["step"] == r < EPOCHS * a.per_epoch
    assert len(b.pieces(target_kl=target)) == r + 1 and b.adam.describe()["step"] == r
    # an ungated update right behind it on the same handles: its bias corrections use the settled count
    got = a.one_call(target_kl=None, n_epochs=1, first_epoch=EPOCHS)
    per = b.pieces(n_epochs=1, first_epoch=EPOCHS)
    want = b.state()
    compare(config + " ungated behind a stop", got, want, np.concatenate([b.block(per, None)[1][:9], np.zeros(7)]))
    assert got["step"] == r + a.per_epoch
    # a stopped call (no host read between), then a gated one that never triggers: the first launch clears the control record
    a.train.train(a.params, n_epochs=1, batch_size=a.batch_size, clip_range=CLIP, vf_coef=VF, ent_coef=ENT, lr=LR, seed=SEED, first_epoch=EPOCHS + 1,
                  target_kl=1e-30)
    per_stop = b.pieces(target_kl=1e-30, n_epochs=1, first_epoch=EPOCHS + 1)
    assert len(per_stop) == 1
    got = a.one_call(target_kl=NEVER, n_epochs=2, first_epoch=EPOCHS + 2)
    per = b.pieces(target_kl=NEVER, n_epochs=2, first_epoch=EPOCHS + 2)
    stop, block = b.block(per, NEVER)
    assert stop is None and block[9] == 2 * a.per_epoch and block[11] == 0.0
    compare(config + " gated behind a stop", got, b.state(), block)
    assert got["step"] == r + a.per_epoch + 2 * a.per_epoch
    a.close(), b.close()


# ---- 8: target_kl=None is the existing call ------------------------------------------------------------------------------------------
def test_target_kl_none_is_the_existing_update_bit_for_bit():
    from fleetrl_amd import _capi

    a, b = Rig("words-17"), Rig("words-17")
    got = a.one_call(target_kl=None)
    x = _capi.FleetTrainPpoArgs()
    x.n_epochs, x.batch_size, x.normalize_advantage, x.clip_range, x.vf_coef, x.ent_coef, x.lr = EPOCHS, 17, 1, CLIP, VF, ENT, LR
    x.beta1, x.beta2, x.eps, x.max_grad_norm, x.seed, x.first_epoch = 0.9, 0.999, EPS, MAXN, SEED, 0
    stats = torch.full((16,), float("nan"), device=dev(), dtype=torch.float64)
    x.stats = stats.data_ptr()
    b.train.use_torch_stream()
    grads = b.train._grad_pointers("train", b.params, b.train._shapes, "the actor's then the critic's, then log_std")
    b.train.train_dev(x, b.train._param_pointers(b.params), grads, len(b.params))
    want = b.state(stats)
    for k in ("params", "image", "exp_avg", "exp_avg_sq", "grads"):
        assert all(pb.same_bits(p, q) for p, q in zip(got[k], want[k])), k
    assert got["step"] == want["step"] == EPOCHS * a.per_epoch and same64(got["stats"], want["stats"]) and not got["stats"][9:].any()
    a.close(), b.close()


# ---- 9: refusals that need the handle ------------------------------------------------------------------------------------------------
def test_a_minibatch_above_max_batch_launches_nothing_and_leaves_the_step_count():
    from fleetrl_amd import FleetHipError

    rig = Rig("small-4")
    before = rig.state()
    with pytest.raises(FleetHipError, match="fleet_train_ppo_kl_dev: a minibatch of 9 rows: B must be at most max_batch = 8, got 9"):
        rig.one_call(target_kl=0.01, batch_size=9)
    for bad in (0.0, -0.01, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="`target_kl` must be positive and finite"):
            rig.one_call(target_kl=bad)
    after = rig.state()
    assert after["step"] == 0 and all(pb.same_bits(x, y) for x, y in zip(after["params"], before["params"]))  # nothing was launched
    assert rig.one_call(target_kl=NEVER)["step"] == EPOCHS * rig.per_epoch
    rig.close()


def test_a_capturing_stream_is_refused_and_nothing_is_launched():
    """The gated call settles the step count through an event: FLEET_ERR_STATE when the policy's stream is capturing a graph."""
    import warnings

    from fleetrl_amd import FleetHipError, _capi

    rig = Rig("small-4")
    before = rig.state()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        rig.train.use_torch_stream()  # (moving the handles to the stream waits for the old one: before the capture begins)
        torch.cuda.synchronize()
        stats = torch.zeros(16, device=dev(), dtype=torch.float64)
        graph, err = torch.cuda.CUDAGraph(), None
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # (torch warns that the captured graph is empty: it is meant to be)
            with torch.cuda.graph(graph, stream=side, capture_error_mode="relaxed"):
                try:
                    rig.train.train(rig.params, n_epochs=1, batch_size=4, clip_range=CLIP, vf_coef=VF, ent_coef=ENT, lr=LR, seed=SEED, first_epoch=0,
                                    stats_out=stats, target_kl=0.01)
                except FleetHipError as e:
                    err = e
    torch.cuda.synchronize()
    assert err is not None and err.status == _capi.ERR_STATE
    assert "fleet_train_ppo_kl_dev: the policy's stream is capturing a graph" in str(err)
    after = rig.state()
    assert after["step"] == 0 and all(pb.same_bits(x, y) for x, y in zip(after["params"], before["params"])) and not host(stats).any()
    assert rig.one_call(target_kl=NEVER)["step"] == EPOCHS * rig.per_epoch  # the handle goes on working
    rig.close()


# ---- 10: the pieces' wrappers --------------------------------------------------------------------------------------------------------
def test_the_gated_step_and_the_gated_gradients_one_by_one():
    a, b = Rig("words-17"), Rig("words-17")
    word = lambda v: torch.full((1,), v, device=dev(), dtype=torch.int32)  # noqa: E731
    idx = tm.indices(a.n, SEED, 0)[:17]
    for rig in (a, b):  # one plain step each: the weights move off the buffer's policy, approx_kl > 0 from here on
        batch = rig.buf.gather(on_device(idx))
        rig.grad.grad(batch, rig.params[-1], CLIP, VF, ENT, into=rig.params)
        rig.adam.step()
    before = a.state()
    # the step: a set word changes nothing but the host's scheduled count, which settle() then puts right
    norm = torch.full((1,), float("nan"), device=dev())
    a.adam.step(skip=word(1), norm_out=norm)
    after = a.state()
    for k in ("params", "image", "exp_avg", "exp_avg_sq"):
        assert all(pb.same_bits(x, y) for x, y in zip(after[k], before[k])), k
    assert np.isnan(host(norm)).all() and after["step"] == before["step"] + 1
    a.adam.settle(before["step"], word(0))
    assert a.adam.describe()["step"] == before["step"]
    # a clear word: step()'s bits
    na, nb = torch.zeros(1, device=dev()), torch.zeros(1, device=dev())
    a.adam.step(skip=word(0), norm_out=na)
    b.adam.step(norm_out=nb)
    x, y = a.state(), b.state()
    for k in ("params", "image", "exp_avg", "exp_avg_sq"):
        assert all(pb.same_bits(p, q) for p, q in zip(x[k], y[k])), k
    assert x["step"] == y["step"] == before["step"] + 1 and pb.same_bits(host(na), host(nb))
    assert not all(pb.same_bits(p, q) for p, q in zip(x["params"], before["params"]))
    # the gradients: decided is the host's comparison on both sides of a threshold; a set skip word leaves everything as it was
    batch = b.buf.gather(on_device(idx))
    ref = host(b.grad.grad(batch, b.params[-1], CLIP, VF, ENT, into=b.params))
    kl = F64(ref[4])
    assert kl > 1e-9
    for cv in (None, CV):
        ref = host(b.grad.grad(batch, b.params[-1], CLIP, VF, ENT, into=b.params, clip_range_vf=cv))
        want = [host(p.grad) for p in b.params]
        for thr, expect in ((0.5 * kl, 1), (2.0 * kl, 0), (kl, 0)):  # (equal does not stop)
            decided = word(7)
            s = a.grad.grad(a.buf.gather(on_device(idx)), a.params[-1], CLIP, VF, ENT, into=a.params, clip_range_vf=cv, gate=(word(0), decided, thr))
            assert pb.same_bits(host(s), ref) and int(host(decided)[0]) == expect == int(klm.stops(ref[4], thr))
            assert all(pb.same_bits(host(p.grad), g) for p, g in zip(a.params, want))
    stats, decided = torch.full((8,), float("nan"), device=dev()), word(7)
    for p in a.params:
        p.grad.fill_(3.0)
    a.grad.grad(a.buf.gather(on_device(idx)), a.params[-1], CLIP, VF, ENT, into=a.params, stats_out=stats, gate=(word(1), decided, 0.0))
    assert np.isnan(host(stats)).all() and int(host(decided)[0]) == 7 and all((host(p.grad) == 3.0).all() for p in a.params)
    a.close(), b.close()


# ---- 11: the example -----------------------------------------------------------------------------------------------------------------
def test_the_example_runs_with_target_kl_and_prints_the_new_statistics():
    """examples/ppo_device_train.py as a child process under a time limit of its own: exit 0, finite train/* values, the new fields."""
    from fleetrl_amd.train import KL_SB3_NAMES, SB3_NAMES

    cmd = ["timeout", "-k", "10", "240", sys.executable, os.path.join(tm.ROOT, "examples", "ppo_device_train.py"), "--target-kl", "0.002",
           "--iterations", "2", "--epochs", "6"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 2
    for d in lines:
        for k in SB3_NAMES + KL_SB3_NAMES:
            assert np.isfinite(d[k]), (k, d)
        assert 1 <= d["train/epochs"] <= 6 and d["train/early_stop"] in (0.0, 1.0) and d["train/optimizer_steps"] >= 0
        if d["train/early_stop"]:
            assert d["train/last_approx_kl"] > 1.5 * 0.002
    assert lines[-1]["train/n_updates"] > lines[0]["train/n_updates"] > 0
