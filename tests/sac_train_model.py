"""Restatement of include/fleet_hip.h "SAC's whole update on the device" (fleet_sactrain_*, fleetrl_amd/csrc/fleet_sactrain.hip) for the
tests: which gradient steps of a call move the targets, the closing launch's statistics block from the per-step slots, the alpha
launch's value, SB3's whole `SAC.train` loop under autograd with the target-update schedule (and two misreadings of it), the case table
of tests/test_sac_train_gpu.py and -- for the GPU tests -- one complete set of handles on small random networks, with the update's
pieces run one by one as `fleetrl_amd.sac.gradient_step` runs them."""
import numpy as np

import sac_grad_model as gm
import sb3_update_ref as ur
import train_model as tm

ROOT = tm.ROOT
F32, F64 = np.float32, np.float64
LANES = tm.LANES                 # fleet_offpolicy.h: kOffpolicyThreads
SLOT, ACTOR_AT = 16, 8           # kOffpolicySlot, kOffpolicyActorAt
MAX_STEPS, SCALE_CHUNK = 65536, 1024
STATS_LEN = tm.STATS_LEN
SAC_TRAIN_STATS = ("critic_loss", "actor_loss", "ent_coef", "ent_coef_loss", "last_critic_loss", "last_actor_loss", "n_updates",
                   "target_updates", "log_prob_mean", "qmin_mean")
MUTANTS = ("polyak_on_update_count", "alpha_after_its_step")


# ---- the schedule, the alpha launch, the closing launch ------------------------------------------------------------------------------
def target_steps(G: int, interval: int) -> list:
    """The steps g of a call of G gradient steps that move the targets: g % interval == 0, g the index INSIDE the call."""
    return [g for g in range(G) if g % interval == 0]


def target_updates(G: int, interval: int) -> int:
    """The header's count: (G - 1) / interval + 1."""
    return (G - 1) // interval + 1


def alpha32(x) -> np.float32:
    """(float)exp((double)x): the double exponential rounded once."""
    return F32(np.exp(F64(F32(x))))


def finish(slots, first_update: int, interval: int, loss_scale: float = 0.5, learned: bool = True) -> np.ndarray:
    """The statistics block f64[16] of a call from its slots f32[G, 16] (the critic launch's stats f32[8], then the actor launch's):
    the header's ordered sum S (train_model.tree_sum) over the G slots."""
    slots = np.asarray(slots, dtype=F32).reshape(-1, SLOT)
    G = slots.shape[0]
    S = lambda k: tm.tree_sum(slots[:, k].astype(F64))  # noqa: E731
    s = F64(F32(loss_scale))
    out = np.zeros(STATS_LEN, F64)
    out[0] = s * S(0) / F64(G)
    out[1] = S(ACTOR_AT) / F64(G)
    out[2] = S(ACTOR_AT + 4) / F64(G)
    out[3] = S(ACTOR_AT + 1) / F64(G) if learned else np.nan
    out[4] = s * F64(slots[G - 1, 0])
    out[5] = F64(slots[G - 1, ACTOR_AT])
    out[6] = F64(first_update + G)
    out[7] = F64(target_updates(G, interval))
    out[8] = S(ACTOR_AT + 2) / F64(G)
    out[9] = S(ACTOR_AT + 3) / F64(G)
    return out


# ---- SB3's loop under autograd, with the schedule -------------------------------------------------------------------------------------
def sac_train_reference(actor, critics, target_actor, target_critics, batches, noise, target_noise, *, activation, dtype="float64", gamma, tau,
                        lr, interval=1, first_update=0, loss_scale=0.5, log_ent_coef=None, ent_coef=None, target_entropy=None, adam_eps=1e-8,
                        mutant=None) -> dict:
    """`sac_grad_model.sac_gradient_steps` -- SB3 2.3.2's `SAC.train` under autograd and `torch.optim.Adam`, one gradient step per batch
    -- extended by the target-update schedule `g % interval == 0` and `loss_scale`.  mutant: "polyak_on_update_count" tests
    (first_update + g + 1) % interval (TD3's rule); "alpha_after_its_step" reads alpha behind the entropy coefficient's optimiser step."""
    import torch
    import torch.nn.functional as F

    assert mutant in (None, *MUTANTS)
    dt = getattr(torch, dtype)
    log = ur.KinkLog()
    pa, ta = ur._params(actor, dt), ur._params(target_actor, dt)
    pc, tc = [ur._params(c, dt) for c in critics], [ur._params(c, dt) for c in target_critics]
    flat = lambda nets: [p for net in nets for p in net]  # noqa: E731
    opt_a, opt_c = torch.optim.Adam(pa, lr=lr, eps=adam_eps), torch.optim.Adam(flat(pc), lr=lr, eps=adam_eps)
    A = np.asarray(actor[-1][0]).shape[0] // 2
    te = -float(A) if target_entropy is None else float(target_entropy)
    lec, opt_e = None, None
    if log_ent_coef is not None:
        lec = torch.tensor([float(log_ent_coef)], dtype=dt, requires_grad=True)
        opt_e = torch.optim.Adam([lec], lr=lr, eps=adam_eps)
    qf = lambda ps, x, a: ur._mlp(ps, torch.cat([x, a], dim=1), activation, log, False)  # noqa: E731

    def action_log_prob(x, e):
        out = ur._mlp(pa, x, activation, log, False)
        mean_actions, raw = out[:, :A], out[:, A:]
        log.add("log_std_clamp", torch.cat([raw - ur.LOG_STD_MIN, raw - ur.LOG_STD_MAX]))
        std = torch.exp(torch.clamp(raw, ur.LOG_STD_MIN, ur.LOG_STD_MAX))
        u = mean_actions + std * e
        a = torch.tanh(u)
        return a, torch.distributions.Normal(mean_actions, std).log_prob(u).sum(dim=1) - torch.sum(torch.log(1 - a ** 2 + 1e-6), dim=1)

    stats = {k: [] for k in ("alphas", "actor_losses", "critic_losses", "ent_coef_losses", "updated")}
    for g, (b, e_pi, e_t) in enumerate(zip(batches, noise, target_noise)):
        obs, actions, next_obs, dones, rewards = ur._batch(b, dt, False)
        actions_pi, log_prob = action_log_prob(obs, ur._tensor(e_pi, dt))
        log_prob = log_prob.reshape(-1, 1)
        if lec is not None:
            alpha = torch.exp(lec.detach())
            ent_coef_loss = -(lec * (log_prob + te).detach()).mean()
            stats["ent_coef_losses"].append(ent_coef_loss.item())
            opt_e.zero_grad()
            ent_coef_loss.backward()
            opt_e.step()
            if mutant == "alpha_after_its_step":
                alpha = torch.exp(lec.detach())
        else:
            alpha = torch.tensor([float(ent_coef)], dtype=torch.float32).to(dt)  # the device keeps alpha in float32
        stats["alphas"].append(float(alpha))
        with torch.no_grad():
            next_actions, next_log_prob = action_log_prob(next_obs, ur._tensor(e_t, dt))
            next_q = torch.cat([qf(t, next_obs, next_actions) for t in tc], dim=1)
            if len(tc) == 2:
                log.add("q_min", next_q[:, 0] - next_q[:, 1])
            next_q, _ = torch.min(next_q, dim=1, keepdim=True)
            next_q = next_q - alpha * next_log_prob.reshape(-1, 1)
            target_q = rewards + (1 - dones) * gamma * next_q
        critic_loss = loss_scale * sum(F.mse_loss(qf(c, obs, actions), target_q) for c in pc)
        stats["critic_losses"].append(critic_loss.item())
        opt_c.zero_grad()
        critic_loss.backward()
        opt_c.step()
        q_pi = torch.cat([qf(c, obs, actions_pi) for c in pc], dim=1)
        if len(pc) == 2:
            log.add("q_min", q_pi[:, 0] - q_pi[:, 1])
        min_qf_pi, _ = torch.min(q_pi, dim=1, keepdim=True)
        actor_loss = (alpha * log_prob - min_qf_pi).mean()
        stats["actor_losses"].append(actor_loss.item())
        opt_a.zero_grad()
        actor_loss.backward()
        opt_a.step()
        hit = (first_update + g + 1) % interval == 0 if mutant == "polyak_on_update_count" else g % interval == 0
        stats["updated"].append(bool(hit))
        if hit:
            ur._polyak(flat(pc), flat(tc), tau)
            ur._polyak(pa, ta, tau)
    out = {"actor": ur._np(pa), "critics": ur._np(flat(pc)), "target_actor": ur._np(ta), "target_critics": ur._np(flat(tc)),
           "actor_opt": ur._adam_state(opt_a, pa), "critic_opt": ur._adam_state(opt_c, flat(pc)), "kinks": log, "stats": stats}
    if lec is not None:
        out["log_ent_coef"], out["ent_opt"] = ur._np([lec]), ur._adam_state(opt_e, [lec])
    return out


TENSOR_CLASSES = ("actor", "critics", "target_actor", "target_critics", "log_ent_coef")
OPTIMISERS = ("actor_opt", "critic_opt", "ent_opt")


def class_ratios(got, ref64, ref32) -> dict:
    """tensor class -> the worst error / bound (`sac_grad_model.ratio`: |got - ref64| over 8 max(max|ref32 - ref64|, 2^-24 max|ref64|) per
    tensor).  got: lists of arrays per class, and {"exp_avg", "exp_avg_sq"} per optimiser, as the reference has them."""
    worst = {k: max(gm.ratio(t, a, b) for t, a, b in zip(got[k], ref64[k], ref32[k])) for k in TENSOR_CLASSES if k in got}
    for k in OPTIMISERS:
        if k in got:
            for mom in ("exp_avg", "exp_avg_sq"):
                worst[f"{k}.{mom}"] = max(gm.ratio(t, a, b) for t, a, b in zip(got[k][mom], ref64[k][mom], ref32[k][mom]))
    return worst


# the float64 parity of the whole call: the two shapes of tests/test_sac_grad_gpu.py's whole-step test
PARITY_SHAPES = {"7-64-64-A5-relu": dict(D=7, A=5, hidden=(64, 64), activation="relu", n_critics=2, B=33, learned=True, given=False, bias=None),
                 "131-130-70-A65-tanh": dict(D=131, A=65, hidden=(130, 70), activation="tanh", n_critics=2, B=17, learned=True, given=False, bias=-1.0)}
PARITY = dict(G=4, interval=2, gamma=0.99, tau=0.005, lr=3e-4)


def parity_inputs(shape, salt) -> dict:
    """The networks of a parity case under `salt` (`sac_grad_model.make`), target critics a little off the online ones, and the ring's
    contents: E = 3 envs, R = 11 rows."""
    c = gm.make(shape, salt, PARITY_SHAPES[shape])
    rng = np.random.default_rng(gm.seed(shape, 2000 + salt))
    c["target_critics"] = [[(w + 0.01 * rng.standard_normal(w.shape).astype(F32), b) for w, b in net] for net in c["critics"]]
    E, R, D, A = 3, 11, c["D"], c["A"]
    c["ring"] = {"observations": np.clip(rng.standard_normal((R, E, D)), -3, 3).astype(F32),
                 "next_observations": np.clip(rng.standard_normal((R, E, D)), -3, 3).astype(F32),
                 "actions": rng.uniform(-1, 1, (R, E, A)).astype(F32), "rewards": rng.standard_normal((R, E)).astype(F32),
                 "dones": (rng.random((R, E)) < 0.2).astype(np.uint8), "timeouts": np.zeros((R, E), np.uint8)}
    c["E"], c["R"] = E, R
    return c


# ---- the equivalence cases of tests/test_sac_train_gpu.py ------------------------------------------------------------------------------
SEED, TARGET_SEED = 0x5AC7A1, 0x7A26E7
BASE = dict(G=5, B=4, interval=1, first_update=0, seed=SEED, target_seed=TARGET_SEED)
WIDE = dict(D=131, A=65, hidden=(130, 70))
EQUIVALENCE = {
    "interval-1": (dict(), BASE),
    "interval-2": (dict(), dict(BASE, interval=2)),
    "interval-3": (dict(), dict(BASE, interval=3)),
    "one-step": (dict(), dict(BASE, G=1)),
    "max-steps": (dict(max_steps=8), dict(BASE, G=8, interval=3)),
    "fixed-alpha": (dict(learned=False), dict(BASE, interval=2)),
    "one-critic": (dict(n_critics=1), BASE),
    "batch-1": (dict(), dict(BASE, B=1)),
    "batch-4": (dict(), dict(BASE, B=4, interval=2)),
    "batch-tile-plus-1": (dict(max_batch=32), dict(BASE, B=17)),
    "ring-partly-filled": (dict(pos=4, full=False), BASE),
    "ring-wrapped": (dict(pos=4, full=True), BASE),
    "tanh": (dict(activation="tanh"), BASE),
    "131-130-70-A65": (dict(max_batch=32, **WIDE), dict(BASE, G=3, B=17, interval=2)),
    "normalised": (dict(with_norm=True), BASE),
    "loss-scale-1": (dict(), dict(BASE, loss_scale=1.0)),
    "first-update-3": (dict(), dict(BASE, first_update=3, interval=2)),
}


# ---- the GPU tests' handles ------------------------------------------------------------------------------------------------------------
def networks(D, A, hidden, n_critics, seed):
    """[(W, b), ...] of a squashed-Gaussian actor over D columns (last width 2A: mu rows, then log_std rows with a bias of -1) and
    n_critics critics over D + A, float32, drawn from `seed`."""
    rng = np.random.default_rng(seed)

    def net(sizes):
        return [((rng.standard_normal((o, i)) / np.sqrt(i)).astype(F32), (0.1 * rng.standard_normal(o)).astype(F32))
                for i, o in zip(sizes[:-1], sizes[1:])]

    actor = net([D, *hidden, 2 * A])
    w, b = actor[-1]
    b = b.copy()
    b[A:] -= F32(1.0)
    actor[-1] = ((0.5 * w).astype(F32), b)
    return actor, [net([D + A, *hidden, 1]) for _ in range(n_critics)]


def contents(E, R, D, A, seed):
    """(the replay ring's six arrays, float32 / uint8, and the generator behind them, for what follows)."""
    rng = np.random.default_rng(seed + 1000)
    out = {"observations": rng.standard_normal((R, E, D)).astype(F32), "next_observations": rng.standard_normal((R, E, D)).astype(F32),
           "actions": rng.uniform(-1, 1, (R, E, A)).astype(F32), "rewards": rng.standard_normal((R, E)).astype(F32)}
    out["dones"] = (rng.random((R, E)) < 0.3).astype(np.uint8)
    out["timeouts"] = (out["dones"] * (rng.random((R, E)) < 0.5)).astype(np.uint8)
    return out, rng


class Stack:
    """Every handle of one SAC agent on random networks and a replay ring of R rows of E envs filled from `seed`; two Stacks from the
    same arguments start from the same bits."""

    def __init__(self, *, E=3, R=7, D=5, A=3, hidden=(8, 8), n_critics=2, activation="relu", seed=1, pos=0, full=True, max_batch=16,
                 max_steps=8, with_norm=False, lr=1e-3, learned=True, nets=None, ring=None):
        import torch
        from fleetrl_amd import DeviceAdam, DeviceNormalizer, DeviceReplayBuffer, DeviceSACGrad, DeviceSACNetworks, DeviceSACTrain

        dev = torch.device("cuda", 0)
        self.dev, self.E, self.R, self.D, self.A, self.n_critics, self.learned = dev, E, R, D, A, n_critics, learned
        actor, critics, t_critics = nets if nets is not None else (*networks(D, A, hidden, n_critics, seed), None)
        self.online = DeviceSACNetworks(actor, critics, activation=activation)
        self.targets = DeviceSACNetworks(actor, critics if t_critics is None else t_critics, activation=activation)
        leaf = lambda a: torch.from_numpy(np.array(a, F32)).to(dev).requires_grad_(True)  # noqa: E731
        self.actor_params = [leaf(a) for pair in actor for a in pair]
        self.critic_params = [leaf(a) for c in critics for pair in c for a in pair]
        self.grad = DeviceSACGrad(self.online, max_batch)
        self.opt_a = DeviceAdam(self.online, self.actor_params, nets="actor", lr=lr)
        self.opt_c = DeviceAdam(self.online, self.critic_params, nets="critic", lr=lr)
        self.log_ent_coef, self.opt_e, self.ent_coef = None, None, None
        if learned:
            self.log_ent_coef = torch.full((1,), float(np.log(F32(0.2))), device=dev, requires_grad=True)
            self.opt_e = DeviceAdam(self.online, [self.log_ent_coef], nets="none", lr=lr)
        else:
            self.ent_coef = torch.full((1,), 0.2, device=dev)
        self.buf = DeviceReplayBuffer(R * E, E, D, A, seed=seed + 77)
        arrays, rng = contents(E, R, D, A, seed) if ring is None else (ring, np.random.default_rng(seed + 5))
        for name, a in arrays.items():
            getattr(self.buf, name).copy_(torch.from_numpy(a).to(dev))
        self.buf.set_position(pos, full, 0)
        self.env = None
        if with_norm:
            self.env = DeviceNormalizer(E, D)
            self.env.reset_torch(torch.from_numpy((rng.standard_normal((E, D)) * 2 + 1).astype(F32)).to(dev))
            for _ in range(2):  # the statistics of two random batches
                self.env.step_torch(torch.from_numpy((rng.standard_normal((E, D)) * 3 - 1).astype(F32)).to(dev),
                                    torch.from_numpy(rng.standard_normal(E)).to(dev), torch.zeros(E, dtype=torch.uint8, device=dev))
        self.train = DeviceSACTrain(self.buf, self.targets, self.grad, self.opt_a, self.opt_c, self.opt_e, max_steps=max_steps)
        self.critic_stats, self.actor_stats = torch.zeros(8, device=dev), torch.zeros(8, device=dev)
        self.alpha = torch.zeros(1, device=dev)

    @property
    def online_params(self):
        return [*self.actor_params, *self.critic_params]

    def step_by_step(self, *, G, B, interval, first_update, seed, target_seed, gamma=0.99, tau=0.005, loss_scale=0.5):
        """The update's pieces one by one, composed from the public ones: `train.alpha`, `critic_update` (with its `torch._foreach_mul_`),
        `actor_update`, `targets.polyak` on the steps the schedule names; returns the per-step slots f32[G, 16]."""
        from fleetrl_amd.sac import actor_update, critic_update

        slots = np.zeros((G, SLOT), F32)
        hits = target_steps(G, interval)
        for g in range(G):
            u = first_update + g
            b = self.buf.sample(B, env=self.env)
            alpha = self.train.alpha(self.log_ent_coef, out=self.alpha) if self.learned else self.ent_coef
            critic_update(self.online, self.targets, self.grad, self.opt_c, b, self.critic_params, gamma=gamma, ent_coef=alpha,
                          seed=target_seed, step=u, stats_out=self.critic_stats, loss_scale=loss_scale)
            actor_update(self.grad, self.opt_a, b.observations, self.actor_params, ent_coef=alpha, seed=seed, step=u,
                         log_ent_coef=self.log_ent_coef, ent_adam=self.opt_e, stats_out=self.actor_stats)
            if g in hits:
                self.targets.polyak(self.online_params, tau)
            slots[g, :8] = self.critic_stats.cpu().numpy()
            slots[g, 8:] = self.actor_stats.cpu().numpy()
        return slots

    def one_call(self, *, G, B, interval, first_update, seed, target_seed, gamma=0.99, tau=0.005, loss_scale=0.5, stats_out=None):
        return self.train.train(self.actor_params, self.critic_params, gradient_steps=G, batch_size=B, gamma=gamma, tau=tau, lr=self.opt_c.lr,
                                seed=seed, target_seed=target_seed, first_update=first_update, target_update_interval=interval,
                                ent_coef=self.ent_coef, log_ent_coef=self.log_ent_coef, loss_scale=loss_scale, env=self.env,
                                stats_out=stats_out)

    def state(self) -> dict:
        """Everything an update may change, as host arrays: the parameters and their .grad, both images, log_ent_coef and its .grad, the
        three optimisers' states and step counts, the replay buffer's call counter."""
        h = lambda t: t.detach().cpu().numpy().copy()  # noqa: E731
        out = {"params": [h(p) for p in self.online_params],
               "grads": [None if p.grad is None else h(p.grad) for p in self.online_params],
               "online_image": [h(t) for t in self.opt_c.export_image()], "online_export": [h(t) for t in self.online.export_torch()],
               "target_image": [h(t) for t in self.targets.export_torch()], "calls": self.buf.calls}
        opts = [("actor", self.opt_a), ("critic", self.opt_c)]
        if self.learned:
            opts.append(("ent", self.opt_e))
            out["log_ent_coef"] = [h(self.log_ent_coef)]
            out["log_ent_coef_grad"] = [None if self.log_ent_coef.grad is None else h(self.log_ent_coef.grad)]
        for name, opt in opts:
            sd = opt.state_dict()["state"]
            out[name + "_m"] = [h(sd[i]["exp_avg"]) for i in range(len(sd))]
            out[name + "_v"] = [h(sd[i]["exp_avg_sq"]) for i in range(len(sd))]
            out[name + "_step"] = opt.describe()["step"]
        return out

    def close(self):
        for x in (self.train, self.opt_e, self.opt_a, self.opt_c, self.grad, self.online, self.targets, self.buf, self.env):
            if x is not None:
                x.close()


def same_state(a: dict, b: dict) -> list:
    """The keys in which two `Stack.state()`s differ in any bit.  A `.grad` that one of the two never allocated is passed over."""
    bad = []
    for k in a:
        x, y = a[k], b[k]
        if isinstance(x, list):
            if len(x) != len(y) or any(p is not None and q is not None and (p.shape != q.shape or p.tobytes() != q.tobytes()) for p, q in zip(x, y)):
                bad.append(k)
        elif x != y:
            bad.append(k)
    return bad
