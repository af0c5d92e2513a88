"""Restatement of include/fleet_hip.h "TD3 / DDPG's whole update on the device" (fleet_offpolicy_*, fleetrl_amd/csrc/fleet_offpolicy.hip)
for the tests: which gradient steps of a call are actor steps, the closing launch's statistics block from the per-step slots, and -- for
the GPU tests -- one complete set of handles (replay buffer, targets, online image, gradient handle, two optimisers, the update) on
small random networks, with the update's pieces run one by one as the loop of examples/td3_device_adam.py runs them."""
import numpy as np

import train_model as tm

ROOT = tm.ROOT
F32, F64 = np.float32, np.float64
LANES = tm.LANES                 # fleet_offpolicy.h: kOffpolicyThreads
SLOT, ACTOR_AT = 16, 8           # kOffpolicySlot, kOffpolicyActorAt
MAX_STEPS, MAX_BLOCKS = 65536, 2048
STATS_LEN = tm.STATS_LEN
STATS = ("critic_loss", "critic_0_loss", "critic_1_loss", "actor_loss", "last_critic_loss", "last_actor_loss", "n_updates", "actor_steps")


def actor_steps(first_update: int, G: int, delay: int) -> list:
    """The header's lines: g_0 = (delay - (first_update % delay + 1) % delay) % delay; g_j = g_0 + j * delay, while below G."""
    g0 = (delay - (first_update % delay + 1) % delay) % delay
    n = (G - 1 - g0) // delay + 1 if g0 < G else 0
    return [g0 + j * delay for j in range(n)]


def finish(slots, first_update: int, delay: int) -> np.ndarray:
    """The statistics block f64[16] of a call from its slots f32[G, 16] (the critic launch's stats f32[8], then the actor launch's):
    the header's ordered sum S (train_model.tree_sum) over the G slots, and over the actor steps' in ascending order."""
    slots = np.asarray(slots, dtype=F32).reshape(-1, SLOT)
    G = slots.shape[0]
    steps = actor_steps(first_update, G, delay)
    out = np.zeros(STATS_LEN, F64)
    for k in range(3):
        out[k] = tm.tree_sum(slots[:, k].astype(F64)) / F64(G)
    if steps:
        out[3] = tm.tree_sum(slots[steps, ACTOR_AT].astype(F64)) / F64(len(steps))
        out[5] = F64(slots[steps[-1], ACTOR_AT])
    else:
        out[3] = out[5] = np.nan
    out[4] = F64(slots[G - 1, 0])
    out[6] = F64(first_update + G)
    out[7] = F64(len(steps))
    return out


# ---- the GPU tests' handles ------------------------------------------------------------------------------------------------------------
def networks(D, A, hidden, n_critics, seed):
    """[(W, b), ...] of an actor over D columns and n_critics critics over D + A, float32, drawn from `seed`."""
    rng = np.random.default_rng(seed)

    def net(sizes):
        return [((rng.standard_normal((o, i)) / np.sqrt(i)).astype(F32), (0.1 * rng.standard_normal(o)).astype(F32))
                for i, o in zip(sizes[:-1], sizes[1:])]

    return net([D, *hidden, A]), [net([D + A, *hidden, 1]) for _ in range(n_critics)]


def contents(E, R, D, A, seed):
    """(the replay ring's six arrays as `Stack` fills them, float32 / uint8, and the generator behind them, for what follows)."""
    rng = np.random.default_rng(seed + 1000)
    out = {"observations": rng.standard_normal((R, E, D)).astype(F32), "next_observations": rng.standard_normal((R, E, D)).astype(F32),
           "actions": rng.uniform(-1, 1, (R, E, A)).astype(F32), "rewards": rng.standard_normal((R, E)).astype(F32)}
    out["dones"] = (rng.random((R, E)) < 0.3).astype(np.uint8)
    out["timeouts"] = (out["dones"] * (rng.random((R, E)) < 0.5)).astype(np.uint8)
    return out, rng


class Stack:
    """Every handle of one TD3 / DDPG agent on random networks and a replay ring of R rows of E envs filled from `seed`; two Stacks
    from the same arguments start from the same bits."""

    def __init__(self, *, E=3, R=7, D=5, A=3, hidden=(8, 8), n_critics=2, activation="relu", seed=1, pos=0, full=True, max_batch=16,
                 max_steps=8, with_norm=False, lr=1e-3):
        import torch
        from fleetrl_amd import DeviceAdam, DeviceNormalizer, DeviceReplayBuffer, DeviceTD3Grad, DeviceTD3Target, DeviceTD3Train

        dev = torch.device("cuda", 0)
        self.dev, self.E, self.R, self.D, self.A, self.n_critics = dev, E, R, D, A, n_critics
        actor, critics = networks(D, A, hidden, n_critics, seed)
        mk = lambda: DeviceTD3Target(actor, critics, activation=activation, output="tanh")  # noqa: E731
        self.targets, self.online = mk(), mk()
        self.actor_params = [torch.nn.Parameter(torch.from_numpy(a.copy()).to(dev)) for pair in actor for a in pair]
        self.critic_params = [torch.nn.Parameter(torch.from_numpy(a.copy()).to(dev)) for c in critics for pair in c for a in pair]
        self.grad = DeviceTD3Grad(self.online, max_batch)
        self.opt_a = DeviceAdam(self.online, self.actor_params, nets="actor", lr=lr)
        self.opt_c = DeviceAdam(self.online, self.critic_params, nets="critic", lr=lr)
        self.buf = DeviceReplayBuffer(R * E, E, D, A, seed=seed + 77)
        arrays, rng = contents(E, R, D, A, seed)
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
        self.train = DeviceTD3Train(self.buf, self.targets, self.grad, self.opt_a, self.opt_c, max_steps=max_steps)
        self.sigma = torch.full((A,), 0.2 if n_critics == 2 else 0.0, device=dev)
        self.critic_stats, self.actor_stats = torch.zeros(8, device=dev), torch.zeros(8, device=dev)

    @property
    def online_params(self):
        return [*self.actor_params, *self.critic_params]

    def step_by_step(self, *, G, B, delay, first_update, seed, gamma=0.99, tau=0.005, noise_clip=0.5, image_polyak=True):
        """The update's pieces one by one; returns the per-step slots f32[G, 16] (the actor half zero where there was no actor step)."""
        slots = np.zeros((G, SLOT), F32)
        for g in range(G):
            u = first_update + g
            b = self.buf.sample(B, env=self.env)
            y = self.targets.target(b.next_observations, b.rewards, b.dones, gamma=gamma, sigma=self.sigma, noise_clip=noise_clip, seed=seed, step=u)
            self.grad.critic_grad(b, y, into=self.critic_params, stats_out=self.critic_stats)
            self.opt_c.step()
            slots[g, :8] = self.critic_stats.cpu().numpy()
            if (u + 1) % delay == 0:
                self.grad.actor_grad(b.observations, into=self.actor_params, stats_out=self.actor_stats)
                self.opt_a.step()
                self.targets.polyak(self.online_params, tau)
                slots[g, 8:] = self.actor_stats.cpu().numpy()
        return slots

    def one_call(self, *, G, B, delay, first_update, seed, gamma=0.99, tau=0.005, noise_clip=0.5, stats_out=None):
        return self.train.train(self.actor_params, self.critic_params, gradient_steps=G, batch_size=B, gamma=gamma, tau=tau, policy_delay=delay,
                                sigma=self.sigma, noise_clip=noise_clip, lr=self.opt_c.lr, seed=seed, first_update=first_update, env=self.env,
                                stats_out=stats_out)

    def state(self) -> dict:
        """Everything an update may change, as host arrays: the parameters and their .grad, both images, both optimisers' states and
        step counts, the replay buffer's call counter."""
        h = lambda t: t.detach().cpu().numpy().copy()  # noqa: E731
        out = {"params": [h(p) for p in self.online_params],
               "grads": [None if p.grad is None else h(p.grad) for p in self.online_params],
               "online_image": [h(t) for t in self.opt_c.export_image()], "online_export": [h(t) for t in self.online.export_torch()],
               "target_image": [h(t) for t in self.targets.export_torch()], "calls": self.buf.calls}
        for name, opt in (("actor", self.opt_a), ("critic", self.opt_c)):
            sd = opt.state_dict()["state"]
            out[name + "_m"] = [h(sd[i]["exp_avg"]) for i in range(len(sd))]
            out[name + "_v"] = [h(sd[i]["exp_avg_sq"]) for i in range(len(sd))]
            out[name + "_step"] = opt.describe()["step"]
        return out

    def close(self):
        for x in (self.train, self.opt_a, self.opt_c, self.grad, self.online, self.targets, self.buf, self.env):
            if x is not None:
                x.close()


def same_state(a: dict, b: dict) -> list:
    """The keys in which two `Stack.state()`s differ in any bit.  A `.grad` that one of the two never allocated is passed over: the
    one call allocates the actor's before its first actor step, the pieces with it."""
    bad = []
    for k in a:
        x, y = a[k], b[k]
        if isinstance(x, list):
            if len(x) != len(y) or any(p is not None and q is not None and (p.shape != q.shape or p.tobytes() != q.tobytes()) for p, q in zip(x, y)):
                bad.append(k)
        elif x != y:
            bad.append(k)
    return bad
