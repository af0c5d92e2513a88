"""The rollout buffer, the replay buffer and the policy forward on arrays of more than 2^32 floats (16 GiB), bit for bit against the
index pattern of tests/large_model.py evaluated in NumPy.  Needs an MI355X.

Every other GPU test stays below 2^31 elements, where an address computed in 32 bits is as good as one computed in 64.  Here an
array is filled with `value(flat index)` through the handle's own torch view, and what a kernel reads (gather, sample, forward) or
writes (add) is compared with `value()` at the index it should have used: rows on both sides of the element offsets 2^30 (a 32-bit
byte offset), 2^31 and 2^32, the low rows a truncated address would meet instead, the first and last row and seeded random ones.
tests/test_large_arrays_cpu.py proves that the pattern differs at every such alias.

What these shapes reach.  The scalar paths (D % 4 != 0) index single floats past 2^32.  The 16-byte paths index 16-byte words, whose
index passes 2^32 only in an array of 64 GiB: at 16 GiB they are covered for byte offsets and for the float arithmetic that finds a
row, not for word indices past 2^32.  Not run at this size: `compute_returns_and_advantage` (its arrays are [K, E], held below 2^31
elements by the create check), and the replay buffer's normalised sampling (it shares sample_row's addressing; the statistics are
indexed by column).

The fill writes slices of 2^26 elements built from a torch.arange of that slice: no temporary is larger than 512 MiB.  A test
needs the array (16 GiB; the replay buffer two of them) and skips, with the numbers, when the device has not that much and 2 GiB
free.  Set FLEET_WRITE_PARITY=1 to record shapes, bytes and seconds in profiles/large_arrays.json."""
import json
import os
import time

import numpy as np
import pytest

import large_model as lm
import policy_bits as pb
import replay_model as rp

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda:0"
GIB = 1 << 30
SLICE = 1 << 26  # elements per fill / compare slice (at most 2^27)
SLICE_BYTES = SLICE * (8 + 8 + 4 + 4 + 4)  # the slice's int64 index and its remainder, two float32 stages, a comparison's result
HEADROOM = 2 * GIB
MOST = 36 * GIB
PROFILE = os.path.join(lm.ROOT, "profiles", "large_arrays.json")
_record = {}


# ---- helpers ------------------------------------------------------------------------------------------------------------------------
def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    a = np.ascontiguousarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    a, b = bits(a), bits(b)
    return a.size == b.size and np.array_equal(a.reshape(-1), b.reshape(-1))


def begin(name, shape, need):
    """Skip unless `need` bytes and the headroom are free; the record of the test, the clock started."""
    assert need <= MOST, (name, need)
    torch.cuda.empty_cache()
    free, total = torch.cuda.mem_get_info()
    rec = _record[name] = {"shape": shape, "bytes_needed": int(need), "free_bytes_seen": int(free), "status": "skipped"}
    if free < need + HEADROOM:
        _write()
        pytest.skip(f"{name}: needs {need / GIB:.2f} GiB + {HEADROOM / GIB:.0f} GiB headroom, {free / GIB:.2f} of {total / GIB:.2f} GiB free")
    torch.cuda.reset_peak_memory_stats()
    rec["held_before"] = int(torch.cuda.memory_allocated())  # what earlier tests of the process still hold is not this test's
    rec["t0"] = time.perf_counter()
    return rec


def end(rec, handle_bytes):
    torch.cuda.synchronize()
    rec["wall_s"] = round(time.perf_counter() - rec.pop("t0"), 3)
    rec["bytes_allocated"] = int(handle_bytes + torch.cuda.max_memory_allocated() - rec.pop("held_before"))
    rec["status"] = "ran"
    assert rec["bytes_allocated"] <= MOST, rec
    print(rec)
    _write()


def _write():
    if os.environ.get("FLEET_WRITE_PARITY") == "1":
        clean = {k: {a: b for a, b in v.items() if a not in ("t0", "held_before")} for k, v in sorted(_record.items())}
        with open(PROFILE, "w") as fh:
            json.dump({"slice_elements": SLICE, "tests": clean}, fh, indent=1)
            fh.write("\n")


def pattern(start, stop, offset):
    """value(i + offset) for i in [start, stop), on the device: the remainder is exact in int64, below 2^24 it converts to float32
    exactly, and the scale is a power of two."""
    i = torch.arange(start + offset, stop + offset, dtype=torch.int64, device=DEV)
    return i.remainder_(lm.M).to(torch.float32).mul_(lm.SCALE)


def fill(t, offset):
    flat = t.view(-1)
    n = flat.numel()
    for s in range(0, n, SLICE):
        e = min(s + SLICE, n)
        flat[s:e] = pattern(s, e, offset)


def mismatches(t, offset, skip=()):
    """How many elements of `t` outside the flat ranges `skip` differ in a bit from the pattern: one pass over the array."""
    flat = t.view(-1).view(torch.int32)
    n = flat.numel()
    total = torch.zeros((), dtype=torch.int64, device=DEV)
    for s in range(0, n, SLICE):
        e = min(s + SLICE, n)
        ne = flat[s:e] != pattern(s, e, offset).view(torch.int32)
        for lo, hi in skip:
            lo, hi = max(lo, s), min(hi, e)
            if lo < hi:
                ne[lo - s:hi - s] = False
        total += ne.sum()
    return int(total)


def wrong_rows(got, rows, width, offset):
    """The rows of `rows` (row b of `got` should be row rows[b] of the pattern) that differ, each with the flat index of its first
    wrong element and whether the row reaches past element 2^32."""
    got = bits(got).reshape(len(rows), width)
    out = []
    for b, r in enumerate(rows):
        ne = got[b] != lm.span(int(r) * width + offset, width).view(np.uint32)
        if ne.any():
            out.append({"row": int(r), "first_wrong_element": int(r) * width + int(np.argmax(ne)), "past_2_32": (int(r) + 1) * width > 1 << 32})
    return out


def small(n, offset):
    """value(i + offset), i < n, as NumPy holds it and on the device."""
    a = lm.value(np.arange(n, dtype=np.int64) + offset)
    return a, up(a)


# ---- rollout ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(lm.ROLLOUT))
def test_rollout_gather_and_add_past_2_32_elements(case):
    from fleetrl_amd import DeviceRolloutBuffer, _capi

    s = lm.ROLLOUT[case]
    E, K, D, A = s["E"], s["K"], s["D"], s["A"]
    W, n_rows = E * D, K * E
    total = int(_capi.rollout_layout(E, K, D, A).total_bytes)
    rec = begin(f"rollout/{case}", dict(s), total + SLICE_BYTES + 64 * D * 4 + 8 * W * 4)
    buf = DeviceRolloutBuffer(E, K, D, A)
    try:
        assert tuple(buf.observations.shape) == (K, E, D) and buf.observations.numel() == n_rows * D > 1 << 32
        fill(buf.observations, lm.OFFSETS["obs"])
        fill(buf.actions, lm.OFFSETS["actions"])
        per_row = ("values", "log_probs", "advantages", "returns")
        for name in per_row:
            fill(getattr(buf, name), lm.OFFSETS[name])

        # gather: buffer row r = t * E + e is flat index e * K + t
        rows = np.array(lm.rollout_rows(case), dtype=np.int64)
        idx = ((rows % E) * K + rows // E).astype(np.int32)
        out = buf.gather(up(idx))
        buf.check_errors()
        assert (D % 4 == 0) == (case == "vec") and out.observations.data_ptr() % 16 == 0  # the path the case is named after
        assert wrong_rows(out.observations, rows, D, lm.OFFSETS["obs"]) == []
        assert wrong_rows(out.actions, rows, A, lm.OFFSETS["actions"]) == []
        for name, got in zip(per_row, (out.old_values, out.old_log_prob, out.advantages, out.returns)):
            assert same(got, lm.value(rows + lm.OFFSETS[name])), name
        del out

        # add: the time rows that straddle 2^31 and 2^32 elements of obs, and the last, from sources of their own
        obs_np, obs_src = small(W, lm.OFFSETS["source"])
        act_np, act_src = small(E * A, lm.OFFSETS["source"] + 1)
        rew_np, rew_src = small(E, lm.OFFSETS["source"] + 2)
        val_np, val_src = small(E, lm.OFFSETS["source"] + 3)
        logp_np, logp_src = small(E, lm.OFFSETS["source"] + 4)
        start_np = (np.arange(E) % 3 == 1).astype(np.uint8)
        added = lm.rollout_add_rows(case)
        assert added[0] * W < 1 << 31 < (added[0] + 1) * W and added[1] * W < 1 << 32 < (added[1] + 1) * W and len(set(added)) == 3
        for t in added:
            buf.pos, buf.full = t, False
            buf.add(obs_src.view(E, D), act_src.view(E, A), rew_src, up(start_np), val_src, logp_src)
        torch.cuda.synchronize()
        for t in added:
            assert same(buf.observations[t], obs_np) and same(buf.actions[t], act_np), t
            assert same(buf.rewards[t], rew_np) and same(buf.episode_starts[t], start_np), t
            assert same(buf.values[t], val_np) and same(buf.log_probs[t], logp_np), t
            for x in [t - 1, t + 1] + lm.alias_rows(t, K, W):  # the neighbours, and where a truncated address would have written
                if 0 <= x < K and x not in added:
                    assert same(buf.observations[x], lm.span(x * W + lm.OFFSETS["obs"], W)), (t, x)
                    assert same(buf.actions[x], lm.span(x * E * A + lm.OFFSETS["actions"], E * A)), (t, x)
        # ... and nowhere else
        assert mismatches(buf.observations, lm.OFFSETS["obs"], [(t * W, (t + 1) * W) for t in added]) == 0
        assert mismatches(buf.actions, lm.OFFSETS["actions"], [(t * E * A, (t + 1) * E * A) for t in added]) == 0
        assert mismatches(buf.advantages, lm.OFFSETS["advantages"]) == 0 and mismatches(buf.returns, lm.OFFSETS["returns"]) == 0
        assert mismatches(buf.values, lm.OFFSETS["values"], [(t * E, (t + 1) * E) for t in added]) == 0
        buf.check_errors()
        end(rec, total)
    finally:
        buf.close()
        torch.cuda.empty_cache()


def test_rollout_gather_refuses_a_batch_its_item_loop_cannot_finish():
    """gather_rows counts batch * D items in an unsigned that advances by up to kRolloutMaxBlocks * kRolloutThreads: a count within one
    stride of 2^32 would wrap the counter to a small value and never end.  The call refuses it before any launch, by name, and
    leaves the output alone.  The indices and the output are allocated at the refused size, and every index is 0: were the call not
    refused, nothing would be out of bounds."""
    from fleetrl_amd import DeviceRolloutBuffer, FleetHipError, RolloutBatch, _capi

    L, D = lm.limits()["rollout_items"], 8193
    batch = L // D + 1
    assert (batch - 1) * D <= L < batch * D < 1 << 32
    with pytest.raises(FleetHipError):  # the library carries the limits (a create-time one, checked without a launch) ...
        _capi.rollout_layout(1 << 16, 1, (1 << 16) - 1, 1)
    rec = begin("rollout/gather_refusal", dict(E=1, K=1, D=D, A=1, batch=batch), batch * D * 4 + batch * 4 + SLICE_BYTES)
    buf = DeviceRolloutBuffer(1, 1, D, 1)
    try:
        sentinel = 0x7FC0BEEF  # a NaN no kernel here produces
        out = torch.full((batch * D,), sentinel, dtype=torch.int32, device=DEV)
        idx = torch.zeros(batch, dtype=torch.int32, device=DEV)
        with pytest.raises(FleetHipError) as ei:  # ... so this launches nothing
            buf.gather(idx, out=RolloutBatch(out.view(torch.float32).view(batch, D), None, None, None, None, None))
        assert ei.value.status == _capi.ERR_INVALID
        assert "fleet_rollout_gather_dev: batch * obs_dim" in str(ei.value) and f"<= {L}" in str(ei.value), str(ei.value)
        torch.cuda.synchronize()
        touched = sum(int((out[s:s + 4 * SLICE] != sentinel).sum()) for s in range(0, batch * D, 4 * SLICE))
        assert touched == 0
        buf.check_errors()
        # the same handle still gathers what it can finish
        buf.observations.view(-1).copy_(pattern(0, D, 0))
        got = buf.gather(idx[:3])
        buf.check_errors()
        assert wrong_rows(got.observations, [0, 0, 0], D, 0) == []
        del out, got
        end(rec, int(_capi.rollout_layout(1, 1, D, 1).total_bytes))
    finally:
        buf.close()
        torch.cuda.empty_cache()


# ---- replay -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(lm.REPLAY))
def test_replay_gather_sample_and_add_past_2_32_elements(case):
    from fleetrl_amd import DeviceReplayBuffer, _capi

    s = lm.REPLAY[case]
    R, E, D, A = s["R"], s["E"], s["D"], s["A"]
    W, B = E * D, lm.REPLAY_BATCH
    total = int(_capi.replay_layout(R * E, E, D, A).total_bytes)
    rec = begin(f"replay/{case}", dict(s), total + SLICE_BYTES + 2 * B * D * 4 + 4 * W * 4)
    buf = DeviceReplayBuffer(R * E, E, D, A, seed=lm.REPLAY_SEED)
    try:
        assert buf.rows == R and tuple(buf.observations.shape) == (R, E, D) and buf.observations.numel() > 1 << 32
        fill(buf.observations, lm.OFFSETS["obs"])
        fill(buf.next_observations, lm.OFFSETS["next_obs"])
        fill(buf.actions, lm.OFFSETS["actions"])
        fill(buf.rewards, lm.OFFSETS["rewards"])
        every = np.arange(R * E)
        dones_np, tmo_np = (every * 7 % 5 < 2).astype(np.uint8), (every % 3 == 0).astype(np.uint8)
        buf.dones.copy_(up(dones_np.reshape(R, E)))
        buf.timeouts.copy_(up(tmo_np.reshape(R, E)))

        def check(out, tr, tag):
            assert wrong_rows(out.observations, tr, D, lm.OFFSETS["obs"]) == [], tag
            assert wrong_rows(out.next_observations, tr, D, lm.OFFSETS["next_obs"]) == [], tag
            assert wrong_rows(out.actions, tr, A, lm.OFFSETS["actions"]) == [], tag
            assert same(out.rewards, lm.value(tr + lm.OFFSETS["rewards"])), tag
            assert same(out.dones, (dones_np[tr] * (1 - tmo_np[tr])).astype(np.float32)), tag

        calls = lm.replay_calls(case)
        for name, pos, full in (("full", 0, True), ("partial", lm.REPLAY_PARTIAL_POS, False)):
            upper = R if full else pos
            buf.set_position(pos, full, calls[name])
            tr = np.array(lm.replay_rows(case, upper), dtype=np.int64)
            assert tr.max() == upper * E - 1 and tr.max() * D > 1 << 32
            out = buf.gather(up((tr // E).astype(np.int32)), up((tr % E).astype(np.int32)))
            buf.check_errors()
            assert (D % 4 == 0) == (case == "vec") and out.observations.data_ptr() % 16 == 0 == out.next_observations.data_ptr() % 16
            check(out, tr, (name, "gather"))
            del out
            ri, ei = torch.full((B,), -1, dtype=torch.int32, device=DEV), torch.full((B,), -1, dtype=torch.int32, device=DEV)
            out = buf.sample(B, indices_out=(ri, ei))
            buf.check_errors()
            want_rows, want_envs = rp.draw(lm.REPLAY_SEED, calls[name], B, upper, E)
            assert np.array_equal(ri.cpu().numpy(), want_rows) and np.array_equal(ei.cpu().numpy(), want_envs), name
            assert buf.calls == calls[name] + 1 and buf.pos == pos and buf.full == full
            tr = want_rows.astype(np.int64) * E + want_envs
            assert (tr * D >= 1 << 32).sum() >= 2
            check(out, tr, (name, "sample"))
            del out

        # add at a position behind 2^32, some envs done: their terminal rows land in next_observations[pos], and nowhere else
        pos = lm.REPLAY_ADD_POS
        buf.set_position(pos, False, 0)
        obs_np, obs_src = small(W, lm.OFFSETS["source"])
        next_np, next_src = small(W, lm.OFFSETS["source"] + 5)
        term_np, term_src = small(W, lm.OFFSETS["terminal"])
        act_np, act_src = small(E * A, lm.OFFSETS["source"] + 1)
        rew_np, rew_src = small(E, lm.OFFSETS["source"] + 2)
        done_np = (np.arange(E) % 3 == 1).astype(np.uint8)
        done_np[E - 1] = 1
        assert 0 < done_np.sum() < E and pos * W > 1 << 32
        buf.add(obs_src.view(E, D), next_src.view(E, D), act_src.view(E, A), rew_src, up(done_np), terminal=term_src.view(E, D))
        torch.cuda.synchronize()
        assert buf.pos == pos + 1 and not buf.full
        assert same(buf.observations[pos], obs_np)
        want_next = np.where(done_np[:, None] != 0, term_np.reshape(E, D), next_np.reshape(E, D))
        assert same(buf.next_observations[pos], want_next)
        assert same(buf.actions[pos], act_np) and same(buf.rewards[pos], rew_np)
        assert same(buf.dones[pos], done_np) and same(buf.timeouts[pos], np.zeros(E, np.uint8))
        for x in [pos - 1, pos + 1] + lm.alias_rows(pos, R, W):  # the neighbours, and where a truncated address would have written
            assert 0 <= x < R and x != pos
            assert same(buf.observations[x], lm.span(x * W + lm.OFFSETS["obs"], W)), x
            assert same(buf.next_observations[x], lm.span(x * W + lm.OFFSETS["next_obs"], W)), x
        written = [(pos * W, (pos + 1) * W)]
        assert mismatches(buf.observations, lm.OFFSETS["obs"], written) == 0
        assert mismatches(buf.next_observations, lm.OFFSETS["next_obs"], written) == 0
        assert mismatches(buf.actions, lm.OFFSETS["actions"], [(pos * E * A, (pos + 1) * E * A)]) == 0
        buf.check_errors()
        end(rec, total)
    finally:
        buf.close()
        torch.cuda.empty_cache()


# ---- policy -------------------------------------------------------------------------------------------------------------------------
def test_policy_forward_past_2_32_elements():
    """One-layer heads, so tests/policy_bits.py models every output bit: the rows of the issue and the rows their aliases fall into,
    bit for bit; then every row against a float64 product made by torch on the device, chunk by chunk, under the project's rule
    |device - ref64| <= 8 * max(max |ref32 - ref64|, 2^-24 * max |ref64|), ref32 being torch's float32 product of the same chunk."""
    from fleetrl_amd import DevicePolicy

    E, D, A = lm.POLICY["E"], lm.POLICY["D"], lm.POLICY["A"]
    chunk = 1 << 15  # rows per reference product (at most 2^16): 2 GiB of float64
    rec = begin("policy", dict(lm.POLICY), E * D * 4 + max(SLICE_BYTES, chunk * D * 12) + E * (A + 1) * 4)
    actor, critic = lm.policy_weights()
    pol = DevicePolicy([actor], critic_layers=[critic], activation="relu", output="none")
    try:
        obs = torch.empty((E, D), dtype=torch.float32, device=DEV)
        assert obs.numel() == (1 << 32) + 131072
        fill(obs, lm.OFFSETS["obs"])
        actions = torch.full((E, A), float("nan"), device=DEV)
        values = torch.full((E, 1), float("nan"), device=DEV)
        assert pol.act(obs, out=actions, values_out=values) is actions
        torch.cuda.synchronize()
        got = torch.cat([actions, values], dim=1)

        rows = lm.policy_rows()
        assert set(lm.POLICY_ROWS) <= set(rows) and len(rows) > len(lm.POLICY_ROWS)
        x = np.stack([lm.span(r * D + lm.OFFSETS["obs"], D) for r in rows])
        w_all, b_all = np.concatenate([actor[0], critic[0]]), np.concatenate([actor[1], critic[1]])
        want = pb.forward_bits([(w_all, b_all)], x, "relu", "none")
        here = got[up(np.array(rows))].cpu().numpy()
        wrong = [r for k, r in enumerate(rows) if not pb.same_bits(here[k], want[k])]
        assert wrong == [], wrong

        w32, b32 = up(w_all.T), up(b_all)
        w64, b64 = w32.double(), b32.double()
        worst, failures = 0.0, []
        for s in range(0, E, chunk):
            xc = obs[s:s + chunk]
            r32, r64 = (xc @ w32 + b32).double(), xc.double() @ w64 + b64
            for head, cols in (("actor", slice(0, A)), ("critic", slice(A, A + 1))):
                eps_ref = float((r32[:, cols] - r64[:, cols]).abs().max())
                bound = 8 * max(eps_ref, 2.0 ** -24 * float(r64[:, cols].abs().max()))
                err = (got[s:s + chunk, cols].double() - r64[:, cols]).abs()
                worst = max(worst, float(err.max()) / bound)
                if not float(err.max()) <= bound:  # (a NaN fails)
                    first = s + int((~(err <= bound)).any(dim=1).nonzero()[0])
                    failures.append({"head": head, "first_row": first, "err": float(err.max()), "bound": bound})
        print(f"policy E={E} D={D}: worst error / bound over the chunks {worst:.3g}")
        assert failures == [], failures
        rec["worst_err_over_bound"] = worst
        del obs, got, actions, values
        end(rec, 0)
    finally:
        pol.close()
        torch.cuda.empty_cache()
