"""Restatement of include/fleet_hip_sac_loop.h (fleet_saccollect_*, fleet_saceval_*) for the tests: the launch counts of SAC's collector and
of its evaluation, and the action either launch of a collector step takes.  The episode ring and the evaluation's bookkeeping are the
existing families' and stay restated in tests/collect_model.py and tests/eval_model.py."""
import collect_model as cm
import eval_model as em

ROOT = cm.ROOT
Ring, Evaluation = cm.Ring, em.Evaluation


def launches_collect(n_steps: int, with_norm: bool) -> int:
    """5 n + 1 with a normaliser, 4 n + 1 without: the action (the uniform draw or the squashed sample: one launch either way), step,
    [normalise], add, episodes per step; the closing launch.  The off-policy loop of the TD3 collector without a noise handle."""
    assert cm.launches_offpolicy(n_steps, with_norm) == (5 if with_norm else 4) * n_steps + 1
    return (5 if with_norm else 4) * n_steps + 1


def launches_eval(n_steps: int, with_norm: bool, with_sync: bool = False) -> int:
    """The evaluation section's own: 4 n + 5 with a normaliser, 3 n + 4 without, one more with sync_from; the deterministic action is one
    launch, as the policy's forward is."""
    return em.launches(n_steps, with_norm, with_sync)


def warm_up(step: int, learning_starts: int) -> bool:
    """Global step s draws a uniform action iff s < learning_starts (SB3: num_timesteps < learning_starts)."""
    return step < learning_starts
