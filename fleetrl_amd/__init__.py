"""fleetrl_amd -- MI355X-native batched FleetRL `FleetEnv.step()` hot path.

    from fleetrl_amd import FleetEnv, FleetVecEnv, FleetVectorEnv, FleetMixedVecEnv
    from fleetrl_amd import FleetVecNormalize, DeviceNormalizer, sync_normalization
    from fleetrl_amd import plan_linear_optimization, run_linear_optimization
    from fleetrl_amd import DeviceRolloutBuffer, DeviceReplayBuffer
    from fleetrl_amd import DevicePolicy, evaluate_policy
    from fleetrl_amd import DevicePinkNoise, DeviceOUNoise
    from fleetrl_amd import DeviceTD3Target
    from fleetrl_amd import DeviceSACNetworks, DeviceSACGrad
    from fleetrl_amd import DevicePPOGrad
    from fleetrl_amd import DeviceTD3Grad
    from fleetrl_amd import DeviceAdam
    from fleetrl_amd import DevicePPOTrain
    from fleetrl_amd import DeviceTD3Train
    from fleetrl_amd import DeviceSACTrain
    from fleetrl_amd import DevicePPOCollect, DeviceTD3Collect, DeviceSACCollect
    from fleetrl_amd import DeviceEvalCallback
    from fleetrl_amd import LogSummary, summarize_log, compare, evaluate_strategies
"""
__version__ = "0.1.0"


def __getattr__(name):  # lazy: importing the package must not require the HIP library (build() imports it first)
    if name in ("FleetEnv", "FleetVecEnv", "FleetVectorEnv", "FleetCore"):
        from . import vec_env

        return getattr(vec_env, name)
    if name == "FleetMixedVecEnv":
        from . import mixed

        return mixed.FleetMixedVecEnv
    if name in ("FleetVecNormalize", "DeviceNormalizer", "sync_normalization"):
        from . import vec_normalize

        return getattr(vec_normalize, name)
    if name in ("DeviceRolloutBuffer", "RolloutBatch", "RolloutSlot"):
        from . import rollout

        return getattr(rollout, name)
    if name in ("DeviceReplayBuffer", "ReplayBatch"):
        from . import replay

        return getattr(replay, name)
    if name in ("DevicePolicy", "evaluate_policy"):
        from . import policy

        return getattr(policy, name)
    if name in ("DevicePinkNoise", "DeviceOUNoise"):
        from . import noise

        return getattr(noise, name)
    if name == "DeviceTD3Target":
        from . import qtarget

        return qtarget.DeviceTD3Target
    if name in ("DeviceSACNetworks", "DeviceSACGrad", "SAC_ACTOR_STATS"):
        from . import sac

        return getattr(sac, name)
    if name == "DevicePPOGrad":
        from . import ppo

        return ppo.DevicePPOGrad
    if name == "DeviceTD3Grad":
        from . import td3

        return td3.DeviceTD3Grad
    if name == "DeviceAdam":
        from . import adam

        return adam.DeviceAdam
    if name == "DevicePPOTrain":
        from . import train

        return train.DevicePPOTrain
    if name == "DeviceTD3Train":
        from . import offpolicy

        return offpolicy.DeviceTD3Train
    if name in ("DeviceSACTrain", "SAC_TRAIN_STATS", "SAC_TRAIN_SB3_NAMES"):
        from . import sac_train

        return getattr(sac_train, name)
    if name in ("DevicePPOCollect", "DeviceTD3Collect", "DeviceSACCollect"):
        from . import collect

        return getattr(collect, name)
    if name == "DeviceEvalCallback":
        from . import eval_callback

        return eval_callback.DeviceEvalCallback
    if name in ("plan_linear_optimization", "run_linear_optimization"):
        from . import lp_benchmark

        return getattr(lp_benchmark, name)
    if name in ("LogSummary", "summarize_log", "compare", "evaluate_strategies"):
        from . import evaluation

        return getattr(evaluation, name)
    if name in ("FleetBatch", "FleetHipError"):
        from . import batch

        return getattr(batch, name)
    raise AttributeError(name)
