#!/usr/bin/env python3
"""The weights of a stable-baselines3 archive as a plain NumPy file: every array of the archive's `policy.pth` under its own
state-dict key, float32.  Needs torch, not SB3; nothing in the archive is executed (`torch.load(weights_only=True)`).

    python tools/export_sb3_policy.py MODEL.zip OUT.npz

`DevicePolicy.from_state_dict(dict(np.load(OUT.npz)))` builds the device policy from the result.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def export(zip_path, out_path) -> dict:
    from fleetrl_amd.policy import read_sb3_state_dict

    arrays = {k: np.ascontiguousarray(v.detach().cpu().numpy(), dtype=np.float32) for k, v in read_sb3_state_dict(zip_path).items()}
    np.savez(out_path, **arrays)
    return arrays


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    for key, a in export(sys.argv[1], sys.argv[2]).items():
        print(key, a.shape)
