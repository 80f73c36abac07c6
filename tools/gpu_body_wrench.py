#!/usr/bin/env python3
"""Cost of the body-wrench input (ss_set_body_wrench_input) at the benchmark's sizes: the step launch timed with device events, with
the wrench NULL and attached, in the same kernel — both envs have the contact-force output on, which selects the optional-I/O
instantiation of the step kernel that also holds the wrench code.  The attached wrench is all zeros: the launch reads and applies
it like any other, and gives the bits of the NULL launch, so the two envs (same seed, same actions, stepped alternately) walk through
the same states and the difference is the cost of the input alone.  Workloads as tools/gpu_contact_force.py: self-collision (4096 SMPL
envs, fresh uniform(-1, 1) actions, autoreset) and the fused imitation step (1024 envs tracking bench.py's synthetic clips).

    python tools/gpu_body_wrench.py [--steps 300] [--warmup 30]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch

from gpu_contact_force import timed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300); ap.add_argument("--warmup", type=int, default=30)
    a = ap.parse_args()
    from smplsim_amd.batch import SMPLSimVecEnv, ShardModel
    from smplsim_amd.imitation import SMPLSimImitationVecEnv
    from smplsim_amd.motion_lib import MotionLibSMPL, Skeleton
    out = {}
    model = ShardModel(device=0)
    envs = [SMPLSimVecEnv(4096, model=model, seed=1234, self_collision=True) for _ in range(2)]
    for e in envs:
        e.enable_contact_forces()
    envs[1].enable_body_wrenches()
    for e in envs:
        e.reset()
    g = torch.Generator(device=envs[0].device); g.manual_seed(7)
    out["self_collision_4096"] = timed(envs, lambda e: torch.rand(4096, e.nu, generator=g, device=e.device) * 2 - 1, a.steps, a.warmup)
    out["self_collision_4096"]["same_bits"] = bool(torch.equal(envs[0].qpos, envs[1].qpos))
    for e in envs:
        e.close()
    import bench
    ml = MotionLibSMPL(bench.synthetic_clips(256, 300, 77), Skeleton.from_model_const(model.mc), device=0, seed=5)
    ml.load_motions()
    envs = [SMPLSimImitationVecEnv(1024, ml, model=model, device=0, seed=1234, fused=True) for _ in range(2)]
    for e in envs:
        e.enable_contact_forces()
    envs[1].enable_body_wrenches()
    for e in envs:
        e.reset()
    out["imitation_fused_1024"] = timed(envs, lambda e: e.reference_actions(), a.steps, a.warmup)
    out["imitation_fused_1024"]["same_bits"] = bool(torch.equal(envs[0].base.qpos, envs[1].base.qpos))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
