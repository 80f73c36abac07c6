#!/usr/bin/env python3
"""Cost of the per-body contact-force output (ss_set_contact_force_output) at the benchmark's sizes: the step launch timed with
device events, output off and on, for the self-collision workload (4096 SMPL envs, fresh uniform(-1, 1) actions, autoreset) and the
fused imitation step (1024 envs tracking bench.py's synthetic clips).  Off and on are two envs with the same seed and actions stepped
alternately, so both see the same state distribution and the same clock (not the same bits: the launch with the output on runs the
CFORCE instantiation of the step kernel, which has the run-time header).

    python tools/gpu_contact_force.py [--steps 300] [--warmup 30]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch


def timed(envs, act_fn, steps, warmup):
    """envs = (off, on): per step the same action to both; mean and median ms of the step launch of each."""
    ms = ([], [])
    for i in range(warmup + steps):
        a = act_fn(envs[0])
        for k, e in enumerate(envs):
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            e.step(a.clone(), _events=ev)
            if i >= warmup:
                ms[k].append(ev)
    torch.cuda.synchronize()
    t = [np.array([a.elapsed_time(b) for a, b in m]) for m in ms]
    return {"off_ms_mean": float(t[0].mean()), "on_ms_mean": float(t[1].mean()), "off_ms_median": float(np.median(t[0])),
            "on_ms_median": float(np.median(t[1])), "cost_frac_mean": float(t[1].mean() / t[0].mean() - 1.0), "steps": steps}


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
    F = envs[1].enable_contact_forces()
    for e in envs:
        e.reset()
    g = torch.Generator(device=envs[0].device); g.manual_seed(7)
    out["self_collision_4096"] = timed(envs, lambda e: torch.rand(4096, e.nu, generator=g, device=e.device) * 2 - 1, a.steps, a.warmup)
    assert bool(torch.isfinite(F).all()) and float(F.abs().max()) > 0
    for e in envs:
        e.close()
    import bench
    ml = MotionLibSMPL(bench.synthetic_clips(256, 300, 77), Skeleton.from_model_const(model.mc), device=0, seed=5)
    ml.load_motions()
    envs = [SMPLSimImitationVecEnv(1024, ml, model=model, device=0, seed=1234, fused=True) for _ in range(2)]
    F = envs[1].enable_contact_forces()
    for e in envs:
        e.reset()
    out["imitation_fused_1024"] = timed(envs, lambda e: e.reference_actions(), a.steps, a.warmup)
    assert bool(torch.isfinite(F).all()) and float(F.abs().max()) > 0
    print(json.dumps(out))


if __name__ == "__main__":
    main()
