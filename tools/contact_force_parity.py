#!/usr/bin/env python3
"""CPU measurement behind the gates of tests/test_contact_force_emu.py (profiles/contact_force.txt): the deviation of the per-body
contact forces (ss_set_contact_force_output) of the wavefront emulator, float64 and float32 builds, from the float64 oracle over
  * the cases of the test file, and
  * control steps of the benchmark's state distribution: envs under fresh uniform(-1, 1) actions with autoreset, EVERY (env, step
    >= skip), the steps that end an episode or hold MuJoCo's bad-state reset included; the float32 emulator makes the states, the
    float64 build and the oracle replay every sample from its pre-step state.
Error per env-step: max_b |F - F_ref|_inf / max(W, max_b |F_ref|_inf), W the model's weight.
No env-step is left out of the float64 comparison.  The float32 comparison may leave out at most 2 % of the env-steps (the share
tests/test_gpu_parity.py allows): --leave-out K takes the K worst out of the float32 gate and lists each with its Newton-iteration
count; they stay in the float64 figures.

    python tools/contact_force_parity.py [--envs 16] [--steps 22] [--skip 6] [--self-collision]
"""
import argparse
import concurrent.futures as cf
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import contact_force_ref as R
import parity_tools as P
import test_contact_force_emu as T
from helpers import model_const, oracle_model


def quant(name, e):
    e = np.asarray(e)
    print(f"{name:34s} n={len(e):4d}  median {np.median(e):.3e}  p90 {np.quantile(e, 0.9):.3e}  p99 {np.quantile(e, 0.99):.3e}  max {e.max():.3e}")
    return e.max()


def test_cases(f64):
    errs = []
    for name, fn, hum, sc in (("standing", T.standing, "smpl_humanoid", False), ("lying", T.lying, "smpl_humanoid", False), ("smplx", T.smplx, "smplx_humanoid", False)):
        mc, eb, pre, acts = fn(f64)
        om = oracle_model(hum, self_collision=sc)
        errs += [R.force_error(eb.cforce[i], R.oracle_contact_force(om, mc.friction, pre[i], acts[i])[0], R.weight(mc)) for i in range(eb.N)]
    mc, om, eb, pre, acts = T.body_body(f64)
    errs += [R.force_error(eb.cforce[i], R.oracle_contact_force(om, mc.friction, pre[i], acts[i])[0], R.weight(mc)) for i in range(eb.N)]
    return errs


def rollout(n_envs, n_steps, skip, seed, self_collision):
    """Samples on the float32 emulator: list of (pre dict, action, F32 [nb, 3], Newton iterations of the control step)."""
    mc = model_const()
    rs = np.random.default_rng(seed)
    acts = rs.uniform(-1, 1, (n_steps, n_envs, mc.nu))

    def run(lo_hi):
        lo, hi = lo_hi
        _, eb = T._batch(hi - lo, False, self_collision=self_collision)
        eb.reset()
        out = []
        for t in range(n_steps):
            pre = [R.pre_of(eb, i) for i in range(hi - lo)]
            nw0 = eb.nwarn.copy()
            _, _, term, trunc = eb.step(acts[t, lo:hi])
            done = term | trunc
            for i in range(hi - lo):
                if t >= skip:                                  # every env-step: none is filtered
                    out.append((pre[i], acts[t, lo + i], eb.cforce[i].astype(np.float64), int(eb.solver_iters[i]), int(eb.nwarn[i] - nw0[i])))
            if done.any():
                eb.reset(mask=done)
        return out

    with cf.ThreadPoolExecutor(P.n_threads()) as ex:
        return [s for part in ex.map(run, P._chunks(n_envs, P.n_threads())) for s in part]


def replay(samples, self_collision):
    """Every sample again from its pre-step state: the float64 emulator and the oracle.  Returns (err64, err32, oracle infos)."""
    mc, om = model_const(), oracle_model(self_collision=self_collision)
    W = R.weight(mc)

    def run(lo_hi):
        lo, hi = lo_hi
        part = samples[lo:hi]
        _, eb = T._batch(hi - lo, True, self_collision=self_collision)
        eb.set_state(*[np.array([s[0][k] for s in part]) for k in R.PRE_FIELDS])
        eb.step(np.array([s[1] for s in part]))
        out = []
        for i, (pre, a, F32, it, nw32) in enumerate(part):
            Fr, info = R.oracle_contact_force(om, mc.friction, pre, a)
            out.append((R.force_error(eb.cforce[i], Fr, W), R.force_error(F32, Fr, W), info, int(eb.nwarn[i])))
        return out

    with cf.ThreadPoolExecutor(P.n_threads()) as ex:
        return [r for part in ex.map(run, P._chunks(len(samples), P.n_threads())) for r in part]


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=16); ap.add_argument("--steps", type=int, default=22); ap.add_argument("--skip", type=int, default=6)
    ap.add_argument("--seed", type=int, default=3); ap.add_argument("--self-collision", action="store_true")
    ap.add_argument("--leave-out", type=int, default=0, help="float32 only: the K worst env-steps are listed and left out of the gate (at most 2 %%)")
    a = ap.parse_args()
    worst = {}
    for f64 in (True, False):
        worst[f64] = quant(f"test cases, {'float64' if f64 else 'float32'} emulator", test_cases(f64))
    S = rollout(a.envs, a.steps, a.skip, a.seed, a.self_collision)
    res = [r for r in replay(S, a.self_collision)]
    e64, e32 = np.array([r[0] for r in res]), np.array([r[1] for r in res])
    resets = [(S[i][4], res[i][3], res[i][2]["nwarn"]) for i in range(len(S))]      # bad-state resets inside the step: float32, float64, oracle
    tag = "benchmark states" + (", self-collision" if a.self_collision else "")
    print(f"{tag}: {len(S)} env-steps, all compared; {sum(1 for r in resets if any(r))} of them with MuJoCo's bad-state reset inside the step; "
          f"loaded bodies per env-step: median {np.median([len(r[2]['loaded']) for r in res]):.0f}, max {max(len(r[2]['loaded']) for r in res)}")
    worst[True] = max(worst[True], quant(f"{tag}, float64", e64))
    assert a.leave_out <= 0.02 * len(S), "at most 2 % of the env-steps may be left out"
    order = np.argsort(-e32)
    out_, kept = order[:a.leave_out], order[a.leave_out:]
    for i in out_:
        print(f"  LEFT OUT of the float32 gate: sample {i}: err {e32[i]:.3e}  (float64 {e64[i]:.3e})  Newton iterations of the control step {S[i][3]}  "
              f"loaded bodies {len(res[i][2]['loaded'])}  bad-state resets f32/f64/oracle {resets[i]}")
    worst[False] = max(worst[False], quant(f"{tag}, float32 ({len(kept)} of {len(S)})", e32[kept]))
    for i in kept[:5]:
        print(f"  float32 sample {i}: err {e32[i]:.3e}  (float64 {e64[i]:.3e})  Newton iterations of the control step {S[i][3]}  loaded bodies {len(res[i][2]['loaded'])}  resets {resets[i]}")
    print(f"worst float64 {worst[True]:.3e} -> gate min(1e-6, 3 x) = {min(1e-6, 3 * worst[True]):.3e} ;  worst float32 {worst[False]:.3e} -> gate 3 x = {3 * worst[False]:.3e}")
