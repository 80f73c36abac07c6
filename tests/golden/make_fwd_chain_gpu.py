"""Records tests/golden/fwd_chain_gpu.npz on an MI355X: the cases of tests/test_fwd_chain_gpu.py run by the library that
SMPLSIM_HIP_LIB names — the build of the commit BEFORE the change under test (tools/build_variant.sh in a checkout of that commit):

    SMPLSIM_HIP_LIB=/path/to/libsmplsim_hip_parent.so python tests/golden/make_fwd_chain_gpu.py

Per case: reset/<qpos qvel qacc_warm> (the state the case's reset left), start/<qpos qvel qacc_warm>, forward/<M bias qacc xpos xmat>
at the start state, and per control step t: act<t>, post<t>/<qpos qvel qacc_warm solver_iters body_vel obs>, float32 / int32 as the
device holds them; step t + 1 starts from post<t>.  Rewriting the file moves the bits every later tree is held to: only do that on purpose."""
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import test_fwd_chain_gpu as T  # noqa: E402


def main():
    lib = os.environ.get("SMPLSIM_HIP_LIB")
    assert lib and os.path.exists(lib), "SMPLSIM_HIP_LIB must name the library of the commit before the change"
    out = {}
    for name in T.CASES:
        env = T.make_env(name)
        task = T.reset_draws(name)[1]
        for k in T.STATE:
            out[f"{name}/reset/{k}"] = getattr(env, k).cpu().numpy().copy()
        pre, acts = T.start_state(name, env)
        for k in T.STATE:
            out[f"{name}/start/{k}"] = pre[k]
        for k, x in T.forward_from(env, pre).items():
            out[f"{name}/forward/{k}"] = x
        for t in range(T.STEPS):
            post = T.step_from(env, pre, acts[t], None if task is None else task[1 + t])
            out[f"{name}/act{t}"] = acts[t]
            for k in T.POST:
                out[f"{name}/post{t}/{k}"] = post[k]
            pre = {k: post[k] for k in T.STATE}
            print(name, "step", t, "Newton iterations", post["solver_iters"].tolist(), "finite", bool(np.isfinite(post["qpos"]).all()))
    path = sys.argv[1] if len(sys.argv) > 1 else T.FIXTURE
    np.savez_compressed(path, **out)
    print("recorded with", lib, "->", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
