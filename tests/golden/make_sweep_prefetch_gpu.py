"""Records tests/golden/sweep_prefetch_gpu.npz on an MI355X: the cases of tests/test_sweep_prefetch_gpu.py stepped by the library that
SMPLSIM_HIP_LIB names — the build of the commit BEFORE the change under test (tools/build_variant.sh in a checkout of that commit):

    SMPLSIM_HIP_LIB=/path/to/libsmplsim_hip_parent.so python tests/golden/make_sweep_prefetch_gpu.py

Per case and control step t: pre<t>/<qpos qvel qpos_prev qvel_prev qacc_warm>, act<t>, post<t>/<qpos qvel solver_iters>, float32 /
int32 as the device holds them.  Rewriting the file moves the bits every later tree is held to: only do that on purpose."""
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import test_sweep_prefetch_gpu as T  # noqa: E402


def main():
    lib = os.environ.get("SMPLSIM_HIP_LIB")
    assert lib and os.path.exists(lib), "SMPLSIM_HIP_LIB must name the library of the commit before the change"
    out = {}
    for name in T.CASES:
        env = T.make_env(name)
        q, v, acts = T.start_state(name, env)
        env.set_state(q, v)
        for t in range(T.STEPS):
            pre = {k: getattr(env, k).cpu().numpy().copy() for k in T.PRE}
            post = T.step_from(env, pre, acts[t])
            for k in T.PRE:
                out[f"{name}/pre{t}/{k}"] = pre[k]
            out[f"{name}/act{t}"] = acts[t]
            for k in T.POST:
                out[f"{name}/post{t}/{k}"] = post[k]
            print(name, "step", t, "Newton iterations", post["solver_iters"].tolist(), "finite", bool(np.isfinite(post["qpos"]).all()))
    path = sys.argv[1] if len(sys.argv) > 1 else T.FIXTURE
    np.savez_compressed(path, **out)
    print("recorded with", lib, "->", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
