"""Records tests/golden/fwd_chain_emu.npz: the cases of tests/test_fwd_chain_emu.py on the wavefront emulator built from the tree
this script runs in — a checkout of the commit BEFORE the change under test, with this script, tests/test_fwd_chain_emu.py and
tests/test_fwd_chain_gpu.py copied into it:

    python tests/golden/make_fwd_chain_emu.py [output.npz]

Rewriting the file moves the bits every later tree is held to: only do that on purpose."""
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import test_fwd_chain_emu as T  # noqa: E402


def main():
    os.environ.pop("SS_EMU_GENERIC", None)
    out = {}
    for name in T.CASES:
        for k, x in T.run_case(name).items():
            out[f"{name}/{k}"] = x
        print(name, "Newton iterations", out[f"{name}/solver_iters"].tolist(), "finite", bool(np.isfinite(out[f"{name}/qpos"]).all()))
    path = sys.argv[1] if len(sys.argv) > 1 else T.FIXTURE
    np.savez_compressed(path, **out)
    print("recorded ->", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
