"""Writes tests/golden/dense_solve_cases.npz: the states of the dense-solve tests with the float64 oracle's answers
(tests/dense_solve_cases.py holds the bins and the seeded search; oracle and placement_cases only).

    python tests/golden/make_dense_solve_cases.py

tests/test_dense_solve_cpu.py runs the same search and requires the committed file byte for byte."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import dense_solve_cases as DC  # noqa: E402


def main():
    arrays = DC.build_all()
    for which in DC.HUMANOIDS:
        size, z = arrays[which + "_size"], arrays[which + "_qpos"][:, 2]
        print(which, len(size), "cases in", int(arrays[which + "_tries"][0]), "tries; root at 0.35 m:", int((z < 1).sum()))
        for name, lo, hi, n_hi, n_lo in DC.BINS[which]:
            got = (size >= lo) & (size <= hi)
            assert (got & (z > 1)).sum() >= n_hi and (got & (z < 1)).sum() >= n_lo, (which, name, "the search ran out of tries")
    data = DC.to_bytes(arrays)
    with open(DC.FIXTURE, "wb") as f:
        f.write(data)
    print(DC.FIXTURE, len(data), "bytes")


if __name__ == "__main__":
    main()
