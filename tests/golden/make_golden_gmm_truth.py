"""Generates tests/golden/gmm_truth_tail_<family>_N16.npz: inputs, 50-digit truth and the torch-CPU sampler's e_ref of
the GMM tail cases (sampler + adjoint of the taped pass) of tests/_gmm_families.py at N = 16, where the oracle's two
directional derivatives over all 65 points take ~10 s per family -- too long for a test; everything at N <= 9 and
every fixed-point truth is computed in the tests.  Truths come from oracle/gmm_mp.py alone; the float64 inputs they belong
to (the responsibilities entering the pass come from a LAPACK run) are stored beside them, so the test does not depend
on rebuilding them bit for bit.

    python tests/golden/make_golden_gmm_truth.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import _gmm_families as F  # noqa: E402


def main():
    N = F.GOLDEN_TAIL_N
    for family in F.TAIL_FAMILIES:
        c = F.make_tail_case(family, N)
        t = F.make_tail_truth(c)
        (d0J, d0h), (d1J, d1h) = c["dirs"]
        path = F.golden_tail_path(family, N)
        np.savez_compressed(path, dir0_J=d0J, dir0_h=d0h, dir1_J=d1J, dir1_h=d1h,
                            samples=t["samples"], samples_ref=t["samples_ref"], e_ref_samples=F.e_block(t["samples_ref"], t["samples"]),
                            jvp0_samples=t["jvp"][0][0], jvp0_kl=t["jvp"][0][1], jvp1_samples=t["jvp"][1][0],
                            jvp1_kl=t["jvp"][1][1], **{k: c[k] for k in F._TAIL_INPUTS[:-4]})
        print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
