"""Generates tests/golden/global_step_n64_<member>.npz: the 50-digit truths of the LDS global step at n = 64, one member
per family of tests/_global_step_families.py (two 64 x 64 inversions and three products in mpmath take ~10 s per
member, too long for a test; everything at n <= 33 is computed in the tests).  Truths come from oracle/expfam_mp.py
alone; the float64 natural parameters they belong to, global factor and prior, are stored beside them, so the test does
not depend on rebuilding them bit for bit.

    python tests/golden/make_golden_global_step.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import _global_step_families as F  # noqa: E402
from oracle import expfam_mp as em  # noqa: E402

N = 64


def main():
    for member in F.N64_MEMBERS:
        (niw, (A, B, C, d)), prior = F.lds_case(N, member)
        es, pair, logZ, kl = em.lds_global_step((niw, (A, B, C, d)), prior)
        path = os.path.join(HERE, "global_step_n%d_%s.npz" % (N, member))
        pniw, (pA, pB, pC, pd) = prior
        np.savez_compressed(path, niw=niw, A=A, B=B, C=C, d=d, prior_niw=pniw, prior_A=pA, prior_B=pB, prior_C=pC, prior_d=pd, es=es, J11=pair[0], J12=pair[1], J22=pair[2],
                            logZ_pair=pair[3], logZ=logZ, kl_full=kl.full, kl_shipped=kl.shipped, kl_scale=kl.scale)
        print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
