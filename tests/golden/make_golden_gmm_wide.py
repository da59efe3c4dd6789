"""Golden fixtures of the GMM local step at latent dimensions 9..16 (svae_amd/csrc/gmm_wide.hip), from the REFERENCE
ITSELF, with the recipes of make_golden.py (its gmm_case / gmm_run_case, imported, not copied):

  python tests/golden/make_golden_gmm_wide.py [case-name ...]

  gmm_K15_N10_T100.npz      local_meanfield (svae/models/gmm.py:62-88), K = 15, N = 10
  gmm_K33_N16_T24.npz       local_meanfield, K = 33, N = 16
  gmm_run_K6_N16_T40.npz    run_inference (gmm.py:12-16), K = 6, N = 16, S = 2, the draws replayed
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from make_golden import build_ref, gmm_case, gmm_run_case   # noqa: E402

CASES = {
    "gmm_K15_N10_T100": lambda n: gmm_case(n, 15, 10, 100, seed=31),
    "gmm_K33_N16_T24": lambda n: gmm_case(n, 33, 16, 24, seed=32),
    "gmm_run_K6_N16_T40": lambda n: gmm_run_case(n, 6, 16, 40, 2, seed=33),
}

if __name__ == "__main__":
    assert build_ref.build(), "reference build failed"
    only = set(sys.argv[1:])
    for name, make in CASES.items():
        if not only or name in only:
            make(name)
