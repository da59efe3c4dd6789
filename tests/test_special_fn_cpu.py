"""The global-step kernels' digamma (svae_amd/csrc/special_fn.hpp) on the HOST: a stand-alone program compiled with
g++ -O2 from the header alone reads doubles and prints psi as %a.  Two properties:

  * it TERMINATES and returns NaN on every non-positive and non-finite-negative input (the unguarded recurrence
    `while (x < 10) x += 1` never ends for x = -inf or below about -9e15, where x + 1 == x).  This is checked here and
    only here: such inputs never go through a GPU kernel;
  * on x > 0 it is within 4 ulp of max(|psi(x)|, 1) of mpmath's digamma (the function is a recurrence of at most 10
    trips plus a 7-term series; a NumPy restatement of it measured 6.5e-16 ~ 3 ulp of 1).

Measured with g++ -O2 on x86-64: worst 1.98 ulp of max(|psi|, 1) over the grid below (at x = 1)."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

mp = pytest.importorskip("mpmath")

HEADER_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "svae_amd", "csrc")

PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include "special_fn.hpp"
int main() {
  char buf[128];
  while (scanf("%127s", buf) == 1) printf("%a\n", svae::digamma_pos(strtod(buf, NULL)));
  return 0;
}
"""


@pytest.fixture(scope="module")
def digamma_program(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to compile the host digamma program"
    d = tmp_path_factory.mktemp("special_fn")
    src, exe = str(d / "digamma_main.cpp"), str(d / "digamma_main")
    with open(src, "w") as f:
        f.write(PROGRAM)
    subprocess.run([gxx, "-O2", "-std=c++17", "-I", HEADER_DIR, src, "-o", exe], check=True, timeout=120)
    return exe


def _run(exe, xs):
    """one child process, 10 s: a hang is a failure (TimeoutExpired), not a wait"""
    text = "\n".join(float(x).hex() if math.isfinite(x) else repr(float(x)) for x in xs) + "\n"
    out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=10, check=True).stdout.split()
    assert len(out) == len(xs)
    return [float.fromhex(v) if "0x" in v else float(v) for v in out]


def test_digamma_terminates_with_nan_on_non_positive_and_non_finite_inputs(digamma_program):
    xs = [-math.inf, -1e300, -1e16, -1.0, 0.0, -0.0, math.nan]
    got = _run(digamma_program, xs)
    assert all(math.isnan(v) for v in got), list(zip(xs, got))


def test_digamma_within_4_ulp_of_mpmath_on_positive_arguments(digamma_program):
    grid = list(np.logspace(-300, 300, 400))
    grid += [np.nextafter(10.0, 0.0), 10.0, np.nextafter(10.0, 20.0), 9.5, 10.5]      # both sides of the series threshold
    grid += [1.4616321449683623]                                                      # the positive root
    grid += [k / 2.0 for k in range(1, 41)]                                           # the Wishart arguments (nu - i)/2
    got = _run(digamma_program, grid)
    eps = 2.0 ** -52
    worst, where = 0.0, None
    old = mp.mp.dps
    mp.mp.dps = 50
    try:
        for x, g in zip(grid, got):
            want = mp.digamma(mp.mpf(float(x)))
            err = float(abs(mp.mpf(g) - want) / max(abs(want), 1)) / eps
            if err > worst:
                worst, where = err, float(x)
    finally:
        mp.mp.dps = old
    print("digamma_pos: worst %.2f ulp of max(|psi|, 1) at x = %r" % (worst, where))
    assert worst <= 4.0, (worst, where)
    assert _run(digamma_program, [math.inf]) == [math.inf]
