"""tests/golden/tube_mp.npz -- the 50-digit evaluation of the tube propagation (tests/tools/gen_tube_mp.py) -- for the tests
that read it, and the tolerances that follow from it.

ORACLE_ERR: the error of oracle/tube_oracle.py (the FP64 numpy/scipy restatement the kernel is also compared with, at 1e-9) against
the fixture, max over the cases of a Ts group of  |E - E_mp| / (1e-3 + |E_mp|),  measured on the CPU (scipy 1.x, OpenBLAS):

      Ts      oracle vs 50 digits    asserted (x 10, rounded up to one digit)
      0.02        2.09e-14               3e-13
      0.05        3.37e-12               4e-11
      0.08        7.57e-13               8e-12
      0.1         2.82e-14               3e-13
      0.15        7.10e-14               8e-13
      0.2         4.90e-14               5e-13
      0.3         6.20e-14               7e-13

The asserted column is at once the oracle's own bound (tests/test_oracle_tube.py) and the tolerance of the kernel
(tests/test_gpu_tube.py, and its arithmetic compiled for the CPU in tests/test_oracle_tube.py): the kernel has to be at least as
good as the FP64 oracle.  It comes from the oracle's error, never from what the kernel gives.
"""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "golden", "tube_mp.npz")

ORACLE_ERR = {0.02: 2.09e-14, 0.05: 3.37e-12, 0.08: 7.57e-13, 0.1: 2.82e-14, 0.15: 7.10e-14, 0.2: 4.90e-14, 0.3: 6.20e-14}
TOL = {0.02: 3e-13, 0.05: 4e-11, 0.08: 8e-12, 0.1: 3e-13, 0.15: 8e-13, 0.2: 5e-13, 0.3: 7e-13}


class Case:
    def __init__(self, g, c):
        s, n = int(g["case_start"][c]), int(g["case_N"][c])
        row = g["consts"][c]
        self.index, self.name, self.N = c, str(g["case_name"][c]), n
        self.consts = dict(mass=float(row[0]), drag=float(row[1]), ego_r=float(row[2]), ego_h=float(row[3]),
                           noise=tuple(float(x) for x in row[4:7]), epsilon=float(row[7]), Ts=float(row[8]))
        self.consts_row = row
        self.plan, self.E, self.Qd, self.G = g["plans"][s:s + n], g["E"][s:s + n], g["Qd"][s:s + n], g["G"][s:s + n]
        self.nu1, self.lam_min = g["nu1"][s:s + n], g["lam_min"][s:s + n]
        self.Ts = self.consts["Ts"]
        self.tol = TOL[self.Ts]


def load():
    g = np.load(PATH)
    return [Case(g, c) for c in range(len(g["case_N"]))]


def rel_E(E, E_mp):
    """The suite's metric for tube matrices (tests/test_gpu_parity.py::test_tube_matches_oracle)."""
    return float(np.max(np.abs(E - E_mp) / (1e-3 + np.abs(E_mp))))
