"""tests/golden/reference_mp.npz -- the 50-digit evaluation of the stage references (tests/tools/gen_reference_mp.py) over the cases of
tests/reference_cases.py -- for the tests that read it, and the tolerance that follows from it.

ORACLE_ERR: the error of oracle/reference_oracle.py's ref_yaw against the fixture, max over the cases of a Ts of
|yaw - yaw_mp| / max(1, |yaw_mp|), measured on the CPU (glibc atan2; tests/test_reference_cpu.py prints it and asserts that it stays
below).  The paths of the 'coord' family that reach 1e3 m (1e3 m from the origin, 1e3 m wide) have a row of their own; its 1e-3 m path
stands under its Ts: a position near 1e3 is rounded
to 1e-13 m before the 0.8 m look-ahead direction is formed from it, which no arithmetic after it can undo.

      Ts       oracle, measured    table (rounded up)    kernel tolerance (x 10)    kernel, measured on an MI355X
      0.02        1.60e-15            1.7e-15               1.7e-14                    1.63e-15
      0.03        1.82e-15            1.9e-15               1.9e-14                    1.82e-15
      0.05        1.28e-15            1.3e-15               1.3e-14                    1.28e-15
      0.1         1.28e-15            1.3e-15               1.3e-14                    1.28e-15
      coord       3.28e-14            3.3e-14               3.3e-13                    3.28e-14

The tolerance comes from the oracle's error, never from what the kernel gives: the kernel has to be as good as the FP64 oracle, the
factor leaves room for a device atan2 a couple of ulp wider than libm's.
"""
import os

import numpy as np

from . import reference_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "golden", "reference_mp.npz")

ORACLE_ERR = {0.02: 1.7e-15, 0.03: 1.9e-15, 0.05: 1.3e-15, 0.1: 1.3e-15, "coord": 3.3e-14}
TOL = {Ts: 10.0 * e for Ts, e in ORACLE_ERR.items()}
B_INTERP, B_AHEAD, B_FAR, B_MINUS, B_PLUS, B_HOSTILE = 1, 2, 4, 8, 16, 32


class Fixture:
    def __init__(self):
        g = np.load(PATH)
        self.g = {k: g[k] for k in g.files}

    def stages(self, c):
        s = int(self.g["case_start"][c.index])
        return slice(s, s + c.N)

    def field(self, c, name):
        return self.g[name][self.stages(c)]

    def replan(self, c):
        return bool(self.g["case_replan"][c.index])

    def inputs_match(self, cases):
        """The fixture belongs to exactly this case table: every input, to the bit."""
        g = self.g
        pids = [str(p) for p in g["path_id"]]
        assert len(cases) == len(g["case_N"]) and sorted(RC.PATHS) == pids
        for j, p in enumerate(pids):
            s = int(g["path_start"][j])
            assert np.array_equal(g["paths"][s:s + int(g["path_K"][j])], RC.PATHS[p]), p
        for c in cases:
            i = c.index
            assert (str(g["case_name"][i]), int(g["case_N"][i]), float(g["case_Ts"][i]), pids[int(g["case_path"][i])]) == (c.name, c.N, c.Ts, c.path_id), c.name
            assert int(g["case_size"][i]) == (RC.NO_SIZE if c.size is None else c.size), c.name
            assert np.array_equal(np.array([g["case_off"][i], g["case_yaw0"][i], *g["case_pos1"][i]]), np.array([c.off, c.yaw0, *c.pos1]), equal_nan=True), c.name


_FIXTURE = None


def load():
    global _FIXTURE
    if _FIXTURE is None:
        _FIXTURE = Fixture()
    return _FIXTURE


def err_key(c):
    """The row of ORACLE_ERR / TOL a case belongs to."""
    return "coord" if c.family == "coord" and c.path_id != "tiny" else c.Ts


def yaw_err(yaw, hi, lo):
    """|yaw - yaw_mp| / max(1, |yaw_mp|), the subtraction of hi exact (Sterbenz) before lo comes in."""
    return np.abs((yaw - hi) - lo.astype(np.float64)) / np.maximum(1.0, np.abs(hi))
