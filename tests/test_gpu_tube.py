"""The tube kernel (csrc/frp_tube.hip) against the 50-digit fixture tests/golden/tube_mp.npz on the MI355X.

TOLERANCE (tests/tube_fixture.py): per Ts group, ten times the error of oracle/tube_oracle.py against the same fixture --
the kernel has to be at least as good as the FP64 oracle.  Metric |E - E_mp| / (1e-3 + |E_mp|).

      Ts      tolerance    kernel, MI355X    (oracle, CPU)
      0.02     3e-13         1.42e-14          2.09e-14
      0.05     4e-11         1.17e-13          3.37e-12
      0.08     8e-12         3.82e-14          7.57e-13
      0.1      3e-13         2.56e-14          2.82e-14
      0.15     8e-13         1.94e-14          7.10e-14
      0.2      5e-13         2.53e-14          4.90e-14
      0.3      7e-13         2.94e-14          6.20e-14

With ONE panel on every stage (a build of the kernel without the panel split), same cases, same machine: Ts 0.02 .. 0.1
the same to rounding; 9.4e-12 at Ts = 0.15 (tolerance 8e-13), 1.0e-11 at 0.2, 3.8e-8 at 0.3.  Of the eight cases
with Ts >= 0.2 it misses six: Ts0.2_rand 7.2e-13, Ts0.2_t3 1.0e-11, Ts0.3_warm 1.0e-12, Ts0.3_rand 4.2e-12, Ts0.3_edge 1.1e-9,
Ts0.3_t3 3.8e-8 -- with no error code.

The constants of frp_nmpc_tube are per launch, so a launch cannot mix them; the cases are batched by (constants, horizon), which
puts up to five different plans into one launch (blockIdx > 0), and the launches alternate between sets of constants.
"""
import numpy as np
import pytest

from forces_resilient_planner_amd import solver, workloads

from . import tube_fixture as TF

pytestmark = pytest.mark.gpu

CASES = TF.load()


def _groups():
    g = {}
    for c in CASES:
        g.setdefault((tuple(c.consts_row), c.N), []).append(c)
    return list(g.values())


def test_kernel_meets_the_multiprecision_reference_on_every_case():
    worst = {}
    groups = _groups()
    assert max(len(g) for g in groups) >= 4 and len({tuple(g[0].consts_row) for g in groups}) >= 10
    for g in groups:
        # every case once more behind a copy of the group's last plan, so that single-case groups run at blockIdx > 0 as well
        E = solver.tube_batch_host(np.stack([g[-1].plan] + [c.plan for c in g]), g[0].consts)[1:]
        for c, Ec in zip(g, E):
            assert np.isfinite(Ec).all(), c.name
            worst[c.Ts] = max(worst.get(c.Ts, 0.0), TF.rel_E(Ec, c.E))
            assert np.max(np.abs(Ec - np.swapaxes(Ec, -1, -2))) < 1e-14, c.name      # symmetric principal root
            assert np.linalg.eigvalsh(Ec).min() > 0, c.name
    print("kernel vs 50 digits, by Ts:", {k: f"{v:.2e}" for k, v in sorted(worst.items())})
    for Ts, w in sorted(worst.items()):
        assert w < TF.TOL[Ts], (Ts, w, TF.TOL[Ts])


def test_long_sampling_times_are_accurate_or_refused():
    """Each case with Ts >= 0.2 -- nu = ||Phi||_1 Ts up to 30, where one quadrature panel loses up to nine digits -- meets its
    tolerance; a sampling time the panels cannot cover for in-bounds thrust is refused, and a plan that leaves the domain on its
    own (thrust 100 times the bound: nu > 80) comes back as NaN, never as wrong digits, without touching its batch neighbours."""
    far = [c for c in CASES if c.Ts >= 0.2]
    assert len(far) == 8 and max(c.nu1.max() for c in far) > 25
    for c in far:
        E = solver.tube_batch_host(c.plan[None], c.consts)[0]
        assert TF.rel_E(E, c.E) < c.tol, (c.name, TF.rel_E(E, c.E))
    c = [c for c in CASES if c.name == "Ts0.3_rand"][0]
    with pytest.raises(RuntimeError):
        solver.tube_batch_host(c.plan[None], dict(c.consts, Ts=1.75))
    wild = c.plan.copy(); wild[2, 3] *= 100.0
    E = solver.tube_batch_host(np.stack([c.plan, wild, c.plan]), c.consts)
    assert np.isnan(E[1]).all() and np.array_equal(E[0], E[2]) and TF.rel_E(E[0], c.E) < c.tol


def test_device_fleet_tube_equals_the_host_wrapper():
    """DeviceFleet.tube() -- the call of the full tick -- on the N = 20 cases: the same bits as solver.tube_batch_host."""
    import torch
    w = workloads.config2(2)
    n20 = [c for c in CASES if c.N == 20]
    assert len(n20) >= 7
    for c in n20:
        fleet = solver.DeviceFleet(2, 20, w["M"], w["M"], w["model"], (15.0, 3.0, 80.0, 15.0, 0.0))
        plan = np.stack([np.concatenate([c.plan, c.plan[-1:]]), np.concatenate([c.plan[::-1], c.plan[:1]])])
        fleet.mpc_output.copy_(fleet.to_device(plan))
        fleet.tube(c.consts)
        torch.cuda.synchronize()
        E = fleet.ellipsoid.cpu().numpy()
        Eh = solver.tube_batch_host(plan[:, :20], c.consts)
        assert np.array_equal(E, Eh), c.name
        assert TF.rel_E(E[0], c.E) < c.tol, c.name


def test_a_planners_result_does_not_depend_on_its_batch():
    """Bit-identical alone, as element 0 and as element B - 1 of a mixed batch (different plans, some with more panels)."""
    for g in _groups():
        if len(g) < 2:
            continue
        plans = np.stack([c.plan for c in g])
        for i, c in enumerate(g):
            alone = solver.tube_batch_host(c.plan[None], c.consts)[0]
            others = np.delete(plans, i, axis=0)
            first = solver.tube_batch_host(np.concatenate([c.plan[None], others]), c.consts)[0]
            last = solver.tube_batch_host(np.concatenate([others, c.plan[None]]), c.consts)[-1]
            assert np.array_equal(alone, first) and np.array_equal(alone, last), c.name
