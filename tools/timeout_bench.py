#!/usr/bin/env python3
"""The wall-clock budget (frp_nmpc_options.timeout) on configs[2], B = 4096, N = 20, and on the 4096-planner tick:
  1. cost of the budget when it never fires: timeout = 0 against timeout = 10 s, launches alternated in one process (HIP events on the
     launch stream), median and spread of each;
  2. budgets of 0.2 / 0.3 / 0.4 / 0.6 ms: launch time, overshoot past the budget, fraction of the batch converged (flag 1);
  3. DeviceFleet.full_tick of 4096 planners (tools/full_tick_bench.py) without a budget and with one.
   python tools/timeout_bench.py [reps=21] [tick_budget_ms=0.5]   -> one JSON object on stdout"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from forces_resilient_planner_amd import solver, workloads  # noqa: E402


def _launch_ms(ds):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    ds.solve()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _stats(v):
    v = np.asarray(v)
    return {"median_ms": float(np.median(v)), "p10_ms": float(np.percentile(v, 10)), "p90_ms": float(np.percentile(v, 90)), "n": int(len(v))}


def run(reps=21, tick_budget_ms=0.5):
    w = workloads.config2(4096)
    ds = solver.DeviceSolver(4096, w["N"], w["M"], 6, w["model"], "cuda:0")
    ds.upload(w)
    for _ in range(3):
        _launch_ms(ds)
    out = {"workload": "configs[2]: B = 4096, N = 20, " + solver.solver_variant(4096, w["N"], w["M"], 6, w["model"], ds.opt)}
    # 1. the budget that never fires, alternated with none
    t = {0.0: [], 10.0: []}
    for _ in range(reps):
        for to in (0.0, 10.0):
            ds.opt.timeout = to
            t[to].append(_launch_ms(ds))
    s0, s10 = _stats(t[0.0]), _stats(t[10.0])
    out["no_budget"] = s0
    out["budget_10s"] = s10
    out["overhead_pct"] = 100.0 * (s10["median_ms"] / s0["median_ms"] - 1.0)
    out["spread_pct"] = 100.0 * (s0["p90_ms"] - s0["p10_ms"]) / s0["median_ms"]
    # 2. budgets that fire
    rows = []
    for b_ms in (0.2, 0.3, 0.4, 0.6):
        ds.opt.timeout = b_ms * 1e-3
        ms = []
        for _ in range(max(5, reps // 4)):
            ms.append(_launch_ms(ds))
        torch.cuda.synchronize()
        fl = ds.exitflag.cpu().numpy(); it = ds.iters.cpu().numpy()
        med = float(np.median(ms))
        rows.append({"budget_ms": b_ms, "launch_ms": med, "overshoot_ms": med - b_ms, "converged_frac": float((fl == 1).mean()),
                     "timed_out_frac": float((fl == 2).mean()), "mean_iters": float(it.mean()), "max_iters": int(it.max())})
    out["budgets"] = rows
    ds.opt.timeout = 0.0
    del ds
    # 3. the fleet tick (full_tick_bench builds its own fleet from solver.default_options)
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import full_tick_bench as FT
    base = FT.run(4096, 10, 20000, 0.5, 0)
    from forces_resilient_planner_amd import batch  # (DeviceSolver looks default_options up in its own module)
    orig = batch.default_options
    batch.default_options = lambda **kw: orig(**{"timeout": tick_budget_ms * 1e-3, **kw})
    try:
        bud = FT.run(4096, 10, 20000, 0.5, 0)
    finally:
        batch.default_options = orig
    pick = lambda r: {k: r[k] for k in ("ms_per_tick", "converged_frac", "mean_iters")}
    out["full_tick_4096"] = {"no_budget": pick(base), f"budget_{tick_budget_ms}ms": pick(bud)}
    return out


if __name__ == "__main__":
    a = sys.argv[1:]
    print(json.dumps(run(int(a[0]) if a else 21, float(a[1]) if len(a) > 1 else 0.5), indent=1))
