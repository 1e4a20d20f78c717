#!/usr/bin/env python3
"""Generate the committed golden fixtures under tests/golden/ (run in the BUILD container only).

Needs oracle/_ref/libref_model_{normal,final}.so = the reference's own CasADi model callbacks
compiled in place from /root/reference by `make -C oracle ref` (nothing from the reference is
copied; only NUMBERS produced by it are stored).

  G1  stage_vectors.npz   seeded (z, p, stage, model) -> f, grad f, c, Jc, h, Jh from the reference
                          callback FORCESNLPsolver_{normal,final}_casadi2forces
                          (solver/*/FORCESNLPsolver_*_casadi2forces.c:42-245).
  G2  hessian_vectors.npz seeded edge points (z, p, stage, model, nu) -> difference Hessians of nu'c and of the cost
                          from the same callbacks' exact Jacobians, with their error estimates (ref_hessian).
  G3  solutions_<family>.npz   independent SciPy SLSQP solutions of the reference NLP
                          (matlab_code/setup.m, mpc/normal/mpc_generator_normal.m) assembled from those
                          same callbacks (objective, dynamics, corridor + analytic Jacobians), for
                          seeded problems of the BASELINE.json config families.  `start` records how
                          SciPy was started: 'cold' = the caller's own initial guess (fully independent),
                          'near' = a N(0, 0.02^2)-perturbed oracle solution (certifies a local minimiser).

The ForcesPro binary itself cannot be run (licence error -100), so these SciPy solutions of the
reference *model* are the solver-level known answers ("parity unpinned" w.r.t. ForcesPro proper).
"""
import ctypes
import os
import sys
import time
from multiprocessing import Pool

import numpy as np
from scipy.optimize import minimize

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from forces_resilient_planner_amd import layout as L  # noqa: E402
from forces_resilient_planner_amd import workloads as W  # noqa: E402

D = ctypes.POINTER(ctypes.c_double)
_REF = {}


def P(a):
    return a.ctypes.data_as(D) if a is not None else None


def ref_callback(model):
    name = 'normal' if model == L.MODEL_NORMAL else 'final'
    if name not in _REF:
        lib = ctypes.CDLL(os.path.join(ROOT, 'oracle', '_ref', f'libref_model_{name}.so'))
        _REF[name] = getattr(lib, f'FORCESNLPsolver_{name}_casadi2forces')
    return _REF[name]


def ref_stage(model, z, p130, stage20, want=('f', 'gf', 'c', 'Jc', 'h', 'Jh')):
    """Call the reference callback for one stage (stage20 in 0..19, reference numbering)."""
    fn = ref_callback(model)
    out = dict(f=np.zeros(1), gf=np.zeros(17), c=np.zeros(13), Jc=np.zeros(13 * 17), h=np.zeros(30), Jh=np.zeros(30 * 17))
    y = np.zeros(13)
    lam = np.zeros(64)
    z = np.ascontiguousarray(z, dtype=np.float64)
    p130 = np.ascontiguousarray(p130, dtype=np.float64)
    fn(P(z), P(y), P(lam), P(p130),
       P(out['f']) if 'f' in want else None, P(out['gf']) if 'gf' in want else None,
       P(out['c']) if 'c' in want else None, P(out['Jc']) if 'Jc' in want else None,
       P(out['h']) if 'h' in want else None, P(out['Jh']) if 'Jh' in want else None,
       None, ctypes.c_int(stage20), ctypes.c_int(0), ctypes.c_int(0))
    return out


def to_p130(p, M):
    """Re-lay a (10+4M)-parameter stage vector into the reference's 130-slot layout (nh = 30)."""
    if M == 30:
        return p
    q = np.zeros(130)
    q[:10] = p[:10]
    m = min(M, 30)
    q[10:10 + 3 * m] = p[10:10 + 3 * m]
    q[100:100 + m] = p[10 + 3 * M:10 + 3 * M + m]
    return q


def ref_stage_index(k, N):
    return 0 if k == 0 else (19 if k == N - 1 else 1)


class RefNLP:
    """The reference NLP assembled from the reference callbacks, for SciPy."""

    def __init__(self, N, M, model, xinit, params, nfaces):
        self.N, self.M, self.model, self.xinit = N, M, model, xinit
        self.p130 = [to_p130(params[k], M) for k in range(N)]
        self.nf = nfaces
        self.lb, self.ub = L.bounds()

    def fun(self, Z):
        z = Z.reshape(self.N, 17)
        f = 0.0
        g = np.zeros_like(z)
        for k in range(self.N):
            o = ref_stage(self.model, z[k], self.p130[k], ref_stage_index(k, self.N), ('f', 'gf'))
            f += o['f'][0]
            g[k] = o['gf']
        return f, g.ravel()

    def eq(self, Z):
        z = Z.reshape(self.N, 17)
        r = [z[0, 8:17] - self.xinit]
        for k in range(self.N - 1):
            o = ref_stage(self.model, z[k], self.p130[k], ref_stage_index(k, self.N), ('c',))
            r.append(o['c'] - np.r_[z[k + 1, 8:17], z[k + 1, 4:8]])
        return np.concatenate(r)

    def eq_jac(self, Z):
        z = Z.reshape(self.N, 17)
        n = 17 * self.N
        J = np.zeros((9 + 13 * (self.N - 1), n))
        J[0:9, 8:17] = np.eye(9)
        E = np.zeros((13, 17))
        E[0:9, 8:17] = np.eye(9)
        E[9:13, 4:8] = np.eye(4)
        for k in range(self.N - 1):
            o = ref_stage(self.model, z[k], self.p130[k], ref_stage_index(k, self.N), ('Jc',))
            r0 = 9 + 13 * k
            J[r0:r0 + 13, 17 * k:17 * k + 17] = o['Jc'].reshape(17, 13).T
            J[r0:r0 + 13, 17 * (k + 1):17 * (k + 2)] = -E
        return J

    def ineq(self, Z):  # SciPy convention: >= 0
        z = Z.reshape(self.N, 17)
        r = []
        for k in range(self.N):
            o = ref_stage(self.model, z[k], self.p130[k], ref_stage_index(k, self.N), ('h',))
            r.append(L.HU - o['h'][:self.nf[k]])
        return np.concatenate(r) if r else np.zeros(0)

    def ineq_jac(self, Z):
        z = Z.reshape(self.N, 17)
        rows = []
        for k in range(self.N):
            o = ref_stage(self.model, z[k], self.p130[k], ref_stage_index(k, self.N), ('Jh',))
            Jh = o['Jh'].reshape(17, 30).T[:self.nf[k]]
            blk = np.zeros((self.nf[k], 17 * self.N))
            blk[:, 17 * k:17 * k + 17] = -Jh
            rows.append(blk)
        return np.concatenate(rows) if rows else np.zeros((0, 17 * self.N))

    def solve(self, Z0, maxiter=400):
        cons = [dict(type='eq', fun=self.eq, jac=self.eq_jac)]
        if int(np.sum(self.nf)) > 0:
            cons.append(dict(type='ineq', fun=self.ineq, jac=self.ineq_jac))
        bnds = list(zip(np.tile(self.lb, self.N), np.tile(self.ub, self.N)))
        Z0 = np.clip(Z0, np.tile(self.lb, self.N), np.tile(self.ub, self.N))
        res = minimize(self.fun, Z0, jac=True, method='SLSQP', bounds=bnds, constraints=cons,
                       options=dict(ftol=1e-13, maxiter=maxiter))
        return res


def _job(args):
    fam, w1, start, seed = args
    N, M, model = w1['N'], w1['M'], w1['model']
    nlp = RefNLP(N, M, model, w1['xinit'], w1['params'], w1['nfaces'])
    if start == 'cold':
        Z0 = w1['x0'].ravel().copy()
    else:
        rng = np.random.default_rng(seed)
        Z0 = w1['z_oracle'].ravel() + 0.02 * rng.normal(size=17 * N)
    t = time.time()
    res = nlp.solve(Z0)
    eqn = float(np.max(np.abs(nlp.eq(res.x))))
    c = nlp.ineq(res.x)
    ineq = float(max(0.0, -c.min())) if c.size else 0.0
    return dict(z=res.x.reshape(N, 17), f=float(res.fun), status=int(res.status), nit=int(res.nit),
                eq=eqn, ineq=ineq, secs=time.time() - t, start=start)


def gen_stage_vectors(path, n=240, seed=W.SEED0):
    rng = np.random.default_rng(seed)
    lb, ub = L.bounds()
    rec = dict(z=[], p=[], stage=[], model=[], f=[], gf=[], c=[], Jc=[], h=[], Jh=[])
    for t in range(n):
        model = t % 2
        stage = [0, 7, 19][t % 3]
        z = lb + (ub - lb) * rng.random(17)
        p = np.zeros(130)
        p[:3] = rng.uniform(-5, 5, 3)
        p[3:6] = rng.uniform(-3, 3, 3)
        p[6:9] = rng.uniform(0.5, 80, 3)
        p[9] = rng.uniform(-3, 3)
        nf = [0, 6, 15, 30][t % 4]
        p[10:10 + 3 * nf] = rng.normal(size=3 * nf)
        p[100:100 + nf] = rng.normal(size=nf)
        o = ref_stage(model, z, p, stage)
        rec['z'].append(z); rec['p'].append(p); rec['stage'].append(stage); rec['model'].append(model)
        for k in ('f', 'gf', 'c', 'Jc', 'h', 'Jh'):
            rec[k].append(o[k].copy())
    np.savez_compressed(path, **{k: np.array(v) for k, v in rec.items()})
    print('wrote', path)


# ---- G2  exact second derivatives from the reference's first derivatives ------------------------------------------
# The reference callbacks never write a Hessian (casadi2forces.c:52), so the Hessians the solver uses are pinned against
# central differences of the callbacks' EXACT Jacobians: column j of the Hessian of nu'c(z) is d(Jc' nu)/dz_j, that of the
# cost d(grad f)/dz_j.  Each difference quotient is Richardson-extrapolated from two step sizes (h, h/2); the same over
# (h/2, h/4) gives the error estimate |R(h) - R(h/2)|.  Steps are scaled to each variable's range.
HESS_STEP = np.array([0.005] * 3 + [0.0125] + [0.005] * 3 + [0.0125] + [0.0125] * 3 + [0.005] * 6)  # (estimates <= 2e-11 relative; 4x these: 1e-9)


def _ref_grad_fn(model, p130, stage20, nu):
    if nu is None:
        return lambda z: ref_stage(model, z, p130, stage20, ('gf',))['gf']
    return lambda z: ref_stage(model, z, p130, stage20, ('Jc',))['Jc'].reshape(17, 13) @ nu


def ref_hessian(model, z, p130, stage20, nu=None, step=HESS_STEP):
    """Difference Hessian (17 x 17) of nu'c (nu: 13 multipliers in the reference's row order [pos vel att | carry]) or, with
    nu None, of the stage cost -- and its elementwise error estimate."""
    g = _ref_grad_fn(model, p130, stage20, nu)
    z = np.asarray(z, dtype=np.float64)

    def dq(j, h):
        e = np.zeros(17); e[j] = h
        return (g(z + e) - g(z - e)) / (2.0 * h)
    H = np.zeros((17, 17)); E = np.zeros((17, 17))
    for j in range(17):
        d1, d2, d4 = dq(j, step[j]), dq(j, step[j] / 2), dq(j, step[j] / 4)
        r1, r2 = (4.0 * d2 - d1) / 3.0, (4.0 * d4 - d2) / 3.0
        H[:, j] = r2
        E[:, j] = np.abs(r2 - r1)
    return H, E


def hessian_points(n, seed):
    """Stage points at the edges of the box and of the trigonometry: roll / pitch at -0.4 pi, 0, 0.4 pi; yaw at 0, +-pi,
    +-2 pi; rates at +-pi/2 (the RK2 midpoint attitude e + DT w moves furthest); T at t_min / t_max; v at +-2; f_ext = 0 or
    |f_ext| = 3; multipliers on the position rows only, the velocity rows only or both (with the linear attitude / carry
    rows set too), magnitudes 1e-3 .. 1e3.  Yields (model, stage20, z, p130, nu)."""
    rng = np.random.default_rng(seed)
    lb, ub = L.bounds()
    ang = [-0.4 * np.pi, 0.0, 0.4 * np.pi]
    yaws = [0.0, np.pi, -np.pi, 2 * np.pi, -2 * np.pi]
    for t in range(n):
        model = t % 2
        stage = [0, 7, 19][(t // 2) % 3]
        z = lb + (ub - lb) * rng.random(17)
        if t % 4 != 3:  # (every fourth point stays in the uniform interior)
            z[14] = ang[t % 3]
            z[15] = ang[(t // 3) % 3]
            z[16] = yaws[t % 5]
            if t % 7 < 4:
                z[0:3] = np.pi / 2 * np.sign(rng.normal(size=3))
            z[3] = (lb[3], ub[3])[t % 2 if t % 3 else 1 - t % 2]
            if t % 5 < 3:
                z[11:14] = 2.0 * np.sign(rng.normal(size=3))
        p = np.zeros(130)
        p[:3] = rng.uniform(-5, 5, 3)
        f = rng.normal(size=3)
        p[3:6] = 0.0 if t % 3 == 0 else 3.0 * f / np.linalg.norm(f)
        p[6:9] = rng.uniform(0.5, 80, 3)
        p[9] = rng.uniform(-3, 3)
        nu = rng.normal(size=13) * 10.0 ** rng.uniform(-3, 3)
        if t % 3 == 0:
            nu[3:6] = 0.0   # position rows only
        elif t % 3 == 1:
            nu[0:3] = 0.0   # velocity rows only
        yield model, stage, z, p, nu


def gen_hessian_vectors(path, n=96, seed=W.SEED0 + 17):
    """G2: difference Hessians of nu'c (stages with dynamics) and of the cost from the reference callbacks."""
    rec = dict(z=[], p=[], stage=[], model=[], nu=[], Hc=[], Hc_err=[], Hf=[], Hf_err=[])
    for model, stage, z, p, nu in hessian_points(n, seed):
        Hf, Ef = ref_hessian(model, z, p, stage)
        Hc, Ec = ref_hessian(model, z, p, stage, nu) if stage != 19 else (np.zeros((17, 17)), np.zeros((17, 17)))
        for k, v in (('z', z), ('p', p[:10]), ('stage', stage), ('model', model), ('nu', nu), ('Hc', Hc), ('Hc_err', Ec), ('Hf', Hf), ('Hf_err', Ef)):
            rec[k].append(v)
    np.savez_compressed(path, **{k: np.array(v) for k, v in rec.items()})
    print('wrote', path, os.path.getsize(path), 'bytes')


def gen_solutions(outdir, workers=int(os.environ.get('GEN_WORKERS', '8'))):
    import tests.oracle_lib as OL
    fams = {
        'config0': [(W.config0(L.MODEL_NORMAL), [0]), (W.config0(L.MODEL_FINAL, weights=W.NORMAL_WEIGHTS), [0]),
                    (W.config0(L.MODEL_NORMAL, (1.5, -2.0, 0.5)), [0]), (W.config0(L.MODEL_FINAL), [0])],
        # >= 100 seeded problems per family, at least half of them solved by SLSQP from the caller's own cold
        # start (fully independent of the oracle); a `final`-model group in every family that the final solver sees
        'config1': [(W.config1(80), list(range(80))), (W.config1(24, model=L.MODEL_FINAL, seed=W.SEED0 + 32), list(range(24)))],
        'config2': [(W.config2(100), list(range(100))), (W.config2(24, model=L.MODEL_FINAL, seed=W.SEED0 + 33), list(range(24)))],
        'config3': [(W.config3(80), list(range(80))), (W.config3(24, model=L.MODEL_FINAL, seed=W.SEED0 + 34), list(range(24)))],
        # round 4: hard-but-feasible instances -- reference 3..5 m away, |f_ext| 6..9 m/s^2, 5..10 cm of
        # corridor slack, post-replan warm starts (workloads.config_hard); the replan kind's old plans come from the oracle
        'hard': [(W.config_hard(160, replan_solver=lambda wo: OL.solve_batch(wo)[0]), list(range(160))),
                 (W.config_hard(32, model=L.MODEL_FINAL, seed=W.SEED0 + 42, replan_solver=lambda wo: OL.solve_batch(wo)[0]), list(range(32)))],
    }
    only = sys.argv[2:] if len(sys.argv) > 2 else None
    for fam, groups in fams.items():
        if only and fam not in only:
            continue
        jobs, meta = [], []
        for w, idx in groups:
            zo, fl, info = OL.solve_batch(w)
            for b in idx:
                w1 = dict(N=w['N'], M=w['M'], model=w['model'], xinit=w['xinit'][b], x0=w['x0'][b],
                          params=w['params'][b], nfaces=w['nfaces'][b], z_oracle=zo[b])
                start = 'cold' if fam == 'config0' or len(jobs) % 2 == 0 or fl[b] != 1 else 'near'
                jobs.append((fam, w1, start, 1000 + len(jobs)))
                meta.append(w1)
        t = time.time()
        with Pool(workers) as pool:
            res = pool.map(_job, jobs, chunksize=1)
        keep = dict(xinit=[], x0=[], params=[], nfaces=[], model=[], z=[], f=[], status=[], start=[], eq=[], ineq=[], nit=[])
        for w1, r in zip(meta, res):
            keep['xinit'].append(w1['xinit']); keep['x0'].append(w1['x0']); keep['params'].append(w1['params'])
            keep['nfaces'].append(w1['nfaces']); keep['model'].append(w1['model'])
            keep['z'].append(r['z']); keep['f'].append(r['f']); keep['status'].append(r['status'])
            keep['start'].append(r['start']); keep['eq'].append(r['eq']); keep['ineq'].append(r['ineq']); keep['nit'].append(r['nit'])
        path = os.path.join(outdir, f'solutions_{fam}.npz')
        np.savez_compressed(path, N=meta[0]['N'], M=meta[0]['M'], **{k: np.array(v) for k, v in keep.items()})
        st = np.array(keep['status'])
        print(f'wrote {path}: {len(res)} problems, status0={np.sum(st == 0)}, other={np.sum(st != 0)}, {time.time() - t:.0f}s', flush=True)


if __name__ == '__main__':
    out = os.path.join(ROOT, 'tests', 'golden')
    os.makedirs(out, exist_ok=True)
    if len(sys.argv) < 2 or sys.argv[1] == 'stage':
        gen_stage_vectors(os.path.join(out, 'stage_vectors.npz'))
    if len(sys.argv) < 2 or sys.argv[1] == 'hessian':
        gen_hessian_vectors(os.path.join(out, 'hessian_vectors.npz'))
    if len(sys.argv) < 2 or sys.argv[1] == 'solutions':
        gen_solutions(out)
