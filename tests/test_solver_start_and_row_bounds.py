"""The two places where the production constraint pipeline departs from the debug dump the stage tests read, checked per env
against the fp64 oracle:

- the solver START (MM_SKIP_QACCSM): an env with rows starts Newton from its warm start without comparing it with qacc_smooth.
  That is harmless only for a usable warm start; a NaN / Inf / far one must fall back to MuJoCo's rule (the oracle's cost
  comparison), and a poisoned env must never change a neighbour's result;
- the ROW BOUND (status bit 8): rows beyond mjModel.njmax are dropped by the oracle's rule (add_row / mmo_collide_and_add): every
  row kind stops at njmax itself (not at the engine's table size, njmax rounded up to 4), a contact whose rows do not all fit is
  dropped whole, and a LATER contact that fits still gets rows.
"""
import numpy as np
import pytest
import torch

from myosuite_amd import engine as E
from myosuite_amd.envs import registry
from myosuite_amd.model import spec as S
from myosuite_amd.model import synth
from oracle import oracle as O

MM_CON_CONTACT = 3
SCAN_MAX, SCAN_P99 = 2e-3, 3e-4     # the all-env scans' bounds (tests/test_gpu_widths.py)
# A FINITE start far from the solution (-1e3 x the env's qacc, or N(0, 1e4) noise) passes the start gate (finite, below 1e10):
# Newton converges from it, but in fp32 the rounding of the far start stays in the result.  Worst measured on MI355X, over every
# case of the warm-start test at the default budget and at 20: max 2.33e-3 (hand, -1e3 x qacc), p99 1.16e-3 (leg_implicit, -1e3 x
# qacc).  These bounds are those values + 30 %; under a budget of 19 the kernel follows MuJoCo's start rule and the far starts
# are held to the scan bounds.
FAR_MAX, FAR_P99 = 3e-3, 1.5e-3


def _variant(cm, **oi):
    """the compiled model with OPT_I words replaced (njmax / iterations): kernel and oracle read both from the blob"""
    arrays = {k: v.copy() for k, v in cm.arrays.items()}
    for k, v in oi.items():
        arrays["OPT_I"][S.C["MM_OI_" + k.upper()]] = v
    out = S.CompiledModel(cm.name, arrays, cm.names)
    for k in ("key_qpos", "key_qvel"):
        if hasattr(cm, k):
            setattr(out, k, getattr(cm, k))
    return out


def sphere_scene(njmax=0):
    """four free spheres on a plane, condim 3, 3, 1, 1 in pair order (4 + 4 + 1 + 1 rows when all touch)"""
    s = S.ModelSpec("spheres", timestep=0.002)
    s.add_geom("floor", "world", "plane", (0, 0, 0))
    for i, cd in enumerate((3, 3, 1, 1)):
        s.add_body(f"b{i}", "world", pos=(0.1 * i, 0.0, 0.03), mass=0.3, inertia=(1e-4, 1e-4, 1e-4))
        s.add_joint(f"f{i}", f"b{i}", "free")
        s.add_geom(f"s{i}", f"b{i}", "sphere", (0.03,))
        s.add_contact_pair("floor", f"s{i}", condim=cd, friction=(0.8, 0.005, 0.0001))
    if njmax:
        s.njmax = njmax
    return s.compile()


def rake_scene(njmax=0):
    """four free rakes of ten spheres each over a plane: 40 pairs, so a 32-lane launch sweeps them in two chunks.  Rakes 0-2 are
    condim 3 (pairs 0-29), rake 3 is condim 1 (pairs 30-39: two in the first chunk, eight in the second).  Sphere k of a rake sits
    k mm above sphere 0, so the rake's height decides how many of its spheres touch"""
    s = S.ModelSpec("rakes", timestep=0.002)
    s.add_geom("floor", "world", "plane", (0, 0, 0))
    for i in range(4):
        s.add_body(f"r{i}", "world", pos=(0.0, 0.6 * i, 0.02), mass=0.5, inertia=(1e-3, 1e-3, 1e-3))
        s.add_joint(f"f{i}", f"r{i}", "free")
        for k in range(10):
            s.add_geom(f"s{i}_{k}", f"r{i}", "sphere", (0.02,), pos=(0.05 * k, 0.0, 0.001 * k))
            s.add_contact_pair("floor", f"s{i}_{k}", condim=1 if i == 3 else 3, friction=(0.8, 0.005, 0.0001))
    s.nconmax = 40
    if njmax:
        s.njmax = njmax
    return s.compile()


def _rake_states(cm, n, seed):
    """each rake from 1 mm above the plane to 11 mm into it: 0 ... 10 of its spheres touch"""
    rng = np.random.default_rng(seed)
    q = np.tile(cm.qpos0.astype(np.float64), (n, 1))
    for i in range(4):
        q[:, 7 * i + 2] = 0.02 - rng.uniform(-0.001, 0.011, n)
    v = 0.05 * rng.standard_normal((n, cm.nv))
    return dict(qpos=q.astype(np.float32), qvel=v.astype(np.float32), act=np.zeros((n, 0), np.float32),
                warm=np.zeros((n, cm.nv), np.float32), ctrl=np.zeros((n, cm.nu), np.float32))


def _sphere_states(cm, n, seed):
    """spheres from 3 mm deep to 1 mm above the plane (a random subset touches), small random velocities"""
    rng = np.random.default_rng(seed)
    q = np.tile(cm.qpos0.astype(np.float64), (n, 1))
    for i in range(4):
        q[:, 7 * i + 2] = 0.03 + rng.uniform(-0.003, 0.001, n)
    v = 0.05 * rng.standard_normal((n, cm.nv))
    return dict(qpos=q.astype(np.float32), qvel=v.astype(np.float32), act=np.zeros((n, 0), np.float32),
                warm=np.zeros((n, cm.nv), np.float32), ctrl=np.zeros((n, cm.nu), np.float32))


def _limit_states(cm, n, seed):
    """test_forward_stages_match_oracle's states: joints spread 5 % past both ends of their ranges, zero warm start"""
    rng = np.random.default_rng(seed)
    lo, hi = cm.jnt_range[:, 0].astype(np.float64), cm.jnt_range[:, 1].astype(np.float64)
    return dict(qpos=((lo - 0.05 * (hi - lo)) + 1.1 * (hi - lo) * rng.random((n, cm.nq))).astype(np.float32),
                qvel=(2 * rng.standard_normal((n, cm.nv))).astype(np.float32), act=rng.random((n, cm.na)).astype(np.float32),
                warm=np.zeros((n, cm.nv), np.float32), ctrl=rng.random((n, cm.nu)).astype(np.float32))


def _oracle_rows(cm, st, e):
    d = O.OracleData(O.OracleModel(cm))
    d.qpos[:] = st["qpos"][e]; d.qvel[:] = st["qvel"][e]; d.forward()
    return d


def _kept_after_drop(d, cm, min_pair=0):
    """did the oracle give rows to a contact of pair >= min_pair after it had dropped an earlier contact?"""
    cond = cm.arrays["PAIR_CONDIM"]
    incl = cm.arrays["PAIR_MARGIN"] - cm.arrays["PAIR_GAP"]
    n, dropped = int(np.sum(d.efc_type != MM_CON_CONTACT)), False
    for c, p in enumerate(d.con_pair):
        if d.con_dist[c] >= incl[p]:
            continue
        k = 1 if cond[p] == 1 else 2 * (cond[p] - 1)
        if n + k > cm.njmax:
            dropped = True
        else:
            if dropped and p >= min_pair:
                return True
            n += k
    return False


def _stop_at_first_drop(d, cm):
    """the row count a kernel that drops every contact after the first dropped one would make"""
    cond = cm.arrays["PAIR_CONDIM"]
    incl = cm.arrays["PAIR_MARGIN"] - cm.arrays["PAIR_GAP"]
    n = int(np.sum(d.efc_type != MM_CON_CONTACT))
    for c, p in enumerate(d.con_pair):
        if d.con_dist[c] >= incl[p]:
            continue
        k = 1 if cond[p] == 1 else 2 * (cond[p] - 1)
        if n + k > cm.njmax:
            break
        n += k
    return n


# ------------------------------------------------------------------ oracle rule (CPU)
def test_oracle_row_bound_rule_on_a_mixed_condim_scene(oracle_lib):
    """all four spheres touch: rows 4 + 4 + 1 + 1.  njmax 6 drops the second (condim-3) contact whole and keeps BOTH condim-1
    contacts behind it; njmax 5 keeps the third and drops the fourth; every drop sets warn bit 2; a bound that fits warns nothing"""
    st = _sphere_states(sphere_scene(), 1, 0)
    for i in range(4):
        st["qpos"][0, 7 * i + 2] = 0.03 - 0.001 * (i + 1)        # distinct depths: a row's efc_pos names its contact
    st["qvel"][:] = 0
    expect = {10: [0, 1, 2, 3], 12: [0, 1, 2, 3], 9: [0, 1, 2], 8: [0, 1], 7: [0, 2, 3], 6: [0, 2, 3], 5: [0, 2], 4: [0], 3: [2, 3]}
    rows_of = [4, 4, 1, 1]
    for njmax, kept in expect.items():
        cm = sphere_scene(njmax)
        assert cm.njmax == njmax
        d = _oracle_rows(cm, st, 0)
        assert d.ncon == 4
        assert d.nefc == sum(rows_of[c] for c in kept), (njmax, d.nefc)
        assert np.all(d.efc_type == MM_CON_CONTACT)
        owner = [int(np.argmin(np.abs(d.con_dist[:4] - d.efc_pos[r]))) for r in range(d.nefc)]     # contact of every row
        assert all(abs(d.con_dist[c] - d.efc_pos[r]) < 1e-12 for r, c in enumerate(owner))
        assert owner == [c for c in kept for _ in range(rows_of[c])], (njmax, owner)
        assert bool(d.warn & 2) == (len(kept) < 4), (njmax, d.warn)
        # (the oracle keeps a contact after a dropped one exactly where the two rules differ)
        assert (_stop_at_first_drop(d, cm) != d.nefc) == (njmax in (7, 6, 5, 3))


def test_oracle_limit_rows_stop_at_njmax(oracle_lib):
    """limit and friction-loss rows beyond njmax are dropped in row order and flagged"""
    for name in ("hand", "friction_toy"):
        cm0 = synth.get_model(name)
        st = _limit_states(cm0, 16, 1)
        full = [_oracle_rows(cm0, st, e) for e in range(16)]
        for nj in (3, 5, 6, 7):
            cm = _variant(cm0, njmax=nj)
            for e in range(16):
                d = _oracle_rows(cm, st, e)
                assert d.nefc == min(nj, full[e].nefc)
                assert np.array_equal(d.efc_type, full[e].efc_type[:d.nefc])
                assert bool(d.warn & 2) == (full[e].nefc > nj)


def test_bench_models_keep_their_kernel_family():
    """the derived njmax counts every limit row: no shipped model is routed to the general-row kernels by the njmax rule"""
    for name in synth.builders():
        cm = synth.get_model(name)
        jt, jl = cm.arrays["JNT_TYPE"], cm.arrays["JNT_LIMITED"]
        nlim = int(np.sum((jl != 0) & ((jt == 2) | (jt == 3))))
        assert cm.njmax >= nlim, (name, cm.njmax, nlim)


# ------------------------------------------------------------------ GPU helpers
def _rollout(env_id, nenv, overrides=None, steps=5):
    """states of a short random-action rollout (as _all_env_solve_scan), with the batch's per-env model deltas"""
    env = registry.make(env_id, num_envs=nenv, seed=23, **(overrides or {}))
    env.rollout_setup(action_seed=3)
    for s in range(steps):
        env.rollout_step(None, stream_id=s)
    torch.cuda.synchronize()
    st, cm = env.state, env.cm
    out = dict(qpos=st.qpos.cpu().numpy(), qvel=st.qvel.cpu().numpy(), act=st.act.cpu().numpy() if cm.na else np.zeros((nenv, 0), np.float32),
               warm=st.qacc_warmstart.cpu().numpy(), ctrl=env.last_ctrl.cpu().numpy())
    for k, idk in (("geom_size_env", "geom_env_id"), ("geom_type_env", None), ("body_mass_env", "body_mass_env_id"), ("body_pos_env", "body_pos_env_id")):
        t = getattr(st, k)
        if t is not None:
            out[k] = t.clone()
            if idk:
                out[idk] = int(getattr(st._c, idk))
    return cm, out


def _batch(hm, st, warm=None):
    """a fresh BatchState of model `hm` holding the states `st` (warm start: `warm` if given) and their per-env model deltas"""
    n = st["qpos"].shape[0]
    b = E.BatchState(hm, n)
    dt = b.qpos.dtype
    b.qpos.copy_(torch.from_numpy(st["qpos"]).to(dt)); b.qvel.copy_(torch.from_numpy(st["qvel"]).to(dt))
    if hm.cm.na:
        b.act.copy_(torch.from_numpy(st["act"]).to(dt))
    b.qacc_warmstart.copy_(torch.from_numpy(st["warm"] if warm is None else warm).to(dt))
    if "geom_size_env" in st:
        b.set_geom_size_env(st["geom_env_id"], st["geom_size_env"])
        if "geom_type_env" in st:
            b.set_geom_type_env(st["geom_type_env"])
    if "body_mass_env" in st:
        b.set_body_mass_env(st["body_mass_env_id"], st["body_mass_env"])
    if "body_pos_env" in st:
        b.set_body_pos_env(st["body_pos_env_id"], st["body_pos_env"])
    return b


def _ctrl(st):
    return torch.from_numpy(np.ascontiguousarray(st["ctrl"], dtype=np.float32)).cuda()


def _gpu(cm, st, warm=None, lanes=0, precision=E.MM_PREC_F32, iterations=None, nsub=0):
    """one mm_forward (nsub = 0: qacc, nefc, status) or one mm_step of nsub substeps (qpos, qvel, status) on a fresh batch"""
    hm = E.HipModel(cm, lanes_per_env=lanes, precision=precision)
    if iterations is not None:
        hm.set_option("iterations", iterations)
    n = st["qpos"].shape[0]
    b = _batch(hm, st, warm)
    if nsub:
        E.step(hm, b, _ctrl(st), nsub)
        torch.cuda.synchronize()
        return b.qpos.cpu().numpy().astype(np.float64), b.qvel.cpu().numpy().astype(np.float64), b.status.cpu().numpy()
    dv = E.Derived(hm, n, ["qacc", "nefc"])
    E.forward(hm, b, _ctrl(st), dv)
    torch.cuda.synchronize()
    return dv["qacc"].cpu().numpy().astype(np.float64), dv["nefc"].cpu().numpy(), b.status.cpu().numpy()


def _oracle(om, st, e, warm=None, nsub=0):
    d = O.OracleData(om)
    if "geom_size_env" in st:
        gt = int(st["geom_type_env"][e]) if "geom_type_env" in st else -1
        d.set_geom_size(st["geom_env_id"], st["geom_size_env"][e].cpu().numpy().astype(np.float64), gt)
    if "body_mass_env" in st:
        d.set_body_mass(st["body_mass_env_id"], float(st["body_mass_env"][e]))
    if "body_pos_env" in st:
        d.set_body_pos(st["body_pos_env_id"], st["body_pos_env"][e].cpu().numpy().astype(np.float64))
    d.qpos[:] = st["qpos"][e]; d.qvel[:] = st["qvel"][e]; d.ctrl[:] = st["ctrl"][e]
    if om.cm.na:
        d.act[:] = st["act"][e]
    d.qacc_warmstart[:] = (st["warm"] if warm is None else warm)[e]
    if nsub:
        d.step(nsub)
    else:
        d.forward()
    return d


def _rel(a, b):
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max()))


# ------------------------------------------------------------------ A. warm starts the solver must not trust (GPU)
POISONS = ["nan1", "inf1", "nanrow", "far_neg", "far_noise", "permuted"]


def _poison(kind, warm, qacc, rng):
    """overwrite the warm start of every other env (odd envs) with `kind`"""
    w = warm.copy()
    n, nv = w.shape
    odd = np.arange(1, n, 2)
    for e in odd:
        j = int(rng.integers(0, nv))
        if kind == "nan1":
            w[e, j] = np.nan
        elif kind == "inf1":
            w[e, j] = np.inf if e % 4 == 1 else -np.inf
        elif kind == "nanrow":
            w[e] = np.nan
        elif kind == "far_neg":
            w[e] = -1e3 * qacc[e]
        elif kind == "far_noise":
            w[e] = rng.normal(0.0, 1e4, nv)
        elif kind == "permuted":
            w[e] = warm[(e + n // 2 + 1) % n]
    return w.astype(np.float32), odd


WARM_CASES = [  # env id, overrides, envs, lanes per env, precision
    ("myoHandPoseRandom-v0", {}, 64, 32, E.MM_PREC_F32),
    ("myoHandPoseRandom-v0", {}, 64, 64, E.MM_PREC_F32),
    ("myoHandPoseRandom-v0", {}, 32, 32, E.MM_PREC_F64_STATE),
    ("myoHandPoseRandom-v0", {"model": "hand_contact"}, 64, 64, E.MM_PREC_F32),     # (63 rows: one env per wave)
    ("myoHandReorient100-v0", {}, 64, 64, E.MM_PREC_F32),
    ("myoFatiLegWalk-v0", {}, 32, 64, E.MM_PREC_F32),
    ("myoFatiLegWalk-v0", {"model": "leg_implicit"}, 32, 64, E.MM_PREC_F32),
]


def _case_id(c):
    return f"{c[0]}{''.join('-' + v for v in c[1].values())}-n{c[2]}-G{c[3]}" + ("-f64state" if c[4] == E.MM_PREC_F64_STATE else "")


@pytest.mark.gpu
@pytest.mark.parametrize("env_id,overrides,nenv,lanes,prec", WARM_CASES, ids=[_case_id(c) for c in WARM_CASES])
def test_poisoned_warm_start_follows_the_oracle(oracle_lib, env_id, overrides, nenv, lanes, prec):
    """every other env's qacc_warmstart poisoned (NaN / Inf entries, a NaN row, far finite starts): per env, mm_forward's qacc and
    row count against the oracle from the same warm start, no bad-state / solver-cap bit the oracle does not have, one mm_step
    substep against the oracle's step, and the clean envs bit-identical to a launch in which nothing is poisoned"""
    cm, st = _rollout(env_id, nenv, overrides)
    om = O.OracleModel(cm)
    clean_qacc, clean_nefc, _ = _gpu(cm, st, lanes=lanes, precision=prec)
    rng = np.random.default_rng(7)
    worst = {}
    for kind in POISONS:
        warm, odd = _poison(kind, st["warm"], clean_qacc, rng)
        budgets = [None, 19, 20] if kind in ("far_neg", "far_noise", "permuted") else [None]
        for it in budgets:
            omx = om if it is None else O.OracleModel(_variant(cm, iterations=it))
            qa, nefc, status = _gpu(cm, st, warm, lanes=lanes, precision=prec, iterations=it)
            assert np.isfinite(qa).all(), (kind, it, np.where(~np.isfinite(qa).all(axis=1))[0][:8])
            # rows are made before the solver runs: the warm start cannot change an env's row count
            assert np.array_equal(nefc, clean_nefc), (kind, it, np.where(nefc != clean_nefc)[0][:8])
            even = np.arange(0, nenv, 2)
            if it is None:     # neighbour independence: the clean envs of the poisoned launch equal the all-clean launch bit for bit
                assert np.array_equal(qa[even], clean_qacc[even]), (kind, np.abs(qa[even] - clean_qacc[even]).max())
            rel = np.zeros(nenv); mism = np.zeros(nenv, bool)
            for e in range(nenv):
                d = _oracle(omx, st, e, warm)
                mism[e] = d.nefc != nefc[e]
                rel[e] = _rel(qa[e], d.qacc)
                if d.solver_niter < (it or cm.arrays["OPT_I"][S.C["MM_OI_ITERATIONS"]]):
                    assert not status[e] & 4, (kind, it, e)
                assert not status[e] & 1, (kind, it, e)
            ok = ~mism
            assert mism.sum() <= max(2, nenv // 100), (kind, it, int(mism.sum()))
            q = np.quantile(rel[ok], [0.99, 1.0])
            worst[(kind, it)] = float(q[1])
            bmax, bp99 = (FAR_MAX, FAR_P99) if kind.startswith("far") and it != 19 else (SCAN_MAX, SCAN_P99)
            assert q[1] < bmax and q[0] < bp99, (kind, it, q, np.argsort(rel)[-4:])
        # one substep of mm_step: no bad-state reset where MuJoCo steps normally
        qp, qv, status = _gpu(cm, st, warm, lanes=lanes, precision=prec, nsub=1)
        for e in range(nenv):
            d = _oracle(om, st, e, warm, nsub=1)
            assert bool(status[e] & 1) == bool(d.warn & 1), (kind, e, int(status[e]), d.warn)
            assert _rel(qp[e], d.qpos) < 1e-4 and _rel(qv[e], d.qvel) < 5e-3, (kind, e)
    print(f"poisoned warm starts {env_id} {overrides} G={lanes}: worst rel qacc err " + ", ".join(f"{k[0]}@{k[1]}: {v:.1e}" for k, v in worst.items()))


# ------------------------------------------------------------------ B. production path at stage tolerance (GPU)
def _implied_force_err(cm, om, st, e, qa):
    d = _oracle(om, st, e)
    M = d.full_M()
    return float(np.abs(M @ (qa - d.qacc)).max() / max(1.0, np.abs(d.qfrc_smooth).max())), _rel(qa, d.qacc)


PROD_CASES = [("limits-hand", None, 64, 32), ("limits-elbow", None, 64, 8),
              ("myoHandPoseRandom-v0", {"model": "hand_contact"}, 512, 0), ("myoHandReorient100-v0", {}, 512, 0),
              ("myoHandReorient100-v0", {"model": "hand_dense"}, 512, 0), ("myoFatiLegWalk-v0", {}, 512, 0),
              ("myoFatiLegWalk-v0", {"model": "leg_implicit"}, 512, 0), ("myoHandPenTwirlRandom-v0", {}, 512, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("src,overrides,nenv,lanes", PROD_CASES, ids=[c[0] + "".join("-" + v for v in (c[1] or {}).values()) for c in PROD_CASES])
def test_production_start_matches_the_debug_start(oracle_lib, src, overrides, nenv, lanes):
    """one production mm_forward (solver start: the warm start) and one debug dump (MuJoCo's start rule) on the same states, both
    against the oracle per env: qacc, and the implied constraint force M (qacc_gpu - qacc_oracle) in units of max(1, |qfrc_smooth|).
    The production error is at most twice the debug path's + 1e-5, and on the limit-only models within the stage tolerance"""
    if src.startswith("limits-"):
        cm = synth.get_model(src.split("-")[1])
        st = _limit_states(cm, nenv, 0)
    else:
        cm, st = _rollout(src, nenv, overrides)
    om = O.OracleModel(cm)
    qa, nefc, _ = _gpu(cm, st, lanes=lanes)
    hm = E.HipModel(cm, lanes_per_env=lanes)
    b = _batch(hm, st)
    dump = E.debug_dump(hm, b, _ctrl(st)).cpu().numpy()
    dq = dump[:, hm.layout("qacc"):hm.layout("qacc") + cm.nv].astype(np.float64)
    ep, ed, fp, fd = (np.zeros(nenv) for _ in range(4))
    mism = np.zeros(nenv, bool)
    for e in range(nenv):
        d = _oracle(om, st, e)
        mism[e] = d.nefc != nefc[e]
        fp[e], ep[e] = _implied_force_err(cm, om, st, e, qa[e])
        fd[e], ed[e] = _implied_force_err(cm, om, st, e, dq[e])
    ok = ~mism
    assert mism.sum() <= max(2, nenv // 100), int(mism.sum())
    print(f"production vs debug start {src} {overrides or ''}: rel qacc p50/p99/max prod {np.quantile(ep[ok], [0.5, 0.99, 1.0])} "
          f"debug {np.quantile(ed[ok], [0.5, 0.99, 1.0])}; implied force prod {np.quantile(fp[ok], [0.5, 0.99, 1.0])} debug {np.quantile(fd[ok], [0.5, 0.99, 1.0])}")
    bad = ok & ((ep > 2 * ed + 1e-5) | (fp > 2 * fd + 1e-5))
    assert not bad.any(), [(int(e), ep[e], ed[e], fp[e], fd[e]) for e in np.where(bad)[0][:6]]
    if src.startswith("limits-"):
        assert ep.max() < 2e-4 and fp.max() < 2e-4, (ep.max(), fp.max())


# ------------------------------------------------------------------ C. row overflow (GPU)
def _overflow_check(cm0, st, njmaxes, lanes=0):
    """per env and njmax: nefc equal, status bit 8 <=> oracle warn & 6, qacc within the scan bounds where nefc agrees.  Returns the
    number of envs that overflowed and the number in which the oracle kept a contact after dropping an earlier one"""
    n = st["qpos"].shape[0]
    n_over = n_after = 0
    for nj in njmaxes:
        cm = _variant(cm0, njmax=nj)
        om = O.OracleModel(cm)
        qa, nefc, status = _gpu(cm, st, lanes=lanes)
        rel = []
        for e in range(n):
            d = _oracle(om, st, e)
            assert nefc[e] == d.nefc, (nj, e, int(nefc[e]), d.nefc)
            assert bool(status[e] & 8) == bool(d.warn & 6), (nj, e, int(status[e]), d.warn)
            rel.append(_rel(qa[e], d.qacc))
            n_over += bool(d.warn & 6)
            n_after += _stop_at_first_drop(d, cm) != d.nefc
        q = np.quantile(rel, [0.99, 1.0])
        assert q[1] < SCAN_MAX and q[0] < SCAN_P99, (nj, q)
    return n_over, n_after


def _base_rows(cm, st, k=64):
    rows = [_oracle(O.OracleModel(cm), st, e).nefc for e in range(min(k, st["qpos"].shape[0]))]
    return max(2, int(np.median(rows)) - 2)


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [32, 64])
def test_row_overflow_sphere_scene(oracle_lib, lanes):
    cm = sphere_scene()
    st = _sphere_states(cm, 256, 5)
    n_over, n_after = _overflow_check(cm, st, [3, 5, 6, 7, 8, 9], lanes=lanes)
    assert n_over >= 200 and n_after >= 50, (n_over, n_after)


@pytest.mark.gpu
@pytest.mark.parametrize("name,lanes", [("hand", 32), ("hand", 64), ("friction_toy", 0)])
def test_row_overflow_limit_and_friction_rows(oracle_lib, name, lanes):
    """limit (and friction-loss) rows past an explicit njmax; for the hand an njmax below its limit count routes it to the
    general-row kernel, whose rows stop at njmax like the oracle's"""
    cm = synth.get_model(name)
    st = _limit_states(cm, 128, 2)
    base = _base_rows(cm, st)
    n_over, _ = _overflow_check(cm, st, [base, base + 1, base + 2, base + 3, max(1, base // 3)], lanes=lanes)
    assert n_over >= 128, n_over


@pytest.mark.gpu
@pytest.mark.parametrize("env_id,overrides", [("myoHandReorient100-v0", {"model": "hand_dense"}), ("myoHandPenTwirlRandom-v0", {})],
                         ids=["hand_dense", "pen"])
def test_row_overflow_contact_models(oracle_lib, env_id, overrides):
    """rollout states of the dense-contact hand (189 candidate pairs: an overflow falls across a pair-chunk boundary) and the
    condim-4 pen under explicit njmax values around their typical row counts"""
    cm, st = _rollout(env_id, 256, overrides)
    base = _base_rows(cm, st)
    n_over, n_after = _overflow_check(cm, st, [base, base + 1, base + 2, base + 3, max(1, base // 3)])
    assert n_over >= 64, (n_over, n_after)
    print(f"row overflow {env_id} {overrides}: base {base}, overflowing env-cases {n_over}, contact kept after a dropped one {n_after}")


@pytest.mark.gpu
def test_row_overflow_carries_the_rows_made_across_pair_chunks(oracle_lib):
    """the rake scene at 32 lanes per env: 40 pairs in two chunks of the pair sweep.  Condim-3 contacts of the first chunk overflow
    njmax and are dropped; condim-1 contacts of the SECOND chunk that still fit get rows, which needs the first chunk to carry the
    rows it actually made, not the rows it asked for.  Per env: nefc equal to the oracle's, bit 8 <=> oracle warning, qacc within
    the scan bounds; and the oracle kept a second-chunk contact after a drop in enough envs for the check to bite"""
    cm = rake_scene()
    st = _rake_states(cm, 256, 11)
    n_over, n_after = _overflow_check(cm, st, [9, 21, 22, 23, 24, 27, 31], lanes=32)
    n_chunk2 = 0
    for nj in (9, 21, 22, 23, 24, 27, 31):
        cmv = _variant(cm, njmax=nj)
        n_chunk2 += sum(_kept_after_drop(_oracle_rows(cmv, st, e), cmv, min_pair=32) for e in range(256))
    print(f"rake scene: overflowing env-cases {n_over}, contact kept after a dropped one {n_after}, of them in the second chunk {n_chunk2}")
    assert n_over >= 1000 and n_after >= 200 and n_chunk2 >= 50, (n_over, n_after, n_chunk2)


@pytest.mark.gpu
def test_kernel_family_routing():
    """the engine's own kernel family (MM_INFO_KERNEL_FAMILY, 2 = general rows): every shipped model with equality, contact,
    friction-loss or tendon-limit rows takes the general-row kernel; every shipped limit-rows-only model keeps its family at
    njmax = its limit count and moves to the general-row kernel one row below it -- the njmax rule fires exactly there, and the
    derived njmax of every shipped model is at least its limit count (test_bench_models_keep_their_kernel_family)"""
    fam = lambda cm_: E.HipModel(cm_).info(E.INFO_KERNEL_FAMILY)
    moved = 0
    for name in synth.builders():
        cm = synth.get_model(name)
        a = cm.arrays
        rows = cm.neq > 0 or cm.npair > 0 or bool(np.any(a["DOF_FRICTIONLOSS"] > 0)) or bool(np.any(a["TENDON_LIMITED"] != 0))
        jt, jl = a["JNT_TYPE"], a["JNT_LIMITED"]
        nlim = int(np.sum((jl != 0) & ((jt == 2) | (jt == 3))))
        f = fam(cm)
        if rows:
            assert f == 2, (name, f)
        elif f != 2 and nlim >= 2:
            assert fam(_variant(cm, njmax=nlim)) == f, name
            assert fam(_variant(cm, njmax=nlim - 1)) == 2, name
            moved += 1
    assert moved >= 3, moved
