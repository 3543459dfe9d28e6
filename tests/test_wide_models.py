"""The 25-40 dof kernels against the fp64 oracle, and a CPU table of which compiled kernel every parity case runs.

No synth model has more than 23 dofs on the limit-rows-only side or more than 34 on the general-row side, so the 32- and 40-wide
limit-row tiles, the 40-wide general-row tile and their RK4 forms were compiled and shipped without a test ever launching them.
`wide_forest` (below, local to the tests like test_rows128.rake_scene) makes forests of hinge trees in the style of
synth.make_tree_toy -- `ntree` trees on the world, each a `stem` of hinges carrying `nb` branches of `bl` hinges, the same link
constants -- that the host-only model compiler routes onto those instantiations (MODELS / ROUTES; asserted on the CPU through
tests/tools/kernel_choice_main.cpp, the compiler and planner as a plain host program under ASan + UBSan).

test_every_compiled_kernel_has_a_parity_case holds the table PARITY_CASES of (model, pinned lanes, precision) -> the test that
launches it, and compares what the host compiler selects for them with the X(...) entries of myosim_inst_list.hpp: the engine list,
the two-rows-per-lane list and the inverse library's Euler list must be covered exactly; the precision-mode and reset-observation
lists are covered or listed in NOT_RUN with a reason.

GPU tests (each new case asserts INFO_LANES / INFO_KERNEL_FAMILY and, per batch size, the width of the launch -- launch_lanes, which
for an unpinned limit-rows-only model is picked from the batch size and is what the host program prints too):
states by test_inverse.make_states' recipe with ctrl ~ U(-1, 1) (the motors' control range), 65 states, batches of 1, 3 and 65;
marginal envs (the only ones left out, at most 2 % per model, asserted on the CPU) decided from the oracle alone.  Bounds: the
forward-stage bounds of tests/test_gpu_widths.py CONFIGS (2e-4 limit rows, 5e-4 general rows; M 2e-5), 5e-5 / 5e-3 on qpos / qvel
after ten substeps (test_teacher_forced_env_step), median 5e-5 / max 2e-3 after 40 RK4 substeps (test_rk4_integrator_matches_oracle),
1e-8 over 20 substeps in precision mode (test_fuzz_models).  Every case runs with the model read through L2 and staged in LDS
(set_option "lds_model" 0 / 2); the two read the same words from another address space (myosim_engine_kernel_body.inc: `mb`), so
their outputs are also asserted bit-identical.  The Euler cases run a third time with waves_per_block pinned to 1: the one-wave-per-env form
that large batches launch (at 1, 3 and 65 envs the planner gives every env group a helper wave).

The descendant table: build_dof_tree packs a dof's descendants one byte each into 8 words, so a list holds 32 entries and the
33rd sends the model to the general-row family.  W32 (31 descendants under the root dof, one byte of the table left as the 0xff
terminator), W33 (32: every byte used, no terminator; Engine::sp_mul_m walks all `desc_words` words) and W34G (33: general rows)
sit on both sides of that limit.
"""
import functools
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from myosuite_amd import engine as E                                                # noqa: E402
from myosuite_amd.model import spec as S                                            # noqa: E402
from myosuite_amd.model import synth                                                # noqa: E402
from oracle import oracle as O                                                      # noqa: E402

from test_gpu_parity import _check_stage_dump                                       # noqa: E402  (same directory)
from test_gpu_widths import _oracle_flips_under_fp32_rounding                       # noqa: E402
from test_solver_start_and_row_bounds import _variant                               # noqa: E402

TOL_LIMIT, TOL_GEN = 2e-4, 5e-4         # tests/test_gpu_widths.py CONFIGS
STEP_Q, STEP_V = 5e-5, 5e-3             # tests/test_gpu_parity.py::test_teacher_forced_env_step
RK4_MEDIAN, RK4_MAX = 5e-5, 2e-3        # tests/test_gpu_parity.py::test_rk4_integrator_matches_oracle
F64_TOL = 1e-8                          # tests/test_fuzz_models.py: precision mode over 20 substeps
NSTATE, SEED = 65, 5                    # tests/test_inverse.py
BATCHES = (1, 3, 65)
NORMAL_JUMP, AXIS_GAP = 1e-3, 1e-4      # tests/test_inverse.py
PLANE_Z = 0.30                          # height of the tilted plane under the feature models' tips (metres)


# ------------------------------------------------------------------ the models
def wide_forest(ntree, stem, nb, bl, integrator=0, features=False, twigs=0):
    """`ntree` hinge trees on the world: a stem of `stem` hinges whose tip carries `nb` branches of `bl` hinges (and, on tree 0,
    `twigs` extra one-link branches); ranges, damping, armature and one motor per joint as synth.make_tree_toy's link().
    features: the general-row content -- a joint equality between the first tree and the LAST dof of the last tree, frictionloss
    on dof 3 and on the last dof but one, a limited fixed tendon over the last branch, a tilted plane under sphere tips (condim 3,
    the last one condim 1); every third joint is left without a range so that the rows stay inside 64."""
    s = S.ModelSpec(f"forest{ntree}x{stem}_{nb}x{bl}" + (f"t{twigs}" if twigs else "") + ("f" if features else ""), timestep=0.002,
                    integrator=integrator)
    n = [0]
    nv = ntree * (stem + nb * bl) + twigs

    def link(parent, axis, length, pos):
        i = n[0]; n[0] += 1
        s.add_body(f"b{i}", parent, pos=pos, mass=0.3 + 0.05 * (i % 3), ipos=(0, 0, -0.5 * length),
                   inertia=(0.3 * length * length / 12 + 1e-4, 0.3 * length * length / 12 + 1e-4, 2e-4))
        limited = not (features and i % 3 == 1)
        floss = 0.05 if features and i in (3, nv - 2) else 0.0
        s.add_joint(f"j{i}", f"b{i}", "hinge", axis=axis, range=(-0.9 + 0.1 * (i % 4), 0.8) if limited else None,
                    damping=0.05 + 0.01 * i, armature=0.002, frictionloss=floss)
        s.add_motor(f"m{i}", f"j{i}", gear=1.0 + 0.2 * (i % 5), ctrlrange=(-1.0, 1.0))
        return i

    ax = ((1, 0, 0), (0, 1, 0), (0.6, 0.8, 0))
    if features:
        s.add_geom("floor", "world", "plane", (0, 0, 0), pos=(0, 0, PLANE_Z), quat=(math.cos(0.04), math.sin(0.04), 0.0, 0.0))
    tips, last_branch = [], []
    for t in range(ntree):
        p = "world"
        for i in range(stem):
            p = f"b{link(p, ax[i % 3], 0.2, (0.7 * t, 0, 1.0) if i == 0 else (0, 0, -0.2))}"
        for k in range(nb):
            q, last_branch = p, []
            for i in range(bl):
                last_branch.append(link(q, ax[(k + i) % 3], 0.15, (0.08 * (k - 0.5 * (nb - 1)), 0, -0.2) if i == 0 else (0, 0, -0.15)))
                q = f"b{last_branch[-1]}"
            tips.append(q)
        if t == 0:
            for k in range(twigs):
                link(p, ax[k % 3], 0.1, (0, 0.08 * (k + 1), -0.2))
    assert n[0] == nv
    if features:
        s.add_equality_joint(f"j{nv - 1}", "j2", (0.0, 0.5), solref=(0.05, 1.0))
        s.add_tendon("branch_stop", [("joint", f"j{i}", 1.0 if k % 2 == 0 else -0.5) for k, i in enumerate(last_branch)], limited=True,
                     range=(-0.4, 0.5), solref=(0.02, 1.0))
        for k, q in enumerate(tips):
            s.add_geom(f"tip{k}", q, "sphere", (0.03,), pos=(0, 0, -0.15))
            s.add_contact_pair("floor", f"tip{k}", condim=1 if k == len(tips) - 1 else 3, friction=(0.8, 0.005, 0.0001))
        s.nconmax = len(tips)
    return s


# name -> (forest arguments, keywords)
MODELS = {
    "W25": ((1, 1, 8, 3), {}),                  # first dofs of the 32 tile; the stem's segment has 8 child segments
    "W28": ((2, 2, 3, 4), {}),                  # interior of the 32 tile, 32 and 64 lanes
    "W32": ((1, 2, 5, 6), {}),                  # full 32 tile (33 bodies: 64 lanes); 8 levels; the root dof has 31 descendants
    "W33": ((1, 2, 5, 6), {"twigs": 1}),        # first dof past 32: nvp 36 -> the 40 tile; the root dof has 32 descendants (a full table)
    "W36": ((2, 2, 4, 4), {}),                  # nvp 36, no limit-row kernel there: choose_width's second loop -> 40
    "W40": ((2, 2, 3, 6), {}),                  # the full 40 tile, no padding dof
    "G30": ((1, 2, 4, 7), {}),                  # 9 levels -> general rows on the 32 tile (row stride 36 at 32 lanes)
    "G38": ((2, 1, 3, 6), {"features": True}),  # general rows on the 40 tile: equality, friction loss, tendon limit, contacts
    # CPU only: the far side of each table limit
    "W34G": ((1, 2, 5, 6), {"twigs": 2}),       # 33 descendants: one more than the table holds
    "W28G": ((1, 1, 9, 3), {}),                 # 9 child segments
}
# (model, integrator, pinned lanes, precision) -> (lanes, nvp, general rows, integrator kernel, rows per lane) a launch must run.
# W25 and W28 are pinned: their default width is 32, but an unpinned limit-rows-only Euler model is launched at the width the
# planner picks from the batch size (pick_lanes: the widest with a kernel for a small batch), which is 64 for both.
ROUTES = {
    ("W25", 0, 32, 0): (32, 32, 0, 0, 1), ("W28", 0, 32, 0): (32, 32, 0, 0, 1), ("W28", 0, 64, 0): (64, 32, 0, 0, 1),
    ("W32", 0, 0, 0): (64, 32, 0, 0, 1), ("W33", 0, 0, 0): (64, 40, 0, 0, 1), ("W36", 0, 0, 0): (64, 40, 0, 0, 1),
    ("W40", 0, 0, 0): (64, 40, 0, 0, 1), ("G30", 0, 0, 0): (32, 32, 1, 0, 1), ("G38", 0, 0, 0): (64, 40, 1, 0, 1),
    ("W28", 1, 0, 0): (32, 32, 0, 1, 1), ("W40", 1, 0, 0): (64, 40, 0, 1, 1), ("G30", 1, 0, 0): (64, 32, 1, 1, 1),
    ("G38", 1, 0, 0): (64, 40, 1, 1, 1), ("G30", 0, 0, E.MM_PREC_F64_STATE): (64, 32, 1, 0, 1),
}
EULER_CASES = [k for k in ROUTES if k[1] == 0 and k[3] == 0]
RK4_CASES = [k for k in ROUTES if k[1] == 1]
# precision mode has no kernel at the 32 / 40 limit-row tiles, at 40 general rows, or on RK4
F64_REFUSED = [("W28", 0), ("W32", 0), ("W40", 0), ("G38", 0), ("G30", 1), ("W28", 1)]

# worst error per case as measured on an MI355X (information; the bounds are the constants above).  Forward: worst stage of the
# debug dump / production qacc, relative; step: |dqpos|, |dqvel| after ten substeps; RK4: median / max |dqpos| after 40.
MEASURED_WORST = {
    "W25-G32": dict(stage=1.9e-6, qacc=1.8e-6, qpos=1.8e-7, qvel=2.7e-6), "W28-G32": dict(stage=2.57e-6, qacc=2.57e-6, qpos=2.0e-7, qvel=5.7e-6),
    "W28-G64": dict(stage=2.55e-6, qacc=2.55e-6, qpos=2.0e-7, qvel=5.7e-6), "W32": dict(stage=5.3e-6, qacc=5.3e-6, qpos=2.1e-7, qvel=1.2e-5),
    "W33": dict(stage=5.5e-6, qacc=5.4e-6, qpos=2.1e-7, qvel=1.4e-5), "W36": dict(stage=2.9e-6, qacc=2.9e-6, qpos=1.7e-7, qvel=7.2e-6),
    "W40": dict(stage=5.2e-6, qacc=4.7e-6, qpos=1.8e-7, qvel=1.3e-5), "G30": dict(stage=1.2e-5, qacc=1.2e-5, qpos=2.6e-7, qvel=1.4e-5),
    "G38": dict(stage=8.3e-6, qacc=4.1e-6, qpos=4.7e-6, qvel=3.8e-4),
    "W28-rk4": dict(median=2.1e-7, max=3.6e-7), "W40-rk4": dict(median=2.1e-7, max=3.9e-7), "G30-rk4": dict(median=2.5e-7, max=4.9e-7),
    "G38-rk4": dict(median=9.5e-7, max=8.4e-6), "leg96": dict(qacc=1.5e-5, qfrc_constraint=4.3e-6),
    "G30-f64": dict(qpos=3.3e-16), "elbow-G4-f64": dict(qpos=2.2e-16), "elbow-G16-f64": dict(qpos=2.2e-16)}


def _case_id(k):
    return f"{k[0]}" + ("-rk4" if k[1] else "") + (f"-G{k[2]}" if k[2] else "") + ("-f64" if k[3] else "")


@functools.lru_cache(maxsize=None)
def wide_model(name, integrator=0):
    args, kw = MODELS[name]
    return wide_forest(*args, integrator=integrator, **kw).compile()


@functools.lru_cache(maxsize=None)
def leg96():
    """the leg with its row bound raised past one row per lane: the two-rows-per-lane kernel of the 36 tile"""
    return _variant(synth.get_model("leg"), njmax=96)


def make_states(cm, n=NSTATE, seed=SEED):
    """test_inverse.make_states' recipe with ctrl ~ U(-1, 1)"""
    from test_inverse import make_states as inverse_states
    st = inverse_states(cm, n, seed)
    st["ctrl"] = np.ascontiguousarray(np.random.default_rng(seed + 100).uniform(-1.0, 1.0, (n, cm.nu)), dtype=np.float32)
    return st


def dof_tree(cm):
    """(depth of every dof, number of descendants of every dof, child segments of every segment) from DOF_PARENTID"""
    par = [int(p) for p in cm.arrays["DOF_PARENTID"]]
    nv = len(par)
    depth, ndesc, nchild = [0] * nv, [0] * nv, [0] * nv
    for i in range(nv):
        if par[i] >= 0:
            depth[i] = depth[par[i]] + 1
            nchild[par[i]] += 1
        k = par[i]
        while k >= 0:
            ndesc[k] += 1
            k = par[k]
    # a dof starts a segment when its parent has another child too: the child segments of a segment are the children of its last dof
    child_segments = [c for c in nchild if c > 1]
    return depth, ndesc, child_segments


# ------------------------------------------------------------------ the compiler as a host program under the sanitizers
@pytest.fixture(scope="session")
def chooser(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("kernel_choice") / "kernel_choice_main")
    cmd = ["c++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
           os.path.join(ROOT, "tests", "tools", "kernel_choice_main.cpp")]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]
    return exe


_CHOICES = {}


BIG_BATCH = 1 << 20      # enough envs for pick_lanes to take the narrowest width a model has a kernel at


def kernel_choice(exe, tmp_path, cm, lanes=0, precision=0, nenv=1):
    """(code, lanes of a launch over `nenv` envs, nvp, general rows, integrator kernel, rows per lane, message) of the host compiler
    and planner for a compiled model"""
    key = (cm.hash(), lanes, precision, nenv)
    if key not in _CHOICES:
        blob = str(tmp_path / "model.blob")
        np.ascontiguousarray(cm.blob, dtype=np.uint32).tofile(blob)
        # (the sanitizer runtime is linked into the program; whatever else the process preloads stays as it is)
        env = dict(os.environ, ASAN_OPTIONS="verify_asan_link_order=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
        p = subprocess.run([exe, blob, str(lanes), str(precision), str(nenv)], capture_output=True, text=True, env=env, timeout=120)
        assert "Sanitizer" not in p.stderr and "runtime error:" not in p.stderr and p.returncode == 0, p.stderr[-6000:]
        lines = p.stdout.splitlines()
        _CHOICES[key] = tuple(int(v) for v in lines[0].split()) + (lines[1] if len(lines) > 1 else "",)
    return _CHOICES[key]


@pytest.mark.parametrize("case", list(ROUTES), ids=_case_id)
def test_wide_models_route_to_the_unreached_kernels(chooser, tmp_path, case):
    name, integ, lanes, prec = case
    for nenv in BATCHES + (BIG_BATCH,):
        got = kernel_choice(chooser, tmp_path, wide_model(name, integ), lanes, prec, nenv)
        assert got[0] == 0 and got[1:6] == ROUTES[case], (nenv, got)


def test_unpinned_w25_and_w28_launch_at_64_lanes(chooser, tmp_path):
    """why they are pinned: default width 32, launch width 64 until the batch fills 512 waves"""
    for name in ("W25", "W28"):
        assert kernel_choice(chooser, tmp_path, wide_model(name), 0, 0, 65)[1] == 64
        assert kernel_choice(chooser, tmp_path, wide_model(name), 0, 0, BIG_BATCH)[1] == 32


def test_wide_models_hit_their_edges(chooser, tmp_path):
    """the edges the models exist for, from the compiled arrays -- an edit to the generator cannot lose one silently"""
    cms = {n: wide_model(n) for n in MODELS}
    assert [cms[n].nv for n in ("W25", "W28", "W32", "W33", "W36", "W40", "G30", "G38")] == [25, 28, 32, 33, 36, 40, 30, 38]
    assert cms["W32"].nbody == 33 and cms["W28"].nbody == 29
    sparse = lambda n: kernel_choice(chooser, tmp_path, cms[n])[3] == 0
    # the descendant table: 31 entries, 32 (full) stay tree-sparse; 33 take the general-row family
    for n, most, keeps in (("W32", 31, True), ("W33", 32, True), ("W34G", 33, False)):
        depth, ndesc, segs = dof_tree(cms[n])
        assert max(ndesc) == most and sparse(n) == keeps, (n, max(ndesc), kernel_choice(chooser, tmp_path, cms[n]))
        assert max(depth) + 1 == 8                      # ... all three exactly 8 levels deep: the depth is not what moves W34G
    # 8 child segments stay, 9 leave
    for n, most, keeps in (("W25", 8, True), ("W28G", 9, False)):
        depth, ndesc, segs = dof_tree(cms[n])
        assert max(segs) == most and sparse(n) == keeps and max(depth) + 1 <= 8 and max(ndesc) <= 32, (n, segs)
    # 9 levels leave
    depth, ndesc, segs = dof_tree(cms["G30"])
    assert max(depth) + 1 == 9 and max(ndesc) <= 32 and max(segs) <= 8 and not sparse("G30")
    # the feature model: an equality across column 32, friction loss on both sides of it, a tendon limit over dofs >= 32, both condims
    g = cms["G38"]
    A = g.arrays
    assert g.njmax <= 64 and g.neq == 1 and g.ntendon == 1 and g.npair == 6
    dofs = sorted(int(A["JNT_DOFADR"][int(j)]) for j in (A["EQ_OBJ1ID"][0], A["EQ_OBJ2ID"][0]))
    assert dofs[0] < 32 <= dofs[1], dofs
    fl = np.flatnonzero(A["DOF_FRICTIONLOSS"] > 0)
    assert len(fl) == 2 and fl[0] < 32 <= fl[1], fl
    assert int(A["TENDON_LIMITED"][0]) == 1 and min(int(x) for x in A["TENJ_DOF"]) >= 32 and len(A["TENJ_DOF"]) == 6
    assert sorted(int(c) for c in A["PAIR_CONDIM"]) == [1, 3, 3, 3, 3, 3]
    # the leg at njmax 96: rows2<36>
    assert kernel_choice(chooser, tmp_path, leg96())[:6] == (0, 64, 36, 1, 0, 2)


def test_a_38_dof_general_row_model_is_accepted(chooser, tmp_path):
    """README limits row: nv <= 40 on both families (the 36-dof figure was the widest model anyone had, not a limit)"""
    assert kernel_choice(chooser, tmp_path, wide_model("G38"))[:4] == (0, 64, 40, 1)
    over = wide_forest(1, 1, 8, 5).compile()
    assert over.nv == 41
    got = kernel_choice(chooser, tmp_path, over)
    assert got[0] != 0 and "largest compiled dense tile (40)" in got[6], got


@pytest.mark.parametrize("name,integ", F64_REFUSED, ids=[f"{n}-{'rk4' if i else 'euler'}" for n, i in F64_REFUSED])
def test_precision_mode_is_refused_on_the_host(chooser, tmp_path, name, integ):
    got = kernel_choice(chooser, tmp_path, wide_model(name, integ), 0, E.MM_PREC_F64)
    assert got[0] == -3 and got[6].startswith("precision: no fp64 kernel"), got          # MM_EUNSUPPORTED (include/myosim.h)


# ------------------------------------------------------------------ the fp64 reference, once per model
class Ref:
    pass


@functools.lru_cache(maxsize=None)
def refs(name, integrator=0):
    """(compiled model, states, Ref): per state the oracle's forward pass (qacc, nefc, marginal) and its state after ten Euler /
    forty RK4 substeps -- computed once, shared by every test, never modified"""
    O.build()
    cm = wide_model(name, integrator)
    om = O.OracleModel(cm)
    st = make_states(cm)
    r = Ref()
    r.qacc, r.nefc, r.ncon, r.warn = np.zeros((NSTATE, cm.nv)), np.zeros(NSTATE, int), np.zeros(NSTATE, int), 0
    r.marginal = np.zeros(NSTATE, bool)
    nsub = 40 if integrator == 1 else 10
    r.qpos, r.qvel, r.time = np.zeros((NSTATE, cm.nq)), np.zeros((NSTATE, cm.nv)), np.zeros(NSTATE)
    gs = cm.arrays["GEOM_SIZE"].reshape(-1, 3)
    for e in range(NSTATE):
        d = O.OracleData(om)
        d.qpos[:] = st["qpos"][e]; d.qvel[:] = st["qvel"][e]; d.ctrl[:] = st["ctrl"][e]
        d.forward()
        r.qacc[e], r.nefc[e], r.ncon[e] = d.qacc, d.nefc, d.ncon
        r.warn |= int(d.warn)
        q64 = st["qpos"][e].astype(np.float64)
        m = _oracle_flips_under_fp32_rounding(om, cm, None, e, q64, st["qvel"][e], st["act"][e], st["ctrl"][e], st["warm"][e], d.nefc, False)
        if not m and cm.npair:      # tests/test_inverse.py: NORMAL_JUMP / AXIS_GAP
            rng = np.random.default_rng(1000 + e)
            nc, n0 = d.ncon, d.con_frame[:d.ncon, :3].copy()
            for _ in range(12):
                d2 = O.OracleData(om)
                d2.qpos[:] = q64 + 3e-7 * np.maximum(1.0, np.abs(q64)) * rng.choice([-1.0, 1.0], size=q64.shape)
                d2.qvel[:] = st["qvel"][e]; d2.ctrl[:] = st["ctrl"][e]
                d2.forward()
                if d2.ncon != nc or (nc and float(np.linalg.norm(d2.con_frame[:nc, :3] - n0, axis=1).max()) > NORMAL_JUMP):
                    m = True
            for c, p in enumerate(d.con_pair):
                g1, g2 = int(cm.arrays["PAIR_GEOM1"][p]), int(cm.arrays["PAIR_GEOM2"][p])
                if all(int(cm.arrays["GEOM_TYPE"][g]) in (S.C["MM_GEOM_SPHERE"], S.C["MM_GEOM_CAPSULE"]) for g in (g1, g2)):
                    m = m or float(d.con_dist[c] + gs[g1, 0] + gs[g2, 0]) < AXIS_GAP
        r.marginal[e] = m
        d.step(nsub)
        r.warn |= int(d.warn)
        r.qpos[e], r.qvel[e], r.time[e] = d.qpos, d.qvel, d.time
    return cm, st, r


REF_CASES = sorted({(k[0], k[1]) for k in ROUTES})


@pytest.mark.parametrize("name,integ", REF_CASES, ids=[f"{n}-{'rk4' if i else 'euler'}" for n, i in REF_CASES])
def test_few_states_are_marginal_and_the_oracle_steps_them(oracle_lib, name, integ):
    cm, st, r = refs(name, integ)
    print(f"{name}: rows {r.nefc.min()}-{r.nefc.max()}, contacts {r.ncon.min()}-{r.ncon.max()}, marginal {np.flatnonzero(r.marginal)}, warn {r.warn}")
    assert np.isfinite(r.qpos).all() and np.isfinite(r.qvel).all() and np.isfinite(r.qacc).all() and r.warn == 0
    assert r.marginal.sum() <= 0.02 * NSTATE, np.flatnonzero(r.marginal)
    assert r.nefc.max() > 0 and r.nefc.max() <= cm.njmax
    if name == "G38":       # the feature rows are live: contacts in at least a third of the states, several at once somewhere
        assert (r.ncon > 0).sum() >= NSTATE // 3 and r.ncon.max() >= 3 and r.ncon.max() <= cm.nconmax, r.ncon


# ------------------------------------------------------------------ which compiled kernel every parity case runs
def listed_kernels():
    """name of the list -> [(lanes, nvp, general rows, integrator kernel)] of myosim_inst_list.hpp"""
    text = open(os.path.join(E.CSRC, "myosim_inst_list.hpp")).read()
    groups = {k: [tuple(int(v) for v in x) for x in re.findall(r"X\((\d+), (\d+), (\d+), (\d+)\)", body)]
              for k, body in re.findall(r"#define MM_KERNELS_(\w+)\(X\)(.*)", text)}
    order = re.findall(r"MM_KERNELS_(\w)\(X\)", re.search(r"#define MM_KERNEL_LIST\(X\)(.*)", text).group(1))
    assert sorted(order) == list("ABCDEFGHIJ")
    f64 = [k for g in re.findall(r"MM_KERNELS_(F64_\w)\(X\)", re.search(r"#define MM_KERNELS_F64\(X\)(.*)", text).group(1)) for k in groups[g]]
    return {"engine": [k for g in order for k in groups[g]], "rows2": groups["S"], "f64": f64, "obs": groups["OBS"]}


def _synth(name):
    return lambda: synth.get_model(name)


def _spec(make, integrator):
    def thunk():
        s = make(); s.integrator = integrator
        return s.compile()
    return thunk


def _fuzz(seed, integrator):
    def thunk():
        from test_fuzz_models import random_model
        return random_model(seed, integrator).compile()
    return thunk


def _rake():
    from test_rows128 import rake_scene
    return rake_scene()


P64, P64S = E.MM_PREC_F64, E.MM_PREC_F64_STATE
# (list, model thunk, pinned lanes, precision, the test that launches it).  The integrator is the model's.
PARITY_CASES = \
    [("engine", _synth("elbow"), g, 0, f"test_gpu_parity::test_forward_stages_match_oracle[elbow-G{g}]") for g in (4, 8, 16, 32, 64)] + \
    [("engine", _synth("hand"), g, 0, f"test_gpu_parity::test_forward_stages_match_oracle[hand-G{g}]") for g in (32, 64)] + [
        ("engine", _synth("friction_toy"), 0, 0, "test_contacts::test_friction_loss_gpu_matches_oracle"),
        ("engine", _synth("contact_toy"), 0, 0, "test_contacts::test_gpu_general_rows_forward_and_rollout_match_oracle[contact_toy]"),
        ("engine", _synth("plane_toy"), 0, 0, "test_contacts::test_gpu_general_rows_forward_and_rollout_match_oracle[plane_toy]"),
        ("engine", _synth("leg"), 0, 0, "test_contacts::test_gpu_general_rows_forward_and_rollout_match_oracle[leg]"),
        ("engine", _synth("hand_hold"), 0, 0, "test_objhold::test_gpu_objhold_env_matches_oracle_env[myoHandObjHoldRandom-v0]"),
        ("engine", _synth("hand_contact"), 0, 0, "test_contacts::test_self_colliding_hand_gpu_matches_oracle"),
        ("engine", _spec(synth.make_elbow, 1), 0, 0, "test_gpu_parity::test_rk4_integrator_matches_oracle[elbow]"),
        ("engine", _spec(synth.make_hand, 1), 0, 0, "test_gpu_parity::test_rk4_integrator_matches_oracle[hand]"),
        ("engine", _spec(synth.make_contact_toy, 1), 0, 0, "test_gpu_parity::test_rk4_integrator_matches_oracle[contact_toy]"),
        ("engine", _fuzz(11, 1), 0, 0, "test_fuzz_models::test_gpu_random_models_on_rk4_and_implicitfast[11-1]"),
        ("engine", _spec(synth.make_elbow, 3), 0, 0, "test_implicitfast::test_hip_implicitfast_matches_oracle[elbow]"),
        ("engine", _spec(synth.make_hand, 3), 0, 0, "test_implicitfast::test_hip_implicitfast_matches_oracle[hand]"),
        ("engine", _synth("leg_implicit"), 0, 0, "test_implicitfast::test_hip_implicitfast_matches_oracle[leg_implicit]"),
        ("rows2", _rake, 0, 0, "test_rows128::test_rows_above_64_are_live"),
        ("rows2", _synth("hand_dense_full"), 0, 0, "test_rows128::test_hand_dense_full_parity_scan"),
        ("rows2", leg96, 0, 0, "test_wide_models::test_leg_at_njmax_96_runs_the_two_row_kernel_of_the_36_tile"),
        ("f64", _synth("elbow"), 8, P64S, "test_gpu_widths::test_north_star_precision_modes_strict_gate[elbow-G8]"),
        ("f64", _synth("hand"), 32, P64S, "test_gpu_widths::test_north_star_precision_modes_strict_gate[hand-G32]"),
        ("f64", _synth("hand"), 64, P64S, "test_gpu_widths::test_north_star_precision_modes_strict_gate[hand-G64]"),
        ("f64", _synth("elbow"), 4, P64S, "test_wide_models::test_precision_mode_elbow_at_the_widths_nothing_else_pins[4]"),
        ("f64", _synth("elbow"), 16, P64S, "test_wide_models::test_precision_mode_elbow_at_the_widths_nothing_else_pins[16]"),
        ("f64", _synth("hand_contact"), 0, P64S, "test_gpu_widths::test_general_row_models_in_precision_mode_track_the_oracle[myoHandPoseRandom-v0-hand_contact]"),
        ("f64", _synth("hand_reorient"), 0, P64S, "test_gpu_widths::test_general_row_models_in_precision_mode_track_the_oracle[myoHandReorient100-v0]"),
        ("f64", _synth("leg"), 0, P64S, "test_gpu_widths::test_general_row_models_in_precision_mode_track_the_oracle[myoLegWalk-v0]"),
        ("f64", _synth("leg_implicit"), 0, P64S, "test_gpu_widths::test_general_row_models_in_precision_mode_track_the_oracle[myoLegWalk-v0-leg_implicit]"),
        # reset-observation kernels: the test whose reference path re-arms the finished envs by a separate masked reset, whose first
        # observation is the reset-observation launch (env.reset(mask=...) -> mm_task.obs_only), against the reset folded into the step
        ("obs", _synth("hand_reorient"), 0, 0, "test_gpu_widths::test_folded_walk_and_reorient_reset_matches_the_separate_reset[reorient]"),
        ("obs", _synth("leg"), 0, 0, "test_gpu_widths::test_folded_walk_and_reorient_reset_matches_the_separate_reset[leg]"),
        ("obs", _synth("leg_implicit"), 0, 0, "test_gpu_widths::test_folded_walk_and_reorient_reset_matches_the_separate_reset[leg-implicitfast]"),
    ] + [("engine", functools.partial(wide_model, k[0], k[1]), k[2], k[3], f"test_wide_models::{'test_rk4_steps' if k[1] else 'test_forward_and_step'}[{_case_id(k)}]")
         for k in ROUTES if not k[3]] + \
    [("f64", functools.partial(wide_model, "G30", 0), 0, P64S, "test_wide_models::test_precision_mode_on_the_wide_models")]
# compiled precision-mode / reset-observation kernels that no test launches, each with its reason (none today)
NOT_RUN = {}


def collected_test_ids(modules):
    """the node ids pytest collects from the cited modules, as "module::test[id]" (one collection run in a process of its own: the
    ids of stacked parametrize marks are pytest's to compose)"""
    files = [os.path.join("tests", m + ".py") for m in sorted(modules)]
    p = subprocess.run([sys.executable, "-m", "pytest", "--collect-only", "-q", "-p", "no:cacheprovider"] + files, cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    return {ln.split("/")[-1].replace(".py::", "::", 1) for ln in p.stdout.splitlines() if "::" in ln}


def test_every_compiled_kernel_has_a_parity_case(chooser, tmp_path):
    listed = listed_kernels()
    assert len(listed["engine"]) == 28 and len(set(listed["engine"])) == 28
    reached = {k: {} for k in listed}
    collected = collected_test_ids({c[4].split("::")[0] for c in PARITY_CASES})
    for which, thunk, lanes, prec, test_id in PARITY_CASES:
        assert test_id in collected, test_id          # the cited case exists under exactly that id
        # the width of the LAUNCH: an unpinned limit-rows-only model runs at the width the batch size picks, so a case counts only
        # if a single-env batch and a huge one launch the same instantiation (pinned, or only one width has a kernel)
        got = kernel_choice(chooser, tmp_path, thunk(), lanes, prec, 1)
        assert got == kernel_choice(chooser, tmp_path, thunk(), lanes, prec, BIG_BATCH), (test_id, got)
        assert got[0] == 0 and (not lanes or got[1] == lanes), (test_id, got)
        key = got[1:5]
        assert (got[5] == 2) == (which == "rows2"), (test_id, got)
        assert key in listed[which], (test_id, got)          # (a case filed under a list its kernel is not in)
        reached[which].setdefault(key, test_id)
    for which in listed:
        print(f"--- {which}")
        for k in listed[which]:
            print(f"  {k}: {reached[which].get(k) or 'NOT RUN: ' + NOT_RUN.get((which,) + k, '?')}")
    for which in ("engine", "rows2"):
        assert set(reached[which]) == set(listed[which]), sorted(set(listed[which]) - set(reached[which]))
    for which in ("f64", "obs"):
        left = set(listed[which]) - set(reached[which])
        assert left == {k[1:] for k in NOT_RUN if k[0] == which}, sorted(left)
    # the inverse library: one k_inverse per Euler entry of the engine list, each reached by a (model, width) of test_inverse.GPU_MODELS
    import test_inverse as TI
    inv = set()
    for name, lanes, _ in TI.GPU_MODELS:
        got = kernel_choice(chooser, tmp_path, TI.get_model(name), lanes, 0)
        assert got[0] == 0 and got[1] == lanes and got[4] == 0 and got[5] == 1, (name, lanes, got)
        inv.add(got[1:4])
    assert inv == {k[:3] for k in listed["engine"] if k[3] == 0} == set(TI.INSTANTIATIONS), sorted({k[:3] for k in listed["engine"] if k[3] == 0} - inv)


# ------------------------------------------------------------------ GPU
def _hip_model(case, lds_model, waves_per_block=0):
    name, integ, lanes, prec = case
    hm = E.HipModel(wide_model(name, integ), lanes_per_env=lanes, precision=prec)
    want = ROUTES[case]
    assert hm.info(E.INFO_LANES) == want[0] and hm.info(E.INFO_KERNEL_FAMILY) == (2 if want[2] else 1), (hm.info(E.INFO_LANES), hm.info(E.INFO_KERNEL_FAMILY))
    for n in BATCHES:          # INFO_LANES is the model's default width; this is the width of the launch
        assert hm.launch_lanes(n) == want[0] and hm.launch_info(n)["lanes"] == want[0], (n, hm.launch_lanes(n))
    hm.set_option("lds_model", lds_model)
    if waves_per_block:
        hm.set_option("waves_per_block", waves_per_block)
    return hm


def _launch_variants(case, n):
    """[(tag, HipModel)]: the model through L2 and staged in LDS (where "always" does not fit in LDS the launch is refused with
    MM_ELDS, asserted, and the planner's own choice runs instead) -- the first two, whose outputs must be bit-identical -- then
    the one-wave-per-env form of the kernel that large batches run (waves_per_block pinned: no helper waves), Euler only"""
    out = [(0, _hip_model(case, 0))]
    hm = _hip_model(case, 2)
    try:
        info = hm.launch_info(n)
        assert info["lds_model"] == 1, info
        out.append((2, hm))
    except E.EngineError as exc:
        assert "LDS" in str(exc), exc
        hm = _hip_model(case, 1)
        hm.launch_info(n)
        out.append((1, hm))
    assert out[0][1].launch_info(n)["lds_model"] == 0
    if case[1] == 0:
        assert out[0][1].launch_info(n)["two_wave"] == 1          # (small batches: every env group has a helper wave)
        hm = _hip_model(case, 1, waves_per_block=1)
        assert hm.launch_info(n)["two_wave"] == 0
        out.append(("one-wave", hm))
    return out


def _dump_and_nefc(hm, b, ctrl, n):
    """engine.debug_dump with the row count of that same launch"""
    buf = torch.zeros(n, hm.layout("total"), dtype=torch.float32, device=hm.device)
    dv = E.Derived(hm, n, ["nefc"])
    E.lib().mm_debug_set_dump(buf.data_ptr())
    try:
        E.forward(hm, b, ctrl, dv)
        torch.cuda.synchronize()
    finally:
        E.lib().mm_debug_set_dump(None)
    return buf.cpu().numpy(), dv["nefc"].cpu().numpy()


def _batch(hm, st, n):
    b = E.BatchState(hm, n)
    dt = b.qpos.dtype
    b.qpos.copy_(torch.from_numpy(st["qpos"][:n]).to(dt)); b.qvel.copy_(torch.from_numpy(st["qvel"][:n]).to(dt))
    return b


def _note(key, **worst):
    print(f"MEASURED {key}: " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()))


@pytest.mark.gpu
@pytest.mark.parametrize("case", EULER_CASES, ids=_case_id)
def test_forward_and_step(oracle_lib, case):
    """every forward stage, M and qfrc_constraint of the debug dump; qacc and nefc of the production path; ten substeps"""
    name, integ, lanes, prec = case
    cm, st, r = refs(name, integ)
    om = O.OracleModel(cm)
    tol = TOL_GEN if ROUTES[case][2] else TOL_LIMIT
    worst = dict(stage=0.0, qacc=0.0, qpos=0.0, qvel=0.0)
    for n in BATCHES:
        keep = [e for e in range(n) if not r.marginal[e]]
        ctrl = torch.from_numpy(st["ctrl"][:n]).cuda()
        outs = []
        for lm, hm in _launch_variants(case, n):
            b = _batch(hm, st, n)
            dump, dump_nefc = _dump_and_nefc(hm, b, ctrl, n)
            for e in keep:
                assert dump_nefc[e] == r.nefc[e], (n, lm, e, int(dump_nefc[e]), int(r.nefc[e]))
            w = _check_stage_dump(cm, hm, om, dump, st["qpos"], st["qvel"], st["act"], st["ctrl"], keep, tol=tol)
            worst["stage"] = max(worst["stage"], max(w.values()) if w else 0.0)
            b = _batch(hm, st, n)
            dv = E.Derived(hm, n, ["qacc", "nefc"])
            E.forward(hm, b, ctrl, dv)
            torch.cuda.synchronize()
            qacc, nefc = dv["qacc"].cpu().numpy().astype(np.float64), dv["nefc"].cpu().numpy()
            assert int(b.status.max()) == 0
            for e in keep:
                assert nefc[e] == r.nefc[e], (n, lm, e, int(nefc[e]), int(r.nefc[e]))
                err = float(np.abs(qacc[e] - r.qacc[e]).max() / max(1e-9, np.abs(r.qacc[e]).max()))
                worst["qacc"] = max(worst["qacc"], err)
                assert err < tol, (n, lm, e, err)
            b = _batch(hm, st, n)
            E.step(hm, b, ctrl, 10)
            torch.cuda.synchronize()
            qp, qv = b.qpos.cpu().numpy(), b.qvel.cpu().numpy()
            assert int(b.status.max()) == 0, b.status.cpu().numpy()
            for e in keep:
                eq, ev = float(np.abs(qp[e] - r.qpos[e]).max()), float(np.abs(qv[e] - r.qvel[e]).max())
                worst["qpos"], worst["qvel"] = max(worst["qpos"], eq), max(worst["qvel"], ev)
                assert eq < STEP_Q and ev < STEP_V, (n, lm, e, eq, ev)
            outs.append((dump, qacc, qp, qv))
        for a, c in zip(outs[0], outs[1]):          # the two model sources: the same words, the same arithmetic
            assert np.array_equal(a, c)
    _note(_case_id(case), **worst)


@pytest.mark.gpu
@pytest.mark.parametrize("case", RK4_CASES, ids=_case_id)
def test_rk4_steps(oracle_lib, case):
    """40 RK4 substeps against the oracle's mmo_rk4, and the time row"""
    name, integ, lanes, prec = case
    cm, st, r = refs(name, integ)
    worst = dict(median=0.0, max=0.0)
    for n in BATCHES:
        keep = [e for e in range(n) if not r.marginal[e]]
        ctrl = torch.from_numpy(st["ctrl"][:n]).cuda()
        outs = []
        for lm, hm in _launch_variants(case, n):
            b = _batch(hm, st, n)
            E.step(hm, b, ctrl, 40)
            torch.cuda.synchronize()
            qp = b.qpos.cpu().numpy()
            err = np.abs(qp - r.qpos[:n]).max(axis=1)[keep]
            worst["median"], worst["max"] = max(worst["median"], float(np.median(err))), max(worst["max"], float(err.max()))
            assert np.median(err) < RK4_MEDIAN and err.max() < RK4_MAX, (n, lm, float(np.median(err)), float(err.max()))
            np.testing.assert_allclose(b.time.cpu().numpy(), r.time[:n], rtol=1e-5)
            assert int(b.status.max()) == 0
            outs.append(qp)
        assert np.array_equal(outs[0], outs[1])
    _note(_case_id(case), **worst)


@pytest.mark.gpu
def test_leg_at_njmax_96_runs_the_two_row_kernel_of_the_36_tile(oracle_lib):
    """k_engine_rows2<36>: the leg with njmax 96, test_rows128's forward check (nefc equal, qacc and qfrc_constraint inside STAGE_TOL)
    on the states of test_inverse's leg case"""
    from test_inverse import refs as inverse_refs
    from test_rows128 import STAGE_TOL, _stage_rel
    cm0, st, rs = inverse_refs("leg")
    cm = leg96()
    om = O.OracleModel(cm)
    worst = dict(qacc=0.0, qfrc_constraint=0.0)
    for lm in (0, 2):
        hm = E.HipModel(cm)
        assert hm.info(E.INFO_EFC_ROWS) == 96 and hm.info(E.INFO_LANES) == 64 and hm.info(E.INFO_KERNEL_FAMILY) == 2
        hm.set_option("lds_model", lm)
        n = NSTATE
        assert hm.launch_lanes(n) == 64
        b = E.BatchState(hm, n)
        b.qpos.copy_(torch.from_numpy(st["qpos"])); b.qvel.copy_(torch.from_numpy(st["qvel"])); b.act.copy_(torch.from_numpy(st["act"]))
        ctrl = torch.from_numpy(st["ctrl"]).cuda()
        dv = E.Derived(hm, n, ["qacc", "nefc"])
        E.forward(hm, b, ctrl, dv)
        dump = E.debug_dump(hm, b, ctrl).cpu().numpy()
        torch.cuda.synchronize()
        o = hm.layout("qfrccon")
        qacc, qfrc, nefc = dv["qacc"].cpu().numpy().astype(np.float64), dump[:, o:o + cm.nv].astype(np.float64), dv["nefc"].cpu().numpy()
        assert int(b.status.max()) == 0
        for e in range(n):
            if rs[e].marginal:
                continue
            d = O.OracleData(om)
            d.qpos[:] = st["qpos"][e]; d.qvel[:] = st["qvel"][e]; d.act[:] = st["act"][e]; d.ctrl[:] = st["ctrl"][e]
            d.forward()
            assert d.warn & 6 == 0 and nefc[e] == d.nefc == rs[e].nefc, (e, int(nefc[e]), d.nefc)
            worst["qacc"] = max(worst["qacc"], _stage_rel(qacc[e], d.qacc))
            worst["qfrc_constraint"] = max(worst["qfrc_constraint"], _stage_rel(qfrc[e], d.qfrc_constraint))
        assert worst["qacc"] < STAGE_TOL and worst["qfrc_constraint"] < STAGE_TOL, (lm, worst)
    _note("leg96", **worst)


def _f64_tracks(cm, hm, nsub=20, n=8, seed=300):
    """tests/test_fuzz_models.py's precision test: fp64 state rows, 20 free-running substeps, max |dqpos|"""
    om = O.OracleModel(cm)
    st = make_states(cm, n, seed)
    b = E.BatchState(hm, n)
    assert b.qpos.dtype == torch.float64
    b.qpos.copy_(torch.from_numpy(st["qpos"].astype(np.float64))); b.qvel.copy_(torch.from_numpy(st["qvel"].astype(np.float64)))
    if cm.na:
        b.act.copy_(torch.from_numpy(st["act"].astype(np.float64)))
    E.step(hm, b, torch.from_numpy(st["ctrl"]).cuda().contiguous(), nsub)
    torch.cuda.synchronize()
    err = 0.0
    for e in range(n):
        d = O.OracleData(om)
        d.qpos[:] = st["qpos"][e]; d.qvel[:] = st["qvel"][e]; d.ctrl[:] = st["ctrl"][e]
        if cm.na:
            d.act[:] = st["act"][e]
        d.step(nsub)
        err = max(err, float(np.abs(b.qpos[e].cpu().numpy() - d.qpos).max()))
    return err


@pytest.mark.gpu
def test_precision_mode_on_the_wide_models(oracle_lib):
    """no fp64 kernel at the 32 / 40 limit-row tiles, at 40 general rows or on RK4: refused, never stepped in fp32; the 30-dof
    general-row model runs on (64, 32, general rows) in fp64 and tracks the oracle to fp64 resolution"""
    for name, integ in F64_REFUSED:
        for p in (P64, P64S):
            with pytest.raises(E.EngineError, match="precision"):
                E.HipModel(wide_model(name, integ), precision=p)
    hm = _hip_model(("G30", 0, 0, P64S), 1)
    err = _f64_tracks(wide_model("G30"), hm)
    _note("G30-f64", qpos=err)
    assert err < F64_TOL, err


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [4, 16])
def test_precision_mode_elbow_at_the_widths_nothing_else_pins(oracle_lib, lanes):
    """mm64::k_engine<4, 4> and <16, 4>: compiled, and reached by no other test (the precision gates pin the elbow to 8 lanes)"""
    cm = synth.get_model("elbow")
    hm = E.HipModel(cm, lanes_per_env=lanes, precision=P64S)
    assert hm.info(E.INFO_LANES) == lanes and hm.launch_lanes(8) == lanes
    err = _f64_tracks(cm, hm)
    _note(f"elbow-G{lanes}-f64", qpos=err)
    assert err < F64_TOL, err
