"""Batched inverse dynamics (myosuite_amd/inverse.py, libmyosim_inverse.so: k_inverse) against an fp64 reference.

Reference (numpy, fp64, inside this file): from one OracleData.forward() on the state,

    ref = full_M() @ qacc + qfrc_bias - qfrc_passive - efc_J[:n].T @ f,     f = row law of (efc_J qacc - efc_aref)

with the oracle's row law (mmo_engine.c: row_cost): an equality row is always quadratic (f = -D jar), a limit / contact row is active
only for jar < 0, a friction-loss row saturates at +-floss.  At the oracle's own forward solution this reproduces qfrc_actuator
(asserted below 1e-12 of the largest term).

States: hinge / slide coordinates uniform over their range widened by 5 % on each side (so limit rows occur), the rest at qpos0;
qvel = 0.5 N(0,1); act, ctrl ~ U[0,1); all rounded to fp32; seed 5.  65 states per model; the GPU tests run the first 1, the first 3
and all 65 (a single env, a partly filled wave, a ragged last wave).

Error measure: max |gpu - ref| over the env, divided by the largest max-abs of the four terms M qacc, bias, passive, constraint of
that env (the cancellation-free scale).  Bounds: the forward-stage bounds of tests/test_gpu_widths.py CONFIGS -- 2e-4 for the
limit-rows-only family, 5e-4 for the general-row family.

The instantiations of the 32 and 40 tiles that no synth model reaches -- <32,32,0>, <64,32,0>, <64,40,0> and <64,40,1> -- run on the
forests of tests/test_wide_models.py (W28 at 32 and 64 lanes, W40, G38): GPU_MODELS reaches all seventeen kernels, which
test_wide_models.py::test_every_compiled_kernel_has_a_parity_case asserts on the CPU.

Measured on an MI355X (worst value of the measure over the 65 states; MEASURED_WORST holds the per-model figures):

    the forests W28 / W40 / G38:                        qfrc_inverse <= 3.3e-6 (limit rows), 9.2e-5 on G38 (its constraint term)
    constraints off, the twenty synth (model, width) cases: every term <= 2.5e-6 (worst: tree_chain-G32 qfrc_inverse 2.46e-6, hand bias 2.0e-6)
    constraints on / round trip, mass, bias, passive:  <= 6.2e-6 everywhere
    constraints on / round trip, constraint term:      <= 4.2e-6, except tendon_limit_toy 3.3e-4 and hand_reorient 3.4e-4 (inside 5e-4)
    actuator outputs (hand / leg / motorfinger):       moment 1.7e-5, gain 3.6e-6, bias 2.3e-6, length 2.0e-6, velocity 9.3e-6 (hand, the worst)
    trajectory helper (hand, 32 frames):               inside 2e-4

Marginal envs (the only ones a GPU test leaves out; at most 2 % of a model's states, asserted on the CPU) are those in which the
fp64 oracle ITSELF is within one fp32 rounding of a discontinuity -- decided from the oracle alone, under the twelve 3e-7 perturbations
of tests/test_gpu_widths.py::_oracle_flips_under_fp32_rounding: its row count changes (that function), or one of its contact normals
jumps (NORMAL_JUMP), or two sphere / capsule axes in contact pass within AXIS_GAP of each other, where the normal is undefined at fp32
resolution.  The last two were found on the object-holding hands, whose uniform-over-the-range finger poses push fingers through the
held object: hand_hold had six states (9 %) in which a finger crosses the middle of the ellipsoid and the oracle's own qfrc_constraint
moves by up to 13x the env's largest term under those perturbations (the GPU differed by 12.9x there) -- over the cap, so its inputs
were changed (LIFTED); hand_reorient has one state (env 32, 1.5 %: axes 1.1e-5 m apart, GPU 1.5e-2 there).
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from myosuite_amd import engine as E                       # noqa: E402
from myosuite_amd import inverse as INV                    # noqa: E402
from myosuite_amd.model import spec as S                   # noqa: E402
from myosuite_amd.model import synth                       # noqa: E402
from oracle import oracle as O                             # noqa: E402

from test_gpu_widths import _oracle_flips_under_fp32_rounding   # noqa: E402  (same directory)

TOL_LIMIT, TOL_GEN = 2e-4, 5e-4      # tests/test_gpu_widths.py CONFIGS
NSTATE, SEED = 65, 5
BATCHES = (1, 3, 65)
NOISE = 0.5          # family (b): qacc = forward solution + NOISE * max|forward solution| * N(0,1) per env (tuned on the reference alone:
                     # test_noise_family_exercises_both_branches_of_the_row_law)
CON_LIMIT_JOINT, CON_LIMIT_TENDON, CON_CONTACT, CON_EQUALITY, CON_FRICTION = (S.C["MM_CON_LIMIT_JOINT"], S.C["MM_CON_LIMIT_TENDON"],
                                                                              S.C["MM_CON_CONTACT"], S.C["MM_CON_EQUALITY"], S.C["MM_CON_FRICTION_DOF"])

# (model, lanes per env, bound): together every k_inverse instantiation -- the last four on tests/test_wide_models.py's forests.  (plane_toy is left out: all its
# joints are free, so every state is qpos0, where its boxes rest exactly at the contact margin -- every state is marginal; its
# instantiation, <64,32,1>, is hand_reorient's.)
GPU_MODELS = [("elbow", 4, TOL_LIMIT), ("elbow", 8, TOL_LIMIT), ("elbow", 16, TOL_LIMIT), ("elbow", 32, TOL_LIMIT), ("elbow", 64, TOL_LIMIT),
              ("finger", 8, TOL_LIMIT), ("hand", 32, TOL_LIMIT), ("hand", 64, TOL_LIMIT), ("tree_star", 32, TOL_LIMIT),
              ("friction_toy", 16, TOL_GEN), ("tendon_limit_toy", 16, TOL_GEN), ("contact_toy", 32, TOL_GEN), ("tree_chain", 32, TOL_GEN),
              ("hand_hold", 32, TOL_GEN), ("hand_reorient", 64, TOL_GEN), ("leg", 64, TOL_GEN),
              ("hand_contact", 64, TOL_GEN), ("hand_keyturn", 64, TOL_GEN), ("torso", 64, TOL_GEN),
              ("W28", 32, TOL_LIMIT), ("W28", 64, TOL_LIMIT), ("W40", 64, TOL_LIMIT), ("G38", 64, TOL_GEN)]
# Inputs changed to keep the marginal share under its cap.  With the object at qpos0, hand_hold's uniform-over-the-range finger poses
# put a finger through the MIDDLE of the held ellipsoid in 6 of 65 states (oracle con_dist -1.8 ... -3.2 cm against semi-axes of 2.5 /
# 3.6 / 3 cm): there the nearest surface point is not unique and the fp64 oracle's own contact normal turns by 50 - 100 degrees under a
# qpos perturbation of one fp32 rounding (its qfrc_constraint moves by up to 13x the env's largest term).  9 % of the states are
# marginal in that sense, over the 2 % cap, whatever the seed; so the object of this model is lifted out of the hand (metres added to
# the free joint's z) and its constraint rows are the joint limits.  No other model has such a state (asserted on the CPU).
LIFTED = {"hand_hold": 0.25}
NORMAL_JUMP = 1e-3     # a contact normal of the oracle that turns by more than this (radians) under a 3e-7 perturbation is a jump: on a smooth
                       # surface the turn is about perturbation x lever arm / radius of curvature ~ 3e-7 x 0.2 m / 5 mm = 1e-5
AXIS_GAP = 1e-4        # metres.  The normal of a sphere / capsule contact is (p2 - p1) / |p2 - p1| between the closest points of the two axes; when
                       # a finger's axis passes THROUGH the object's axis that length goes to zero and the normal is undefined.  fp32 holds
                       # the points (coordinates up to ~0.3 m) to ~2e-8 m, so the normal -- and with it the contact's force direction -- is
                       # known to 2e-8 / gap: a gap under 1e-4 m cannot give the 5e-4 bound (2e-8 / 1e-4 = 2e-4, with the factor two to
                       # three of several contributing coordinates).  Such an env is marginal: the oracle's contact is within fp32
                       # resolution of a singular configuration.  (hand_reorient env 32: 1.1e-5 m between the object's and a metacarpal's axes.)
GPU_IDS = [f"{n}-G{g}" for n, g, _ in GPU_MODELS]
MODEL_NAMES = sorted({n for n, _, _ in GPU_MODELS} | {"motorfinger"})
TERMS = ("qfrc_inverse", "qfrc_mass", "qfrc_bias", "qfrc_passive", "qfrc_constraint")

# worst value of the error measure per (model-G, test, term) as measured on an MI355X (information; the bounds are TOL_*)
MEASURED_WORST = {   # qfrc_inverse, n = 65
    "off": {"elbow": 2.3e-7, "finger": 4.6e-7, "hand": 1.8e-6, "tree_star": 8.4e-7, "friction_toy": 2.8e-7, "tendon_limit_toy": 2.3e-7,
            "contact_toy": 1.3e-7, "tree_chain": 2.5e-6, "hand_hold": 1.6e-7, "hand_reorient": 1.2e-7, "leg": 3.3e-7, "hand_contact": 1.8e-6,
            "hand_keyturn": 1.8e-6, "torso": 5.4e-7,
            "W28": 8.0e-7, "W40": 1.2e-6, "G38": 7.7e-7},
    "on-a": {"elbow": 7.6e-7, "finger": 3.0e-7, "hand": 1.0e-6, "tree_star": 2.5e-6, "friction_toy": 1.6e-6, "tendon_limit_toy": 3.3e-4,
             "contact_toy": 4.1e-6, "tree_chain": 6.2e-6, "hand_hold": 12.9, "hand_reorient": 1.5e-2, "leg": 1.3e-6, "hand_contact": 1.8e-6,
             "hand_keyturn": 4.2e-6, "torso": 1.2e-6,
             "W28": 1.9e-6, "W40": 3.1e-6, "G38": 9.2e-5},
    "on-b": {"elbow": 2.8e-7, "finger": 3.1e-7, "hand": 8.7e-7, "tree_star": 8.1e-7, "friction_toy": 5.4e-7, "tendon_limit_toy": 2.7e-4,
             "contact_toy": 3.4e-7, "tree_chain": 2.0e-6, "hand_hold": 1.14, "hand_reorient": 3.4e-4, "leg": 3.4e-7, "hand_contact": 2.6e-6,
             "hand_keyturn": 2.5e-6, "torso": 5.2e-7,
             "W28": 1.0e-6, "W40": 1.2e-6, "G38": 1.2e-6},
    "trip": {"elbow": 7.4e-7, "finger": 3.1e-7, "hand": 1.1e-6, "tree_star": 2.4e-6, "friction_toy": 1.7e-6, "tendon_limit_toy": 3.3e-4,
             "contact_toy": 4.1e-6, "tree_chain": 5.5e-6, "hand_hold": 1.3, "hand_reorient": 1.5e-2, "leg": 1.3e-6, "hand_contact": 1.8e-6,
             "hand_keyturn": 4.0e-6, "torso": 9.3e-7,
             "W28": 1.8e-6, "W40": 3.3e-6, "G38": 8.7e-5}}


# ------------------------------------------------------------------ inputs and the fp64 reference
def get_model(name):
    """a synth model by name, or one of the forests of tests/test_wide_models.py (not in synth.builders(): test models only)"""
    if name in synth.builders():
        return synth.get_model(name)
    from test_wide_models import wide_model          # (same directory; imported here: that module imports this one)
    return wide_model(name)


def make_states(cm, n=NSTATE, seed=SEED, lift=0.0):
    rng = np.random.default_rng(seed)
    q = np.tile(cm.qpos0.astype(np.float64), (n, 1))
    jt, qa, rg = cm.arrays["JNT_TYPE"], cm.arrays["JNT_QPOSADR"], cm.jnt_range
    for j in range(cm.njnt):
        if int(jt[j]) in (S.C["MM_JNT_HINGE"], S.C["MM_JNT_SLIDE"]) and rg[j, 1] > rg[j, 0]:
            w = float(rg[j, 1] - rg[j, 0])
            q[:, int(qa[j])] = rng.uniform(rg[j, 0] - 0.05 * w, rg[j, 1] + 0.05 * w, n)
    if lift:      # see LIFTED
        for j in range(cm.njnt):
            if int(jt[j]) == S.C["MM_JNT_FREE"]:
                q[:, int(qa[j]) + 2] += lift
    f32 = lambda x: np.ascontiguousarray(x, dtype=np.float32)
    return dict(qpos=f32(q), qvel=f32(0.5 * rng.standard_normal((n, cm.nv))), act=f32(rng.uniform(0, 1, (n, cm.na))),
                ctrl=f32(rng.uniform(0, 1, (n, cm.nu))), warm=np.zeros((n, cm.nv), np.float32))


def oracle_forward(om, st, e, act=None, ctrl=None):
    d = O.OracleData(om)
    d.qpos[:] = st["qpos"][e]; d.qvel[:] = st["qvel"][e]
    d.ctrl[:] = st["ctrl"][e] if ctrl is None else ctrl
    if om.cm.na:
        d.act[:] = st["act"][e] if act is None else act
    d.qacc_warmstart[:] = 0.0
    d.forward()
    return d


def row_law(jar, D, floss, typ):
    """the oracle's row force at jar = J qacc - aref (row_cost)"""
    f = -D * jar
    out = np.where(jar < 0.0, f, 0.0)                            # limit / contact rows
    out = np.where(typ == CON_EQUALITY, f, out)
    out = np.where(typ == CON_FRICTION, np.clip(f, -floss, floss), out)
    return out


class Ref:
    """everything the reference needs from one forward pass of the oracle, copied out"""

    def __init__(self, d, cm):
        n = d.nefc
        self.nefc = n
        self.M = d.full_M(); self.bias = d.qfrc_bias.copy(); self.passive = d.qfrc_passive.copy()
        self.J = d.efc_J[:n].copy(); self.D = d.efc_D[:n].copy(); self.aref = d.efc_aref[:n].copy()
        self.floss = d.efc_floss[:n].copy(); self.typ = d.efc_type.astype(np.int64)
        self.qacc = d.qacc.copy(); self.actuator = d.qfrc_actuator.copy()
        self.moment = d.actuator_moment.copy(); self.length = d.actuator_length.copy(); self.velocity = d.actuator_velocity.copy()
        self.force = d.actuator_force.copy()
        self.marginal = False

    def jar(self, qacc):
        return self.J @ qacc - self.aref

    def terms(self, qacc, constraints):
        qacc = np.asarray(qacc, np.float64)
        con = np.zeros_like(self.bias)
        if constraints and self.nefc:
            con = self.J.T @ row_law(self.jar(qacc), self.D, self.floss, self.typ)
        mass = self.M @ qacc
        return dict(qfrc_mass=mass, qfrc_bias=self.bias, qfrc_passive=self.passive, qfrc_constraint=con,
                    qfrc_inverse=mass + self.bias - self.passive - con)


def scale_of(t):
    return max(1e-30, max(float(np.abs(t[k]).max()) for k in ("qfrc_mass", "qfrc_bias", "qfrc_passive", "qfrc_constraint")))


@functools.lru_cache(maxsize=None)
def refs(name):
    """(compiled model, states, [Ref per state]) -- computed once per model and shared by every test; never modified"""
    O.build()
    cm = get_model(name)
    om = O.OracleModel(cm)
    st = make_states(cm, lift=LIFTED.get(name, 0.0))
    out = []
    for e in range(NSTATE):
        d = oracle_forward(om, st, e)
        r = Ref(d, cm)
        r.marginal = _oracle_flips_under_fp32_rounding(om, cm, None, e, st["qpos"][e].astype(np.float64), st["qvel"][e], st["act"][e],
                                                       st["ctrl"][e], st["warm"][e], r.nefc, False)
        # the same twelve perturbations once more, keeping what the oracle computes on them: a contact normal that jumps makes the
        # env marginal too (LIFTED / NORMAL_JUMP)
        r.normal_jump = False
        if not r.marginal and cm.npair:
            rng = np.random.default_rng(1000 + e)
            nc, n0 = d.ncon, d.con_frame[:d.ncon, :3].copy()
            for _ in range(12):
                q = st["qpos"][e].astype(np.float64)
                q = q + 3e-7 * np.maximum(1.0, np.abs(q)) * rng.choice([-1.0, 1.0], size=q.shape)
                d2 = O.OracleData(om)
                d2.qpos[:] = q; d2.qvel[:] = st["qvel"][e]; d2.ctrl[:] = st["ctrl"][e]
                if cm.na:
                    d2.act[:] = st["act"][e]
                d2.forward()
                if d2.ncon != nc or (nc and float(np.linalg.norm(d2.con_frame[:nc, :3] - n0, axis=1).max()) > NORMAL_JUMP):
                    r.normal_jump = True
            r.marginal = r.normal_jump
        # ... and so does a sphere / capsule contact whose axes come closer than AXIS_GAP
        r.axis_gap = np.inf
        gt, gs = cm.arrays["GEOM_TYPE"], cm.arrays["GEOM_SIZE"].reshape(-1, 3)
        for c, p in enumerate(d.con_pair):
            g1, g2 = int(cm.arrays["PAIR_GEOM1"][p]), int(cm.arrays["PAIR_GEOM2"][p])
            if all(int(gt[g]) in (S.C["MM_GEOM_SPHERE"], S.C["MM_GEOM_CAPSULE"]) for g in (g1, g2)):
                r.axis_gap = min(r.axis_gap, float(d.con_dist[c] + gs[g1, 0] + gs[g2, 0]))
        r.marginal = r.marginal or r.axis_gap < AXIS_GAP
        out.append(r)
    return cm, st, out


def qacc_family(name, family):
    """[NSTATE, nv] fp32: 'random' 10 N(0,1); 'a' the oracle's forward solution; 'b' that plus per-env noise of scale NOISE"""
    cm, st, rs = refs(name)
    rng = np.random.default_rng(SEED + 1)
    if family == "random":
        return (10.0 * rng.standard_normal((NSTATE, cm.nv))).astype(np.float32)
    qa = np.stack([r.qacc for r in rs])
    if family == "b":
        qa = qa + NOISE * np.abs(qa).max(axis=1, keepdims=True) * rng.standard_normal(qa.shape)
    return np.ascontiguousarray(qa, dtype=np.float32)


# ------------------------------------------------------------------ CPU: the reference itself, the inputs, the library, the helper
@pytest.mark.parametrize("name", MODEL_NAMES)
def test_reference_reproduces_qfrc_actuator_and_few_states_are_marginal(oracle_lib, name):
    cm, st, rs = refs(name)
    worst = 0.0
    for r in rs:
        t = r.terms(r.qacc, True)
        worst = max(worst, float(np.abs(t["qfrc_inverse"] - r.actuator).max()) / max(scale_of(t), float(np.abs(r.actuator).max())))
    print(f"{name}: identity {worst:.2e}, rows {min(r.nefc for r in rs)}-{max(r.nefc for r in rs)}, marginal {sum(r.marginal for r in rs)} "
          f"(contact-normal jumps {sum(r.normal_jump for r in rs)}, axes closer than {AXIS_GAP} m {sum(r.axis_gap < AXIS_GAP for r in rs)})")
    assert worst < 1e-12, worst
    assert sum(r.marginal for r in rs) <= 0.02 * NSTATE, [e for e, r in enumerate(rs) if r.marginal]


ACTUATOR_MODELS = [("hand", 32, TOL_LIMIT), ("leg", 64, TOL_GEN), ("motorfinger", 8, TOL_LIMIT)]


def test_actuator_models_are_not_force_limited():
    """the gain / bias reference of test_actuator_outputs (two forward passes, force linear in the input) needs this"""
    for name, _, _ in ACTUATOR_MODELS:
        assert not np.any(synth.get_model(name).arrays["ACT_FORCELIMITED"]), name


def test_noise_family_exercises_both_branches_of_the_row_law(oracle_lib):
    """on the reference alone: family (b) puts at least 10 % of the limit / contact rows on each side of jar = 0, and on friction_toy
    it has rows in the quadratic zone and in both saturated zones"""
    neg = pos = 0
    for name in ("hand", "hand_contact", "leg", "contact_toy", "hand_keyturn"):
        cm, st, rs = refs(name)
        qb = qacc_family(name, "b").astype(np.float64)
        for e, r in enumerate(rs):
            if not r.nefc:
                continue
            jar = r.jar(qb[e])
            one_sided = (r.typ == CON_LIMIT_JOINT) | (r.typ == CON_LIMIT_TENDON) | (r.typ == CON_CONTACT)
            neg += int((jar[one_sided] < 0).sum()); pos += int((jar[one_sided] >= 0).sum())
    print(f"limit / contact rows: jar < 0 {neg}, jar >= 0 {pos}")
    assert neg >= 0.1 * (neg + pos) and pos >= 0.1 * (neg + pos) and neg + pos > 500, (neg, pos)
    cm, st, rs = refs("friction_toy")
    qb = qacc_family("friction_toy", "b").astype(np.float64)
    zones = [0, 0, 0]
    for e, r in enumerate(rs):
        fr = r.typ == CON_FRICTION
        f = -r.D[fr] * r.jar(qb[e])[fr]
        zones[0] += int((f <= -r.floss[fr]).sum()); zones[1] += int((np.abs(f) < r.floss[fr]).sum()); zones[2] += int((f >= r.floss[fr]).sum())
    print(f"friction rows: saturated- {zones[0]}, quadratic {zones[1]}, saturated+ {zones[2]}")
    assert min(zones) >= 5, zones


INSTANTIATIONS = [(4, 4, 0), (8, 4, 0), (16, 4, 0), (32, 4, 0), (64, 4, 0), (32, 24, 0), (64, 24, 0), (32, 32, 0), (64, 32, 0), (64, 40, 0),
                  (16, 4, 1), (32, 24, 1), (64, 32, 1), (32, 32, 1), (64, 40, 1), (64, 36, 1), (64, 24, 1)]
# scratch bytes per lane of each kernel as built (the ratchet: zero is the goal, a spilling kernel is recorded here, not hidden)
SCRATCH_BYTES = {}


def _kernel_symbol(g, nvp, gen):
    return f"_Z9k_inverseILi{g}ELi{nvp}ELb{gen}EEv5KArgs7InvArgs"


@pytest.mark.skipif(not (os.path.exists(INV.LIB_PATH) and os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump")), reason="needs the built library and llvm-objdump")
def test_library_holds_the_seventeen_kernels():
    """libmyosim_inverse.so holds one k_inverse per Euler entry of the engine's kernel list and no other kernel; each fits the
    register file (VGPRs <= 256); scratch bytes are the recorded ratchet"""
    import kernel_table
    tab = kernel_table.table(INV.LIB_PATH)
    assert sorted(tab) == sorted(_kernel_symbol(*i) for i in INSTANTIATIONS), sorted(tab)
    for i in INSTANTIATIONS:
        row = tab[_kernel_symbol(*i)]
        print(i, {k: row[k] for k in ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "private_segment_fixed_size", "instructions")})
        assert row["vgpr_count"] <= 256, (i, row)
        assert row["private_segment_fixed_size"] <= SCRATCH_BYTES.get(i, 0), (i, row)


def test_engine_library_has_no_inverse_kernel():
    """the inverse sources live in a subdirectory that the engine library's build does not sweep"""
    top = [f for f in os.listdir(E.CSRC) if f.endswith(".hip")]
    assert top and not any("inverse" in f for f in top)
    assert sorted(f for f in os.listdir(INV.CSRC) if f.endswith(".hip"))[0].startswith("myosim_inverse")


def _smooth_trajectory(cm, npoint=33):
    """a smooth joint-angle trajectory inside the middle of every joint's range"""
    rg = cm.jnt_range
    mid, half = 0.5 * (rg[:, 0] + rg[:, 1]), 0.5 * (rg[:, 1] - rg[:, 0])
    t = np.arange(npoint)[:, None] * cm.timestep
    ph = np.linspace(0.0, 2.0, cm.nq)[None, :]
    return (mid[None, :] + 0.3 * half[None, :] * np.sin(2 * np.pi * 3.0 * t + ph)).astype(np.float32)


def test_trajectory_finite_differences():
    """inverse.trajectory_frames against the tutorial's arithmetic (get_qfrc: qacc = ((q_target - qpos) / h - qvel) / h with the
    state left by the previous frame), restated in numpy; no launch"""
    cm = synth.get_model("hand")
    q = _smooth_trajectory(cm)
    h = np.float32(cm.timestep)
    qp, qv, qa = INV.trajectory_frames(torch.from_numpy(q), float(cm.timestep))
    T = q.shape[0] - 1
    vel, acc = np.zeros((T, cm.nv), np.float32), np.zeros((T, cm.nv), np.float32)
    for t in range(T):
        if t > 0:
            vel[t] = (q[t] - q[t - 1]) / h
        acc[t] = ((q[t + 1] - q[t]) / h - vel[t]) / h
    assert qp.shape == (T, cm.nq) and qv.shape == qa.shape == (T, cm.nv)
    np.testing.assert_array_equal(qp.numpy(), q[:-1])
    np.testing.assert_allclose(qv.numpy(), vel, rtol=1e-6, atol=0)
    np.testing.assert_allclose(qa.numpy(), acc, rtol=1e-5, atol=1e-5 * float(np.abs(acc).max()))
    with pytest.raises(ValueError, match="free or ball"):
        INV.inverse_dynamics_trajectory(synth.get_model("contact_toy"), np.zeros((3, 13), np.float32))


# ------------------------------------------------------------------ GPU
@functools.lru_cache(maxsize=None)
def inv_model(name, lanes):
    return INV.InverseModel(get_model(name), lanes_per_env=lanes)


@functools.lru_cache(maxsize=None)
def hip_model(name, lanes):
    return E.HipModel(get_model(name), lanes_per_env=lanes)


def batch_state(hm, st, n):
    b = E.BatchState(hm, n)
    b.qpos.copy_(torch.from_numpy(st["qpos"][:n])); b.qvel.copy_(torch.from_numpy(st["qvel"][:n]))
    if hm.cm.na:
        b.act.copy_(torch.from_numpy(st["act"][:n]))
    b.time.fill_(0.25)
    return b


def run_inverse(im, b, qacc, constraints, want, out=None):
    """INV.inverse on a BatchState, asserting that the call leaves every state row bit-identical"""
    rows = ("qpos", "qvel", "act", "qacc_warmstart", "time", "status")
    before = {k: getattr(b, k).clone() for k in rows}
    res = INV.inverse(im, b, qacc, constraints=constraints, want=want, out=out)
    torch.cuda.synchronize()
    for k in rows:
        assert torch.equal(getattr(b, k), before[k]), k
    return {k: v.cpu().numpy() for k, v in res.items()}


def compare(tag, name, rs, got, qacc, constraints, tol, n, keys=TERMS, skip_marginal=False):
    worst = {k: 0.0 for k in keys}
    bad = []
    for e in range(n):
        if skip_marginal and rs[e].marginal:
            continue
        t = rs[e].terms(qacc[e], constraints)
        sc = scale_of(t)
        for k in keys:
            err = float(np.abs(got[k][e] - t[k]).max()) / sc
            worst[k] = max(worst[k], err)
            if not err <= tol:
                bad.append((e, k, err))
    print(f"{tag} {name} n={n}: " + " ".join(f"{k[5:]} {v:.2e}" for k, v in worst.items()))
    assert not bad, (tag, name, n, bad[:6], tol)
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("name,lanes,tol", GPU_MODELS, ids=GPU_IDS)
def test_constraints_off(oracle_lib, name, lanes, tol):
    cm, st, rs = refs(name)
    im = inv_model(name, lanes)
    assert im.info(INV.INFO_LANES) == lanes
    qa = qacc_family(name, "random")
    for n in BATCHES:
        b = batch_state(hip_model(name, lanes), st, n)
        got = run_inverse(im, b, torch.from_numpy(qa[:n]).cuda(), False, TERMS + ("nefc",))
        assert not got["qfrc_constraint"].any() and not got["nefc"].any()
        compare("off", f"{name}-G{lanes}", rs, got, qa, False, tol, n)


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["a", "b"])
@pytest.mark.parametrize("name,lanes,tol", GPU_MODELS, ids=GPU_IDS)
def test_constraints_on(oracle_lib, name, lanes, tol, family):
    cm, st, rs = refs(name)
    im = inv_model(name, lanes)
    qa = qacc_family(name, family)
    for n in BATCHES:
        b = batch_state(hip_model(name, lanes), st, n)
        got = run_inverse(im, b, torch.from_numpy(qa[:n]).cuda(), True, TERMS + ("nefc",))
        for e in range(n):
            if not rs[e].marginal:
                assert got["nefc"][e] == rs[e].nefc, (e, got["nefc"][e], rs[e].nefc)
        compare("on-" + family, f"{name}-G{lanes}", rs, got, qa, True, tol, n, skip_marginal=True)


@pytest.mark.gpu
@pytest.mark.parametrize("name,lanes,tol", GPU_MODELS, ids=GPU_IDS)
def test_round_trip_on_the_device(oracle_lib, name, lanes, tol):
    """qacc from mm_forward of the engine library, mm_inverse of it against the reference evaluated at that same qacc"""
    cm, st, rs = refs(name)
    im, hm = inv_model(name, lanes), hip_model(name, lanes)
    for n in BATCHES:
        b = batch_state(hm, st, n)
        der = E.Derived(hm, n, ["qacc", "nefc"])
        E.forward(hm, b, torch.from_numpy(st["ctrl"][:n]).cuda(), der)
        torch.cuda.synchronize()
        qacc = der["qacc"].clone()
        got = run_inverse(im, b, qacc, True, TERMS + ("nefc",))
        assert np.array_equal(got["nefc"], der["nefc"].cpu().numpy())
        compare("trip", f"{name}-G{lanes}", rs, got, qacc.cpu().numpy().astype(np.float64), True, tol, n, skip_marginal=True)


@pytest.mark.gpu
@pytest.mark.parametrize("name,lanes,tol", ACTUATOR_MODELS, ids=[m[0] for m in ACTUATOR_MODELS])
def test_actuator_outputs(oracle_lib, name, lanes, tol):
    """moment (dense nu x nv), length, velocity straight from the oracle; bias = actuator_force(input 0), gain = actuator_force(input 1)
    - bias from two more forward passes (input: act, or ctrl for actuators without activation state)"""
    cm, st, rs = refs(name)
    om = O.OracleModel(cm)
    im = inv_model(name, lanes)
    n = NSTATE
    b = batch_state(hip_model(name, lanes), st, n)
    qa = qacc_family(name, "random")
    keys = ("actuator_moment", "actuator_gain", "actuator_bias", "actuator_length", "actuator_velocity")
    got = run_inverse(im, b, torch.from_numpy(qa).cuda(), False, keys)
    worst = {k: 0.0 for k in keys}
    for e in range(n):
        z, o = np.zeros(max(cm.na, cm.nu)), np.ones(max(cm.na, cm.nu))
        d0, d1 = oracle_forward(om, st, e, act=z[:cm.na], ctrl=z[:cm.nu]), oracle_forward(om, st, e, act=o[:cm.na], ctrl=o[:cm.nu])
        f0, f1 = d0.actuator_force.copy(), d1.actuator_force.copy()      # (the views die with d0 / d1: copy while they live)
        ref = dict(actuator_moment=rs[e].moment, actuator_gain=f1 - f0, actuator_bias=f0, actuator_length=rs[e].length, actuator_velocity=rs[e].velocity)
        # gain and bias are forces of the same actuators (force = gain * act + bias, act in [0, 1]): one scale for both, the largest
        # of either in the env -- the passive force alone is ~0 whenever no muscle is stretched past its optimal length
        fscale = max(float(np.abs(ref["actuator_gain"]).max()), float(np.abs(ref["actuator_bias"]).max()))
        for k in keys:
            sc = fscale if k in ("actuator_gain", "actuator_bias") else float(np.abs(ref[k]).max())
            err = float(np.abs(got[k][e] - ref[k]).max()) / max(1e-30, sc)
            if err > worst[k]:
                worst[k] = err
                if err > tol:
                    i = int(np.abs(got[k][e] - ref[k]).reshape(-1).argmax())
                    print(f"  {name} env {e} {k}[{i}]: gpu {got[k][e].reshape(-1)[i]:.6g} ref {ref[k].reshape(-1)[i]:.6g} scale {sc:.4g}")
    print(f"actuators {name}: " + " ".join(f"{k[9:]} {v:.2e}" for k, v in worst.items()))
    assert all(v <= tol for v in worst.values()), worst


@pytest.mark.gpu
def test_isolation_of_a_nan_acceleration(oracle_lib):
    """elbow at 4 lanes per env (sixteen envs per wave): one env's qacc is NaN -- its force is NaN, every other env is bit-identical"""
    cm, st, rs = refs("elbow")
    im = inv_model("elbow", 4)
    n, bad = NSTATE, 21
    b = batch_state(hip_model("elbow", 4), st, n)
    qa = torch.from_numpy(qacc_family("elbow", "b")).cuda()
    clean = run_inverse(im, b, qa, True, TERMS + ("nefc",))
    qn = qa.clone(); qn[bad] = float("nan")
    dirty = run_inverse(im, b, qn, True, TERMS + ("nefc",))
    assert np.isnan(dirty["qfrc_inverse"][bad]).all() and np.isnan(dirty["qfrc_mass"][bad]).all()
    keep = np.arange(n) != bad
    for k in clean:
        assert np.array_equal(clean[k][keep], dirty[k][keep]), k
        assert not np.isnan(clean[k].astype(np.float64)).any(), k


@pytest.mark.gpu
def test_refusals_leave_the_outputs_alone(oracle_lib):
    with pytest.raises(E.EngineError, match="njmax > 64"):
        INV.InverseModel(synth.get_model("hand_dense_full"))
    with pytest.raises(E.EngineError, match="lanes_per_env"):
        INV.InverseModel(synth.get_model("hand"), lanes_per_env=8)
    cm, st, rs = refs("elbow")
    im, hm = inv_model("elbow", 8), hip_model("elbow", 8)
    n = 3
    qa = torch.from_numpy(qacc_family("elbow", "random")[:n]).cuda()
    sentinel = lambda: {k: torch.full((n, cm.nv), -7.5, device="cuda") for k in TERMS}
    # a state that carries a per-env model delta
    b = batch_state(hm, st, n)
    b.set_body_mass_env(1, torch.full((n,), 2.0, device="cuda"))
    out = sentinel()
    with pytest.raises(E.EngineError, match="per-env model delta"):
        INV.inverse(im, b, qa, want=TERMS, out=out)
    # null qfrc_inverse; a size beyond the library's
    b = batch_state(hm, st, n)
    a = INV.mm_inverse_args()
    a.qfrc_mass = out["qfrc_mass"].data_ptr()
    rc = INV.lib().mm_inverse(im.h, b.c, qa.data_ptr(), C.byref(a), None)
    assert rc == -5 and b"qfrc_inverse is NULL" in INV.lib().mm_inverse_last_error()
    a.qfrc_inverse = out["qfrc_inverse"].data_ptr()
    a.size = C.sizeof(INV.mm_inverse_args) + 8
    rc = INV.lib().mm_inverse(im.h, b.c, qa.data_ptr(), C.byref(a), None)
    assert rc == -5 and b"size is larger" in INV.lib().mm_inverse_last_error()
    b2 = E.BatchState(hm, 1); b2._c.nenv = 0
    a.size = C.sizeof(INV.mm_inverse_args)
    rc = INV.lib().mm_inverse(im.h, b2.c, qa.data_ptr(), C.byref(a), None)
    assert rc == -5 and b"nenv < 1" in INV.lib().mm_inverse_last_error()
    torch.cuda.synchronize()
    for k, t in out.items():
        assert bool((t == -7.5).all()), k
    # and the same arguments, accepted, do write
    got = run_inverse(im, b, qa, False, TERMS, out=out)
    assert not (got["qfrc_inverse"] == -7.5).any()


@pytest.mark.gpu
def test_trajectory_helper(oracle_lib):
    """a 33-point smooth hand trajectory: one launch of 32 frames, against the reference frame by frame"""
    cm = synth.get_model("hand")
    om = O.OracleModel(cm)
    q = _smooth_trajectory(cm)
    got = INV.inverse_dynamics_trajectory(cm, q, model=inv_model("hand", 32)).cpu().numpy()
    assert got.shape == (32, cm.nv)
    qp, qv, qa = (x.numpy() for x in INV.trajectory_frames(torch.from_numpy(q), float(cm.timestep)))
    worst = 0.0
    for t in range(32):
        d = O.OracleData(om)
        d.qpos[:] = qp[t]; d.qvel[:] = qv[t]
        d.forward()
        mass = d.full_M() @ qa[t].astype(np.float64)
        ref = mass + d.qfrc_bias - d.qfrc_passive
        sc = max(float(np.abs(x).max()) for x in (mass, d.qfrc_bias, d.qfrc_passive))
        worst = max(worst, float(np.abs(got[t] - ref).max()) / sc)
    print(f"trajectory hand: {worst:.2e}")
    assert worst <= TOL_LIMIT, worst
