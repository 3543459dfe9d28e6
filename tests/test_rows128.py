"""General-row models with 64 < njmax <= 128: the two-rows-per-lane kernels (k_engine_rows2, Engine's RPL = 2: lane g owns rows g and
g + 64 of an env that is one wavefront), against the fp64 oracle.

`hand_dense_full` (model/synth.py) is the dense reorient hand with its bounds raised to what these kernels hold: nconmax 26 / njmax 128.
How much of that the parity scan's inputs need was measured on the CPU with the oracle alone (tests/tools/rows128_oracle_bounds.py:
2048 envs, seed 23, seven env-steps of in-kernel actions, action seed 3, every substep and trailing forward pass):

    max contacts 11, max rows 52; no env raises warn bit 2 or 4 -- not at 256 / 1024, not at hand_dense's own 12 / 56
    (30 env-steps on the first 192 envs, every env re-armed at least once: the same maxima, 11 / 52)

so the smallest bounds that drop nothing on this stream (11 / 52) lie BELOW hand_dense's 12 / 56 and below the 64-row boundary: they
would not reach the new kernels.  The variant therefore carries the kernels' capacity instead; the oracle drops nothing on the
scan's inputs under any bound >= 11 / 52, which the scan asserts (no warn bit, no status bit 8, on any env).  Rows above 64 are made
live by the rake scenes below (up to 126 rows)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from myosuite_amd import engine as E
from myosuite_amd.envs import registry
from myosuite_amd.model import spec as S
from myosuite_amd.model import synth
from oracle import oracle as O

from test_gpu_parity import _rel as _stage_rel                                      # noqa: E402  (same directory)
from test_gpu_widths import _all_env_solve_scan                                     # noqa: E402
from test_solver_start_and_row_bounds import (SCAN_MAX, SCAN_P99, _batch, _ctrl, _kept_after_drop, _oracle, _overflow_check,  # noqa: E402
                                              _variant)

STAGE_TOL = 5e-4          # tests/test_gpu_widths.py CONFIGS: the forward-pass stage bound of the 64-lane general-row kernels
SCAN_ROWS_MAX, SCAN_CONTACTS_MAX = 52, 11      # measured with the oracle over the scan's inputs (module docstring)
RAKE_CONDIM = (3, 4, 1, 3)


def rake_scene(njmax=128, condims=RAKE_CONDIM):
    """four free rakes of ten spheres each over a plane (tests/test_solver_start_and_row_bounds.py's rake scene): 40 pairs; rake i has
    condim `condims[i]` -- 4, 6, 1, 4 rows per contact -- so all forty touching would ask for 150 rows.  Sphere k of a rake sits k mm
    above sphere 0: the rake's height decides how many of its spheres touch."""
    s = S.ModelSpec("rakes128", timestep=0.002)
    s.add_geom("floor", "world", "plane", (0, 0, 0))
    for i in range(4):
        s.add_body(f"r{i}", "world", pos=(0.0, 0.6 * i, 0.02), mass=0.5, inertia=(1e-3, 1e-3, 1e-3))
        s.add_joint(f"f{i}", f"r{i}", "free")
        for k in range(10):
            s.add_geom(f"s{i}_{k}", f"r{i}", "sphere", (0.02,), pos=(0.05 * k, 0.0, 0.001 * k))
            s.add_contact_pair("floor", f"s{i}_{k}", condim=condims[i], friction=(0.8, 0.005, 0.0001))
    s.nconmax = 40
    s.njmax = njmax
    return s.compile()


def _rake_states(cm, n, seed, depth_mm):
    """rake i pushed depth_mm[i] = (lo, hi) millimetres into the plane (uniform): about that many of its spheres touch"""
    rng = np.random.default_rng(seed)
    q = np.tile(cm.qpos0.astype(np.float64), (n, 1))
    for i, (lo, hi) in enumerate(depth_mm):
        q[:, 7 * i + 2] = 0.02 - 1e-3 * rng.uniform(lo, hi, n)
    v = 0.05 * rng.standard_normal((n, cm.nv))
    return dict(qpos=q.astype(np.float32), qvel=v.astype(np.float32), act=np.zeros((n, 0), np.float32),
                warm=np.zeros((n, cm.nv), np.float32), ctrl=np.zeros((n, cm.nu), np.float32))


# rows: 4 x (6..10) + 6 x (4..8) + (5..10) + 4 x (3..7) = 65 ... 126
LIVE_DEPTHS = ((5.5, 9.9), (3.5, 7.9), (4.5, 9.9), (2.5, 6.9))


# ------------------------------------------------------------------ CPU
def test_hand_dense_full_is_hand_dense_with_the_bounds_raised():
    a, b = synth.get_model("hand_dense"), synth.get_model("hand_dense_full")
    assert (a.nconmax, a.njmax) == (12, 56) and (b.nconmax, b.njmax) == (26, 128)
    assert b.njmax <= E.MM_MAX_EFC_ROWS and b.npair == a.npair == 189
    oi = S.C["MM_OI_NJMAX"], S.C["MM_OI_NCONMAX"]
    for k in a.arrays:
        x, y = a.arrays[k].copy(), b.arrays[k].copy()
        if k == "OPT_I":
            x[list(oi)] = 0; y[list(oi)] = 0
        assert np.array_equal(x, y), k


def test_rake_scene_rows_above_64_in_the_oracle(oracle_lib):
    """the states of the live-rows test: more than 64 and fewer than 128 rows at once, nothing dropped (oracle alone)"""
    cm = rake_scene()
    st = _rake_states(cm, 64, 3, LIVE_DEPTHS)
    om = O.OracleModel(cm)
    rows = []
    for e in range(64):
        d = _oracle(om, st, e)
        assert d.warn & 6 == 0
        rows.append(d.nefc)
    assert min(rows) > 64 and max(rows) < 128, (min(rows), max(rows))


BEFORE = os.path.join(ROOT, "profiles", "kernel_table_before_rows128.json")


@pytest.mark.skipif(not (os.path.exists(E.LIB_PATH) and os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump")), reason="needs the built library and llvm-objdump")
def test_one_row_kernels_did_not_move():
    """every kernel of the library before the two-rows-per-lane kernels went in (MM_KERNEL_LIST / _OBS / _F64, both model variants,
    and the reset / Philox / PPO kernels; profiles/kernel_table_before_rows128.json, tools/kernel_table.py on that commit's build) is
    in the built library under the same symbol with the same instruction count, VGPR / AGPR / SGPR numbers, spills and scratch --
    and the same machine code (hash of the disassembly)"""
    import kernel_table
    before = json.load(open(BEFORE))
    now = kernel_table.table(E.LIB_PATH)
    assert len(before) >= 90
    moved = {}
    for name, row in before.items():
        assert name in now, name
        if now[name] != row:
            moved[name] = {k: (row[k], now[name].get(k)) for k in row if now[name].get(k) != row[k]}
    assert not moved, moved
    new = sorted(set(now) - set(before))
    assert new == sorted(f"_Z14k_engine_rows2ILi{w}ELb{lm}EEv5KArgs" for w in (24, 32, 36) for lm in (0, 1)), new


@pytest.mark.skipif(not (os.path.exists(E.LIB_PATH) and os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump")), reason="needs the built library and llvm-objdump")
def test_two_row_kernel_resources():
    """resources of the new kernels as DESIGN.md section 3 states them: within the 256-VGPR budget of a 512-thread block, and the
    vector-register spills they do have (the target was none) bounded by what was measured when they went in"""
    import kernel_table
    now = kernel_table.table(E.LIB_PATH)
    measured = {(32, 1): 0, (32, 0): 0, (24, 1): 0, (24, 0): 0, (36, 1): 4, (36, 0): 8}     # (width, model in LDS): spilled VGPRs
    for (w, lm), spills in measured.items():
        r = now[f"_Z14k_engine_rows2ILi{w}ELb{lm}EEv5KArgs"]
        assert r["vgpr_count"] <= 256 and r["agpr_count"] == 0, r
        assert r["vgpr_spill_count"] <= spills and r["private_segment_fixed_size"] <= 4 * spills + 4, ((w, lm), r)


# ------------------------------------------------------------------ GPU
def _forward(cm, st):
    """one mm_forward with the debug record: qacc, qfrc_constraint (per dof), nefc, status"""
    hm = E.HipModel(cm)
    n = st["qpos"].shape[0]
    b = _batch(hm, st)
    dv = E.Derived(hm, n, ["qacc", "nefc"])
    E.forward(hm, b, _ctrl(st), dv)
    dump = E.debug_dump(hm, b, _ctrl(st)).cpu().numpy()
    torch.cuda.synchronize()
    o = hm.layout("qfrccon")
    return hm, dv["qacc"].cpu().numpy().astype(np.float64), dump[:, o:o + cm.nv].astype(np.float64), dv["nefc"].cpu().numpy(), b.status.cpu().numpy()


@pytest.mark.gpu
def test_njmax_96_loads_reports_its_rows_and_steps(oracle_lib):
    """a general-row model with njmax = 96: refused (MM_EUNSUPPORTED, "constraint rows > 64") before the two-rows-per-lane kernels"""
    cm = rake_scene(njmax=96)
    hm = E.HipModel(cm)
    assert hm.info(E.INFO_EFC_ROWS) == 96 and hm.info(E.INFO_LANES) == 64 and hm.info(E.INFO_KERNEL_FAMILY) == 2
    assert hm.info(E.INFO_FWD_CARRY) == 0 and hm.info(E.INFO_FOLDED_RESET) == 0
    li = hm.launch_info(256)
    assert li["lanes"] == 64 and li["two_wave"] == 0 and li["vgprs"] <= 256
    # njmax <= 64 routes as before: the same scene at 64 rows reports 64 rows on the one-row kernel (forward carry available there is
    # decided by the actuators: this scene has none)
    assert E.HipModel(rake_scene(njmax=64)).info(E.INFO_EFC_ROWS) == 64
    assert E.HipModel(synth.get_model("hand_dense")).info(E.INFO_EFC_ROWS) == 56 and E.HipModel(synth.get_model("hand")).info(E.INFO_EFC_ROWS) == 0
    st = _rake_states(cm, 64, 4, ((1.5, 4.9),) * 4)
    b = _batch(hm, st)
    E.step(hm, b, _ctrl(st), 3)
    torch.cuda.synchronize()
    om = O.OracleModel(cm)
    assert int(b.status.max()) == 0
    for e in range(0, 64, 7):
        d = _oracle(om, st, e, nsub=3)
        # (the teacher-forced bounds of tests/test_gpu_parity.py: 5e-5 on qpos, 5e-3 on qvel)
        assert np.abs(b.qpos[e].cpu().numpy() - d.qpos).max() < 5e-5 and np.abs(b.qvel[e].cpu().numpy() - d.qvel).max() < 5e-3


@pytest.mark.gpu
def test_rows_above_64_are_live(oracle_lib):
    """the rake scene with condim 3 / 4 / 1 / 3 rakes, 65 ... 126 rows active at once under njmax 128: nefc equal to the oracle's on
    every env, qacc and qfrc_constraint within the stage tolerance of the 64-lane general-row kernels"""
    cm = rake_scene()
    n = 256
    st = _rake_states(cm, n, 3, LIVE_DEPTHS)
    hm, qacc, qfrc, nefc, status = _forward(cm, st)
    assert hm.info(E.INFO_EFC_ROWS) == 128
    om = O.OracleModel(cm)
    rows, worst = [], {"qacc": 0.0, "qfrc_constraint": 0.0}
    for e in range(n):
        d = _oracle(om, st, e)
        rows.append(d.nefc)
        assert d.warn & 6 == 0 and status[e] == 0, (e, d.warn, int(status[e]))
        assert nefc[e] == d.nefc, (e, int(nefc[e]), d.nefc)
        worst["qacc"] = max(worst["qacc"], _stage_rel(qacc[e], d.qacc))
        worst["qfrc_constraint"] = max(worst["qfrc_constraint"], _stage_rel(qfrc[e], d.qfrc_constraint))
    print(f"rows above 64: oracle nefc min {min(rows)} median {int(np.median(rows))} max {max(rows)}; worst stage errors {worst}")
    assert max(rows) > 64 and min(rows) > 64 and max(rows) < 128, (min(rows), max(rows))
    assert worst["qacc"] < STAGE_TOL and worst["qfrc_constraint"] < STAGE_TOL, worst


@pytest.mark.gpu
def test_row_overflow_above_64_rows(oracle_lib):
    """the same scene family with njmax below what the states need but above 64: bit 8 <=> the oracle's warning, nefc (the surviving
    row set's size) equal per env, qacc within the scan bounds -- only the same surviving rows give the same qacc -- and, in
    enough envs to bite, a later, smaller contact (condim 1 behind a dropped condim 3 / 4) still got its row"""
    cm = rake_scene()
    n = 192
    st = _rake_states(cm, n, 9, ((5.5, 9.9), (5.5, 9.9), (4.5, 9.9), (2.5, 6.9)))       # 87 ... 150 rows asked for
    njmaxes = [66, 71, 77, 83, 90, 97, 101, 110]
    n_over, n_after = _overflow_check(cm, st, njmaxes)
    n_small = 0
    for nj in njmaxes:
        cmv = _variant(cm, njmax=nj)
        om = O.OracleModel(cmv)
        n_small += sum(_kept_after_drop(_oracle(om, st, e), cmv, min_pair=20) for e in range(n))
    print(f"overflow above 64 rows: overflowing env-cases {n_over}, contact kept after a dropped one {n_after}, of them a condim-1 / last-rake one {n_small}")
    assert n_over >= 800 and n_after >= 200 and n_small >= 100, (n_over, n_after, n_small)


@pytest.mark.gpu
def test_refusals_of_the_two_row_kernels(oracle_lib):
    """njmax = 129; forward carry, folded reset and the precision option on a two-rows-per-lane model: an error with its message each,
    and no launch (the state buffers are untouched)"""
    with pytest.raises(E.EngineError, match="128"):
        E.HipModel(rake_scene(njmax=129))
    env = registry.make("myoHandReorient100-v0", num_envs=64, seed=1, model="hand_dense_full")
    hm = env.hm
    assert hm.info(E.INFO_EFC_ROWS) == 128 and env._fwd_carry is None
    torch.cuda.synchronize()
    before = {k: getattr(env.state, k).clone() for k in ("qpos", "qvel", "act", "qacc_warmstart", "time", "status")}
    with pytest.raises(E.EngineError, match="fp32 only"):
        hm.set_option("precision", E.MM_PREC_F64)
    # (MM_PREC_F64_STATE on a handle that already has a BatchState is refused by the binding before it reaches the library -- the
    # state-row width cannot change under live buffers -- so the library's own refusal is asked of handles without one)
    fresh = E.HipModel(synth.get_model("hand_dense_full"))
    for value in (E.MM_PREC_F64, E.MM_PREC_F64_STATE):
        with pytest.raises(E.EngineError, match="fp32 only"):
            fresh.set_option("precision", value)
        with pytest.raises(E.EngineError, match="fp32 only"):
            E.HipModel(synth.get_model("hand_dense_full"), precision=value)
    assert fresh.precision == E.MM_PREC_F32 and fresh.info(E.INFO_EFC_ROWS) == 128
    # forward carry
    carry = torch.zeros(64, 2 * env.cm.nv + 1, device="cuda")
    t = E.mm_task.from_buffer_copy(env._task)
    t.fwd_carry = carry.data_ptr()
    a = torch.rand(64, env.cm.nu, device="cuda")
    with pytest.raises(E.EngineError, match="fwd_carry.*two-rows-per-lane"):
        E.env_step(hm, env.state, a, t)
    # folded reset
    env.rollout_setup(action_seed=0)
    ro = env._ro
    assert ro.autoreset == 0
    ro.autoreset = 1
    ro.reor_init_qpos = env._init_qpos_dev.data_ptr()
    ro.reor_size_tables = env._size_tables.data_ptr(); ro.reor_ntab = int(env._size_tables.shape[1]); ro.reor_tar_length = float(env.tar_length)
    ro.reor_geom_size_env = env.state.geom_size_env.data_ptr(); ro.reor_geom_type_env = env.state.geom_type_env.data_ptr()
    ro.reor_axis_half = env.axis_half.data_ptr(); ro.reor_des_rot = env.des_rot.data_ptr(); ro.episode = env.episode.data_ptr()
    with pytest.raises(E.EngineError, match="folded.*two-rows-per-lane"):
        E.rollout_step(hm, env.state, env._task, ro)
    ro.autoreset = 0
    torch.cuda.synchronize()
    for k, v in before.items():
        assert torch.equal(getattr(env.state, k), v), k
    assert float(carry.abs().max()) == 0.0
    # ... and the model still steps
    env.rollout_step(None, stream_id=0)
    torch.cuda.synchronize()
    assert int(env.state.status.max()) & ~1 == 0


@pytest.mark.gpu
def test_hand_dense_full_parity_scan(oracle_lib, monkeypatch):
    """`hand_dense_full` at 2048 envs, from reset through the all-env scan's action stream (tests/test_gpu_widths.py: seed 23, seven
    rollout steps of in-kernel actions, action seed 3), every env against the oracle on the same state: the scan's statistic and
    bounds.  Stricter here: nefc equal on EVERY env, and no env carries status bit 8 -- nor the oracle its warn bits -- (the inputs
    are the ones for which the oracle was shown to drop nothing: module docstring)."""
    nenv = 2048
    warn = []                                            # the oracle's warn bits after each of its forward passes (sticky in its data)
    forward = O.OracleData.forward
    monkeypatch.setattr(O.OracleData, "forward", lambda self: (forward(self), warn.append(self.warn))[0])
    rel, mism, rows, status, deep = _all_env_solve_scan("myoHandReorient100-v0", nenv, {"model": "hand_dense_full"})
    assert len(warn) == nenv and max(warn) & 6 == 0, max(warn)
    forgiven = deep & (rel > 1e-3) & ~mism
    ok = ~mism & ~forgiven
    q = np.quantile(rel[ok], [0.5, 0.99, 1.0])
    print(f"hand_dense_full scan: rows median {int(np.median(rows))} max {rows.max()}, row-count mismatches {int(mism.sum())}, deep capsule-in-convex envs "
          f"{int(deep.sum())} (off and left out: {int(forgiven.sum())}), rel |dqacc| median {q[0]:.1e} p99 {q[1]:.1e} max {q[2]:.1e}, status {status}")
    assert np.all(np.isfinite(rel)) and forgiven.sum() <= 2 + nenv // 500, int(forgiven.sum())
    assert status & ~1 == 0, status                      # bit 8 not tolerated (sticky over the whole stream, every env)
    assert int(mism.sum()) == 0, np.nonzero(mism)[0][:8]
    assert q[2] < SCAN_MAX and q[1] < SCAN_P99, q
