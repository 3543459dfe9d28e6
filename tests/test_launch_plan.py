"""The launch planner (myosuite_amd/csrc/myosim_launch_plan.hpp: model image + launch options + batch size -> lanes per env, waves
per block, helper waves, model in LDS or through L2, LDS bytes, grid) against the geometry recorded from the build before it was
split out of launch_on_device (profiles/launch_plans_before_host_core.json, written by tests/tools/record_launch_plans.py on that
commit):

  * on the CPU, the two host-only headers compiled into a plain host program under AddressSanitizer + UndefinedBehaviorSanitizer give
    the recorded lanes / waves per block / two_wave / lds_model / LDS bytes / blocks for every recorded case, also after the
    set_lanes / set_option calls (whose refusals keep their codes and messages);
  * on the GPU, mm_model_launch_info gives all eight recorded values (occupancy and VGPRs too) on a subset with one case of every
    branch of the planner;
  * on the CPU, the planner as the inverse library calls it (model through L2, no helper waves) gives the geometry of the loop that
    library's launch_on_device held before, restated here;
  * with two GPUs, a launch on another device's handle computes what it computes on its own device and leaves the current device alone.
"""
import ctypes as C
import json
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
from myosuite_amd.model import synth                                                # noqa: E402
from test_model_image import fixture_models                                         # noqa: E402  (same directory)

FIXTURE = os.path.join(ROOT, "profiles", "launch_plans_before_host_core.json")
KEYS = E.HipModel.LAUNCH_KEYS                        # MM_LAUNCH_* (include/myosim.h); the planner decides the first six
NPLAN = 6
WIDTHS = (4, 8, 16, 32, 64)
OPTION_MODELS = ("elbow", "hand", "leg", "torso", "hand_reorient", "leg_implicit", "rake")
OPTION_CALLS = [("set_lanes", 64), ("set_lanes", 32), ("set_lanes", 8), ("lds_model", 0), ("lds_model", 2), ("waves_per_block", 1),
                ("waves_per_block", 2), ("waves_per_block", 8), ("precision", E.MM_PREC_F64)]
OPTION_NENV = (1, 63, 64, 65, 1000, 4096, 16385, 65537, 262144)


def nenv_list(lanes: int, general_rows: bool) -> list:
    """batch sizes that cross the planner's thresholds for a model whose default width is `lanes`: one env; one short of, at and
    one over a full wave; the batches at which the waves wanted per CU go 1 -> 2, 4 -> 5 and 8 -> 9 (256, 1024 and 2048 waves and
    their successors -- and the same counts taken as envs of a 64-envs-per-wave launch: 16 384, 65 536, 131 072); for the models
    whose width the batch size picks (no general rows), the 512-wave boundary of pick_lanes at every width"""
    epw = 64 // lanes
    ns = {1, max(epw - 1, 1), epw, epw + 1, 16384, 16385, 65536, 65537, 131072, 131073}
    for waves in (256, 1024, 2048):
        ns |= {waves * epw, waves * epw + 1}
    if not general_rows:
        for c in WIDTHS:
            ns |= {511 * (64 // c), 511 * (64 // c) + 1}
    return sorted(ns)


def open_model(cm):
    """mm_model_create on a compiled model: (code, HipModel or None)"""
    blob = np.ascontiguousarray(cm.blob, dtype=np.uint32)
    h = C.c_void_p()
    rc = E.lib().mm_model_create(blob.ctypes.data, int(blob.size), C.byref(h))
    if rc:
        return rc, None
    hm = E.HipModel.__new__(E.HipModel)
    hm.cm, hm.h, hm.device, hm.precision, hm._n_states = cm, h, torch.device("cuda", torch.cuda.current_device()), E.MM_PREC_F32, 0
    return 0, hm


def apply_call(hm, call, arg):
    """(code, message) of a set_lanes / set_option call on the raw handle"""
    rc = E.lib().mm_model_set_lanes(hm.h, int(arg)) if call == "set_lanes" else E.lib().mm_model_set_option(hm.h, call.encode(), int(arg))
    return rc, (E.lib().mm_last_error().decode() if rc else "")


def device_plans(hm, nenvs) -> list:
    """mm_model_launch_info per batch size: the eight MM_LAUNCH_* values, or [code] of a refused launch"""
    rows = []
    for n in nenvs:
        out = (C.c_int * len(KEYS))()
        rc = E.lib().mm_model_launch_info(hm.h, int(n), out, len(KEYS))
        rows.append([rc] if rc else [int(v) for v in out])
    return rows


def model_record(cm) -> dict:
    rc, hm = open_model(cm)
    if rc:
        return {"refused": rc}
    nenvs = nenv_list(hm.info(E.INFO_LANES), hm.info(E.INFO_KERNEL_FAMILY) == 2)
    return {"nenv": nenvs, "info": device_plans(hm, nenvs)}


def option_record(cm, call, arg) -> dict:
    rc, hm = open_model(cm)
    assert rc == 0
    rc, msg = apply_call(hm, call, arg)
    if rc:
        return {"refused": [rc, msg]}
    return {"nenv": list(OPTION_NENV), "info": device_plans(hm, OPTION_NENV)}


def option_cases():
    return [(m, call, arg) for m in OPTION_MODELS for call, arg in OPTION_CALLS]


def get_model(name):
    return fixture_models()[name]()


def want_waves(row, nenv, f64=False) -> int:
    """waves per CU the planner wants for this batch at the recorded width"""
    waves = -(-nenv // (64 // row[0]))
    return min(max(-(-waves // 256), 1), 4 if f64 else 8)


def branches(rec) -> dict:
    """branch of the planner -> [(section, key, index into its nenv list)], every recorded case that takes it"""
    out = {k: [] for k in ("two_wave_1", "two_wave_0", "lds_model_1", "lds_model_0", "lds_limited", "rows2", "fp64") +
           tuple(f"auto_{c}" for c in WIDTHS)}
    for name, r in rec["models"].items():
        if "refused" in r:
            continue
        auto = len({row[0] for row in r["info"] if len(row) > 1}) > 1
        for i, (n, row) in enumerate(zip(r["nenv"], r["info"])):
            if len(row) == 1:
                continue
            at = ("models", name, i)
            out["two_wave_1" if row[2] else "two_wave_0"].append(at)
            out["lds_model_1" if row[3] else "lds_model_0"].append(at)
            if row[1] < want_waves(row, n):
                out["lds_limited"].append(at)
            if auto:
                out[f"auto_{row[0]}"].append(at)
            if name.startswith("rake"):
                out["rows2"].append(at)
    for key, r in rec["options"].items():
        if key.endswith(f":precision:{E.MM_PREC_F64}") and "refused" not in r:
            out["fp64"] += [("options", key, i) for i, row in enumerate(r["info"]) if len(row) > 1]
    return out


def gpu_subset(rec) -> list:
    """(section, key) of the cases the GPU test replays: per branch, the first model (and option call) that takes it"""
    keys = []
    for at in branches(rec).values():
        if at and at[0][:2] not in keys:
            keys.append(at[0][:2])
    return keys


def _recorded():
    return json.load(open(FIXTURE)) if os.path.exists(FIXTURE) else {"models": {}, "options": {}}


@pytest.fixture(scope="module")
def recorded():
    return json.load(open(FIXTURE))


def test_the_record_holds_every_branch(recorded):
    assert all(branches(recorded).values()), {k: len(v) for k, v in branches(recorded).items()}
    assert sorted(recorded["models"]) == sorted(fixture_models()) and \
        sorted(recorded["options"]) == sorted(f"{m}:{c}:{a}" for m, c, a in option_cases())


# ------------------------------------------------------------------ CPU: the planner as a host program under the sanitizers
@pytest.fixture(scope="session")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("launch_plan") / "launch_plan_main")
    cmd = ["c++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
           os.path.join(ROOT, "tests", "tools", "launch_plan_main.cpp")]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]
    return exe


def run_harness(exe, tmp_path, args, script=None):
    """run the harness on a command script; the lines it wrote, split into fields"""
    src, dst = str(tmp_path / "plan.script"), str(tmp_path / "plan.out")
    with open(src, "w") as f:
        f.write("\n".join(script or []) + "\n")
    # (the sanitizer runtime is linked into the program; whatever else the process preloads stays as it is)
    env = dict(os.environ, ASAN_OPTIONS="verify_asan_link_order=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([exe] + args + [src, dst], capture_output=True, text=True, env=env, timeout=120)
    assert "Sanitizer" not in p.stderr and "runtime error:" not in p.stderr and p.returncode == 0, p.stderr[-6000:]
    return [ln.split(" ", 2) if ln.startswith("call") else ln.split() for ln in open(dst).read().splitlines()]


def host_plans(exe, tmp_path, cm, nenvs, call=None):
    """(refusal of the call or None, plan rows [lanes, waves per block, two_wave, lds_model, LDS bytes, blocks] or [code])"""
    blob = str(tmp_path / "model.blob")
    np.ascontiguousarray(cm.blob, dtype=np.uint32).tofile(blob)
    script = ([f"{'lanes' if call[0] == 'set_lanes' else 'option ' + call[0]} {call[1]}"] if call else []) + [f"plan {n} 0" for n in nenvs]
    lines = run_harness(exe, tmp_path, ["model", blob], script)
    assert lines[0] == ["create", "0"], lines[0]
    lines = lines[1:]
    refusal = None
    if call:
        if int(lines[0][1]):
            refusal = [int(lines[0][1]), lines[0][2]]
        lines = lines[1:]
    rows = [[int(v) for v in ln[1:]] for ln in lines]
    assert all(ln[0] == "plan" for ln in lines) and len(rows) == len(nenvs)
    return refusal, [r[1:1 + NPLAN] if r[0] == 0 else [r[0]] for r in rows]


def _assert_plans(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == (w[:NPLAN] if len(w) > 1 else w), (g, w)


@pytest.mark.parametrize("name", list(fixture_models()))
def test_host_planner_under_sanitizers_gives_the_recorded_plans(recorded, harness, tmp_path, name):
    want = recorded["models"][name]
    if "refused" in want:
        return          # (mm_model_create refuses the model: tests/test_model_image.py holds the refusal)
    _, got = host_plans(harness, tmp_path, get_model(name), want["nenv"])
    _assert_plans(got, want["info"])


@pytest.mark.parametrize("name,call,arg", option_cases())
def test_host_planner_after_set_lanes_and_set_option(recorded, harness, tmp_path, name, call, arg):
    want = recorded["options"][f"{name}:{call}:{arg}"]
    refusal, got = host_plans(harness, tmp_path, get_model(name), want.get("nenv", [1]), (call, arg))
    if "refused" in want:
        assert refusal == want["refused"]
        return
    assert refusal is None
    _assert_plans(got, want["info"])


def listed_euler_kernels() -> list:
    """(lanes, nvp, general rows) of MM_KERNEL_LIST with integrator 0 (myosim_inst_list.hpp)"""
    text = open(os.path.join(E.CSRC, "myosim_inst_list.hpp")).read()
    groups = dict(re.findall(r"#define MM_KERNELS_(\w)\(X\)(.*)", text))
    order = re.findall(r"MM_KERNELS_(\w)\(X\)", re.search(r"#define MM_KERNEL_LIST\(X\)(.*)", text).group(1))
    return [(int(g), int(n), int(gn)) for k in order for g, n, gn, rk in re.findall(r"X\((\d+), (\d+), (\d+), (\d+)\)", groups[k]) if rk == "0"]


def test_inverse_library_geometry_is_the_one_its_own_loop_gave(harness, tmp_path):
    """The planner with lds_model = 0 and the helper waves off, against launch_on_device of myosim_inverse.hip before it called the
    planner:
        int wpb = (waves_needed + 255) / 256;  if (wpb < 1) wpb = 1;  if (wpb > 8) wpb = 8;
        while (wpb > 1 && (size_t)wpb * epw * m->lds_per_env > kLds) wpb--;
        epb = epw * wpb;  lds = (size_t)epb * m->lds_per_env;  if (lds > kLds) -> MM_ELDS;  grid = (nenv + epb - 1) / epb
    over every Euler (lanes, nvp, general rows) of MM_KERNEL_LIST; per-env LDS tables of 1 KB (the batch decides), 24 KB and 60 KB
    (LDS decides) and 170 KB (refused)."""
    kernels = listed_euler_kernels()
    assert len(kernels) >= 16 and len(set(kernels)) == len(kernels)
    lines = run_harness(harness, tmp_path, ["inverse"])
    rows = [[int(v) for v in ln[1:]] for ln in lines if ln[0] == "inverse"]
    k_lds = 160 * 1024
    seen = set()
    for G, nvp, gen, per_env, nenv, rc, lanes, wpb, two_wave, lm, lds, blocks, threads in rows:
        seen.add((G, nvp, gen, per_env, nenv))
        epw = 64 // G
        w = min(max(-(-(-(-nenv // epw)) // 256), 1), 8)
        while w > 1 and w * epw * per_env > k_lds:
            w -= 1
        if w * epw * per_env > k_lds:
            assert rc == -4, (G, nvp, gen, per_env, nenv, rc)          # MM_ELDS (include/myosim.h)
            continue
        assert (rc, lanes, wpb, two_wave, lm, lds, blocks, threads) == (0, G, w, 0, 0, epw * w * per_env, -(-nenv // (epw * w)), 64 * w), \
            (G, nvp, gen, per_env, nenv)
    assert seen == {(G, nvp, gen, pe, n) for G, nvp, gen in kernels for pe in (1024, 24 * 1024, 60 * 1024, 170 * 1024) for n in (1, 4096, 200000)}


# ------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("section,key", gpu_subset(_recorded()))
def test_gpu_launch_info_is_the_recorded_one(recorded, section, key):
    want = recorded[section][key]
    if section == "models":
        rc, hm = open_model(get_model(key))
        assert rc == 0
    else:
        name, call, arg = key.split(":")
        rc, hm = open_model(get_model(name))
        assert rc == 0 and apply_call(hm, call, int(arg)) == (0, "")
    assert device_plans(hm, want["nenv"]) == want["info"]


@pytest.mark.gpu
def test_gpu_launch_on_another_devices_handle():
    """model created on device 1, launched with device 0 current: the same result as with device 1 current, device 0 still current"""
    if torch.cuda.device_count() < 2:
        pytest.skip("one GPU visible")
    from myosuite_amd import inverse as I
    cm = synth.get_model("elbow")
    d1 = torch.device("cuda", 1)
    torch.cuda.set_device(0)
    hm, im = E.HipModel(cm, device=d1), I.InverseModel(cm, device=d1)
    ctrl = torch.full((8, cm.nu), 0.25, device=d1)
    qacc = torch.linspace(-1.0, 1.0, 8 * cm.nv, device=d1).reshape(8, cm.nv).contiguous()
    res = {}
    for cur in (0, 1):
        torch.cuda.set_device(cur)
        st = E.BatchState(hm, 8)
        E.step(hm, st, ctrl)
        inv = I.inverse(im, st, qacc)["qfrc_inverse"]
        assert torch.cuda.current_device() == cur
        torch.cuda.synchronize(d1)
        res[cur] = [t.cpu().numpy().copy() for t in (st.qpos, st.qvel, st.act, inv)]
    torch.cuda.set_device(0)
    assert np.abs(res[1][0] - cm.qpos0).max() > 0 or np.abs(res[1][1]).max() > 0          # the step moved the state
    for a, b in zip(res[0], res[1]):
        assert np.array_equal(a, b)
