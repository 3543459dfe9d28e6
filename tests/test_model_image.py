"""The model compiler (myosuite_amd/csrc/myosim_model_compile.hpp: model blob -> everything a model's kernels read besides state)
against the images recorded from the build before it was split out of mm_model_create (profiles/model_image_before_split.json,
written by tests/tools/record_model_image.py on that commit):

  * on the GPU, the device image read back through mm_debug_model_image is the recorded one bit for bit -- the two ten_len0 tables
    included -- with the same mm_model_info / mm_debug_layout values, also after set_lanes / set_option;
  * on the CPU, the same header compiled into a plain host program under AddressSanitizer + UndefinedBehaviorSanitizer gives the same
    integer packing word for word, the same Dims / Aux / Layouts / DbgLayout, and the floating-point ten_len0 tables to the rounding
    of another compiler (fp64: relative 1e-12 -- a sum of a few hundred rounded operations moves by a few hundred units of 2.2e-16
    without fast-math; fp32: one ulp);
  * the refusals keep their order, codes and messages.

The three floating-point sums behind ten_len0 (quaternion to matrix, frame position + R v, segment length) are written with a fixed
order of additions in the header: host code is built with -ffast-math, and left free the compiler reassociated them by the code around
them, which moved the fp64 table of the five rotated-mount hands by up to 71 ulp when the code was split into functions.
"""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from myosuite_amd import engine as E                                                # noqa: E402
from myosuite_amd.model import blob as B                                            # noqa: E402
from myosuite_amd.model import synth                                                # noqa: E402
from test_fuzz_models import random_contact_scene, random_model                     # noqa: E402  (same directory)

FIXTURE = os.path.join(ROOT, "profiles", "model_image_before_split.json")
LAYOUT_NAMES = ("xpos", "xquat", "xipos", "cdof", "cvel", "tenlen", "tenvel", "tenj", "actfrc", "actdot", "M", "bias", "smooth",
                "qaccsm", "qacc", "qfrccon", "efc_active", "efc_D", "efc_aref", "scal", "total")     # DbgLayout, in member order
NINFO = 20                                                                          # MM_INFO_* (include/myosim.h)
# set_lanes / set_option calls whose ConstBlocks are recorded too: (model, call, argument)
OPTION_CALLS = [("hand", "set_lanes", 64), ("elbow", "set_lanes", 8)] + \
               [(n, "iterations", 6) for n in ("hand", "torso", "elbow")] + [(n, "origin_shift", 0) for n in ("hand", "torso", "elbow")] + \
               [("hand", "precision", E.MM_PREC_F64)]


def _rake(njmax):
    from test_rows128 import rake_scene
    return rake_scene(njmax=njmax)


def fixture_models() -> dict:
    """name -> thunk of the compiled model, every model of the fixture"""
    out = {name: (lambda n=name: synth.get_model(n)) for name in synth.builders()}
    for seed in range(32):
        for integ in (0, 1, 3):
            out[f"fuzz{seed}_integ{integ}"] = lambda s=seed, i=integ: random_model(s, i).compile()
    for seed in range(12):
        out[f"contact_scene{seed}"] = lambda s=seed: random_contact_scene(s).compile()
    out["rake"] = lambda: _rake(128)
    out["rake_njmax96"] = lambda: _rake(96)
    return out


def _sec(blob, name):
    """(first word, words) of a section of a model blob"""
    i = B.SEC_INDEX[name]
    return int(blob[B.HEADER_WORDS + 2 * i]), int(blob[B.HEADER_WORDS + 2 * i + 1])


def refusal_cases() -> dict:
    """name -> (blob, nwords): a valid blob with one word edited (or one word short) that mm_model_create refuses"""
    Cn = B.C
    toy = np.array(synth.get_model("contact_toy").blob, dtype=np.uint32)
    arr = B.unpack(toy)

    def edit(blob, section, index, value, dtype=np.int32):
        out = blob.copy()
        out[_sec(blob, section)[0] + index] = np.array([value], dtype=dtype).view(np.uint32)[0]
        return out, int(out.size)
    cases = {}
    cases["integrator_2"] = edit(toy, "OPT_I", Cn["MM_OI_INTEGRATOR"], 2)
    cases["equality_not_joint"] = edit(toy, "EQ_TYPE", 0, Cn["MM_EQ_JOINT"] + 1)
    cases["condim_5"] = edit(toy, "PAIR_CONDIM", 0, 5)
    cases["njmax_129"] = edit(toy, "OPT_I", Cn["MM_OI_NJMAX"], 129)
    j = int(np.flatnonzero(arr["JNT_LIMITED"])[0])
    cases["joint_range_narrower_than_margins"] = edit(toy, "JNT_MARGIN", j, 100.0, np.float32)
    ten = np.array(synth.get_model("tendon_limit_toy").blob, dtype=np.uint32)
    t = int(np.flatnonzero(B.unpack(ten)["TENDON_LIMITED"])[0])
    cases["tendon_range_narrower_than_margins"] = edit(ten, "TENDON_MARGIN", t, 100.0, np.float32)
    # a plane-box pair takes two consecutive identical entries: point the second one at an ellipsoid instead
    pl = np.array(synth.get_model("plane_toy").blob, dtype=np.uint32)
    pa = B.unpack(pl)
    gt, g1, g2 = pa["GEOM_TYPE"], pa["PAIR_GEOM1"], pa["PAIR_GEOM2"]
    p = next(k for k in range(len(g1)) if gt[g1[k]] == Cn["MM_GEOM_PLANE"] and gt[g2[k]] == Cn["MM_GEOM_BOX"])
    assert g2[p + 1] == g2[p] and (p == 0 or g2[p - 1] != g2[p])
    cases["lone_plane_box_entry"] = edit(pl, "PAIR_GEOM2", p + 1, int(np.flatnonzero(gt == Cn["MM_GEOM_ELLIPSOID"])[0]))
    # (sphere, capsule) -> (sphere, plane)
    ta = arr
    p = next(k for k in range(len(ta["PAIR_GEOM1"])) if ta["GEOM_TYPE"][ta["PAIR_GEOM1"][k]] == Cn["MM_GEOM_SPHERE"])
    cases["sphere_plane_in_the_wrong_order"] = edit(toy, "PAIR_GEOM2", p, int(np.flatnonzero(ta["GEOM_TYPE"] == Cn["MM_GEOM_PLANE"])[0]))
    cases["nwords_one_short"] = (toy.copy(), int(toy.size) - 1)
    bad = toy.copy(); bad[0] ^= 1
    cases["wrong_magic"] = (bad, int(bad.size))
    return cases


def _sha(words) -> str:
    return hashlib.sha256(np.ascontiguousarray(words, dtype=np.uint32).tobytes()).hexdigest()


def image_record(img: np.ndarray, blob_words: int, ntendon: int) -> dict:
    """what the fixture keeps of an image (model words, then the two ConstBlocks): the hash of the model words with the two ten_len0
    tables zeroed, those tables verbatim, the hash of each ConstBlock"""
    ncb = (len(img) - blob_words) // 2
    assert ncb > 0 and blob_words + 2 * ncb == len(img)
    cb, cb_tw = img[blob_words:blob_words + ncb], img[blob_words + ncb:]
    t32, t64 = int(cb[-2]), int(cb[-1])                  # Aux::ten_len0 / ten_len0_f64, the last members of ConstBlock
    nt = max(ntendon, 1)
    assert t64 == t32 + ((nt + 1) & ~1) and t64 + 2 * nt <= blob_words and (int(cb_tw[-2]), int(cb_tw[-1])) == (t32, t64)
    words = img[:blob_words].copy()
    words[t32:t64 + 2 * nt] = 0
    return {"words": _sha(words), "ten_len0_f32": [int(w) for w in img[t32:t64]], "ten_len0_f64": [int(w) for w in img[t64:t64 + 2 * nt]],
            "const_block": _sha(cb), "const_block_two_wave": _sha(cb_tw)}


def create(blob: np.ndarray, nwords: int):
    """mm_model_create on raw words: (code, message, handle)"""
    blob = np.ascontiguousarray(blob, dtype=np.uint32)
    h = C.c_void_p()
    rc = E.lib().mm_model_create(blob.ctypes.data, int(nwords), C.byref(h))
    return rc, (E.lib().mm_last_error().decode() if rc else ""), h


def device_record(cm) -> dict:
    """the fixture entry of a model from the library on the GPU: image_record of the read-back, info and layout values -- or the
    refusal"""
    rc, msg, h = create(cm.blob, cm.blob.size)
    if rc:
        return {"refused": [rc, msg]}
    hm = E.HipModel.__new__(E.HipModel)
    hm.h, hm.device = h, __import__("torch").device("cuda", 0)
    return handle_record(hm, cm.ntendon)


def handle_record(hm, ntendon) -> dict:
    rec = image_record(hm.debug_image(), hm.info(E.INFO_MODEL_WORDS), ntendon)
    rec["info"] = [hm.info(k) for k in range(NINFO)]
    rec["layout"] = [hm.layout(n) for n in LAYOUT_NAMES]
    return rec


def apply_option(hm, call, arg):
    if call == "set_lanes":
        hm.set_lanes(arg)
    else:
        hm.set_option(call, arg)


@pytest.fixture(scope="module")
def recorded():
    return json.load(open(FIXTURE))


# ------------------------------------------------------------------ GPU: the device image is the recorded one
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(fixture_models()))
def test_gpu_device_image_is_the_recorded_one(recorded, name):
    assert device_record(fixture_models()[name]()) == recorded["models"][name]


@pytest.mark.gpu
@pytest.mark.parametrize("name,call,arg", OPTION_CALLS)
def test_gpu_const_blocks_after_set_lanes_and_set_option(recorded, name, call, arg):
    cm = synth.get_model(name)
    hm = E.HipModel(cm)
    apply_option(hm, call, arg)
    assert handle_record(hm, cm.ntendon) == recorded["options"][f"{name}:{call}:{arg}"]


@pytest.mark.gpu
def test_gpu_model_image_refuses_a_short_buffer():
    hm = E.HipModel(synth.get_model("elbow"))
    n = len(hm.debug_image())
    out = np.zeros(n, dtype=np.uint32)
    assert E.lib().mm_debug_model_image(hm.h, out.ctypes.data, n - 1) == -5          # MM_EARG (include/myosim.h)
    assert E.lib().mm_debug_model_image(hm.h, out.ctypes.data, n) == n


# ------------------------------------------------------------------ CPU: the compiler as a host program under the sanitizers
@pytest.fixture(scope="session")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("model_image") / "model_image_main")
    cmd = ["c++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
           os.path.join(ROOT, "tests", "tools", "model_image_main.cpp")]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]
    return exe


def host_compile(exe, tmp_path, blob, nwords):
    """run the harness: (code, message or None, head, DbgLayout, origin, image words)"""
    src, dst = str(tmp_path / "model.blob"), str(tmp_path / "model.image")
    np.ascontiguousarray(blob, dtype=np.uint32)[:nwords].tofile(src)
    # (the sanitizer runtime is linked into the program; whatever else the process preloads stays as it is)
    env = dict(os.environ, ASAN_OPTIONS="verify_asan_link_order=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([exe, src, dst], capture_output=True, text=True, env=env, timeout=120)
    assert "Sanitizer" not in p.stderr and "runtime error:" not in p.stderr and p.returncode == 0, p.stderr[-6000:]
    raw = open(dst, "rb").read()
    head = np.frombuffer(raw[:64], dtype=np.int32)
    if head[0]:
        return int(head[0]), raw[64:].decode(), head, None, None, None
    nl = 4 * len(LAYOUT_NAMES)
    return 0, None, head, np.frombuffer(raw[64:64 + nl], dtype=np.int32), np.frombuffer(raw[64 + nl:76 + nl], dtype=np.float32), \
        np.frombuffer(raw[76 + nl:], dtype=np.uint32)


@pytest.mark.parametrize("name", list(fixture_models()))
def test_host_compiler_under_sanitizers_gives_the_recorded_image(recorded, harness, tmp_path, name):
    cm = fixture_models()[name]()
    want = recorded["models"][name]
    rc, msg, head, dbg, origin, img = host_compile(harness, tmp_path, cm.blob, cm.blob.size)
    if "refused" in want:
        assert [rc, msg] == want["refused"]
        return
    assert rc == 0 and len(img) == head[13]
    got = image_record(img, int(head[8]), cm.ntendon)
    # integer packing: every word outside the two ten_len0 tables, Dims / Layout / Aux of both launch forms (the origin among them)
    for k in ("words", "const_block", "const_block_two_wave"):
        assert got[k] == want[k], k
    assert [int(v) for v in dbg] == want["layout"]
    info = want["info"]
    assert (int(head[1]), int(head[11]), int(head[8]), int(head[7])) == \
        (info[E.INFO_LANES], info[E.INFO_LDS_PER_ENV], info[E.INFO_MODEL_WORDS], info[E.INFO_TENDON_FOLDED])
    assert (int(head[9]), int(head[10])) == (int(head[8]), int(head[8]) + (len(img) - int(head[8])) // 2)
    # the folded tendon lengths: floating point, another compiler and no fast-math here
    f64 = lambda ws: np.array(ws, dtype=np.uint32).view(np.float64)
    f32 = lambda ws: np.array(ws, dtype=np.uint32).view(np.float32)
    a, b = f64(got["ten_len0_f64"]), f64(want["ten_len0_f64"])
    assert np.all(np.abs(a - b) <= 1e-12 * np.abs(b)), (a, b)
    a, b = f32(got["ten_len0_f32"]), f32(want["ten_len0_f32"])
    assert np.all(np.abs(a.astype(np.float64) - b.astype(np.float64)) <= np.spacing(np.abs(b)).astype(np.float64)), (a, b)


def test_refusals_keep_their_codes_and_messages(recorded, harness, tmp_path):
    cases = refusal_cases()
    assert sorted(cases) == sorted(recorded["refusals"])
    got = {}
    for name, (blob, nwords) in cases.items():
        rc, msg, *_ = host_compile(harness, tmp_path, blob, nwords)
        got[name] = [rc, msg]
    assert got == recorded["refusals"]
