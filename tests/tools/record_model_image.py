"""Record profiles/model_image_before_split.json: what tests/test_model_image.py holds the model compiler to.  Run on the GPU with the
library of the commit BEFORE the compiler was split out of mm_model_create, plus only the mm_debug_model_image read-back:

    python tests/tools/record_model_image.py [out.json]

Per model: image_record() of the device image, every mm_model_info value and mm_debug_layout offset -- or (code, message) of a
refused one; the same after the set_lanes / set_option calls of OPTION_CALLS; (code, message) of every refusal case."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import test_model_image as T          # noqa: E402
from myosuite_amd import engine as E  # noqa: E402
from myosuite_amd.model import synth  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else T.FIXTURE
    rec = {"what": "device images of mm_model_create before the model compiler was split out of it (tests/tools/record_model_image.py)",
           "version": E.lib().mm_version().decode(), "models": {}, "options": {}, "refusals": {}}
    for name, make in T.fixture_models().items():
        rec["models"][name] = T.device_record(make())
    for name, call, arg in T.OPTION_CALLS:
        cm = synth.get_model(name)
        hm = E.HipModel(cm)
        T.apply_option(hm, call, arg)
        rec["options"][f"{name}:{call}:{arg}"] = T.handle_record(hm, cm.ntendon)
    for name, (blob, nwords) in T.refusal_cases().items():
        rc, msg, h = T.create(blob, nwords)
        assert rc != 0, name
        rec["refusals"][name] = [rc, msg]
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(rec, f, indent=0, separators=(",", ":"))
    refused = [n for n, r in rec["models"].items() if "refused" in r]
    print(f"{len(rec['models'])} models ({len(refused)} refused: {refused}), {len(rec['options'])} option calls, {len(rec['refusals'])} refusals -> {out}")


if __name__ == "__main__":
    main()
