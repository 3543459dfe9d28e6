"""Record profiles/launch_plans_before_host_core.json: what tests/test_launch_plan.py holds the launch planner to.  Run on the GPU with
the library of the commit BEFORE the planner was split out of launch_on_device:

    python tests/tools/record_launch_plans.py [out.json]

Per model of test_model_image.fixture_models() that mm_model_create accepts: the eight mm_model_launch_info values (or the code of a
refused launch) at every batch size of test_launch_plan.nenv_list(); the same at OPTION_NENV after each set_lanes / set_option call
of option_cases(), or (code, message) of a refused call.  Asserts that every branch of the planner is in the record."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import test_launch_plan as T          # noqa: E402
from myosuite_amd import engine as E  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else T.FIXTURE
    rec = {"what": "mm_model_launch_info before the launch planner was split out of launch_on_device (tests/tools/record_launch_plans.py)",
           "version": E.lib().mm_version().decode(), "keys": list(T.KEYS), "models": {}, "options": {}}
    for name, make in T.fixture_models().items():
        rec["models"][name] = T.model_record(make())
    for name, call, arg in T.option_cases():
        rec["options"][f"{name}:{call}:{arg}"] = T.option_record(T.get_model(name), call, arg)
    missing = [k for k, v in T.branches(rec).items() if not v]
    assert not missing, f"no recorded case takes: {missing}"
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(json.dumps(rec, separators=(",", ":")).replace('"models":{', '"models":{\n').replace("},", "},\n"))
    refused = [n for n, r in rec["models"].items() if "refused" in r]
    print(f"{len(rec['models'])} models ({len(refused)} refused: {refused}), {len(rec['options'])} option calls "
          f"({sum('refused' in r for r in rec['options'].values())} refused), {len(T.gpu_subset(rec))} in the GPU subset -> {out}")


if __name__ == "__main__":
    main()
