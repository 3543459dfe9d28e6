#!/usr/bin/env python
"""How many contacts and constraint rows does the dense reorient hand need?  (CPU only: the fp64 oracle.)

    python tests/tools/rows128_oracle_bounds.py [--envs 2048] [--steps 7] [--jobs 16] [--nconmax N --njmax M]

Rolls the oracle over the inputs of tests/test_rows128.py's parity scan -- `myoHandReorient100-v0`, seed 23, the device-side reset
draws of every env, seven env-steps of in-kernel U[0,1) actions (action seed 3, stream = step), the masked auto-reset of an env
that drops its object -- with the contact / row bounds given (default: far above anything reached) and reports, over every
substep and trailing forward pass of every env: max contacts, max rows, and how many envs raise the oracle's overflow
warnings (2: rows beyond njmax, 4: contacts beyond nconmax).  `hand_dense_full`'s bounds in model/synth.py are the smallest
nconmax and the smallest njmax (rounded up to 4) for which this script reports no warning; `--nconmax 12 --njmax 56` gives the drop
rate of `hand_dense` over the same stream."""
import argparse
import concurrent.futures
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def _model(nconmax, njmax):
    from myosuite_amd.model import synth

    def edit(s):
        s.nconmax, s.njmax = nconmax, njmax
    return synth.compile_spec("hand_dense", edit)


def _roll(args):
    e0, e1, nenv, steps, seed, action_seed, nconmax, njmax = args
    from myosuite_amd.model import synth
    from oracle import env_oracle as EO
    cm = _model(nconmax, njmax)
    tables = synth.reorient_tables("100")
    acts = [EO.uniform_stream(nenv * cm.nu, action_seed, s).reshape(nenv, cm.nu) for s in range(steps)]
    out = []
    for e in range(e0, e1):
        o = EO.ReorientEnvOracle(cm, frame_skip=5)
        episode = 0
        gt, size, ah, des = EO.reorient_reset_draws(tables, e, episode, seed, o.tar_length)
        o.reset(size, ah, des, gt)
        mcon, mrow, step_warn = o.d.ncon, o.d.nefc, 0
        for s in range(steps):
            a = acts[s][e].astype(np.float64)
            ctrl = a.copy()
            ctrl[o.muscle] = 1.0 / (1.0 + np.exp(-5.0 * (ctrl[o.muscle] - 0.5)))
            o.d.ctrl[:] = ctrl
            for _ in range(o.frame_skip):
                o.d.step(1)
                mcon, mrow = max(mcon, o.d.ncon), max(mrow, o.d.nefc)
            o.d.forward()
            mcon, mrow = max(mcon, o.d.ncon), max(mrow, o.d.nefc)
            step_warn |= o.d.warn
            if bool(o._obs_rwd()[1]["done"]):
                episode += 1
                gt, size, ah, des = EO.reorient_reset_draws(tables, e, episode, seed, o.tar_length)
                o.reset(size, ah, des, gt)
                mcon, mrow = max(mcon, o.d.ncon), max(mrow, o.d.nefc)
        # the scan's own forward pass: the last controls on the final state
        o.d.forward()
        mcon, mrow = max(mcon, o.d.ncon), max(mrow, o.d.nefc)
        out.append((e, mcon, mrow, step_warn | o.d.warn, episode))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=23)
    ap.add_argument("--action-seed", type=int, default=3)
    ap.add_argument("--jobs", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--nconmax", type=int, default=256)
    ap.add_argument("--njmax", type=int, default=1024)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from oracle import oracle as O
    O.build()
    chunk = max(1, a.envs // (4 * a.jobs))
    jobs = [(e0, min(a.envs, e0 + chunk), a.envs, a.steps, a.seed, a.action_seed, a.nconmax, a.njmax) for e0 in range(0, a.envs, chunk)]
    rows = []
    with concurrent.futures.ProcessPoolExecutor(max_workers=a.jobs) as ex:
        for r in ex.map(_roll, jobs):
            rows += r
    r = np.array(rows)
    rec = {"envs": a.envs, "steps": a.steps, "seed": a.seed, "action_seed": a.action_seed, "nconmax": a.nconmax, "njmax": a.njmax,
           "max_contacts": int(r[:, 1].max()), "max_rows": int(r[:, 2].max()),
           "envs_above_64_rows": int((r[:, 2] > 64).sum()), "envs_above_56_rows": int((r[:, 2] > 56).sum()),
           "envs_with_row_overflow_warning": int(((r[:, 3] & 2) != 0).sum()),
           "envs_with_contact_overflow_warning": int(((r[:, 3] & 4) != 0).sum()),
           "envs_with_either_warning": int(((r[:, 3] & 6) != 0).sum()), "envs_reset_in_stream": int((r[:, 4] > 0).sum())}
    print(json.dumps(rec))
    if a.out:
        json.dump(rec, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
