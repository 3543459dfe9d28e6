"""How often does a model drop contacts / rows (status bit 8) under the perf tool's action stream?
python tools/gpu_bit8_rate.py [hand_dense hand_dense_full ...] [--steps 54]
Rolls `myoHandReorient100-v0` at 2048 envs as tools/gpu_perf.py does (seed 0, in-kernel actions, action seed 0) and counts, after every
env-step, the envs whose sticky status carries bit 8 (an env re-armed in that step has just had its status cleared)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from myosuite_amd.envs import registry
steps = int(sys.argv[sys.argv.index("--steps") + 1]) if "--steps" in sys.argv else 54
names = [a for a in sys.argv[1:] if not a.startswith("--") and not a.isdigit()] or ["hand_dense", "hand_dense_full"]
n = 2048
for nm in names:
    env = registry.make("myoHandReorient100-v0", num_envs=n, seed=0, model=nm)
    env.rollout_setup(action_seed=0)
    seen = torch.zeros(n, dtype=torch.bool, device=env.device)
    flagged_steps = 0
    for s in range(steps):
        env.rollout_step(None, stream_id=s if s < 6 else 1000 + s - 6)
        f = (env.state.status & 8) != 0
        seen |= f
        flagged_steps += int(f.sum())
    print(f"{nm:16s} njmax {env.cm.njmax:3d} nconmax {env.cm.nconmax:2d}: {int(seen.sum())} of {n} envs carried bit 8 after at least one of {steps} env-steps; "
          f"{flagged_steps} of {n * steps} env-steps ended with it set ({100.0 * flagged_steps / (n * steps):.3f} %)")
