"""Fused PPO learner kernels (include/myosim_ppo.h, myosuite_amd/csrc/myosim_ppo.hip) against an fp64 restatement of the learner
written here from the header alone: flat parameter vector (policy first; per layer W[out][in] then b[out]), SiLU hidden layers,
std = softplus(o) + 1e-3, the squashed-action log-density, the clipped surrogate / entropy / value loss, clamp((obs - mean) / std,
-5, 5), clip_grad_norm_ + bias-corrected Adam.  Everything is driven through engine.FusedPPO with synthetic tensors: no env.

Bound of every comparison, per parameter tensor (every W and every b of both networks) or per output:
    err(t) = max|kernel - fp64| / max|fp64|  <=  2e-4   (the figure of tests/test_ppo_fused.py, there per network)
or, where a tensor does not meet it,       <=  4 x err32(t), err32 = the same figure for the SAME function evaluated by torch in fp32
on the device (an independent fp32 evaluation: rocBLAS summation order instead of MFMA tile order, reductions of up to 512 terms).

Tensors that needed the second form on an MI355X (all of them; every other tensor and every mm_ppo_act output of every case met
2e-4; also in NOTES.md, "fp64 check of the PPO learner kernels").  They are in the regime where fp32 itself is far from fp64: with
std at its 1e-3 floor z = (raw - mean) / std carries the rounding of the mean (~1e-7 relative) times 1 / std = 1000.  The figures
are the same under 16 and 32 samples per workgroup.

    case (mm_ppo_grad)     tensor     err        err32
    wide_o-clamp-tanh      pi.b2      2.76e-04   3.04e-04
    wide_o-sigmoid         pi.b0      2.46e-04   2.59e-04
    wide_o-sigmoid         pi.W1      2.07e-04   2.11e-04
    wide_o-sigmoid         pi.b1      2.39e-04   1.96e-04
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

F64 = torch.float64
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)
EPS_CLIP, ENT_COST, VALUE_COST = 0.2, 1e-2, 0.5
RHOS = (0.5, 0.7, 0.9, 1.1, 1.3, 1.6)          # importance ratios of the synthetic minibatches: each >= 0.1 from 1 +- 0.2
BOUND, FACTOR32 = 2e-4, 4.0


# ------------------------------------------------------------------ the reference (plain torch; float64 on the CPU is the checker) --
class Spec:
    def __init__(self, obs_dim, act_dim, policy_hidden, value_hidden):
        self.obs_dim, self.act_dim = obs_dim, act_dim
        self.ph, self.vh = tuple(policy_hidden), tuple(value_hidden)
        self.pw, self.vw = self.ph + (2 * act_dim,), self.vh + (1,)
        self.tensors, o = [], 0                                    # (name, offset, out, in) in the order of the flat vector
        for net, widths in (("pi", self.pw), ("vf", self.vw)):
            if net == "vf":
                self.value_offset = o
            k = obs_dim
            for l, w in enumerate(widths):
                self.tensors.append((f"{net}.W{l}", o, w, k)); o += w * k
                self.tensors.append((f"{net}.b{l}", o, w, 0)); o += w
                k = w
        self.param_count = o

    def layers(self, p, net):
        out = []
        for name, o, w, k in self.tensors:
            if name.startswith(net + ".W"):
                out.append([p[o:o + w * k].view(w, k), None])
            elif name.startswith(net + ".b"):
                out[-1][1] = p[o:o + w]
        return out


def softplus(x):
    """log(1 + exp(x)) with no threshold: literally in float64; in float32 (the err32 evaluation) the algebraically identical
    max(x, 0) + log1p(exp(-|x|)), which does not overflow where raw reaches 100"""
    if x.dtype == F64:
        return torch.log1p(torch.exp(x))
    return x.clamp(min=0) + torch.log1p(torch.exp(-x.abs()))


def mlp(layers, x):
    for i, (W, b) in enumerate(layers):
        x = x @ W.t() + b
        if i + 1 < len(layers):
            x = x * torch.sigmoid(x)               # SiLU
    return x


def normalise(obs, om, os_):
    return obs if om is None else ((obs - om) / os_).clamp(-5.0, 5.0)


def log_det_squash(x, squash):
    """log |d squash(x) / d x|: log(1 - tanh^2) = 2 (log 2 - x - softplus(-2x)); log(s (1 - s)) = -softplus(-x) - softplus(x)"""
    if squash == "tanh":
        return 2.0 * (math.log(2.0) - x - softplus(-2.0 * x))
    return -softplus(-x) - softplus(x)


def squash_fn(x, squash):
    return torch.tanh(x) if squash == "tanh" else torch.sigmoid(x)


def policy_dist(spec, p, x):
    out = mlp(spec.layers(p, "pi"), x)
    ad = spec.act_dim
    return out[:, :ad], softplus(out[:, ad:]) + 1e-3, out[:, ad:]


def log_density(mean, std, raw, squash):
    """log-density of the squashed action squash(raw), raw ~ N(mean, std), summed over the action dimensions"""
    z = (raw - mean) / std
    return (-0.5 * z * z - torch.log(std) - HALF_LOG_2PI - log_det_squash(raw, squash)).sum(-1)


def ppo_loss(spec, p, obs, om, os_, raw, logp_old, adv, ret, enoise, squash, eps=EPS_CLIP, entc=ENT_COST, vc=VALUE_COST):
    """-mean(min(r A, clip(r) A)) - entropy_cost mean(H) + value_cost mean((V - ret)^2) of the rows given; returns (loss, ratio)"""
    x = normalise(obs, om, os_)
    mean, std, _ = policy_dist(spec, p, x)
    ratio = torch.exp(log_density(mean, std, raw, squash) - logp_old)
    surr = torch.minimum(ratio * adv, ratio.clamp(1.0 - eps, 1.0 + eps) * adv)
    H = (0.5 + HALF_LOG_2PI + torch.log(std)).sum(-1)
    if enoise is not None:
        H = H + log_det_squash(mean + std * enoise, squash).sum(-1)
    V = mlp(spec.layers(p, "vf"), x)[:, 0]
    return -surr.mean() - entc * H.mean() + vc * ((V - ret) ** 2).mean(), ratio


def ppo_grad(spec, p, *args, **kw):
    p = p.detach().clone().requires_grad_(True)
    loss, ratio = ppo_loss(spec, p, *args, **kw)
    loss.backward()
    return p.grad.detach(), ratio.detach()


def adam_reference(p, grads, lr, b1, b2, eps, max_norm, gscale):
    """clip_grad_norm_ (coef = min(1, max_norm / (norm + 1e-6))) then bias-corrected Adam with eps outside the root, in p's dtype"""
    p = p.clone()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for t, g in enumerate(grads, 1):
        g = g.to(p.dtype) * gscale
        if max_norm:
            g = g * min(1.0, max_norm / (float(g.norm()) + 1e-6))
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g * g
        p = p - (lr / (1 - b1 ** t)) * m / (v.sqrt() / math.sqrt(1 - b2 ** t) + eps)
    return p


# ------------------------------------------------------------------ synthetic minibatches -----------------------------------------
def f32(x):
    """round to float32, keep float64: kernel and reference are given the same numbers"""
    return x.float().double()


def clipped_randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=F64).clamp(-4.0, 4.0)


class Data:
    pass


def make_data(spec, squash, B, regime="plain", norm=True, clamp=False, ent=True, seed=0):
    """Parameters and unroll buffers of B rows, float32-representable, held in float64.  regime shapes the policy's output layer on
    THESE observations: "plain" (mean ~ 0.5, std ~ 0.5), "wide_o" (raw scale o spanning [-29.5, 29.5]: std at its floor and
    softplus beyond its threshold), "big_raw" (means spanning [-13, 13], |raw| up to 15)."""
    g = torch.Generator().manual_seed(1000 + seed)
    d = Data()
    d.spec, d.squash, d.B = spec, squash, B
    od, ad = spec.obs_dim, spec.act_dim
    if norm:
        d.om = f32(torch.randn(od, generator=g, dtype=F64))
        d.os = f32(0.5 + 1.5 * torch.rand(od, generator=g, dtype=F64))
        t = torch.randn(B, od, generator=g, dtype=F64)
        if clamp:
            u = torch.rand(B, od, generator=g, dtype=F64)
            far = 6.0 + 2.0 * torch.rand(B, od, generator=g, dtype=F64)
            t = torch.where(u < 0.15, -far, torch.where(u > 0.85, far, t))
            d.os[od // 2] = 1e-6                                   # one column at the floor of the running std
            d.os = f32(d.os)
        d.obs = f32(d.om + d.os * t)
    else:
        assert not clamp
        d.om = d.os = None
        d.obs = f32(torch.randn(B, od, generator=g, dtype=F64))
    p = torch.zeros(spec.param_count, dtype=F64)
    for name, o, w, k in spec.tensors:
        p[o:o + (w * k if k else w)] = (torch.randn(w * k, generator=g, dtype=F64) / math.sqrt(k)) if k else 0.1 * torch.randn(w, generator=g, dtype=F64)
    p = f32(p)
    # shape the policy's output layer: its input rows are fixed by the layers below
    x = normalise(d.obs, d.om, d.os)
    hid = spec.layers(p, "pi")[:-1]
    a = x
    for W, b in hid:
        a = a @ W.t() + b
        a = a * torch.sigmoid(a)
    (_, o_w, w_out, k_in), (_, o_b, _, _) = [t for t in spec.tensors if t[0].startswith("pi.")][-2:]
    W = p[o_w:o_w + w_out * k_in].view(w_out, k_in)
    bias = p[o_b:o_b + w_out]

    def span(rows, lo, hi):
        """rescale rows of W (and set their bias) so that the outputs over the buffer span exactly [lo, hi]"""
        u = a @ W[rows].t()
        c, h = 0.5 * (u.max() + u.min()), 0.5 * (u.max() - u.min())
        assert h > 0
        s = 0.5 * (hi - lo) / h
        W[rows] *= s
        bias[rows] = 0.5 * (hi + lo) - c * s

    def spread(rows, sd, centre):
        u = a @ W[rows].t()
        W[rows] *= sd / max(float(u.std()) if u.numel() > 1 else 1.0, 1e-3)
        bias[rows] = centre + 0.1 * torch.randn(ad, generator=g, dtype=F64)

    m_rows, o_rows = slice(0, ad), slice(ad, 2 * ad)
    if regime == "plain":
        spread(m_rows, 0.5, 0.0); spread(o_rows, 0.5, -0.5)
    elif regime == "wide_o":
        span(m_rows, -2.0, 2.0); span(o_rows, -29.5, 29.5)
    elif regime == "big_raw":
        span(m_rows, -13.0, 13.0); spread(o_rows, 0.3, -1.2)
    else:
        raise ValueError(regime)
    d.p = f32(p)
    with torch.no_grad():
        mean, std, _ = policy_dist(spec, d.p, x)
        d.e = f32(clipped_randn(g, B, ad))                         # |e| <= 4: z stays bounded
        d.raw = f32(mean + std * d.e)
        rho = torch.tensor(RHOS, dtype=F64)[torch.randperm(B, generator=g) % len(RHOS)]
        d.logp_old = f32(log_density(mean, std, d.raw, squash) - torch.log(rho))
    d.adv = f32(torch.randn(B, generator=g, dtype=F64))
    d.adv[::3] = 0.0                                               # both signs and exact zeros
    d.ret = f32(torch.randn(B, generator=g, dtype=F64))
    d.enoise = f32(clipped_randn(g, B, ad)) if ent else None
    return d


def make_idx(B, mb, seed, repeat):
    """non-monotone rows of the buffer; repeat: some rows taken twice"""
    g = torch.Generator().manual_seed(77 + seed)
    idx = torch.randperm(B, generator=g)[:mb].clone()
    if mb >= 3 and bool((idx[1:] > idx[:-1]).all()):
        idx = idx.flip(0)
    if repeat and mb >= 6:
        idx[-3:] = idx[:3]
    return idx


def reference_grad(d, idx, dtype=F64, device="cpu"):
    c = lambda t: None if t is None else t.to(device=device, dtype=dtype)
    i = idx.to(device)
    rows = lambda t: None if t is None else c(t)[i]
    return ppo_grad(d.spec, c(d.p), rows(d.obs), c(d.om), c(d.os), rows(d.raw), rows(d.logp_old), rows(d.adv), rows(d.ret), rows(d.enoise), d.squash)


def assert_preconditions(d, idxs, regime, clamp):
    """what the case is meant to exercise holds on the fp64 reference, over the rows of all the launches of the case"""
    idx = torch.cat(list(idxs))
    with torch.no_grad():
        x = normalise(d.obs[idx], d.om, d.os)
        mean, std, o = policy_dist(d.spec, d.p, x)
        raw, adv = d.raw[idx], d.adv[idx]
        ratio = torch.exp(log_density(mean, std, raw, d.squash) - d.logp_old[idx])
    for t in (x, mean, std, o, raw, ratio, d.p, d.ret):
        assert bool(torch.isfinite(t).all())
    assert float(((ratio - (1 + EPS_CLIP)).abs()).min()) > 0.05 and float(((ratio - (1 - EPS_CLIP)).abs()).min()) > 0.05
    hi, lo = ratio > 1 + EPS_CLIP, ratio < 1 - EPS_CLIP
    assert bool(hi.any()) and bool(lo.any()) and bool((~hi & ~lo).any()), "all three clip branches"
    if idx.numel() >= 15:
        assert bool((adv > 0).any()) and bool((adv < 0).any()) and bool((adv == 0).any())
        dead = (hi & (adv > 0)) | (lo & (adv < 0))                     # min() picks the clipped, constant arm
        assert bool(dead.any()) and bool((~dead & (adv != 0)).any())
    assert float((((raw - mean) / std).abs()).max()) <= 4.0 + 1e-3
    if regime == "wide_o":
        assert float(o.min()) < -20.0 and float(o.max()) > 20.0 and float(o.abs().max()) <= 30.0
        assert bool(((o > 0) & (o < 20.0)).any()) and bool((softplus(o) < 1e-4).any()), "both sides of the threshold; std at its floor"
    if regime == "big_raw":
        assert 10.0 <= float(raw.abs().max()) <= 16.0
    if clamp:
        assert float((x == -5.0).double().mean()) >= 0.10 and float((x == 5.0).double().mean()) >= 0.10
        assert float(d.os.min()) == float(f32(torch.tensor(1e-6, dtype=F64)))


# ------------------------------------------------------------------ CPU: the reference checks itself -------------------------------
@pytest.mark.parametrize("squash", ["tanh", "sigmoid"])
@pytest.mark.parametrize("ent", [True, False], ids=["entropy+squash", "entropy-normal"])
def test_reference_gradient_agrees_with_central_differences(squash, ent):
    spec = Spec(9, 3, (5,), (4,))
    d = make_data(spec, squash, 24, "plain", norm=True, clamp=False, ent=ent, seed=3)
    idx = make_idx(24, 18, 3, repeat=True)
    assert_preconditions(d, [idx], "plain", False)
    g, _ = reference_grad(d, idx)
    args = [t[idx] if t is not None and t.shape[:1] == (24,) else t for t in (d.obs, d.om, d.os, d.raw, d.logp_old, d.adv, d.ret, d.enoise)]
    h, fd = 1e-5, torch.zeros_like(g)
    with torch.no_grad():
        for i in range(spec.param_count):
            pp, pm = d.p.clone(), d.p.clone()
            pp[i] += h; pm[i] -= h
            fd[i] = (ppo_loss(spec, pp, *args, squash)[0] - ppo_loss(spec, pm, *args, squash)[0]) / (2 * h)
    for name, o, w, k in spec.tensors:
        n = w * k if k else w
        scale = float(g[o:o + n].abs().max())
        assert scale > 0 and float((g[o:o + n] - fd[o:o + n]).abs().max()) < 1e-6 * scale, name      # O(h^2) = 1e-10 truncation + 1e-16 / h = 1e-11 rounding


@pytest.mark.parametrize("squash", ["tanh", "sigmoid"])
def test_reference_log_density_integrates_to_one_over_the_squashed_action(squash):
    n = 400_000
    lo, hi = (-1.0, 1.0) if squash == "tanh" else (0.0, 1.0)
    a = lo + (hi - lo) * (torch.arange(n, dtype=F64) + 0.5) / n              # midpoint rule over the action
    raw = torch.atanh(a) if squash == "tanh" else torch.log(a) - torch.log1p(-a)
    for mean, std in ((0.3, 0.6), (-1.2, 0.25)):
        lp = log_density(torch.full((n, 1), mean, dtype=F64), torch.full((n, 1), std, dtype=F64), raw[:, None], squash)
        assert abs(float(torch.exp(lp).sum()) * (hi - lo) / n - 1.0) < 1e-6, (squash, mean, std)


def test_reference_adam_first_step_is_lr_and_matches_torch_adam_in_fp64():
    g = torch.Generator().manual_seed(0)
    p0 = torch.randn(37, generator=g, dtype=F64)
    grads = [torch.randn(37, generator=g, dtype=F64) * (10.0 ** (k % 5 - 3)) for k in range(40)]
    one = adam_reference(p0, [torch.sign(grads[0]) * (1.0 + grads[0].abs())], 3e-3, 0.9, 0.999, 1e-8, None, 1.0)
    assert float(((one - p0).abs() - 3e-3).abs().max()) < 1e-9             # lr |g| / (|g| + eps), |g| >= 1
    ref = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([ref], lr=3e-3)
    for gk in grads:
        ref.grad = gk.clone()
        torch.nn.utils.clip_grad_norm_([ref], 0.5)
        opt.step()
    assert float((adam_reference(p0, grads, 3e-3, 0.9, 0.999, 1e-8, 0.5, 1.0) - ref.detach()).abs().max()) < 1e-12


# ------------------------------------------------------------------ GPU ------------------------------------------------------------
def _handle(spec, squash, max_minibatch, **kw):
    from myosuite_amd import engine as E
    args = dict(learning_rate=3e-3, clipping_epsilon=EPS_CLIP, entropy_cost=ENT_COST, value_cost=VALUE_COST, max_grad_norm=0.5)
    args.update(kw)
    K = E.FusedPPO(spec.obs_dim, spec.act_dim, spec.ph, spec.vh, squash, max_minibatch=max_minibatch, **args)
    assert K.param_count == spec.param_count and K.value_offset == spec.value_offset
    return K


def _dev(t):
    return None if t is None else t.float().cuda().contiguous()


class DevData:
    def __init__(self, d):
        for k in ("p", "obs", "om", "os", "raw", "logp_old", "adv", "ret", "enoise", "e"):
            setattr(self, k, _dev(getattr(d, k)))


def _kernel_grad(K, dd, idx):
    out = torch.full((K.param_count,), 7.0, device="cuda")          # sentinel: the kernels overwrite every entry
    K.grad(dd.p, dd.obs, dd.om, dd.os, idx.cuda(), dd.raw, dd.logp_old, dd.adv, dd.ret, out)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())
    return out


def _compare(label, names_slices, got, ref64, ref32):
    """the bound of the module docstring on every (name, slice); prints every figure, then asserts"""
    bad = []
    for name, sl in names_slices:
        a, b, c = got[sl].double().cpu(), ref64[sl].double().cpu(), ref32[sl].double().cpu()
        scale = float(b.abs().max())
        assert scale > 0 and math.isfinite(scale), (label, name, scale)
        err, err32 = float((a - b).abs().max()) / scale, float((c - b).abs().max()) / scale
        how = "2e-4" if err <= BOUND else ("4xerr32" if err <= FACTOR32 * err32 else "FAIL")
        print(f"FP64CHK {label:<44s} {name:<8s} err {err:.2e} err32 {err32:.2e} {how}")
        if how == "FAIL":
            bad.append((name, err, err32))
    assert not bad, (label, bad)


def _grad_case(monkeypatch, samples, spec, squash, mb, B=None, max_minibatch=None, regime="plain", norm=True, clamp=False, ent=True,
               repeat=False, seed=0, label=""):
    """one shape / regime: preconditions on the reference, then every parameter tensor of mm_ppo_grad against fp64; returns the
    kernel's gradients (one per launch)"""
    monkeypatch.setenv("MYOSIM_PPO_SAMPLES", str(samples))
    B = B or max(mb + 13, 48)
    d = make_data(spec, squash, B, regime, norm, clamp, ent, seed)
    if mb >= 3:
        idxs = [make_idx(B, mb, seed, repeat)]
    else:       # too few rows for the three clip branches in one launch: one launch per branch
        assert mb == 1
        with torch.no_grad():
            x = normalise(d.obs, d.om, d.os)
            mean, std, _ = policy_dist(spec, d.p, x)
            ratio = torch.exp(log_density(mean, std, d.raw, squash) - d.logp_old)
        nz = d.adv != 0
        pick = lambda m: torch.nonzero(m & nz)[:1, 0]
        idxs = [pick(ratio > 1 + EPS_CLIP), pick(ratio < 1 - EPS_CLIP), pick((ratio - 1).abs() < EPS_CLIP)]
        assert all(i.numel() == 1 for i in idxs)
    if repeat:
        assert idxs[0].unique().numel() < idxs[0].numel()
    assert_preconditions(d, idxs, regime, clamp)
    K = _handle(spec, squash, max_minibatch or max(mb, 1))
    dd = DevData(d)
    K.set_entropy_noise(dd.enoise)
    slices = [(name, slice(o, o + (w * k if k else w))) for name, o, w, k in spec.tensors]
    outs = []
    for n, idx in enumerate(idxs):
        g64, _ = reference_grad(d, idx)
        assert bool(torch.isfinite(g64).all())
        g32, _ = reference_grad(d, idx, torch.float32, "cuda")
        got = _kernel_grad(K, dd, idx)
        _compare(f"grad {label} S{samples} #{n}", slices, got, g64, g32)
        outs.append(got)
    return outs


W24 = (24,) * 7          # eight linear layers with the output layer
GRAD_CASES = {   # name: Spec arguments, squash, keyword arguments of _grad_case
    "h20x33-v7-obs17-act5-mb33": ((17, 5, (20, 33), (7,)), "tanh", dict(mb=33, repeat=True)),
    "h100-obs403-act17-mb31": ((403, 17, (100,), (100,)), "sigmoid", dict(mb=31, repeat=True)),
    "nohidden-obs15-act16-mb17": ((15, 16, (), ()), "tanh", dict(mb=17)),
    "nohidden-nonorm-obs15-act16-mb17": ((15, 16, (), ()), "sigmoid", dict(mb=17, norm=False, ent=False)),
    "8layers-obs3-act1-mb15": ((3, 1, W24, W24), "sigmoid", dict(mb=15)),
    "h128x3-obs512-act80-mb16": ((512, 80, (128, 128, 128), (128, 128, 128)), "tanh", dict(mb=16)),
    "obs1-act128-mb1": ((1, 128, (64,), (16,)), "tanh", dict(mb=1, B=48)),
    "h33-v7-obs9-act3-mb81-of-81": ((9, 3, (33,), (7,)), "sigmoid", dict(mb=81, max_minibatch=81, B=96, repeat=True, ent=False)),
    "wide_o-clamp-tanh": ((17, 5, (20, 33), (7,)), "tanh", dict(mb=49, B=64, regime="wide_o", clamp=True, repeat=True)),
    "wide_o-sigmoid": ((40, 17, (64, 64), (64,)), "sigmoid", dict(mb=64, B=80, regime="wide_o", ent=False)),
    "wide_o-sigmoid-entropy": ((12, 6, (32,), (32,)), "sigmoid", dict(mb=47, B=64, regime="wide_o")),
    "big_raw-tanh-clamp": ((33, 7, (48, 20), (33,)), "tanh", dict(mb=40, B=64, regime="big_raw", clamp=True)),
    "big_raw-sigmoid": ((33, 7, (48, 20), (33,)), "sigmoid", dict(mb=40, B=64, regime="big_raw", repeat=True)),
}


@pytest.mark.gpu
@pytest.mark.parametrize("samples", [16, 32])
@pytest.mark.parametrize("name", list(GRAD_CASES))
def test_grad_matches_fp64_per_parameter_tensor(monkeypatch, name, samples):
    sp, squash, kw = GRAD_CASES[name]
    _grad_case(monkeypatch, samples, Spec(*sp), squash, seed=list(GRAD_CASES).index(name), label=name, **kw)


LDS_LIMIT = 150 * 1024


def plan_bytes(spec, S=16):
    """dynamic LDS of a workgroup of S samples: plan() of myosim_ppo.hip (every row stride = width rounded up to 16, + 4 floats)"""
    r16 = lambda x: (x + 15) & ~15

    def net(widths, aux):
        maxh = max([16] + [r16(w) for w in widths[:-1]])
        per = r16(spec.obs_dim) + 4 + sum(2 * (r16(w) + 4) for w in widths[:-1]) + r16(widths[-1]) + 4 + 2 * (maxh + 4) + aux
        return 4 * S * per
    return max(net(spec.pw, 2 * spec.act_dim), net(spec.vw, 0))


@pytest.mark.gpu
def test_32_samples_requested_falls_back_to_16_when_the_plan_does_not_fit(monkeypatch):
    sp, squash, kw = GRAD_CASES["h128x3-obs512-act80-mb16"]
    spec = Spec(*sp)
    assert plan_bytes(spec, 16) <= LDS_LIMIT < plan_bytes(spec, 32)
    kw = dict(kw, mb=45, B=64, repeat=True)
    a = _grad_case(monkeypatch, 16, spec, squash, seed=50, label="lds-fallback", **kw)
    b = _grad_case(monkeypatch, 32, spec, squash, seed=50, label="lds-fallback", **kw)
    assert torch.equal(a[0], b[0])


def _lds_family():
    """policies around the LDS limit: obs 512, four hidden layers of 128 and a fifth of w, act_dim near 128"""
    out = []
    for ad in range(112, 129):
        for w in (1, 16, 17, 32, 33, 48, 64):
            spec = Spec(512, ad, (128, 128, 128, 128, w), (16,))
            out.append((plan_bytes(spec), spec))
    return sorted(out, key=lambda t: t[0])


@pytest.mark.gpu
def test_lds_limit_refusal_and_the_largest_plan_under_it(monkeypatch):
    from myosuite_amd import engine as E
    fam = _lds_family()
    over = [t for t in fam if t[0] > LDS_LIMIT][0]
    under = [t for t in fam if t[0] <= LDS_LIMIT][-1]
    assert 0 < over[0] - LDS_LIMIT <= 1024 and 0 <= LDS_LIMIT - under[0] <= 1024, (over[0], under[0])
    with pytest.raises(E.EngineError, match=rf"rc=-?\d+\): mm_ppo_create: a 16-sample workgroup needs {over[0]} B of LDS"):
        _handle(over[1], "tanh", 32)
    _grad_case(monkeypatch, 16, under[1], "tanh", mb=20, seed=60, label=f"lds-{under[0]}B")


@pytest.mark.gpu
def test_two_live_handles_do_not_disturb_each_other(monkeypatch):
    monkeypatch.setenv("MYOSIM_PPO_SAMPLES", "16")
    big, small = Spec(512, 80, (128, 128, 128), (128, 128, 128)), Spec(3, 1, (16,), (16,))
    d = make_data(big, "tanh", 48, seed=70)
    idx = make_idx(48, 33, 70, True)
    dd = DevData(d)

    def run(K):
        K.set_entropy_noise(dd.enoise)
        return _kernel_grad(K, dd, idx)
    K0 = _handle(big, "tanh", 33)
    alone = run(K0)
    del K0
    Kb = _handle(big, "tanh", 33)
    Ks = _handle(small, "tanh", 33)
    ds = make_data(small, "tanh", 48, seed=71)
    dds = DevData(ds)
    Ks.set_entropy_noise(dds.enoise)
    _kernel_grad(Ks, dds, idx)
    both = run(Kb)
    del Ks
    after = run(Kb)
    assert torch.equal(alone, both) and torch.equal(alone, after)


# mm_ppo_act -------------------------------------------------------------------------------------------------------------------------
ACT_CASES = {   # name: Spec arguments, squash, nenv, make_data keywords
    "h20x33-obs17-act5-n33": ((17, 5, (20, 33), (7,)), "tanh", 33, dict()),
    "h100-obs403-act17-n17": ((403, 17, (100,), (100,)), "sigmoid", 17, dict()),
    "nohidden-obs15-act16-n16": ((15, 16, (), ()), "tanh", 16, dict(norm=False)),
    "8layers-obs3-act1-n15": ((3, 1, W24, W24), "sigmoid", 15, dict()),
    "h128x3-obs512-act80-n1000": ((512, 80, (128, 128, 128), (128, 128, 128)), "tanh", 1000, dict()),
    "obs1-act128-n1": ((1, 128, (64,), (16,)), "tanh", 1, dict()),
    "wide_o-clamp-tanh-n1000": ((17, 5, (20, 33), (7,)), "tanh", 1000, dict(regime="wide_o", clamp=True)),
    "wide_o-sigmoid-n33": ((40, 17, (64, 64), (64,)), "sigmoid", 33, dict(regime="wide_o")),
    "big_raw-tanh-clamp-n17": ((33, 7, (48, 20), (33,)), "tanh", 17, dict(regime="big_raw", clamp=True)),
    "big_raw-sigmoid-n15": ((33, 7, (48, 20), (33,)), "sigmoid", 15, dict(regime="big_raw")),
}


def _act_reference(d, dtype=F64, device="cpu"):
    c = lambda t: None if t is None else t.to(device=device, dtype=dtype)
    with torch.no_grad():
        x = normalise(c(d.obs), c(d.om), c(d.os))
        mean, std, o = policy_dist(d.spec, c(d.p), x)
        raw = mean + std * c(d.e)
        return dict(raw=raw, action=squash_fn(raw, d.squash), logp=log_density(mean, std, raw, d.squash),
                    value=mlp(d.spec.layers(c(d.p), "vf"), x)[:, 0], o=o, x=x)


@pytest.mark.gpu
@pytest.mark.parametrize("samples", [16, 32])
@pytest.mark.parametrize("name", list(ACT_CASES))
def test_act_matches_fp64(monkeypatch, name, samples):
    monkeypatch.setenv("MYOSIM_PPO_SAMPLES", str(samples))
    sp, squash, n, kw = ACT_CASES[name]
    spec = Spec(*sp)
    regime, clamp = kw.get("regime", "plain"), kw.get("clamp", False)
    d = make_data(spec, squash, n, seed=200 + list(ACT_CASES).index(name), **kw)
    r64, r32 = _act_reference(d), _act_reference(d, torch.float32, "cuda")
    for v in r64.values():
        assert bool(torch.isfinite(v).all())
    if regime == "wide_o":
        o = r64["o"]
        assert float(o.min()) < -20.0 and float(o.max()) > 20.0 and bool(((o > 0) & (o < 20)).any()) and bool((softplus(o) < 1e-4).any())
    if regime == "big_raw":
        assert 10.0 <= float(r64["raw"].abs().max()) <= 16.0
    if clamp:
        assert float((r64["x"] == -5.0).double().mean()) >= 0.10 and float((r64["x"] == 5.0).double().mean()) >= 0.10
    K = _handle(spec, squash, 16)
    dd = DevData(d)
    pad, SENT = 5, -77.0
    mk = lambda *s: torch.full(s, SENT, device="cuda")
    od, ad = spec.obs_dim, spec.act_dim
    obs_in = torch.cat([dd.obs, mk(pad, od)])                       # the input rows past nenv are not to be read into the outputs either
    noise = torch.cat([dd.e, mk(pad, ad)])
    o_obs, o_raw, o_lp, o_v, o_act = mk(n + pad, od), mk(n + pad, ad), mk(n + pad), mk(n + pad), mk(n + pad, ad)

    def act(obs_out, raw, lp, v, action):
        # the binding takes the row count from obs: hand it views of the first n rows of the over-allocated buffers
        f = lambda t: None if t is None else t[:n]
        K.act(dd.p, obs_in[:n], dd.om, dd.os, noise[:n], f(obs_out), f(raw), f(lp), f(v), f(action))
        torch.cuda.synchronize()
    act(o_obs, o_raw, o_lp, o_v, o_act)
    for t in (o_obs, o_raw, o_lp, o_v, o_act):
        assert bool((t[n:] == SENT).all()), "rows >= nenv were written"
    assert torch.equal(o_obs[:n], dd.obs)
    got = dict(raw=o_raw[:n], action=o_act[:n], logp=o_lp[:n], value=o_v[:n])
    full = slice(None)
    for k in ("raw", "action", "logp", "value"):
        assert bool(torch.isfinite(got[k]).all())
        _compare(f"act {name} S{samples}", [(k, full)], got[k].reshape(-1), r64[k].reshape(-1), r32[k].reshape(-1))
    # no observation copy requested
    r2, l2, v2, a2 = mk(n + pad, ad), mk(n + pad), mk(n + pad), mk(n + pad, ad)
    act(None, r2, l2, v2, a2)
    assert torch.equal(r2, o_raw) and torch.equal(l2, o_lp) and torch.equal(v2, o_v) and torch.equal(a2, o_act)
    # value network only
    v3 = mk(n + pad)
    act(None, None, None, v3, None)
    assert torch.equal(v3, o_v)


# mm_ppo_adam ------------------------------------------------------------------------------------------------------------------------
ADAM_SPEC = (9, 3, (33,), (7,))          # 612 parameters: not a multiple of 64 or 256
LR = 3e-3


def _adam_grads(P, steps, seed=0):
    g = torch.Generator().manual_seed(seed)
    scale = torch.tensor([10.0 ** (k % 5 - 3) for k in range(steps)], dtype=F64)         # 1e-3 ... 1e1: the clip is sometimes active
    return f32(torch.randn(steps, P, generator=g, dtype=F64) * scale[:, None])


@pytest.mark.gpu
@pytest.mark.parametrize("max_norm,gscale", [(None, 1.0), (0.5, 1.0), (0.5, 0.5)], ids=["noclip", "clip0.5", "clip0.5-scale0.5"])
def test_adam_2000_steps_against_fp64(max_norm, gscale):
    """drift of mm_ppo_adam from fp64 Adam over 2000 steps <= 4 x the drift of torch.optim.Adam in fp32 on the same gradients.
    Measured on an MI355X (max |p - p64|, kernel / torch fp32): no clip 9.38e-06 / 9.15e-06, clip 0.5 7.07e-06 / 5.58e-06,
    clip 0.5 with grad_scale 0.5 6.34e-06 / 6.11e-06."""
    spec = Spec(*ADAM_SPEC)
    assert spec.param_count % 64 and spec.param_count % 256
    steps, P = 2000, spec.param_count
    G = _adam_grads(P, steps)
    g = torch.Generator().manual_seed(5)
    p0 = f32(torch.randn(P, generator=g, dtype=F64))
    norms = (G * gscale).norm(dim=1)
    if max_norm:
        assert bool((norms > max_norm).any()) and bool((norms < max_norm).any())
    p64 = adam_reference(p0, G, LR, 0.9, 0.999, 1e-8, max_norm, gscale)
    assert bool(torch.isfinite(p64).all()) and float((p64 - p0).abs().max()) > 100 * LR
    K = _handle(spec, "tanh", 16, learning_rate=LR, max_grad_norm=max_norm)
    Gd = G.float().cuda()
    p = p0.float().cuda()
    ref = p0.float().cuda().requires_grad_(True)
    opt = torch.optim.Adam([ref], lr=LR)
    for k in range(steps):
        K.adam(p, Gd[k], gscale, recompute_norm=True)
        ref.grad = Gd[k] * gscale
        if max_norm:
            torch.nn.utils.clip_grad_norm_([ref], max_norm)
        opt.step()
    torch.cuda.synchronize()
    drift, drift32 = float((p.double().cpu() - p64).abs().max()), float((ref.detach().double().cpu() - p64).abs().max())
    print(f"FP64CHK adam max_norm {max_norm} gscale {gscale}: drift {drift:.3e} torch-fp32 drift {drift32:.3e}")
    assert drift32 > 0 and drift <= FACTOR32 * drift32, (drift, drift32)
    # after a reset the first step is lr in magnitude (bias correction of step 1; eps / |g| < 1e-4 here)
    K.reset_optimizer()
    q = torch.zeros(P, device="cuda")
    gk = Gd[4]
    K.adam(q, gk, gscale, recompute_norm=True)
    torch.cuda.synchronize()
    big = gk.abs() > 1.0                        # clipped and scaled they stay above 1e-3: eps / |g| <= 1e-5
    assert int(big.sum()) > P // 2
    assert float(((q.abs() - LR).abs())[big].max()) < 1e-4 * LR


@pytest.mark.gpu
def test_adam_zero_gradient_leaves_parameters_unchanged():
    spec = Spec(*ADAM_SPEC)
    K = _handle(spec, "tanh", 16, learning_rate=LR, max_grad_norm=0.5)
    p0 = torch.randn(spec.param_count, device="cuda")
    p, z = p0.clone(), torch.zeros(spec.param_count, device="cuda")
    for rn in (True, False, True):
        K.adam(p, z, 1.0, recompute_norm=rn)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(p).all()) and torch.equal(p, p0)


@pytest.mark.gpu
def test_adam_graph_replay_equals_eager_launches_bit_for_bit():
    """ten captured mm_ppo_adam launches replayed twice = twenty eager launches: the step counter lives on the device"""
    spec = Spec(*ADAM_SPEC)
    P = spec.param_count
    Gd = _adam_grads(P, 10, seed=9).float().cuda()
    p0 = torch.randn(P, device="cuda")
    K = _handle(spec, "tanh", 16, learning_rate=LR, max_grad_norm=0.5)
    eager = p0.clone()
    for k in range(20):
        K.adam(eager, Gd[k % 10], 1.0, recompute_norm=True)
    torch.cuda.synchronize()
    K.reset_optimizer()
    p = p0.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for k in range(10):
            K.adam(p, Gd[k], 1.0, recompute_norm=True)
    torch.cuda.synchronize()
    assert torch.equal(p, p0), "capture must not run the launches"
    graph.replay(); graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(p, eager)
    assert float((p - p0).abs().max()) > 10 * LR


# mm_ppo_store and the refusals ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("nenv", [1, 255, 257])
@pytest.mark.parametrize("with_trunc", [True, False], ids=["truncated", "truncated-None"])
def test_store_is_exact(nenv, with_trunc):
    K = _handle(Spec(3, 1, (16,), (16,)), "tanh", 16)
    rng = np.random.default_rng(nenv)
    cols, col, scale = 7, 3, np.float32(0.37)
    rwd = rng.standard_normal((nenv, cols)).astype(np.float32)
    combos = np.array([(0, 0), (0, 1), (1, 0), (1, 1)], dtype=np.uint8)                   # (ended, truncated): all four
    et = combos[(np.arange(nenv) + nenv) % 4]
    ended, trunc = et[:, 0].copy(), et[:, 1].copy()
    if nenv >= 4:
        assert len({tuple(r) for r in et}) == 4
    t = trunc if with_trunc else np.zeros_like(trunc)
    want = ((rwd[:, col] * scale).astype(np.float32), (t & ended).astype(np.float32), (ended & (1 - t)).astype(np.float32))
    pad, SENT = 3, -77.0
    outs = [torch.full((nenv + pad,), SENT, device="cuda") for _ in range(3)]
    K.store(torch.from_numpy(rwd).cuda(), col, float(scale), torch.from_numpy(ended).cuda(), torch.from_numpy(trunc).cuda() if with_trunc else None,
            *[o[:nenv] for o in outs])
    torch.cuda.synchronize()
    for o, w in zip(outs, want):
        assert np.array_equal(o[:nenv].cpu().numpy(), w) and bool((o[nenv:] == SENT).all())


@pytest.mark.gpu
def test_refusals_are_error_returns():
    from myosuite_amd import engine as E
    spec = Spec(9, 3, (33,), (7,))
    K = _handle(spec, "tanh", 20)
    d = make_data(spec, "tanh", 48, seed=90)
    dd = DevData(d)
    out = torch.full((K.param_count,), 7.0, device="cuda")
    idx = torch.arange(21, device="cuda")
    with pytest.raises(E.EngineError, match="minibatch of 21 rows, workspace sized for 20"):
        K.grad(dd.p, dd.obs, dd.om, dd.os, idx, dd.raw, dd.logp_old, dd.adv, dd.ret, out)
    L = E.lib()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    rc = L.mm_ppo_grad(K.h, ptr(dd.p), ptr(dd.obs), ptr(dd.om), ptr(dd.os), ptr(idx), 0, ptr(dd.raw), ptr(dd.logp_old), ptr(dd.adv), ptr(dd.ret),
                       ptr(out), None)
    assert rc != 0 and b"minibatch of 0 rows" in L.mm_ppo_last_error()
    with pytest.raises(E.EngineError, match="mm_ppo_grad"):
        K.grad(dd.p, dd.obs, dd.om, None, idx[:8], dd.raw, dd.logp_old, dd.adv, dd.ret, out)            # obs_mean without obs_std
    v = torch.full((48,), 7.0, device="cuda")
    with pytest.raises(E.EngineError, match="mm_ppo_act"):
        K.act(dd.p, dd.obs, dd.om, None, None, None, None, None, v, None)
    rc = L.mm_ppo_act(K.h, ptr(dd.p), ptr(dd.obs), None, None, None, 48, None, None, None, ptr(v), ptr(dd.raw), None)   # action without noise
    assert rc != 0 and b"required with action_out" in L.mm_ppo_last_error()
    rc = L.mm_ppo_act(K.h, ptr(dd.p), ptr(dd.obs), None, None, None, 0, None, None, None, ptr(v), None, None)
    assert rc != 0
    rwd, ended = torch.zeros(8, 4, device="cuda"), torch.zeros(8, dtype=torch.uint8, device="cuda")
    o = [torch.full((8,), 7.0, device="cuda") for _ in range(3)]
    for col in (4, -1):
        with pytest.raises(E.EngineError, match="mm_ppo_store"):
            K.store(rwd, col, 1.0, ended, None, *o)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((v == 7.0).all()) and all(bool((t == 7.0).all()) for t in o), "a refused call launched something"
    with pytest.raises(E.EngineError, match="the policy's last layer|layers"):
        E.FusedPPO(9, 3, (8,) * 8, (7,), "tanh", max_minibatch=8, learning_rate=LR, clipping_epsilon=0.2, entropy_cost=0.0, value_cost=0.5,
                   max_grad_norm=None)
