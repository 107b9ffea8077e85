"""The update rules of ``optim.FusedLARS`` and ``optim.FusedLAMB`` restated in fp64 on CPU tensors, and the cases the host and
device tests share.  Plain module: no fixtures, no device.

LARS    r   = trust_coefficient |p| / (|g| + weight_decay |p| + eps)    if adapt and |p| > 0 and |g| > 0, else 1
        d   = r (g + weight_decay p);  buf = d on the first step taken, else momentum buf + (1 - dampening) d
        p  <- p - lr (d + momentum buf if nesterov else buf)
LAMB    m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;  t = steps taken + 1
        u = (m / (1 - b1^t)) / (sqrt(v / (1 - b2^t)) + eps) + weight_decay p
        r = |p| / |u|  if adapt and |p| > 0 and |u| > 0, else 1;  r = min(r, trust_clip) when trust_clip is set
        p <- p - lr r u
``g`` is the gradient in memory times ``coef`` (1 / scale and the clip coefficient), negated by ``maximize``; the norms are
2-norms over one tensor."""
import functools

import torch

CHUNK = 4096
BAR = 2e-6                      # parameters: BAR * max|ref| (tests/test_optim_decay_clip_gpu.py:23); ratios: BAR, relative
STEPS = 5
# chunk edges; 300 chunks + 5 elements is more chunks than the finalize has lanes
SIZES = [1, 3, 255, 4095, 4096, 4097, 8193, 3 * 4096, 300 * 4096 + 5]
ZERO_PARAM, ZERO_GRAD = 2, 3    # the 255-element tensor starts as zeros; the 4095-element one gets a zero gradient in step 1

LARS_HP = dict(lr=0.5, momentum=0.9, dampening=0.0, nesterov=False, weight_decay=1e-4, trust_coefficient=0.02, eps=1e-8)
LAMB_HP = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, trust_clip=None)


# ---- the rules ---------------------------------------------------------------------------------------------------------------
def lars_step(p, g, buf, hp, first, adapt=True, coef=1.0):
    """One LARS step of one tensor in the dtype of its operands: returns (p, buf, (|p|, |g|, r)); ``buf`` is None with momentum 0."""
    g = g * coef
    if hp.get("maximize", False):
        g = -g
    wd = hp["weight_decay"]
    pn, gn = p.norm().item(), g.norm().item()
    r = hp["trust_coefficient"] * pn / (gn + wd * pn + hp["eps"]) if adapt and pn > 0 and gn > 0 else 1.0
    d = r * (g + wd * p)
    momentum = hp["momentum"]
    if momentum != 0:
        buf = d.clone() if first else momentum * buf + (1 - hp["dampening"]) * d
        d = d + momentum * buf if hp["nesterov"] else buf
    return p - hp["lr"] * d, buf, (pn, gn, r)


def lamb_step(p, g, m, v, t, hp, adapt=True, coef=1.0):
    """One LAMB step of one tensor: returns (p, m, v, (|p|, |u|, r)); ``t`` counts from 1."""
    g = g * coef
    b1, b2 = hp["betas"]
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    u = (m / (1 - b1 ** t)) / ((v / (1 - b2 ** t)).sqrt() + hp["eps"]) + hp["weight_decay"] * p
    pn, un = p.norm().item(), u.norm().item()
    r = pn / un if adapt and pn > 0 and un > 0 else 1.0
    if hp.get("trust_clip") is not None:
        r = min(r, hp["trust_clip"])
    return p - hp["lr"] * r * u, m, v, (pn, un, r)


def run(kind, params, grads, groups, skipped=(), coefs=None, dtype=torch.float64):
    """The rule over ``len(grads)`` steps.  ``groups``: [(indices, hyper-parameters with ``adapt``)]; ``skipped``: steps the scaler
    skips (nothing changes, the next taken step is the first); ``coefs``: one factor on the gradients per step.  Returns one entry
    per step: (parameters, records in the order of the groups, states) -- states are (buf,) or (m, v) per tensor."""
    p = [x.to(dtype) for x in params]
    state = [None] * len(p)
    taken, out = 0, []
    records = {i: (float("nan"),) * 3 for i in range(len(p))}
    for step, gs in enumerate(grads):
        if step not in skipped:
            coef = 1.0 if coefs is None else coefs[step]
            for indices, hp in groups:
                for i in indices:
                    g = gs[i].to(dtype)
                    if kind == "lars":
                        p[i], buf, records[i] = lars_step(p[i], g, state[i] and state[i][0], hp, taken == 0, hp.get("adapt", True), coef)
                        state[i] = (buf,)
                    else:
                        m, v = state[i] or (torch.zeros_like(p[i]), torch.zeros_like(p[i]))
                        p[i], m, v, records[i] = lamb_step(p[i], g, m, v, taken + 1, hp, hp.get("adapt", True), coef)
                        state[i] = (m, v)
            taken += 1
        out.append(([x.clone() for x in p], [records[i] for indices, _ in groups for i in indices], list(state)))
    return out


# ---- the cases ---------------------------------------------------------------------------------------------------------------
def _hp(kind, **extra):
    return dict(LARS_HP if kind == "lars" else LAMB_HP, **extra)


@functools.lru_cache(maxsize=None)
def sizes_case():
    """(parameters, gradients per step) in fp32: p = 0.05 randn, g = 0.01 randn, fixed seeds.  One group."""
    gen = torch.Generator().manual_seed(20240521)
    ps = [0.05 * torch.randn(n, generator=gen) for n in SIZES]
    ps[ZERO_PARAM].zero_()
    grads = [[0.01 * torch.randn(n, generator=gen) for n in SIZES] for _ in range(STEPS)]
    grads[0][ZERO_GRAD].zero_()
    return ps, grads


def sizes_groups(kind):
    return [(list(range(len(SIZES))), _hp(kind, adapt=True))]


MANY, MANY_ADAPT = 70, 40        # 70 tensors of 5 elements, |p_i| = i + 1; the last 30 form the group with adapt=False


@functools.lru_cache(maxsize=None)
def many_case():
    gen = torch.Generator().manual_seed(20240522)
    ps = []
    for i in range(MANY):
        x = torch.randn(5, generator=gen, dtype=torch.float64)
        ps.append((x * ((i + 1) / x.norm())).float())
    grads = [[0.01 * torch.randn(5, generator=gen) for _ in range(MANY)] for _ in range(STEPS)]
    return ps, grads


def many_groups(kind):
    return [(list(range(MANY_ADAPT)), _hp(kind, adapt=True)), (list(range(MANY_ADAPT, MANY)), _hp(kind, adapt=False))]


CASES = {"sizes": (sizes_case, sizes_groups), "many": (many_case, many_groups)}


@functools.lru_cache(maxsize=None)
def reference(kind, case):
    """The fp64 run of a case, computed once and shared (treat it as read-only)."""
    make, groups = CASES[case]
    ps, grads = make()
    return run(kind, ps, grads, groups(kind))


# every intermediate a power of two: the bits must equal the fp64 result, whatever the order of the sums
EXACT_SIZES = (4096, 16384)
EXACT_LARS = dict(lr=0.5, momentum=0.5, dampening=0.0, nesterov=False, weight_decay=0.0, trust_coefficient=2.0 ** -10, eps=0.0)
EXACT_LAMB = dict(lr=2.0 ** -3, betas=(0.5, 0.5), eps=0.0, weight_decay=0.0, trust_clip=None)
EXACT_AFTER = {"lars": 2.0 - 2.0 ** -10, "lamb": 1.75}


def exact_case(n):
    return [torch.full((n,), 2.0)], [[torch.ones(n)]]


def exact_groups(kind):
    return [([0], dict(EXACT_LARS if kind == "lars" else EXACT_LAMB, adapt=True))]
