"""Float64 references, error bounds and seeded input families for the encoder kernels -- TEST INFRASTRUCTURE ONLY.

The kernels: K8 ``hr_add_layernorm`` and K7 ``hr_pool_normalize`` / ``_packed`` (csrc/hr_pool.hip),
``hr_attn_varlen`` and ``hr_gelu_erf`` (csrc/hr_attn.hip).  Every reference runs on the CPU in float64 from the very
values the kernel reads (the 16-bit tensors widened), and returns, besides the result, the per-element quantities its
bound ``|kernel - reference| <= E`` is made of.  ``u = 2^-24`` is fp32's unit roundoff, ``u_dt`` that of the tensor type.
The ``*_emul`` functions restate each kernel's arithmetic in fp32 on the CPU (same rounding points, torch's summation
order): tests/test_enc_ref_cpu.py holds them to the same bounds, which shows that the bounds are not satisfied by the
float64 reference alone but leave room for an fp32 evaluation; tests/test_gpu_encoder_kernels.py holds the kernels to
them.
"""
from __future__ import annotations

import math

import numpy as np
import torch

U32 = 2.0 ** -24
TD = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
U_DT = {"f32": 2.0 ** -24, "bf16": 2.0 ** -8, "f16": 2.0 ** -11}

# ---------------------------------------------------------------- K8: add + LayerNorm
# The constant of the fp32 terms of the K8 bound, from the kernels' operation count (errors in units of u, first order):
#   mean:  a lane adds its N C values one after the other (at most 32: the (8,4) / (4,8) instantiations; 16 in the
#          generic kernel), then 6 shuffle steps (the generic kernel: + 2 adds over the four waves), then one division:
#          at most 31 + 6 + 1 = 38 roundings along the longest chain, 15 + 8 + 1 = 24 in the generic kernel at H = 4096.  A
#          rounding of a partial sum is at most u times that partial sum, and a lane's partial sums grow from one
#          element to the lane's share, so the chain's weight is reached only when each lane's mass sits in the element
#          it loads first: over the row the error is <= 38 u mean|v| a priori and about (16 + 6 + 1) u mean|v| for
#          rows whose magnitude is spread over the lanes' elements.
#   rstd:  d = v - mean (1), d * d + q fused (1 per term), the same tree, / H, + eps, rsqrtf (<= 2 ulp = 4 u): the sum
#          has positive terms only, so its (1 + 31 + 6 + 2) u is a relative error and rsqrt halves it: <= 24 u relative.
#   y:     (v - mean) (1), * rstd (1), * g fused with + b (1 on the result): 3 u (|g| |v - mu| rstd + |b|).
# c = 32 bounds the rstd + y chain (24 + 3) with room and the mean chain for every row whose magnitude is not
# concentrated in the lanes' first elements; the tensor type's rounding of y is the separate term u_dt |ref|.
K8_C = 32.0


def layernorm_ref(x, r, g, b, eps, dtype):
    """LayerNorm(x + r) * g + b as K8 defines it: the sum rounded to the tensor type (IEEE fp32 add, one rounding to
    ``dtype`` -- the kernel's round_to, bit for bit), everything after in float64.  Returns a dict: ``ref`` (rows, H)
    float64, ``v`` (the rounded sums), ``mu``, ``rstd`` (rows, 1) and ``mean_abs_v`` (rows, 1)."""
    td = TD[dtype]
    v = (x.float() + r.float()).to(td).double()
    mu = v.mean(-1, keepdim=True)
    var = ((v - mu) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + float(eps))
    ref = (v - mu) * rstd * g.double() + b.double()
    return {"ref": ref, "v": v, "mu": mu, "rstd": rstd, "mean_abs_v": v.abs().mean(-1, keepdim=True)}


def layernorm_bound(R, g, b, dtype):
    """E = u_dt |ref| + |g| rstd (c u mean|v|) + c u (|g| |v - mu| rstd + |b|), per element."""
    ga, ba = g.double().abs(), b.double().abs()
    return (U_DT[dtype] * R["ref"].abs() + ga * R["rstd"] * (K8_C * U32 * R["mean_abs_v"])
            + K8_C * U32 * (ga * (R["v"] - R["mu"]).abs() * R["rstd"] + ba))


def layernorm_emul(x, r, g, b, eps, dtype):
    """K8's arithmetic in fp32 on the CPU (torch's summation order)."""
    td = TD[dtype]
    H = x.shape[-1]
    v = (x.float() + r.float()).to(td).float()
    mean = v.sum(-1, keepdim=True) / float(H)
    d = v - mean
    rstd = torch.rsqrt((d * d).sum(-1, keepdim=True) / float(H) + torch.tensor(eps, dtype=torch.float32))
    return (d * rstd * g.float() + b.float()).to(td)


LN_FAMILIES = ("gauss", "offset", "outlier", "nearconst", "const_exact")


def ln_inputs(family, rows, H, dtype, seed=0):
    """(x, r, g, b) CPU tensors of ``dtype`` for one family (g ~ 1 + 0.1 N, b ~ 0.1 N, as a trained LayerNorm's):
    gauss x ~ 3 N, r ~ N (the inputs of the older test); offset row mean 1000 with unit spread; outlier one feature
    column at 1e4, the rest N(0, 3); nearconst 0.3 +- 1e-3; const_exact x = r = 0.25 (every partial sum exact)."""
    gen = torch.Generator().manual_seed(1000003 * LN_FAMILIES.index(family) + 7919 * H + 31 * rows + seed)
    rn = lambda *s: torch.randn(s, generator=gen)
    if family == "gauss":
        x, r = rn(rows, H) * 3, rn(rows, H)
    elif family == "offset":
        x, r = 1000.0 + rn(rows, H), rn(rows, H) * 0.01
    elif family == "outlier":
        x, r = rn(rows, H) * 3, rn(rows, H)
        x[:, H // 3] = 1e4
    elif family == "nearconst":
        x, r = 0.3 + 1e-3 * (2 * torch.rand((rows, H), generator=gen) - 1), 0.3 + 1e-3 * (2 * torch.rand((rows, H), generator=gen) - 1)
    elif family == "const_exact":
        x, r = torch.full((rows, H), 0.25), torch.full((rows, H), 0.25)
    else:
        raise ValueError(family)
    g = 1 + 0.1 * rn(H)
    b = 0.1 * rn(H)
    td = TD[dtype]
    return x.to(td), r.to(td), g.to(td), b.to(td)


# ---------------------------------------------------------------- K7: masked mean-pool + normalize
def pool_ref(hidden, mask, n_instr):
    """Masked mean over the sequence with the first n_instr positions masked out, then x / max(||x||, 1e-12), in
    float64.  hidden (B, T, H), mask (B, T) of 0 / 1.  Returns a dict: ``ref`` (B, H; NaN rows where every token is
    masked), ``a`` = sum_t |x| m / d (B, H), ``norm`` = ||mean|| (B, 1), ``kept`` = d (B,)."""
    x = hidden.double()
    m = mask.double().clone()
    m[:, :n_instr] = 0
    d = m.sum(1)
    mean = (x * m[:, :, None]).sum(1) / d[:, None]
    a = (x.abs() * m[:, :, None]).sum(1) / d[:, None]
    norm = mean.norm(dim=-1, keepdim=True)
    return {"ref": mean / norm.clamp_min(1e-12), "a": a, "norm": norm, "kept": d}


def pool_bound(R, T):
    """(T u a_h + |ref_h| T u ||a||) / ||mean|| + 8 u: the T-term fp32 sum of a column (T - 1 adds and the division)
    moves the mean by at most T u a_h, hence the norm by at most T u ||a||; 8 u covers the sum of squares, the square
    root, the reciprocal and the final product on a unit vector's elements."""
    an = R["a"].norm(dim=-1, keepdim=True)
    return (T * U32 * R["a"] + R["ref"].abs() * T * U32 * an) / R["norm"] + 8 * U32


def pool_emul(hidden, mask, n_instr):
    x = hidden.float()
    m = mask.float().clone()
    m[:, :n_instr] = 0
    mean = (x * m[:, :, None]).sum(1) / m.sum(1)[:, None]
    n = torch.sqrt((mean * mean).sum(-1, keepdim=True))
    return mean * (1.0 / n.clamp_min(1e-12))


POOL_FAMILIES = ("gauss", "offset", "outlier", "nearconst")


def pool_hidden(family, B, T, H, dtype, seed=0):
    """Hidden states of one family; ``cancel`` (token pairs +a, -a at positions 2i, 2i + 1: the mean is exactly 0) has
    no bound (||mean|| = 0) and is checked for exact zeros."""
    gen = torch.Generator().manual_seed(99991 * (1 + (POOL_FAMILIES + ("cancel",)).index(family)) + 131 * B + 17 * T + H + seed)
    x = torch.randn((B, T, H), generator=gen)
    if family == "offset":
        x = x + 1000.0
    elif family == "outlier":
        x = x * 3
        x[:, :, H // 3] = 1e4
    elif family == "nearconst":
        x = 0.3 + 1e-3 * x.clamp(-1, 1)
    elif family == "cancel":
        x[:, 1::2] = -x[:, 0:2 * (T // 2):2]
    elif family != "gauss":
        raise ValueError(family)
    return x.to(TD[dtype])


def prefix_mask(lens, T):
    return (torch.arange(T)[None, :] < torch.as_tensor(lens)[:, None]).to(torch.int32)


def pool_lens(B, T, seed=0):
    """Ragged lengths in 1..T; the first sequence full, the second (if any) a single token."""
    gen = torch.Generator().manual_seed(4441 + 7 * B + T + seed)
    lens = torch.randint(1, T + 1, (B,), generator=gen)
    lens[0] = T
    if B > 1:
        lens[1] = 1
    return lens


# ---------------------------------------------------------------- short attention
ATTN_D = 64


def attn_ref(qkv, cu, nH, scale):
    """softmax(scale q k^T) v of every sequence (tokens [cu[b], cu[b+1])) and head in float64, from the packed fused
    projections qkv (N, 3 nH 64).  Returns a dict of (N, nH, 64) float64 tensors ``ref``, ``A`` = p |v| and ``S`` =
    (sum_j |v_j|) / l with l = sum_j exp(s_j - max s), and (N, nH, 1) ``eps_s``: the bound on the error of a scaled
    fp32 score difference that the kernel's exponent sees (see attn_bound)."""
    n = qkv.shape[0]
    x = qkv.double().view(n, 3, nH, ATTN_D)
    out = {k: torch.zeros((n, nH, ATTN_D), dtype=torch.float64) for k in ("ref", "A", "S")}
    out["eps_s"] = torch.zeros((n, nH, 1), dtype=torch.float64)
    cu = [int(c) for c in cu]
    for s0, s1 in zip(cu[:-1], cu[1:]):
        if s1 <= s0:
            continue
        q, k, v = (x[s0:s1, i].transpose(0, 1) for i in range(3))  # (nH, L, d)
        s = scale * (q @ k.transpose(1, 2))
        smax = s.max(-1, keepdim=True).values
        e = torch.exp(s - smax)
        l = e.sum(-1, keepdim=True)
        p = e / l
        out["ref"][s0:s1] = (p @ v).transpose(0, 1)
        out["A"][s0:s1] = (p @ v.abs()).transpose(0, 1)
        out["S"][s0:s1] = (v.abs().sum(1, keepdim=True) / l).transpose(0, 1)
        absdot = scale * (q.abs() @ k.abs().transpose(1, 2)).max(-1, keepdim=True).values  # scale max_j sum_d |q_d k_d|
        spread = (smax - s.min(-1, keepdim=True).values)
        out["eps_s"][s0:s1] = (ATTN_D * U32 * absdot + U32 * (2 * spread + 4) + 132 * U32).transpose(0, 1)
    return out


def attn_bound(R, dtype):
    """E = u_dt (A + |ref|) + sub S + 2 eps_s A.
    u_dt A: P rounded to the tensor type (relative u_dt per weight); u_dt |ref|: the output's rounding; sub S: an f16 P
    below 2^-14 is rounded on the subnormal grid (absolute 2^-25 per key, 0 for bf16, whose exponent range is fp32's).
    2 eps_s A: a relative error eps_j of every unnormalised weight moves the output by at most 2 max|eps_j| A.  eps_s
    bounds it: the products q_d k_d are exact in fp32 (8- or 11-bit significands), their 64-term fp32 accumulation (any
    order, round to nearest) errs by at most 64 u sum_d |q_d k_d|, times scale; (s_j - m) and the product with scale
    round once each (2 u |s_j - max s|), expf is good to 2 ulp (4 u); the row sum l and the P V accumulation are
    64-term fp32 sums of same-sign / arbitrary terms (64 u each, relative to l and to A), and 1 / l and the final
    product round once each (together 132 u)."""
    sub = 2.0 ** -25 if dtype == "f16" else 0.0
    return U_DT[dtype] * (R["A"] + R["ref"].abs()) + sub * R["S"] + 2 * R["eps_s"] * R["A"]


def attn_emul(qkv, cu, nH, scale):
    """k_attn_mfma's arithmetic in fp32 on the CPU: raw fp32 scores, p = exp((s - max s) * scale), the row sum of the
    unrounded p, P rounded to the tensor type, (P V) * (1 / l), one rounding."""
    n = qkv.shape[0]
    td = qkv.dtype
    x = qkv.float().view(n, 3, nH, ATTN_D)
    out = torch.zeros((n, nH, ATTN_D), dtype=td)
    cu = [int(c) for c in cu]
    sc = torch.tensor(scale, dtype=torch.float32)
    for s0, s1 in zip(cu[:-1], cu[1:]):
        if s1 <= s0:
            continue
        q, k, v = (x[s0:s1, i].transpose(0, 1) for i in range(3))
        s = q @ k.transpose(1, 2)
        p = torch.exp((s - s.max(-1, keepdim=True).values) * sc)
        inv = 1.0 / p.sum(-1, keepdim=True)
        out[s0:s1] = ((p.to(td).float() @ v) * inv).transpose(0, 1).to(td)
    return out.view(n, nH * ATTN_D)


ATTN_FAMILIES = ("gauss", "peaked", "flat", "zero_q", "outlier_v", "peaked_outlier_v")
ATTN_BASE_LENGTHS = [1, 2, 7, 29, 31, 32, 33, 63, 64]


def attn_lengths(B, seed=0):
    """B sequence lengths: the edge lengths first (B >= 16), random 1..64 after, empty sequences in the middle and as
    the second to last, and a last sequence of 64 tokens (a graph pack's pad sequence).  B = 1: one 37-token sequence
    when seed is even, one 64-token sequence otherwise."""
    if B == 1:
        return [37 if seed % 2 == 0 else 64]
    gen = torch.Generator().manual_seed(2221 + B + seed)
    lens = list(ATTN_BASE_LENGTHS) if B >= 16 else [1, 33]
    lens += [int(v) for v in torch.randint(1, 65, (B - len(lens),), generator=gen)]
    lens = lens[:B]
    if B >= 4:
        lens[B // 2] = 0
        lens[-2] = 0
    lens[-1] = 64
    return lens


def attn_inputs(family, lengths, nH, dtype, seed=0):
    """(qkv (N, 3 nH 64) CPU tensor of ``dtype``, cu int64 numpy (B + 1,)).  Base: 2 N(0, 1) projections (as the
    older test).  peaked: q x 6 (score differences of ~100: most weights underflow); flat: every key row of a sequence
    and head equal to its first; zero_q: q = 0; outlier_v: one V row of every sequence with two tokens or more x 3000;
    peaked_outlier_v: both.  All scores stay finite (|s| < 1e4)."""
    gen = torch.Generator().manual_seed(77003 * (1 + ATTN_FAMILIES.index(family)) + 101 * nH + len(lengths) + seed)
    cu = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    n = int(cu[-1])
    x = (torch.randn((n, 3, nH, ATTN_D), generator=gen) * 2.0)
    if family in ("peaked", "peaked_outlier_v"):
        x[:, 0] *= 6.0
    if family == "zero_q":
        x[:, 0] = 0.0
    for s0, s1 in zip(cu[:-1], cu[1:]):
        if family == "flat" and s1 > s0:
            x[s0:s1, 1] = x[s0:s0 + 1, 1]
        if family in ("outlier_v", "peaked_outlier_v") and s1 - s0 >= 2:
            x[s0 + (s1 - s0) // 2, 2] *= 3000.0  # N(0, 6000): inside f16's range up to 10 sigma
    if family in ("outlier_v", "peaked_outlier_v"):
        x[:, 2].clamp_(-6.0e4, 6.0e4)
    return x.reshape(n, 3 * nH * ATTN_D).to(TD[dtype]), cu


# ---------------------------------------------------------------- erf GELU
# max over all finite f16 inputs of |gelu_fp32(x) - gelu_ref(x)| / |x| in units of 2^-24, for torch's own fp32 CPU
# evaluation of 0.5 x (1 + erf(x / sqrt 2)) (measured and asserted in tests/test_enc_ref_cpu.py); the kernel's bound
# takes twice that: one more ulp in the device's erff.
GELU_C_TORCH = 4.8
GELU_C = 2 * GELU_C_TORCH


def gelu_ref(x):
    """0.5 x erfc(-x / sqrt 2) in float64 (not 1 + erf, which cancels in the negative tail)."""
    x = x.double()
    return 0.5 * x * torch.special.erfc(-x / math.sqrt(2.0))


def gelu_emul(x):
    """k_gelu_erf's expression in fp32 on the CPU, in its order ((0.5 x) first: no overflow at the largest bf16)."""
    v = x.float()
    return (0.5 * v * (1.0 + torch.erf(v * 0.70710678118654752440))).to(x.dtype)


def ulp_of(ref, dtype):
    """Spacing of ``dtype``'s values at |ref| (float64 tensor), the subnormal spacing below the smallest normal."""
    p, emin = {"f32": (24, -126), "bf16": (8, -126), "f16": (11, -14)}[dtype]
    e = torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** emin)))
    return torch.exp2(e - (p - 1))


def gelu_bound(x, ref, dtype):
    """0.5 ulp_dt(ref) + c |x| 2^-24 (x, ref float64)."""
    return 0.5 * ulp_of(ref, dtype) + GELU_C * x.abs() * U32


def all_bit_patterns(dtype):
    """All 65,536 values of a 16-bit type, in bit-pattern order (CPU tensor)."""
    return torch.from_numpy(np.arange(65536, dtype=np.uint16).view(np.int16)).view(TD[dtype])
