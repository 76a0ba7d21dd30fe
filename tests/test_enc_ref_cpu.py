"""CPU: the float64 references of tests/enc_ref.py against torch's own float64 operators, the exact cases, and an fp32
restatement of every encoder kernel held to the bounds the GPU kernels are held to (tests/test_gpu_encoder_kernels.py).

The last part is what makes the bounds meaningful: an evaluation with the kernels' rounding points (fp32 statistics,
P and the outputs rounded to the tensor type) stays inside E for every family and type, so a kernel that leaves E
computes something else.  The max err / E of every (kernel, type, family) is printed (pytest -s).
"""
import math

import pytest
import torch
import torch.nn.functional as F

import enc_ref as E

DTS = ("f32", "bf16", "f16")


def _ratio(got, ref, bound):
    err = (got.double() - ref).abs()
    assert bool((bound > 0).all())
    return float((err / bound).max())


# ---------------------------------------------------------------- references == torch float64
@pytest.mark.parametrize("H", [1, 7, 256, 1000])
@pytest.mark.parametrize("eps", [1e-12, 1e-5])
def test_layernorm_ref_is_torch_float64(H, eps):
    x, r, g, b = E.ln_inputs("gauss", 5, H, "f32")
    R = E.layernorm_ref(x, r, g, b, eps, "f32")
    v = (x + r).double()  # fp32: the rounded sum is the fp32 sum
    want = F.layer_norm(v, (H,), g.double(), b.double(), eps)
    assert float((R["ref"] - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    assert torch.equal(R["mean_abs_v"], v.abs().mean(-1, keepdim=True))
    # 16-bit: v is the tensor type's rounding of the fp32 sum
    xb, rb, gb, bb = E.ln_inputs("gauss", 5, H, "bf16")
    assert torch.equal(E.layernorm_ref(xb, rb, gb, bb, eps, "bf16")["v"], (xb + rb).double())


def test_gelu_ref_is_torch_float64():
    x = torch.cat([torch.linspace(-8, 8, 20001, dtype=torch.float64), E.all_bit_patterns("f16").double()])
    x = x[torch.isfinite(x)]
    assert float((E.gelu_ref(x) - F.gelu(x)).abs().max()) <= 1e-12
    # the negative tail, where 1 + erf has cancelled to a few digits: erfc keeps full relative precision
    t = torch.tensor([-6.0, -8.0, -10.0, -13.0], dtype=torch.float64)
    want = torch.tensor([-6 * 9.8658764503769e-10, -8 * 6.2209605742718e-16, -10 * 7.6198530241605e-24,
                         -13 * 6.1171643995497e-39], dtype=torch.float64)
    assert bool(((E.gelu_ref(t) - want).abs() <= 1e-10 * want.abs()).all())


@pytest.mark.parametrize("nH", [1, 4])
def test_attn_ref_is_torch_float64(nH):
    lengths = [1, 5, 0, 33, 64]
    qkv, cu = E.attn_inputs("gauss", lengths, nH, "bf16")
    scale = 64 ** -0.5
    R = E.attn_ref(qkv, cu, nH, scale)
    x = qkv.double().view(-1, 3, nH, 64)
    for s0, s1 in zip(cu[:-1], cu[1:]):
        if s1 == s0:
            continue
        q, k, v = (x[s0:s1, i].transpose(0, 1) for i in range(3))
        want = F.scaled_dot_product_attention(q, k, v, scale=scale).transpose(0, 1)
        assert float((R["ref"][s0:s1] - want).abs().max()) <= 1e-12
        wantA = F.scaled_dot_product_attention(q, k, v.abs(), scale=scale).transpose(0, 1)
        assert float((R["A"][s0:s1] - wantA).abs().max()) <= 1e-12
    assert bool((R["S"] >= R["A"] * (1 - 1e-12)).all())  # p_j <= 1 / l for every key


@pytest.mark.parametrize("n_instr", [0, 3, 20])
def test_pool_ref_is_torch_float64(n_instr):
    B, T, H = 6, 37, 100
    hidden = E.pool_hidden("gauss", B, T, H, "f32")
    mask = E.prefix_mask(E.pool_lens(B, T), T)
    mask[3, 5] = 0  # a hole
    R = E.pool_ref(hidden, mask, n_instr)
    m = mask.double().clone()
    m[:, :n_instr] = 0
    want = F.normalize((hidden.double() * m[:, :, None]).sum(1) / m.sum(1)[:, None], dim=-1)
    empty = m.sum(1) == 0
    assert not bool(empty.all()) and (n_instr != 20 or int(empty.sum()) >= 2)
    assert torch.isnan(R["ref"]).all(1).tolist() == empty.tolist() and torch.isnan(R["ref"]).any(1).tolist() == empty.tolist()
    assert float((R["ref"][~empty] - want[~empty]).abs().max()) <= 1e-12


# ---------------------------------------------------------------- exact cases
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("H", [7, 256, 4096])
def test_const_exact_gives_beta(dt, H):
    x, r, g, b = E.ln_inputs("const_exact", 3, H, dt)
    for eps in (1e-12, 1e-5):
        assert torch.equal(E.layernorm_ref(x, r, g, b, eps, dt)["ref"], b.double().expand(3, H))
        assert torch.equal(E.layernorm_emul(x, r, g, b, eps, dt), b.expand(3, H))


@pytest.mark.parametrize("dt", DTS)
def test_cancel_gives_zero_not_nan(dt):
    B, T, H = 3, 36, 257
    hidden = E.pool_hidden("cancel", B, T, H, dt)
    mask = E.prefix_mask([36, 2, 20], T)
    R = E.pool_ref(hidden, mask, 0)
    assert bool((R["ref"] == 0).all()) and bool((R["norm"] == 0).all())
    assert bool((E.pool_emul(hidden, mask, 0) == 0).all())


# ---------------------------------------------------------------- the fp32 restatements stay inside the bounds
def test_k8_emulation_within_bound():
    worst = {}
    for dt in DTS:
        for fam in E.LN_FAMILIES:
            for H in (7, 256, 1536, 4096):
                for eps in (1e-12, 1e-5):
                    x, r, g, b = E.ln_inputs(fam, 5, H, dt)
                    R = E.layernorm_ref(x, r, g, b, eps, dt)
                    bound = E.layernorm_bound(R, g, b, dt)
                    q = _ratio(E.layernorm_emul(x, r, g, b, eps, dt), R["ref"], bound)
                    worst[dt, fam] = max(worst.get((dt, fam), 0.0), q)
    for k, v in worst.items():
        print("K8 emulation err/E", *k, f"{v:.3f}")
    assert max(worst.values()) <= 1.0, worst


def test_k7_emulation_within_bound():
    worst = {}
    for dt in DTS:
        for fam in E.POOL_FAMILIES:
            for B, T, H in ((3, 1, 257), (6, 37, 1000), (4, 512, 64)):
                hidden = E.pool_hidden(fam, B, T, H, dt)
                mask = E.prefix_mask(E.pool_lens(B, T), T)
                for n_instr in (0, 3):
                    R = E.pool_ref(hidden, mask, n_instr)
                    got = E.pool_emul(hidden, mask, n_instr)
                    ok = R["kept"] > 0
                    assert torch.isnan(got).any(1).tolist() == (~ok).tolist()
                    if ok.any():
                        q = _ratio(got[ok], R["ref"][ok], E.pool_bound(R, T)[ok])
                        worst[dt, fam] = max(worst.get((dt, fam), 0.0), q)
    for k, v in worst.items():
        print("K7 emulation err/E", *k, f"{v:.3f}")
    assert max(worst.values()) <= 1.0, worst


def test_attn_emulation_within_bound():
    worst = {}
    scale = 64 ** -0.5
    for dt in ("bf16", "f16"):
        for fam in E.ATTN_FAMILIES:
            for nH, B in ((1, 1), (4, 20)):
                lengths = E.attn_lengths(B)
                qkv, cu = E.attn_inputs(fam, lengths, nH, dt)
                R = E.attn_ref(qkv, cu, nH, scale)
                assert bool(torch.isfinite(R["ref"]).all())
                got = E.attn_emul(qkv, cu, nH, scale).view(-1, nH, 64)
                q = _ratio(got, R["ref"], E.attn_bound(R, dt))
                worst[dt, fam] = max(worst.get((dt, fam), 0.0), q)
    for k, v in worst.items():
        print("attention emulation err/E", *k, f"{v:.3f}")
    assert max(worst.values()) <= 1.0, worst


def test_gelu_constant_and_emulation_within_bound():
    """The constant c of the GELU bound: torch's fp32 CPU evaluation of the kernel's formula over every finite f16
    input against the float64 reference, max |err| / |x| in units of 2^-24 (GELU_C_TORCH; the kernels get twice that).
    Then the kernel's fp32 expression rounded once to each 16-bit type stays inside 0.5 ulp + c |x| 2^-24 over its whole
    domain.  (Not F.gelu there: torch's CPU kernel multiplies in an order that overflows for x >= 2^127 in bf16.)"""
    x16 = E.all_bit_patterns("f16")
    x16 = x16[torch.isfinite(x16) & (x16 != 0)]
    err = (F.gelu(x16.float()).double() - E.gelu_ref(x16)).abs() / x16.double().abs() / E.U32
    c = float(err.max())
    print(f"GELU fp32-vs-float64 constant: max err/|x| = {c:.2f} x 2^-24 at x = {float(x16[err.argmax()])}")
    assert c <= E.GELU_C_TORCH
    for dt in ("bf16", "f16"):
        x = E.all_bit_patterns(dt)
        x = x[torch.isfinite(x)]
        ref = E.gelu_ref(x)
        got = E.gelu_emul(x)
        q = _ratio(got, ref, E.gelu_bound(x.double(), ref, dt).clamp_min(1e-300))
        print("GELU emulation err/E", dt, f"{q:.3f}")
        assert q <= 1.0
        big = x.float() >= 6
        assert torch.equal(got[big], x[big])


def test_ulp_of():
    r = torch.tensor([1.0, 1.5, 2.0, 2.0 ** -14, 2.0 ** -20, 0.0, -3.0], dtype=torch.float64)
    assert E.ulp_of(r, "f16").tolist() == [2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 2.0 ** -24, 2.0 ** -24, 2.0 ** -24, 2.0 ** -9]
    assert E.ulp_of(r, "bf16")[:3].tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6]
    assert math.isclose(float(E.ulp_of(torch.tensor([0.3], dtype=torch.float64), "bf16")), 2.0 ** -9)


# ---------------------------------------------------------------- the bounds are sharp: near-miss variants leave them
def test_bounds_reject_subtly_wrong_variants():
    """Each variant below is a plausible kernel slip that a Gaussian / global-tolerance check lets through; every one
    leaves its per-element bound on the family built for it."""
    # K8: one-pass variance E[v^2] - mean^2 in fp32 (cancels when the row mean is large)
    x, r, g, b = E.ln_inputs("offset", 5, 1536, "f32")
    R = E.layernorm_ref(x, r, g, b, 1e-12, "f32")
    v = x + r
    mean = v.mean(-1, keepdim=True)
    bad = (v - mean) * torch.rsqrt((v * v).mean(-1, keepdim=True) - mean * mean + 1e-12) * g + b
    assert _ratio(bad, R["ref"], E.layernorm_bound(R, g, b, "f32")) > 1.0
    # K8: the statistics taken from the unrounded sum (the 16-bit sum is a tensor of its own in the model)
    x, r, g, b = E.ln_inputs("gauss", 5, 768, "bf16")
    R = E.layernorm_ref(x, r, g, b, 1e-12, "bf16")
    v = x.float() + r.float()
    d = v - v.mean(-1, keepdim=True)
    bad = (d * torch.rsqrt((d * d).mean(-1, keepdim=True) + 1e-12) * g.float() + b.float()).bfloat16()
    assert _ratio(bad, R["ref"], E.layernorm_bound(R, g, b, "bf16")) > 1.0
    # K7: the instruction mask one token short
    hidden = E.pool_hidden("gauss", 6, 37, 1000, "f32")
    mask = E.prefix_mask(E.pool_lens(6, 37), 37)
    R = E.pool_ref(hidden, mask, 3)
    ok = R["kept"] > 0
    assert _ratio(E.pool_emul(hidden, mask, 2)[ok], R["ref"][ok], E.pool_bound(R, 37)[ok]) > 1.0
    # attention: the last key of every sequence dropped where its weight is small (< 2 %): under the old global floor
    lengths = E.attn_lengths(20)
    scale = 64 ** -0.5
    for dt in ("bf16", "f16"):
        qkv, cu = E.attn_inputs("gauss", lengths, 4, dt)
        R = E.attn_ref(qkv, cu, 4, scale)
        x = qkv.double().view(-1, 3, 4, 64)
        bad = R["ref"].clone()
        for s0, s1 in zip(cu[:-1], cu[1:]):
            if s1 - s0 < 8:
                continue
            q, k, vv = (x[s0:s1, i].transpose(0, 1) for i in range(3))
            p = torch.softmax(scale * (q @ k.transpose(1, 2)), -1)
            small = (p[:, :, -1:] < 0.02).double()
            bad[s0:s1] -= (small * p[:, :, -1:] * vv[:, -1:, :]).transpose(0, 1)
        assert _ratio(bad.to(E.TD[dt]), R["ref"], E.attn_bound(R, dt)) > 1.0
    # GELU: the tanh approximation, and 1 + erf evaluated in the tensor type
    for dt in ("bf16", "f16"):
        x = E.all_bit_patterns(dt)
        x = x[torch.isfinite(x)]
        ref = E.gelu_ref(x)
        bound = E.gelu_bound(x.double(), ref, dt)
        assert _ratio(F.gelu(x.float(), approximate="tanh").to(E.TD[dt]), ref, bound) > 1.0
        lowp = (0.5 * x.float() * (1.0 + torch.erf(x.float() * 0.70710678).to(E.TD[dt]).float())).to(E.TD[dt])
        assert _ratio(lowp, ref, bound) > 1.0
