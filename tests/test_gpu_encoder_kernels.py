"""GPU: the encoder kernels against float64 on every dispatch path (references, bounds and families: tests/enc_ref.py).

* K8 ``hr_add_layernorm``: the 12 wave-per-row instantiations (the case ids name them), the generic kernel, the
  unaligned fallback, rows 1..5 and 37 (four rows per workgroup), five input families, eps 1e-12 and 1e-5; per element
  |y - ref| <= E; nothing written past ``rows``; H > 4096 rejected, rows = 0 a no-op.
* K7 ``hr_pool_normalize`` / ``_packed``: six shapes, instruction lengths 0 / inside / T - 1 / T / past T, prefix masks
  and masks with holes; per element bound, NaN rows exactly where every token is masked, packed == padded bit for bit,
  power-of-two scaling leaves the bits unchanged, cancelling tokens give exact zeros.
* ``hr_attn_varlen``: nH 1 / 4 / 12 / 16, one and 75 sequences with empty ones among them, six families; per element
  bound, a single-token sequence returns its V row bit for bit, nothing written past the batch's rows.
* ``hr_gelu_erf``: all 65,536 inputs of each type through the vector path and through the tail path; torch parity (bf16
  bit-identical, f16 one ulp), the float64 bound, exact facts, nothing written past the last element.

Every test prints its max err / E (pytest -s); DESIGN.md §4b records them.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import enc_ref as E
from hiprag import _native

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
DTS = ("f32", "bf16", "f16")
EPS = (1e-12, 1e-5)
ROWS = (1, 2, 3, 4, 5, 37)
# K8 dispatch (csrc/hr_pool.hip launch_add_ln): width -> (C, N) of k_add_layernorm_w per type; any other width, and any
# unaligned pointer, runs the generic k_add_layernorm
K8_FAST = {"f32": {256: (4, 1), 512: (4, 2), 768: (4, 3), 1024: (4, 4), 1536: (4, 6), 2048: (4, 8)},
           "16": {256: (4, 1), 512: (8, 1), 768: (4, 3), 1024: (8, 2), 1536: (8, 3), 2048: (8, 4)}}
K8_GENERIC = (1, 7, 100, 255, 257, 4095, 4096)
K8_FAMILY_H = (256, 1536, 4096)


def _k8_path(dt, H):
    cn = K8_FAST["f32" if dt == "f32" else "16"].get(H)
    return f"wave{cn[0]}x{cn[1]}" if cn else "generic"


K8_CASES = [pytest.param(dt, H, fam, id=f"{dt}-H{H}-{_k8_path(dt, H)}-{fam}")
            for dt in DTS for H in sorted(set(K8_GENERIC) | set(K8_FAST["f32"]))
            for fam in (E.LN_FAMILIES if H in K8_FAMILY_H else ("gauss",))]


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _sentinel(n, td):
    """n elements of ``td`` on the device, every byte 0x5A."""
    it = torch.int32 if td == torch.float32 else torch.int16
    return torch.full((n,), 0x5A5A5A5A if td == torch.float32 else 0x5A5A, dtype=it, device=DEV).view(td)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _untouched(t):
    return bool((_bits(t) == _bits(_sentinel(1, t.dtype))).all())


def _k8_raw(x, r, g, b, out, rows, H, eps, dt):
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    return _native.load_library().hr_add_layernorm(p(x), p(r), p(g), p(b), p(out), int(rows), int(H), float(eps),
                                                   _native.DTYPES[dt], _stream())


def _shifted(t, fill=False):
    """A contiguous view with t's shape that starts one element into a fresh allocation (2- or 4-byte aligned), and the
    allocation; holds t's values, or the sentinel when fill is set."""
    n = t.numel()
    buf = _sentinel(n + 9, t.dtype)
    v = buf[1:1 + n].view(t.shape)
    if not fill:
        v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 != 0
    return v, buf


def _report(kernel, dt, family, ratio):
    print(f"ENC err/E {kernel} {dt} {family} {ratio:.3f}")


def _check_bound(got, ref, bound, what):
    err = (got.detach().cpu().double() - ref).abs()
    ratio = err / bound
    worst = float(ratio.max())
    assert worst <= 1.0, (what, worst, float(err.max()), np.unravel_index(int(ratio.argmax()), ratio.shape))
    return worst


# ================================================================ K8
@pytest.mark.parametrize("dt,H,family", K8_CASES)
def test_k8_within_float64_bound(dt, H, family):
    """hr_add_layernorm vs float64 on the path the id names: per element |y - ref| <= E (enc_ref.layernorm_bound) for
    rows 1, 2, 3, 4, 5 and 37 and both eps; const_exact is bit-equal to beta."""
    x, r, g, b = E.ln_inputs(family, max(ROWS), H, dt)
    xd, rd, gd, bd = (t.to(DEV) for t in (x, r, g, b))
    worst = 0.0
    for eps in EPS:
        R = E.layernorm_ref(x, r, g, b, eps, dt)
        bound = E.layernorm_bound(R, g, b, dt)
        for rows in ROWS:
            out = _native.add_layernorm(xd[:rows], rd[:rows], gd, bd, eps)
            assert out.shape == (rows, H) and out.dtype == E.TD[dt]
            if family == "const_exact":
                assert torch.equal(out.cpu(), b.expand(rows, H)), (rows, eps)
            worst = max(worst, _check_bound(out, R["ref"][:rows], bound[:rows], (dt, H, family, rows, eps)))
    _report(f"K8/{_k8_path(dt, H)}/H{H}", dt, family, worst)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("H", [768, 100])
def test_k8_unaligned_pointers_take_the_generic_kernel(dt, H):
    """Views one element into a larger buffer (pointers 2- or 4-byte aligned): the scalar generic kernel serves them
    for every width.  Same bound; within 2 E of the aligned run; one unaligned pointer gives the bits that five do
    (the same kernel ran, not a vector kernel that happens to tolerate some of them); nothing written outside out."""
    rows, eps = 5, 1e-12
    x, r, g, b = E.ln_inputs("gauss", rows, H, dt)
    R = E.layernorm_ref(x, r, g, b, eps, dt)
    bound = E.layernorm_bound(R, g, b, dt)
    al = [t.to(DEV) for t in (x, r, g, b)]
    aligned = _native.add_layernorm(*al, eps)
    un = [_shifted(t)[0] for t in al]
    out_u, out_buf = _shifted(aligned, fill=True)
    assert _k8_raw(*un, out_u, rows, H, eps, dt) == 0
    torch.cuda.synchronize()
    worst = _check_bound(out_u, R["ref"], bound, (dt, H, "unaligned"))
    _report(f"K8/unaligned/H{H}", dt, "gauss", worst)
    assert bool(((out_u.cpu().double() - aligned.cpu().double()).abs() <= 2 * bound).all())
    assert _untouched(out_buf[:1]) and _untouched(out_buf[1 + rows * H:])
    for which in range(5):  # exactly one unaligned pointer: x, r, gamma, beta, out
        args = [un[i] if i == which else al[i] for i in range(4)]
        out = _shifted(aligned, fill=True)[0] if which == 4 else torch.empty_like(aligned)
        assert _k8_raw(*args, out, rows, H, eps, dt) == 0
        assert torch.equal(_bits(out), _bits(out_u)), which
    if H == 768:
        print(f"K8 H768 {dt}: generic differs from wave kernel in {int((_bits(aligned) != _bits(out_u)).sum())} elements")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("H", [256, 768, 2048, 100])
@pytest.mark.parametrize("rows", [1, 2, 3, 5])
def test_k8_writes_no_row_past_rows(dt, H, rows):
    """An output buffer 8 rows longer than ``rows``, pre-filled with a bit pattern: the wave kernels' workgroups hold
    four rows each, so rows % 4 != 0 leaves lanes that must not store."""
    x, r, g, b = (t.to(DEV) for t in E.ln_inputs("gauss", rows, H, dt))
    out = _sentinel((rows + 8) * H, E.TD[dt]).view(rows + 8, H)
    assert _k8_raw(x, r, g, b, out, rows, H, 1e-12, dt) == 0
    torch.cuda.synchronize()
    assert _untouched(out[rows:])
    assert torch.equal(_bits(out[:rows]), _bits(_native.add_layernorm(x, r, g, b, 1e-12)))


def test_k8_rejects_wide_rows_and_ignores_empty_input():
    for dt in DTS:
        x, r, g, b = (t.to(DEV) for t in E.ln_inputs("gauss", 2, 4097, dt))
        with pytest.raises(ValueError):
            _native.add_layernorm(x, r, g, b, 1e-12)
        x, r, g, b = (t.to(DEV) for t in E.ln_inputs("gauss", 2, 768, dt))
        out = _sentinel(2 * 768, E.TD[dt]).view(2, 768)
        assert _k8_raw(x, r, g, b, out, 0, 768, 1e-12, dt) == 0  # rows = 0: no launch
        torch.cuda.synchronize()
        assert _untouched(out)
        assert _native.add_layernorm(x[:0], r[:0], g, b, 1e-12).shape == (0, 768)
        assert _k8_raw(x, r, g, b, out, -1, 768, 1e-12, dt) == _native.E_INVALID
        assert _k8_raw(x, r, g, b, out, 2, 0, 1e-12, dt) == _native.E_INVALID


# ================================================================ K7
K7_SHAPES = [(1, 1, 1), (3, 1, 257), (6, 37, 1000), (70, 64, 256), (4, 512, 1024), (2, 37, 255)]
K7_FAMILY_SHAPES = [(6, 37, 1000), (2, 37, 255)]


def _pool(hidden_d, dt, mask_d, n_instr):
    B, T, H = hidden_d.shape
    out = torch.empty((B, H), dtype=torch.float32, device=DEV)
    _native.pool_normalize(hidden_d.data_ptr(), dt, mask_d.data_ptr(), B, T, H, n_instr, out.data_ptr(),
                           torch.cuda.current_stream(DEV).cuda_stream)
    return out


def _pool_packed(hidden, lens, dt, n_instr):
    B, T, H = hidden.shape
    keep = E.prefix_mask(lens, T).bool()
    packed = hidden[keep].contiguous().to(DEV)
    cu = torch.tensor([0, *torch.cumsum(torch.as_tensor(lens), 0).tolist()], dtype=torch.int32, device=DEV)
    out = torch.empty((B, H), dtype=torch.float32, device=DEV)
    _native.pool_normalize_packed(packed.data_ptr(), dt, cu.data_ptr(), B, H, n_instr, out.data_ptr(),
                                  torch.cuda.current_stream(DEV).cuda_stream)
    return out


def _same_bits_nan_aware(a, b):
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(_bits(torch.nan_to_num(a, nan=7.0)),
                                                                       _bits(torch.nan_to_num(b, nan=7.0)))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("shape,family", [(s, "gauss") for s in K7_SHAPES] +
                         [(s, f) for s in K7_FAMILY_SHAPES for f in E.POOL_FAMILIES[1:]],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v)
def test_k7_within_float64_bound(dt, shape, family):
    """hr_pool_normalize on prefix masks and masks with holes, hr_pool_normalize_packed on the prefix masks: per element
    bound (enc_ref.pool_bound), NaN rows exactly where every token is masked, packed == padded bit for bit."""
    B, T, H = shape
    hidden = E.pool_hidden(family, B, T, H, dt)
    hidden_d = hidden.to(DEV)
    lens = E.pool_lens(B, T)
    gen = torch.Generator().manual_seed(5 + B + T)
    holes = (torch.rand((B, T), generator=gen) < 0.6).to(torch.int32)
    holes[0] = 1
    worst = 0.0
    for n_instr in sorted({0, 3, T - 1, T, T + 5}):
        for kind, mask in (("prefix", E.prefix_mask(lens, T)), ("holes", holes)):
            R = E.pool_ref(hidden, mask, n_instr)
            out = _pool(hidden_d, dt, mask.to(DEV), n_instr)
            torch.cuda.synchronize()
            ok = R["kept"] > 0
            assert torch.isnan(out).any(1).cpu().tolist() == (~ok).tolist(), (kind, n_instr)
            assert torch.isnan(out).all(1).cpu().tolist() == (~ok).tolist(), (kind, n_instr)
            if ok.any():
                worst = max(worst, _check_bound(out[ok.to(DEV)], R["ref"][ok], E.pool_bound(R, T)[ok],
                                                (dt, shape, family, kind, n_instr)))
            if kind == "prefix":
                out_p = _pool_packed(hidden, lens, dt, n_instr)
                torch.cuda.synchronize()
                assert _same_bits_nan_aware(out_p, out), n_instr
    _report(f"K7/{B}x{T}x{H}", dt, family, worst)


@pytest.mark.parametrize("dt,k", [("f32", 40), ("bf16", 20), ("f16", 4)])
def test_k7_power_of_two_scaling_keeps_the_bits(dt, k):
    """Hidden states times 2^k and 2^-k: every step of K7 (the sums, the division by the count, the squares, the square
    root, the reciprocal, the product) scales exactly by a power of two, so the unit vector's bits do not move.  The
    inputs sit on a grid (multiples of 1/16 below 8) that all three types hold exactly at both scales."""
    B, T, H = 6, 37, 1000
    gen = torch.Generator().manual_seed(31)
    base = torch.randint(-127, 128, (B, T, H), generator=gen).float() / 16.0
    lens = E.pool_lens(B, T)
    mask = E.prefix_mask(lens, T).to(DEV)
    outs = []
    for s in (1.0, 2.0 ** k, 2.0 ** -k):
        h = (base * s).to(E.TD[dt])
        assert torch.equal(h.float() / s, base)  # the scaled tensor holds the same values
        outs.append(_pool(h.to(DEV), dt, mask, 3))
        outs.append(_pool_packed(h, lens, dt, 3))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(outs[0][lens.to(DEV) > 3]).all())
    for o in outs[1:]:
        assert _same_bits_nan_aware(o, outs[0])


@pytest.mark.parametrize("dt", DTS)
def test_k7_cancelling_tokens_give_exact_zeros(dt):
    """Token pairs +a, -a: every column's running sum returns to 0 after each pair, the mean is exactly 0, the norm 0,
    and x / max(||x||, 1e-12) is 0 -- not NaN, not 0 * inf."""
    B, T, H = 3, 36, 257
    hidden = E.pool_hidden("cancel", B, T, H, dt)
    lens = torch.tensor([36, 2, 20])
    for n_instr in (0, 2):
        out = _pool(hidden.to(DEV), dt, E.prefix_mask(lens, T).to(DEV), n_instr)
        out_p = _pool_packed(hidden, lens, dt, n_instr)
        torch.cuda.synchronize()
        for o in (out, out_p):
            exp_nan = (lens <= n_instr).tolist()
            assert torch.isnan(o).all(1).cpu().tolist() == exp_nan
            assert bool((o[~torch.tensor(exp_nan)] == 0).all())


# ================================================================ short attention
SCALE = 64 ** -0.5
ATTN_CASES = [pytest.param(dt, nH, B, fam, id=f"{dt}-nH{nH}-B{B}-{fam}")
              for dt in ("bf16", "f16") for nH in (1, 4, 12, 16) for B in (1, 75)
              for fam in (E.ATTN_FAMILIES if B == 75 else ("gauss", "flat", "peaked_outlier_v"))]


@functools.lru_cache(maxsize=2)
def _attn_case(dt, nH, B, family):
    lengths = E.attn_lengths(B, seed=nH)
    qkv, cu = E.attn_inputs(family, lengths, nH, dt)
    return lengths, qkv, cu, E.attn_ref(qkv, cu, nH, SCALE)


@pytest.mark.parametrize("dt,nH,B,family", ATTN_CASES)
def test_attention_within_float64_bound(dt, nH, B, family):
    """hr_attn_varlen vs float64 softmax(scale q k^T) v per sequence and head: per element |out - ref| <= E
    (enc_ref.attn_bound: no global floor -- a wrong small weight in a row of small values shows).  The true max_len is
    passed.  Single-token sequences return their V row bit for bit; flat / zero_q rows equal the float64 mean of V within E."""
    lengths, qkv, cu, R = _attn_case(dt, nH, B, family)
    n = qkv.shape[0]
    assert bool(torch.isfinite(R["ref"]).all()) and bool(torch.isfinite(R["eps_s"]).all())
    out = _native.attn_varlen(qkv.to(DEV), torch.from_numpy(cu.astype(np.int32)).to(DEV), B, nH, 64, max(lengths), SCALE)
    assert out is not None and out.shape == (n, nH * 64) and out.dtype == E.TD[dt]
    got = out.cpu().view(n, nH, 64)
    worst = _check_bound(got, R["ref"], E.attn_bound(R, dt), (dt, nH, B, family))
    _report(f"attn/nH{nH}/B{B}", dt, family, worst)
    v = qkv.view(n, 3, nH, 64)[:, 2]
    for s0, s1 in zip(cu[:-1], cu[1:]):
        if s1 - s0 == 1:
            assert torch.equal(_bits(got[s0]), _bits(v[s0]))
    if family in ("flat", "zero_q"):  # equal scores: every weight 1 / L, the output the plain float64 mean of V
        mean_v = torch.zeros_like(R["ref"])
        for s0, s1 in zip(cu[:-1], cu[1:]):
            if s1 > s0:
                mean_v[s0:s1] = v[s0:s1].double().mean(0, keepdim=True)
        _check_bound(got, mean_v, E.attn_bound(R, dt), (dt, nH, B, family, "mean of V"))


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("nH", [1, 12])
def test_attention_writes_its_rows_and_no_other(dt, nH):
    """out= a tensor 64 rows longer than the batch, pre-filled with a bit pattern: every row of the batch is
    overwritten (both waves' query rows, every head), every row past it untouched (query rows past a sequence's length
    live in the same workgroup as real ones)."""
    B = 75
    lengths, qkv, cu, R = _attn_case(dt, nH, B, "gauss")
    n = qkv.shape[0]
    out = _sentinel((n + 64) * nH * 64, E.TD[dt]).view(n + 64, nH * 64)
    ret = _native.attn_varlen(qkv.to(DEV), torch.from_numpy(cu.astype(np.int32)).to(DEV), B, nH, 64, max(lengths), SCALE,
                              out=out)
    assert ret is out
    torch.cuda.synchronize()
    assert _untouched(out[n:])
    assert bool((_bits(out[:n]) != _bits(_sentinel(1, E.TD[dt]))).all())  # (|out| <= max |v| ~ 10; the pattern is 203 / 1.5e13)
    _check_bound(out[:n].cpu().view(n, nH, 64), R["ref"], E.attn_bound(R, dt), (dt, nH, "out="))


def test_attention_declines_what_it_does_not_serve():
    """None (the caller's flash kernel) for d = 32, max_len = 65, fp32 projections and a non-contiguous qkv."""
    cu = torch.tensor([0, 5, 12], dtype=torch.int32, device=DEV)
    qkv = torch.randn((12, 3 * 4 * 64), device=DEV).to(torch.bfloat16)
    assert _native.attn_varlen(qkv, cu, 2, 4, 64, 7, SCALE) is not None
    assert _native.attn_varlen(qkv, cu, 2, 8, 32, 7, 32 ** -0.5) is None
    assert _native.attn_varlen(qkv, cu, 2, 4, 64, 65, SCALE) is None
    assert _native.attn_varlen(qkv.float(), cu, 2, 4, 64, 7, SCALE) is None
    wide = torch.randn((12, 2 * 3 * 4 * 64), device=DEV).to(torch.bfloat16)
    assert _native.attn_varlen(wide[:, :3 * 4 * 64], cu, 2, 4, 64, 7, SCALE) is None


# ================================================================ erf GELU
GELU_TAIL = [1.0, -1.0, 0.5, 6.0, -3.0]  # appended: 65,541 elements, n % 8 == 5


def _gelu_inputs(dt, tail):
    x = E.all_bit_patterns(dt)
    return torch.cat([x, torch.tensor(GELU_TAIL).to(E.TD[dt])]) if tail else x


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("tail", [False, True], ids=["vector", "tail"])
def test_gelu_whole_domain(dt, tail):
    """hr_gelu_erf over all 65,536 bit patterns, as one aligned tensor (16-byte vector path) and with five more
    elements (n % 8 != 0: the last thread's scalar path): torch parity, the float64 bound, the exact facts, and the
    bytes after the last element untouched."""
    x = _gelu_inputs(dt, tail)
    n = x.numel()
    buf = _sentinel(n + 27, E.TD[dt])
    got_d = buf[:n]
    got_d.copy_(x)
    want = F.gelu(got_d.clone())
    assert _native.gelu_erf_(got_d) is got_d
    torch.cuda.synchronize()
    assert _untouched(buf[n:])
    got, want = got_d.cpu(), want.cpu()
    # ---- torch on the same device tensor
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    live = ~torch.isnan(got)
    if dt == "bf16":
        assert torch.equal(_bits(got[live]), _bits(want[live]))
    else:
        diff = (got[live].double() - want[live].double()).abs()
        both_inf = torch.isinf(got[live]) & (got[live] == want[live])
        assert bool(((diff <= E.ulp_of(want[live].double(), "f16")) | both_inf).all())
        same = float((_bits(got[live]) == _bits(want[live])).float().mean())
        print(f"f16 gelu identical to torch on {same:.5f} of the domain")
        assert same >= 0.999
    # ---- float64
    fin = torch.isfinite(x)
    xf = x[fin].double()
    ref = E.gelu_ref(x[fin])
    worst = _check_bound(got[fin], ref, E.gelu_bound(xf, ref, dt), (dt, tail))
    _report("gelu/" + ("tail" if tail else "vector"), dt, "all-bits", worst)
    # ---- exact facts
    big = fin & (x.float() >= 6)
    assert int(big.sum()) > 1000 and torch.equal(_bits(got[big]), _bits(x[big]))  # the largest finite value included
    zero = x.float() == 0
    assert int(zero.sum()) == 2 and torch.equal(_bits(got[zero]), _bits(x[zero]))  # +0 -> +0, -0 -> -0
    pinf = torch.isinf(x) & (x.float() > 0)
    assert int(pinf.sum()) == 1 and torch.equal(_bits(got[pinf]), _bits(x[pinf]))
    assert bool(torch.isnan(got[torch.isnan(x)]).all()) and int(torch.isnan(x).sum()) > 0


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("n", [1, 5, 8, 13])
def test_gelu_small_lengths_stay_inside_the_tensor(dt, n):
    x = (torch.linspace(-4, 4, n)).to(E.TD[dt])
    buf = _sentinel(n + 27, E.TD[dt])
    buf[:n].copy_(x)
    assert _native.gelu_erf_(buf[:n]) is not None
    torch.cuda.synchronize()
    assert _untouched(buf[n:])
    ref = E.gelu_ref(x)
    _check_bound(buf[:n], ref, E.gelu_bound(x.double(), ref, dt), (dt, n))
