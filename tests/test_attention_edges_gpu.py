"""HIP attention (csrc/kernels/attention.hip), every kernel variant, per element against an exact
float64 reference: componentwise error bounds, a bit-exact gather, guard bands, and the same
cases again in child processes for the variants that environment switches select.

The reference is plain PyTorch in float64 on the bf16 inputs upcast. Next to each exact result
``R`` it returns the magnitude array ``A_R`` of the sums that a bf16-staged evaluation rounds
(``P`` the softmax, ``dP = dO V^T``, ``Dabs = rowsum(|dO||O|)``, ``E = P * (|dP| + Dabs)``):

    A_O = P |V|     A_dV = P^T |dO|     A_dQ = scale E |K|     A_dK = scale E^T |Q|

and a kernel output passes when ``|got - R| <= c * 2^-9 * A_R + 1e-12 * max(A_R)`` holds for
every element. The constants ``c`` do not come from the kernels: ``emulate`` below is a second
plain-PyTorch path that rounds to bf16 where the kernels' header comments say they do, its worst
ratio over every (family, T) of this file was measured on the CPU, and ``c`` is twice that,
rounded up (accumulation order, the 1-ulp v_exp_f32). A CPU test keeps the emulation within c / 2.

Kernels and the configurations (``CONFIGS``) whose dispatch test names them; every value test of
a configuration runs whatever ``attn_dispatch`` names for its T:

    kernel                               configuration (T)
    attn_fwd_kernel                      default (257), blocked (197)
    attn_fwd_res_kernel<0>               default (64), generic (197)
    attn_fwd_res_kernel<13>              default (197), pair (197)
    attn_bwd_dq_kernel                   default (257), blocked (197)
    attn_bwd_dkv_kernel                  default (257), blocked (197)
    attn_bwd_dq_res_kernel<0>            default (64), generic (197)
    attn_bwd_dq_res_kernel<13>           pair (197), pair_nopipe (197)
    attn_bwd_dkv_res_kernel<0,0>         default (64), generic (197)
    attn_bwd_dkv_res_kernel<13,0>        pair_nopipe (197)
    attn_bwd_dkv_res_kernel<13,1>        pair (197), parts1 / parts3 / parts16 (197)
    attn_bwd_fused_kernel<13>            default (197)
"""
import math
import os
import subprocess
import sys

import pytest
import torch

SCALE = 0.125
LOG2E = 1.4426950408889634
U = 2.0 ** -9  # the bounds' unit: half of bf16's unit roundoff 2^-8 (8 significand bits)

# Worst |err| / (2^-9 A) of `emulate` against `reference` over every family and every shape of
# CASES (CPU, float32 products), and the bounds' constants c = ceil(2 * ratio):
EMU_RATIO = {"O": 3.31, "dQ": 1.45, "dK": 2.19, "dV": 3.80}  # all four in the peaked family, T 192..257
C = {"O": 7, "dQ": 3, "dK": 5, "dV": 8}

FAMILIES = ("gaussian", "peaked", "offpos", "offneg", "gather")
T_ALL = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 191, 192, 193, 197, 207, 208, 209, 240, 255, 256, 257, 289, 320)
T_REMAP = (17, 197, 208, 257)  # again at (B, H) = (2, 4): workgroup total a multiple of 8, XCD remap on
SHAPES = [(t, 2, 3) for t in T_ALL] + [(t, 2, 4) for t in T_REMAP]
CASES = [(f, t, b, h) for f in FAMILIES for (t, b, h) in SHAPES]
T_CHILD = (1, 17, 33, 64, 193, 197, 208, 209, 256, 257)
T_EMU_CPU = (1, 17, 64, 197, 257)  # the CPU test's subset
CHILD = os.environ.get("FLUXMPI_ATTN_EDGES_CHILD") == "1"


def _id(f, t, b, h):
    return f"{f}-T{t}-B{b}H{h}"


def _perm(t):
    """pi(i) = (7 i + 3) mod T, or the identity when 7 does not generate Z_T."""
    i = torch.arange(t)
    return (7 * i + 3) % t if math.gcd(7, t) == 1 else i


def _nonzero_ints(x):
    """0..254 -> the integers of [-128, 127] without 0 (a zero target would show the gather's
    2^-40 leakage as a non-zero bit pattern; every other bf16 integer absorbs it)."""
    return torch.where(x < 128, x - 128, x - 127)


def make_inputs(family, t, b, h):
    """Seeded bf16 (qkv [B, T, 3*H*64], dO [B, T, H*64]) of one input family, made on the CPU."""
    gen = torch.Generator().manual_seed(FAMILIES.index(family) * 100003 + t * 101 + b * 17 + h)
    rn = lambda *s: torch.randn(*s, generator=gen)
    q, k, v = rn(b, t, h, 64) * 1.5, rn(b, t, h, 64) * 1.5, rn(b, t, h, 64) * 1.5
    g = rn(b, t, h, 64)
    if family == "peaked":  # score standard deviation sigma^2 = 20: a nearly one-hot softmax
        q, k = q / 1.5 * 20 ** 0.5, k / 1.5 * 20 ** 0.5
    elif family == "offpos":  # every score about +200
        q = 5 + q / 6
        k = q.clone()
    elif family == "offneg":  # every score about -128: lse2 about -185 + log2(T)
        q, k = 4 + q / 6, -4 + k / 6
    elif family == "gather":
        k = 3.0 * (torch.randint(0, 2, (b, t, h, 64), generator=gen) * 2 - 1)
        q = k[:, _perm(t)]
        v = _nonzero_ints(torch.randint(0, 255, (b, t, h, 64), generator=gen))
        rid = (torch.arange(b).view(b, 1, 1) * h + torch.arange(h).view(1, 1, h)) * t + torch.arange(t).view(1, t, 1)
        for c in range(3):  # the row id, base 255, in the first three channels: rows are distinct
            v[..., c] = _nonzero_ints((rid // 255 ** c) % 255)
        v = v.float()
        g = _nonzero_ints(torch.randint(0, 255, (b, t, h, 64), generator=gen)).float()
    qkv = torch.stack([q, k, v], 2).reshape(b, t, 3 * h * 64).to(torch.bfloat16)
    return qkv, g.reshape(b, t, h * 64).to(torch.bfloat16)


def _split(qkv, dout, heads, dtype):
    """q, k, v, dO as [B, H, T, 64] in `dtype`."""
    b, t, _ = qkv.shape
    q, k, v = qkv.to(dtype).view(b, t, 3, heads, 64).permute(2, 0, 3, 1, 4)
    return q, k, v, dout.to(dtype).view(b, t, heads, 64).permute(0, 2, 1, 3)


def reference(qkv, dout, heads):
    """Exact (float64) attention, its gradient and the magnitude arrays of the bounds; all [B, H, T, 64]
    except lse2 / lse2_cond [B, H, T] and p_off_max (the largest softmax weight off pi's match)."""
    q, k, v, g = _split(qkv, dout, heads, torch.float64)
    t = q.shape[2]
    s = (q @ k.transpose(-1, -2)) * SCALE
    lse = torch.logsumexp(s, -1, keepdim=True)
    p = torch.exp(s - lse)
    o = p @ v
    dp = g @ v.transpose(-1, -2)
    ds = p * (dp - (g * o).sum(-1, keepdim=True))
    e = p * (dp.abs() + (g.abs() * o.abs()).sum(-1, keepdim=True))
    match = torch.zeros(t, t, dtype=torch.bool, device=q.device)
    match[torch.arange(t), _perm(t)] = True
    return {
        "O": o, "lse2": lse[..., 0] * LOG2E, "dQ": SCALE * (ds @ k), "dK": SCALE * (ds.transpose(-1, -2) @ q),
        "dV": p.transpose(-1, -2) @ g,
        "A_O": p @ v.abs(), "A_dV": p.transpose(-1, -2) @ g.abs(), "A_dQ": SCALE * (e @ k.abs()),
        "A_dK": SCALE * (e.transpose(-1, -2) @ q.abs()),
        "lse2_cond": SCALE * LOG2E * (q.abs() @ k.abs().transpose(-1, -2)).amax(-1),
        "p_off_max": float(p.masked_fill(match, 0.0).max()),
    }


def _bf(x):
    return x.to(torch.bfloat16).float()


def emulate(qkv, dout, heads):
    """The kernels' arithmetic in plain PyTorch: float32 products of the bf16 operands, rounded to
    bf16 where attention.hip rounds: P before P V and before dO^T P, dS before both of its products,
    the stored O before D = rowsum(dO * O), and every output."""
    q, k, v, g = _split(qkv, dout, heads, torch.float32)
    c2 = torch.tensor(SCALE * LOG2E, dtype=torch.float32)
    x = (q @ k.transpose(-1, -2)) * c2
    m = x.amax(-1, keepdim=True)
    p = torch.exp2(x - m)
    l = p.sum(-1, keepdim=True)
    o = ((_bf(p) @ v) / l).to(torch.bfloat16)
    lse2 = m + torch.log2(l)
    pb = torch.exp2(x - lse2)
    ds = pb * (g @ v.transpose(-1, -2) - (g * o.float()).sum(-1, keepdim=True))
    return {
        "O": o, "lse2": lse2[..., 0],
        "dQ": ((_bf(ds) @ k) * SCALE).to(torch.bfloat16),
        "dK": ((_bf(ds).transpose(-1, -2) @ q) * SCALE).to(torch.bfloat16),
        "dV": (_bf(pb).transpose(-1, -2) @ g).to(torch.bfloat16),
    }


def ratio(got, ref, a):
    """Worst |got - ref| / (2^-9 A) over the elements with A > 0: the figure behind EMU_RATIO, and what
    the tests print before they assert."""
    err = (got.double() - ref).abs()
    return float((err / (U * a).clamp_min(1e-300))[a > 0].max()) if bool((a > 0).any()) else 0.0


def check_bound(name, got, ref, a, c, errs, tag=""):
    """|got - ref| <= c 2^-9 A + 1e-12 max(A) for every element (NaN fails), all finite."""
    got = got.double()
    if not bool(torch.isfinite(got).all()):
        errs.append(f"{tag}{name}: {int((~torch.isfinite(got)).sum())} non-finite of {got.numel()}")
        return
    err = (got - ref).abs()
    bad = ~(err <= c * U * a + 1e-12 * a.max())
    if bool(bad.any()):
        i = torch.argmax(torch.where(bad, err / (U * a).clamp_min(1e-300), torch.zeros_like(err)))
        idx = tuple(int(j) for j in torch.unravel_index(i, err.shape))
        errs.append(f"{tag}{name}: {int(bad.sum())} of {got.numel()} outside c = {c}; worst at {idx}: got "
                    f"{float(got[idx]):.6g} ref {float(ref[idx]):.6g} A {float(a[idx]):.6g}")


def check_lse2(got, ref, errs):
    """2^-16 (1 + c2 max_k sum_d |q_d||k_d|): a 64-term fp32 dot errs by about 2^-18 of the sum of its
    absolute terms, with a 4x margin."""
    bad = ~((got.double() - ref["lse2"]).abs() <= 2.0 ** -16 * (1 + ref["lse2_cond"]))
    if bool(bad.any()):
        errs.append(f"lse2: {int(bad.sum())} of {got.numel()} outside the bound; worst error "
                    f"{float((got.double() - ref['lse2']).abs().max()):.3g}")


# ---------------------------------------------------------------------------------- CPU tests

def test_reference_gradient_is_autograd_cpu():
    """The closed-form float64 gradient of `reference` is the autograd gradient of its forward."""
    qkv, g = make_inputs("gaussian", 33, 2, 3)
    ref = reference(qkv, g, 3)
    x = qkv.double().requires_grad_()
    q, k, v, gd = _split(x, g, 3, torch.float64)
    o = torch.softmax((q @ k.transpose(-1, -2)) * SCALE, -1) @ v
    o.backward(gd)
    dq, dk, dv = x.grad.view(2, 33, 3, 3, 64).permute(2, 0, 3, 1, 4)
    for name, got in (("dQ", dq), ("dK", dk), ("dV", dv)):
        torch.testing.assert_close(got, ref[name], rtol=1e-10, atol=1e-12)
    torch.testing.assert_close(o, ref["O"], rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize("family", FAMILIES)
def test_emulation_within_half_c_cpu(family):
    """The bf16-staged emulation stays within c / 2 of the float64 reference: the bounds the GPU
    tests use leave the kernels twice the emulation's own error."""
    for t in T_EMU_CPU:
        qkv, g = make_inputs(family, t, 2, 3)
        ref, emu = reference(qkv, g, 3), emulate(qkv, g, 3)
        errs = []
        for name in ("O", "dQ", "dK", "dV"):
            r = ratio(emu[name], ref[name], ref["A_" + name])
            print(f"{family} T={t} {name}: emulation ratio {r:.3f} (c = {C[name]})")
            check_bound(name, emu[name], ref[name], ref["A_" + name], C[name] / 2, errs, tag=f"T={t} ")
        check_lse2(emu["lse2"], ref, errs)
        assert not errs, "\n".join(errs)


def test_bounds_constants_cpu():
    assert all(C[n] == math.ceil(2 * EMU_RATIO[n]) for n in C)


@pytest.mark.parametrize("t,b,h", SHAPES, ids=[f"T{t}-B{b}H{h}" for t, b, h in SHAPES])
def test_gather_precondition_cpu(t, b, h):
    """The gather family's claim for its seed: every weight off the match is below 2^-40, the exact
    output is the matched V row, dV the matched dO row, and dQ, dK vanish (below 2^-21)."""
    qkv, g = make_inputs("gather", t, b, h)
    ref = reference(qkv, g, h)
    assert ref["p_off_max"] < 2.0 ** -40, ref["p_off_max"]
    _, _, v, gd = _split(qkv, g, h, torch.float64)
    pi = _perm(t)
    assert float((ref["O"] - v[:, :, pi]).abs().max()) < 2.0 ** -24
    assert float((ref["dV"][:, :, pi] - gd).abs().max()) < 2.0 ** -24
    assert float(ref["dQ"].abs().max()) < 2.0 ** -21 and float(ref["dK"].abs().max()) < 2.0 ** -21
    rows = v.reshape(-1, 64)[:, :3]
    assert len({tuple(r) for r in rows.tolist()}) == rows.shape[0]  # V rows distinct per (b, h, t)


# ---------------------------------------------------------------------------------- GPU tests

def _run(qkv, g, heads):
    """Forward, backward, a second backward; outputs in the reference's [B, H, T, 64] layout."""
    from fluxmpi_amd.ops.attention import attn_bwd_packed, attn_fwd_packed, take_colpart
    b, t, _ = qkv.shape
    out, stats = attn_fwd_packed(qkv, heads)
    lse_before = stats[..., 0].clone()
    dqkv = attn_bwd_packed(qkv, out, g, heads, stats)
    part = take_colpart(dqkv.view(b * t, -1))
    dqkv2 = attn_bwd_packed(qkv, out, g, heads, stats)
    part2 = take_colpart(dqkv2.view(b * t, -1))
    dq, dk, dv = dqkv.view(b, t, 3, heads, 64).permute(2, 0, 3, 1, 4)
    return {"O": out.view(b, t, heads, 64).permute(0, 2, 1, 3), "dQ": dq, "dK": dk, "dV": dv, "stats": stats,
            "lse_before": lse_before, "dqkv": dqkv, "dqkv2": dqkv2, "part": part, "part2": part2}


@pytest.mark.gpu
@pytest.mark.parametrize("family,t,b,h", CASES, ids=[_id(*c) for c in CASES])
def test_attention_case(gpu_ext, family, t, b, h):
    """Forward and backward of one (family, shape) per element against float64; the column-sum
    partials against the reference gradient's column sums; lse2 not clobbered; deterministic."""
    qkv, g = (x.cuda() for x in make_inputs(family, t, b, h))
    ref = reference(qkv, g, h)
    got = _run(qkv, g, h)
    print(f"{_id(family, t, b, h)}: {gpu_ext.attn_dispatch(b, t, h)}")
    errs = []
    for name in ("O", "dQ", "dK", "dV"):
        print(f"  {name}: ratio {ratio(got[name], ref[name], ref['A_' + name]):.3f} (c = {C[name]})")
        check_bound(name, got[name], ref[name], ref["A_" + name], C[name], errs)
    check_lse2(got["stats"][..., 0], ref, errs)
    # the per-wave column sums (the packed QKV bias gradient), present exactly when the variant writes them
    rows = gpu_ext.attn_bwd_colpart_rows(b, t, h, 3 * h * 64, h * 64)
    if rows == 0:
        if got["part"] is not None:
            errs.append("take_colpart returned partials for a variant that writes none")
    elif got["part"] is None or tuple(got["part"].shape) != (rows, 3 * h * 64):
        errs.append(f"take_colpart: expected [{rows}, {3 * h * 64}] partials, got {got['part']}")
    else:
        sums = got["part"].double().sum(0).view(3, h, 64)
        for i, name in enumerate(("dQ", "dK", "dV")):
            check_bound(name, sums[i], ref[name].sum((0, 2)), ref["A_" + name].sum((0, 2)), C[name], errs,
                        tag="column sums of ")
        if not torch.equal(got["part"], got["part2"]):
            errs.append("column-sum partials differ between two identical backward calls")
    if not torch.equal(got["stats"][..., 0], got["lse_before"]):
        errs.append("the backward changed stats[..., 0]")
    if not torch.equal(got["dqkv"].view(torch.int16), got["dqkv2"].view(torch.int16)):
        errs.append("dQKV differs between two identical backward calls")
    assert not errs, "\n".join(errs)


GATHER = [(t, b, h) for (f, t, b, h) in CASES if f == "gather"]


@pytest.mark.gpu
@pytest.mark.parametrize("t,b,h", GATHER, ids=[_id("gather", *c) for c in GATHER])
def test_exact_gather(gpu_ext, t, b, h):
    """One-hot attention moves rows without arithmetic: out[b, i, h] is v[b, pi(i), h] and
    dV[b, pi(i), h] is dO[b, i, h] bit for bit, dQ and dK vanish. No tolerance: any row, head, batch or
    tile mapping error fails it."""
    qkv, g = (x.cuda() for x in make_inputs("gather", t, b, h))
    ref = reference(qkv, g, h)
    assert ref["p_off_max"] < 2.0 ** -40, ref["p_off_max"]  # the precondition, for this very input
    got = _run(qkv, g, h)
    pi = _perm(t).cuda()
    _, _, v, gd = _split(qkv, g, h, torch.bfloat16)
    bits = lambda x: x.contiguous().view(torch.int16)
    errs = []
    for name, a, e in (("out", got["O"], v[:, :, pi]), ("dV[pi]", got["dV"][:, :, pi], gd)):
        bad = (bits(a) != bits(e)).any(-1)
        if bool(bad.any()):
            errs.append(f"{name}: {int(bad.sum())} of {bad.numel()} rows differ, first (b, h, row) "
                        f"{tuple(int(j) for j in bad.nonzero()[0])}")
    for name in ("dQ", "dK"):
        x = got[name].float()
        if not bool((x.abs() <= 2.0 ** -20).all()):  # NaN fails
            errs.append(f"{name}: max |x| {float(x.abs().max()):.3g} above 2^-20")
    assert not errs, "\n".join(errs)


@pytest.mark.gpu
@pytest.mark.parametrize("t", [1, 17, 197, 257])
def test_guard_bands(gpu_ext, t):
    """The raw bindings with every operand in the middle of a larger allocation: NaN around the inputs,
    a sentinel bit pattern around the outputs. Results equal the packed wrappers' bit for bit and
    every sentinel survives."""
    from fluxmpi_amd.ops.attention import attn_bwd_packed, attn_fwd_packed
    from fluxmpi_amd.ops.fused_block import _stream
    b, h, pad = 2, 3, 4096  # elements on either side (a multiple of 8: the operands stay 16-byte aligned)
    d = h * 64
    qkv, g = (x.cuda() for x in make_inputs("gaussian", t, b, h))
    out_ref, stats_ref = attn_fwd_packed(qkv, h)
    dqkv_ref = attn_bwd_packed(qkv, out_ref, g, h, stats_ref, colsum=False)

    def banded_in(x):
        big = torch.full((x.numel() + 2 * pad,), float("nan"), device="cuda", dtype=x.dtype)
        big[pad:pad + x.numel()] = x.reshape(-1)
        return big, big[pad:pad + x.numel()].view(x.shape)

    def banded_out(shape, dtype):
        n = math.prod(shape)
        ints, pattern = (torch.int16, 0x5A5A) if dtype == torch.bfloat16 else (torch.int32, 0x5A5A5A5A)
        big = torch.full((n + 2 * pad,), pattern, device="cuda", dtype=ints)
        return big, big.view(dtype)[pad:pad + n].view(shape), pattern

    def intact(big, pattern, n):
        return bool((big[:pad] == pattern).all()) and bool((big[pad + n:] == pattern).all())

    _, xq = banded_in(qkv)
    _, xg = banded_in(g)
    out_big, out, s16 = banded_out((b, t, d), torch.bfloat16)
    stats_big, stats, s32 = banded_out((b, h, t, 2), torch.float32)
    dq_big, dqkv, _ = banded_out((b, t, 3 * d), torch.bfloat16)
    p, es, st = xq.data_ptr(), 2, _stream(qkv)
    gpu_ext.attn_fwd(p, p + d * es, p + 2 * d * es, out.data_ptr(), stats.data_ptr(), t * 3 * d, 3 * d, t * d, d, 64,
                     b, t, h, 64, SCALE, st)
    assert intact(out_big, s16, out.numel()) and intact(stats_big, s32, stats.numel())
    assert torch.equal(out.view(torch.int16), out_ref.view(torch.int16))
    assert torch.equal(stats[..., 0], stats_ref[..., 0])
    _, xo = banded_in(out_ref)
    q = dqkv.data_ptr()
    gpu_ext.attn_bwd(p, p + d * es, p + 2 * d * es, xo.data_ptr(), xg.data_ptr(), q, q + d * es, q + 2 * d * es,
                     stats.data_ptr(), t * 3 * d, 3 * d, t * d, d, 64, t * d, d, b, t, h, 64, SCALE, st)
    torch.cuda.synchronize()
    assert intact(dq_big, s16, dqkv.numel()) and intact(stats_big, s32, stats.numel())
    assert intact(out_big, s16, out.numel())
    assert torch.equal(dqkv.view(torch.int16), dqkv_ref.view(torch.int16))
    assert torch.equal(stats[..., 0], stats_ref[..., 0])


# ------------------------------------------------------------------- dispatch and the variants

FWD0, FWD13, FWDB = "attn_fwd_res_kernel<0>", "attn_fwd_res_kernel<13>", "attn_fwd_kernel"
PAIR0 = "attn_bwd_dq_res_kernel<0>+attn_bwd_dkv_res_kernel<0,0>"
PAIR13 = "attn_bwd_dq_res_kernel<13>+attn_bwd_dkv_res_kernel<13,0>"
PAIR13P = "attn_bwd_dq_res_kernel<13>+attn_bwd_dkv_res_kernel<13,1>"
FUSED, BWDB = "attn_bwd_fused_kernel<13>", "attn_bwd_dq_kernel+attn_bwd_dkv_kernel"
SWITCHES = ("FLUXMPI_ATTN_FWD", "FLUXMPI_ATTN_BWD", "FLUXMPI_ATTN_GENERIC", "FLUXMPI_ATTN_DKV_PIPE",
            "FLUXMPI_ATTN_PARTS", "FLUXMPI_ATTN_FWD_PARTS")
# name: (environment, {T: attn_dispatch(2, T, 3)})
CONFIGS = {
    "default": ({}, {197: (FWD13, FUSED, 2, 1), 64: (FWD0, PAIR0, 2, 2), 257: (FWDB, BWDB, 5, 5)}),
    "pair": ({"FLUXMPI_ATTN_BWD": "pair"}, {197: (FWD13, PAIR13P, 2, 2), 209: (FWD0, PAIR0, 2, 2)}),
    "pair_nopipe": ({"FLUXMPI_ATTN_BWD": "pair", "FLUXMPI_ATTN_DKV_PIPE": "0"},
                    {197: (FWD13, PAIR13, 2, 2), 193: (FWD13, PAIR13, 2, 2)}),
    "generic": ({"FLUXMPI_ATTN_GENERIC": "1"}, {197: (FWD0, PAIR0, 2, 2), 208: (FWD0, PAIR0, 2, 2)}),
    "blocked": ({"FLUXMPI_ATTN_FWD": "blocked", "FLUXMPI_ATTN_BWD": "blocked"},
                {197: (FWDB, BWDB, 4, 4), 17: (FWDB, BWDB, 1, 1)}),
    "parts1": ({"FLUXMPI_ATTN_BWD": "pair", "FLUXMPI_ATTN_PARTS": "1", "FLUXMPI_ATTN_FWD_PARTS": "1"},
               {197: (FWD13, PAIR13P, 1, 1), 256: (FWD0, PAIR0, 1, 1)}),
    "parts3": ({"FLUXMPI_ATTN_BWD": "pair", "FLUXMPI_ATTN_PARTS": "3", "FLUXMPI_ATTN_FWD_PARTS": "3"},
               {197: (FWD13, PAIR13P, 3, 3), 17: (FWD0, PAIR0, 2, 2)}),
    "parts16": ({"FLUXMPI_ATTN_BWD": "pair", "FLUXMPI_ATTN_PARTS": "16", "FLUXMPI_ATTN_FWD_PARTS": "16"},
                {197: (FWD13, PAIR13P, 13, 13), 256: (FWD0, PAIR0, 16, 16)}),
}
ALL_KERNELS = {FWDB, FWD0, FWD13, "attn_bwd_dq_kernel", "attn_bwd_dkv_kernel", "attn_bwd_dq_res_kernel<0>",
               "attn_bwd_dq_res_kernel<13>", "attn_bwd_dkv_res_kernel<0,0>", "attn_bwd_dkv_res_kernel<13,0>",
               "attn_bwd_dkv_res_kernel<13,1>", FUSED}


def test_configs_name_every_kernel_cpu():
    named = set()
    for _, expect in CONFIGS.values():
        for fwd, bwd, _, _ in expect.values():
            named |= {fwd, *bwd.split("+")}
    assert named == ALL_KERNELS


@pytest.mark.gpu
def test_dispatch(gpu_ext):
    """attn_dispatch names the kernels this process's switches select (the launchers take their
    choice from the same function), and the column-sum rows follow it."""
    env = {k: os.environ[k] for k in SWITCHES if k in os.environ}
    hit = [name for name, (e, _) in CONFIGS.items() if e == env]
    if not hit:
        pytest.skip(f"switch combination {env} is not one of CONFIGS")
    for t, expect in CONFIGS[hit[0]][1].items():
        got = gpu_ext.attn_dispatch(2, t, 3)
        assert tuple(got) == expect, (hit[0], t, got)
        waves = 13 if got[1] == FUSED else -(-((t + 15) // 16) // got[3])
        rows = 0 if got[1] == BWDB else 2 * got[3] * waves
        assert gpu_ext.attn_bwd_colpart_rows(2, t, 3, 576, 192) == rows


CHILD_K = ("test_dispatch or ((test_attention_case or test_exact_gather) and (gaussian or offneg or gather) and ("
           + " or ".join(f"T{t}-B2H3" for t in T_CHILD) + "))")


@pytest.mark.gpu
@pytest.mark.parametrize("config", [c for c in CONFIGS if c != "default"])
def test_variant(gpu_ext, config):
    """This file's dispatch, value and gather tests at the boundary T, in a fresh interpreter whose
    switches (read once per process by the native library) select another set of kernels."""
    if CHILD:
        pytest.skip("a child process spawns no children")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(CONFIGS[config][0], FLUXMPI_ATTN_EDGES_CHILD="1")
    cmd = [sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
           os.path.join(root, "tests", "test_attention_edges_gpu.py"), "-k", CHILD_K]
    try:
        r = subprocess.run(cmd, env=env, cwd=root, capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired as e:
        pytest.exit(f"attention variant {config}: the child process hung: {str(e.stdout)[-2000:]}", returncode=1)
    tail = r.stdout[-3000:] + r.stderr[-3000:]
    if r.returncode < 0:
        pytest.exit(f"attention variant {config}: the child process died of signal {-r.returncode}: {tail}",
                    returncode=1)
    assert r.returncode == 0, tail
    assert " skipped" not in r.stdout.splitlines()[-1], tail  # the child's dispatch test knew its configuration
