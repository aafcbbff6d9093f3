"""The normalisation and pooling kernels (batchnorm.hip, layernorm.hip, groupnorm.hip, pool.hip) per
element against float64 references: derived bounds (``norm_edges``' docstring writes out every term),
exact integer families, guard bands around every output, the BatchNorm workspace invariant, and a CPU
half that shows the bounds hold for a float32 evaluation of the kernels' formulas in the worst
summation order of the geometry and that planted defects trip the same checkers.

Input families (``norm_edges.rows_inputs``; seeded, made on the CPU):
    uniform      x, res in [-2, 2), dy in [-1, 1), w in +-[0.5, 1.5), |b| in [2^-4, 1)
    offset       uniform plus mean / std = 4, 32 (and 256 for fp32) per channel / row / group: the
                 single-pass variance's kappa = (mean^2 + var) / var term (none for LayerNorm)
    constant     a channel / row / group of one value (variance exactly 0); constant1000 adds a channel at
                 1000, where E[x^2] - mean^2 may come out negative and is clamped (run without a ReLU)
    integer      x balanced in {+-1, +-2}, dy in {-2 .. 2}, res in {-2, 0, 2}, w = +-1, b = 0.25, rows a
                 power of two: every sum is an integer below 2^24, so save_mean is fl(s fl(1 / n)) exactly,
                 save_invstd and the running statistics are within 2 ulp of the float32 evaluation, db is
                 EQUAL to the integer sum, dres = dy (y > 0) and the mask bytes are the bits of y > 0
    fp16 underflow   bn_apply + ReLU + residual in fp16 with pre-activations of exactly 2^-26 (y rounds to 0,
                 the mask bit is set), 1.25 * 2^-24 (y is the smallest subnormal) and +-0.5

Kernel / template variants and the cases that reach them (geometry asserted in the tests from
``norm_edges.bn_geometry`` / ``ln_vpl`` / ``gn_pl``, the documented formulas):

    batchnorm.hip  (test_bn_raw[group-key-dtype] walks ``BN_GROUPS``; T = bf16 / fp16 / fp32 everywhere)
      bn_stats_kernel<T>, bn_bwd_reduce_kernel<T, RM>  one row (1, 8); tail loop only (37, 8); two blocks,
        unrolled loop + tail (4100, 8); idle lane 255 (301, 24); idle lanes 129 .. 255 (33, 1032); rpi = 1
        (50, 2040), (277, 2048); 18 blocks, so the shards wrap: (277, 2048) and, exactly, the integer
        (512, 2048); RM 0 none / res, RM 1 raw y pointer, RM 2 recompute, RM 3 saved bits (RM 2 and RM 3 must
        give bit-equal dres, and equal dx / dw / db in the integer family)
      bn_norm_kernel<T, RELU, RES, FIXED>, bn_bwd_dx_kernel<T, RM, DRES, FIXED>  the four modes at FIXED
        (8, 64, 128, 2048) and LDS-coefficient (24, 96, 1032, 2040) channel counts; U = 2 loop and tail: an
        odd vector count (37, 8), (301, 24); several grid-stride iterations: every shape of more than 1024
        vectors; grid capped at the resident workgroups: test_bn_large (32 M elements)
      null w / b (stand-in array), null running statistics   the "null" group
      bn_finalize_fwd_kernel scale / shift outputs, bn_apply  test_bn_stats_finalize_apply
      bn_norm_dual_kernel, bn_bwd_reduce_dual_kernel, bn_bwd_dx_dual_kernel  test_bn_dual (C = 8, 256, 2048;
        nvec 1, odd, even), test_bn_dual_refuses_non_fixed
      eval (train = 0: rsqrt(running_var + eps))     test_bn_infer (running_var 0 and 1e-12 included)
      fp16 underflow of y under a set mask bit       test_bn_fp16_underflow
      wrappers                                       test_bn_wrappers (4-D channels_last (2, 64, 7, 9), 2-D
                                                     (64, 128), momentum=None, affine=False, eval, masked
                                                     GradLink, bn_from_stats, dual_bn_relu)
      workspace                                      zero after EVERY raw call above (all 64 shards, guard
                                                     bands intact); test_bn_workspace_sequence runs
                                                     C = 2048 -> 8 -> 1032 -> 24 -> 2048 on one workspace
    layernorm.hip  ln_fwd_kernel<T, ADD, VPL, A>, ln_bwd_kernel<T, DH, VPL, A, CS>
      VPL 1 (8, 64, 512), 2 (520, 768), 3 (1032), 4 (2048), 6 (2056, 3072), 8 (4096), 12 (4104, 6144),
      16 (8184, 8192): test_ln_raw; slots inactive in all lanes: 4104 (VPL 12, 9 vectors per lane: slots
      9 .. 11); prefetch on (VPL <= 4) and off; ADD / DH / CS on and off; A = T, fp32, absent (ones / zeros);
      several rows per wave: test_ln_rows_per_wave (asserted against the returned block count) and the
      max_blocks = 2 case of test_ln_raw; offsets / constant rows / integers: test_ln_families; autograd
      wrappers incl. linear_add_layer_norm's column sums: test_ln_wrappers
    groupnorm.hip  gn_fwd_kernel<T, ADD, RELU, SAVEH>, gn_bwd_kernel<T, RELU>  test_gn_raw at GN_SHAPES:
      HW = 1; a group boundary inside a vector (48 / 8); one channel per group; one pixel lane (2048);
      kU loop + tail (33 x 31); HW < PL; the out= slot with a sample stride; w / b null; test_gn_families;
      FusedGroupNorm: test_gn_module
    pool.hip  bn_relu_maxpool_fwd_kernel<T, KK = 3 | 0>, maxpool_bwd_gather_kernel<T, NW = 1, 2, 3>
      test_pool_exact at POOL_SHAPES (bf16 K = 3 compiled window and, by FLUXMPI_POOL_GENERIC, the loop;
      fp16 / fp32 always the loop); test_pool_end_to_end; test_pool_unsupported_geometry

Measured on the MI355X (one run of the whole suite). Worst |err| / bound per kernel file: batchnorm.hip 0.997
(an fp16 eval output), layernorm.hip 0.996 (a bf16 dx), groupnorm.hip 0.993 (a bf16 y), pool.hip exact
(end to end under the BatchNorm bounds 0.968): the output rounding u_T |y| dominates every bound, so a ratio
just under 1 is what a correctly rounded store gives. The statistics themselves stay far inside:
save_invstd at most 0.05 of its bound. Most undecided ReLU elements in one case: 51 of 65568 (0.078 %, offset
32, fp16, ReLU + residual) against the 0.1 % cap. No kernel exceeded a derived bound; the float32
emulation found the one term the first derivation lacked (fp16 subnormal spacing). Wall time: the 228 GPU
tests of this file 17 s, next to 98 s for the rest of the GPU suite (114.9 s together).
"""
import math

import pytest
import torch
import torch.nn.functional as F

from . import mfma_edges as E
from . import norm_edges as N
from .norm_edges import TINY, U32, UT

gpu = pytest.mark.gpu
DT = [torch.bfloat16, torch.float16, torch.float32]
DT_IDS = ["bf16", "fp16", "fp32"]
MODES = {"none": (0, False), "relu": (1, False), "relu_res": (1, True), "res": (0, True)}


# =============================================================================== CPU half

BN_CPU = [("uniform", 0, 301, 24), ("uniform", 0, 4100, 8), ("uniform", 0, 33, 1032), ("offset", 4, 683, 96),
          ("offset", 32, 683, 96), ("offset", 256, 683, 96), ("constant", 0, 301, 24), ("constant1000", 0, 64, 128),
          ("integer", 0, 64, 24), ("integer", 0, 512, 2048)]


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
def test_unit_roundoffs_cpu(dtype):
    """``UT``: the worst relative error of rounding [1, 1 + 2^-6) to each format is reached to within 1 % and never
    exceeded (bf16 has 8 significand bits with the implicit one: 2^-8, not 2^-9)."""
    x = 1 + torch.rand(1 << 20, dtype=torch.float64, generator=N._g("roundoff")) * 2.0 ** -6
    rel = ((x.float().to(dtype).double() - x).abs() / x).max() if dtype != torch.float32 else \
        ((x.float().double() - x).abs() / x).max()
    assert 0.99 * UT[dtype] < float(rel) <= UT[dtype]


def _modes_of(family, ratio, rows, C):
    """The ReLU modes are left out where the forward bound itself swallows the pre-activations, so that the
    reference alone would break the 0.1 % cap: a constant channel at 1000 (dz > |b| on the whole channel), and
    offsets whose first-order invstd bound kappa (L + 3) 2^-23 / 2, kappa = 1 + ratio^2, reaches 0.5 % (then
    |z| <= dz on a band of that relative width around z = 0): ratio 256 everywhere, ratio 32 at (4100, 8)."""
    eps_inv = (1 + ratio * ratio) * (N.bn_L(rows, C) + 3) * N.E23 / 2
    return ("none", "res") if (family == "constant1000" or eps_inv >= 5e-3) else tuple(MODES)


def _ws_zero(tag, ws, errs):
    if int(torch.count_nonzero(ws)):
        errs.append(f"{tag}: {int(torch.count_nonzero(ws))} workspace floats left non-zero")


def _bn_cpu_case(family, ratio, rows, C, dtype, mode, defect=None, bwd_defect=None, affine_on=True, ws=None,
                 calls=1):
    relu, use_res = MODES[mode]
    inp = N.rows_inputs(family, rows, C, dtype, ratio)
    errs = []
    ws = torch.zeros(16, 2, C) if ws is None else ws
    run0 = (torch.full((C,), 0.25), torch.full((C,), 0.75))
    for call in range(calls):
        tag = f"cpu {family}{ratio} ({rows}, {C}) {mode} call {call}"
        out = N.bn_emulate_fwd(inp, relu, use_res, affine_on, dtype, ws, run0, defect=defect if call == 0 else None)
        _ws_zero(tag, ws, errs)
        N.bn_check_fwd(tag, inp, out, relu, use_res, affine_on, dtype, errs, running=run0,
                       exact=family == "integer")
    g32 = inp["dy"].float() * (N.mask_bits(out["mask"], (rows, C)) if relu else 1)
    back = N.bn_emulate_bwd(inp, out["mean"], out["inv"], g32, affine_on, dtype, ws, bwd_defect)
    _ws_zero(tag + " bwd", ws, errs)
    N.bn_check_bwd(tag + " bwd", inp, back, out["mean"], out["inv"], g32.double(), affine_on, dtype, errs,
                   exact=family == "integer")
    return errs


def _with_dtypes(cases):
    """(case..., dtype) for the three dtypes; mean / std = 256 (the second entry) is an fp32-input case."""
    return [(*c, d) for c in cases for d in DT if not (c[1] == 256 and d != torch.float32)]


def _ids(cases):
    return ["-".join(str(v).replace("torch.", "") for v in c) for c in cases]


@pytest.mark.parametrize("family,ratio,rows,C,dtype", _with_dtypes(BN_CPU), ids=_ids(_with_dtypes(BN_CPU)))
def test_bn_emulation_meets_bounds_cpu(family, ratio, rows, C, dtype):
    """batchnorm.hip's formulas in float32 (lanes, workgroups, shards and finalize summed one addition at
    a time) stay inside the derived bounds, the exact family's exact facts hold, and the references keep
    the undecided ReLU elements under the cap."""
    for mode in _modes_of(family, ratio, rows, C):
        errs = _bn_cpu_case(family, ratio, rows, C, dtype, mode)
        assert not errs, "\n".join(errs)


def _ln_inputs(family, rows, D, dtype, ratio=0):
    t = N.rows_inputs(family, D, rows, dtype, ratio)
    g = N._g("ln-affine", D)
    w, b = N.affine(g, D)
    if family == "integer":
        w, b = N._sign(g, (D,)), torch.full((D,), 0.25)
    return dict(x=t["x"].t().contiguous(), r=t["res"].t().contiguous(), dy=t["dy"].t().contiguous(), w=w, b=b)


LN_CPU = [("uniform", 0, 5, 520), ("offset", 32, 3, 1032), ("offset", 256, 3, 64), ("constant", 0, 9, 8),
          ("integer", 0, 4, 768)]


@pytest.mark.parametrize("family,ratio,rows,D,dtype", _with_dtypes(LN_CPU), ids=_ids(_with_dtypes(LN_CPU)))
def test_ln_emulation_meets_bounds_cpu(family, ratio, rows, D, dtype):
    """layernorm.hip's forward in float32 with its lane layout: no kappa term is needed at any offset."""
    inp = _ln_inputs(family, rows, D, dtype, ratio)
    for add in (False, True):
        errs = []
        out = N.ln_emulate_fwd(inp["x"], inp["r"] if add else None, inp["w"], inp["b"], dtype)
        tag = f"cpu ln {family}{ratio} ({rows}, {D}) add={add}"
        N.ln_check_fwd(tag, out["h"], inp["w"], inp["b"], out, dtype, errs)
        dh = inp["r"] if add else None
        back = N.ln_emulate_bwd(inp["dy"], out["h"], out["mean"], out["rstd"], inp["w"], dh, dtype)
        N.ln_check_bwd(tag, inp["dy"], out["h"], out["mean"], out["rstd"], inp["w"], dh, back, dtype, errs,
                       exact=family == "integer")
        assert not errs, "\n".join(errs)


def _gn_inputs(family, n, hw, c, g, dtype, ratio=0):
    """x, a, dy [n, hw, c]: the per-group statistics of sample i run over (hw, c / g); the offset family is
    positive so that it survives a ReLU."""
    gen = N._g("gn", family, n, hw, c, g, str(dtype), ratio)
    cpg = c // g
    if family == "integer":
        assert (hw * cpg) % 4 == 0
        x = N.balanced(gen, hw * cpg, n * g).t().reshape(n, g, hw, cpg).permute(0, 2, 1, 3).reshape(n, hw, c)
        a = (torch.randint(0, 3, (n, hw, c), generator=gen) - 1).float() * 2
        dy = (torch.randint(0, 5, (n, hw, c), generator=gen) - 2).float()
        w, b = N._sign(gen, (c,)), torch.full((c,), 0.25)
    else:
        x, a, dy = N._uni(gen, (n, hw, c), -2, 2), N._uni(gen, (n, hw, c), -0.5, 0.5), N._uni(gen, (n, hw, c), -1, 1)
        w, b = N.affine(gen, c)
        grp = torch.arange(c) // cpg
        if family == "offset":
            x = x + ratio * N.X_STD * (1 + grp % 2).float()
        elif family == "constant":
            x[:, :, grp == 0] = 3.0
            a[:, :, grp == 0] = 0.5
    return dict(x=x.to(dtype), a=a.to(dtype), dy=dy.to(dtype), w=w, b=b)


GN_CPU = [("uniform", 0, (2, 9, 48, 8)), ("offset", 32, (2, 15, 520, 5)), ("offset", 256, (3, 35, 16, 4)),
          ("constant", 0, (2, 9, 48, 8)), ("integer", 0, (2, 4, 2048, 64))]


@pytest.mark.parametrize("family,ratio,shape,dtype", _with_dtypes(GN_CPU), ids=_ids(_with_dtypes(GN_CPU)))
def test_gn_emulation_meets_bounds_cpu(family, ratio, shape, dtype):
    n, hw, c, g = shape
    inp = _gn_inputs(family, n, hw, c, g, dtype, ratio)
    for add, relu in ((False, False), (True, True)):
        errs = []
        h = N.gn_h(inp["x"], inp["a"] if add else None, relu)
        out = N.gn_emulate_fwd(h, inp["w"], inp["b"], g, dtype)
        tag = f"cpu gn {family}{ratio} {shape} add={add} relu={relu}"
        N.gn_check_fwd(tag, h, inp["w"], inp["b"], g, out, dtype, errs)
        back = N.gn_emulate_bwd(inp["dy"], h, out["mean"], out["rstd"], inp["w"], g, relu, dtype)
        N.gn_check_bwd(tag, inp["dy"], h, out["mean"], out["rstd"], inp["w"], g, relu, back, dtype, errs,
                       exact=family == "integer")
        assert not errs, "\n".join(errs)


DEFECTS = ["drop_last_row", "stale_shard", "coef_off_by_vector", "biased_running_var", "mask_reversed",
           "relu_before_residual", "truncate", "masked_lane_counted", "group_per_vector", "last_max", "border_wrap",
           "no_mean_dy"]


def _defect_errs(defect):
    """The checker's complaints for one planted defect (None: the same scenario without it)."""
    bn = {"drop_last_row": ("uniform", 301, 24, torch.float32, "none"),
          "stale_shard": ("uniform", 277, 2048, torch.float32, "none"),
          "coef_off_by_vector": ("uniform", 301, 24, torch.float32, "none"),
          "biased_running_var": ("integer", 64, 8, torch.float32, "none"),
          "mask_reversed": ("uniform", 301, 24, torch.bfloat16, "relu"),
          "relu_before_residual": ("uniform", 301, 24, torch.bfloat16, "relu_res"),
          "truncate": ("uniform", 301, 24, torch.bfloat16, "none")}

    def run(name, on):
        if name in bn:
            family, rows, C, dtype, mode = bn[name]
            return _bn_cpu_case(family, 0, rows, C, dtype, mode, defect=name if on else None,
                                calls=2 if name == "stale_shard" else 1)
        if name == "no_mean_dy":
            return _bn_cpu_case("uniform", 0, 301, 24, torch.float32, "none", bwd_defect=name if on else None)
        errs = []
        if name == "masked_lane_counted":
            inp = _ln_inputs("uniform", 5, 520, torch.float32)
            out = N.ln_emulate_fwd(inp["x"], None, inp["w"], inp["b"], torch.float32, defect=name if on else None)
            N.ln_check_fwd(name, out["h"], inp["w"], inp["b"], out, torch.float32, errs)
        elif name == "group_per_vector":
            inp = _gn_inputs("uniform", 2, 9, 48, 8, torch.float32)
            out = N.gn_emulate_fwd(inp["x"], inp["w"], inp["b"], 8, torch.float32, defect=name if on else None)
            N.gn_check_fwd(name, inp["x"], inp["w"], inp["b"], 8, out, torch.float32, errs)
        else:  # pool: the reference with the defect against the reference
            x, sc, sh = N.pool_inputs(2, 8, 7, 5, torch.float32)
            y, idx = N.pool_ref(x, sc, sh, 3, 2, 1, defect=name if on else None)
            N.pool_check(name, y, idx, x, sc, sh, 3, 2, 1, errs)
        return errs

    return run


@pytest.mark.parametrize("defect", DEFECTS)
def test_planted_defect_fails_cpu(defect):
    run = _defect_errs(defect)
    clean = run(defect, False)
    assert not clean, "\n".join(clean)
    errs = run(defect, True)
    print("\n".join(errs))
    assert errs, f"the checker did not notice the planted defect {defect}"


def test_pool_reference_properties_cpu():
    """The pool inputs have ties in most windows, whole windows <= 0 and a fully blocked channel, and the
    backward reference conserves the gradient per channel."""
    x, sc, sh = N.pool_inputs(2, 8, 9, 11, torch.float32)
    y, idx = N.pool_ref(x, sc, sh, 3, 1, 1)
    z = F.pad((x * sc + sh).permute(0, 3, 1, 2), (1, 1, 1, 1), value=-math.inf)
    win = F.unfold(z, 3).view(2, 8, 9, -1)
    ties = ((win == win.max(2, keepdim=True).values).sum(2) > 1).float().mean()
    assert float(ties) > 0.3 and bool((idx == 255).any()) and bool((idx[..., 0] == 255).all())
    assert bool((idx[:, 0, 0, 1:] != 255).any()) or bool((idx[:, 0, 0] == 255).all())
    dy = torch.randint(-3, 4, y.shape).float()
    dz = N.pool_bwd_ref(dy, idx, 9, 11, 3, 1, 1)
    assert torch.equal(dz.sum((0, 1, 2)), (dy.double() * (idx != 255)).sum((0, 1, 2)))


def test_pool_geometry_supported_cpu():
    """Geometries the backward cannot run are not 'supported', so the forward takes the reference path."""
    from fluxmpi_amd.ops.pool import geometry_supported
    assert geometry_supported(3, 2, 1) and geometry_supported(2, 2, 0) and geometry_supported(3, 1, 1)
    assert geometry_supported(3, 3, 0) and geometry_supported(15, 5, 7)
    assert not geometry_supported(4, 1, 1)      # ceil(K / S) = 4
    assert not geometry_supported(16, 8, 0)     # K * K > 255
    assert not geometry_supported(3, 2, 3)      # P >= K
    assert not geometry_supported(7, 2, 3)      # ceil(7 / 2) = 4


def test_geometry_reaches_paths_cpu():
    """The chosen shapes reach the paths they are listed for (documented geometry formulas)."""
    g = N.bn_geometry
    assert g(1, 8)[3] == 1 and g(37, 8)[2] // g(37, 8)[1] == 1                     # one row per lane: tail only
    cv, rpi, rpb, blocks = g(4100, 8)
    assert blocks == 2 and rpb // rpi >= 9 and (rpb // rpi) % 8 != 0                # U = 8 loop, then the tail
    assert g(301, 24)[0] * g(301, 24)[1] == 255 and not N.bn_fixed(24)              # lane 255 idle, LDS coefficients
    assert g(33, 1032)[1] == 1 and g(33, 1032)[0] == 129 and not N.bn_fixed(1032)   # lanes 129 .. 255 idle
    assert not N.bn_fixed(96) and not N.bn_fixed(2040) and N.bn_fixed(2048) and N.bn_fixed(64) and N.bn_fixed(128)
    assert g(277, 2048)[3] == 18 and g(512, 2048)[3] == 32                          # > 16 blocks: the shards wrap
    assert 301 * 24 // 8 % 2 == 1 and 37 % 2 == 1                                   # an odd vector count: U = 2 tail
    assert 131072 * 256 >= 32 * 2 ** 20 and 131072 * 256 // 8 // 1024 > 2048        # more blocks wanted than resident
    assert [N.ln_vpl(d) for d in LN_D] == [1, 1, 1, 2, 2, 3, 4, 6, 6, 8, 12, 12, 16, 16]
    assert N.ceil_div(4104 // 8, 64) == 9 and N.ln_vpl(4104) == 12                  # slots 9 .. 11 inactive everywhere
    assert 520 // 8 % 64 == 1 and 8184 // 8 % 64 == 63                              # masked lanes in the last slot
    assert (48 // 8) % 8 != 0 and N.gn_pl(2048, 64) == 1 and N.gn_pl(8, 1) == 256   # boundary in a vector; 1 pixel lane
    assert N.gn_pl(24, 3) == 85 and 33 * 31 > 4 * 85 and (33 * 31) % (4 * 85) != 0  # kU loop plus tail
    assert 9 < N.gn_pl(48, 8) and 35 < N.gn_pl(16, 4)                               # HW < PL: idle pixel lanes
    nw = {(k, s): -(-k // s) for _, _, _, _, k, s, _ in POOL_SHAPES}
    assert nw[3, 1] == 3 and nw[3, 2] == 2 and nw[2, 2] == 1 and nw[3, 3] == 1      # every NW of the backward gather
    assert ((20 + 2 - 3) // 2 + 1) * (1024 // 8) > 1024                             # more lane-slots than one workgroup


# =============================================================================== GPU: shared plumbing

LN_D = [8, 64, 512, 520, 768, 1032, 2048, 2056, 3072, 4096, 4104, 6144, 8184, 8192]
WS_FLOATS = 64 * 2 * 2048


def _code(dtype):
    from fluxmpi_amd.ops.multi_tensor import DTYPE_CODE
    return DTYPE_CODE[dtype]


def _st():
    return torch.cuda.current_stream().cuda_stream


def _cuda(d):
    return {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in d.items()}


def _act(rows, C, dtype):
    return E.guarded(rows, C, C, dtype, "cuda")


def _ch(C, init=None):
    buf, view = E.guarded(1, C, C + 8, torch.float32, "cuda")
    if init is not None:
        view.copy_(init.view(1, C))
    return buf, view


def _new_ws():
    return E.guarded(1, WS_FLOATS, WS_FLOATS + 64, torch.float32, "cuda", fill=0.0)


def _ws_check(tag, ws, errs):
    """The whole workspace (all 64 shards of the widest layout) is exactly zero and its guards are intact."""
    buf, view = ws
    nz = int(torch.count_nonzero(view.view(torch.int32)))
    if nz:
        errs.append(f"{tag}: {nz} workspace floats are not +0 after the call")
    E.take_guarded(f"{tag} workspace", buf, view, errs)
    view.zero_()


def _p(t):
    return t.data_ptr() if t is not None else 0


def _bn_fwd(ext, tag, inp, relu, use_res, affine_on, running, dtype, ws, errs, exact=False, want_mask=True,
            eps=1e-5, momentum=0.1):
    x = inp["x"]
    rows, C = x.shape
    y, sm, si = _act(rows, C, dtype), _ch(C), _ch(C)
    mask = N.guarded_bytes(rows * C // 8, "cuda") if (relu and want_mask) else None
    run0 = rm = rv = None
    if running:
        run0 = (torch.linspace(-1, 1, C, device="cuda"), torch.linspace(0.5, 2, C, device="cuda"))
        rm, rv = _ch(C, run0[0]), _ch(C, run0[1])
    nbt = torch.tensor([5], dtype=torch.int64, device="cuda")
    ext.bn_fwd_train(x.data_ptr(), y[1].data_ptr(), _p(inp["res"]) if use_res else 0,
                     _p(inp["w"]) if affine_on else 0, _p(inp["b"]) if affine_on else 0,
                     rm[1].data_ptr() if running else 0, rv[1].data_ptr() if running else 0, sm[1].data_ptr(),
                     si[1].data_ptr(), ws[1].data_ptr(), rows, C, momentum, eps, relu,
                     mask[1].data_ptr() if mask else 0, _code(dtype), _st(), nbt.data_ptr())
    _ws_check(tag, ws, errs)
    if int(nbt) != 6:
        errs.append(f"{tag}: num_batches_tracked went from 5 to {int(nbt)}")
    out = dict(y=E.take_guarded(f"{tag} y", *y, errs), mean=E.take_guarded(f"{tag} save_mean", *sm, errs)[0],
               inv=E.take_guarded(f"{tag} save_invstd", *si, errs)[0])
    if mask:
        out["mask"] = N.take_bytes(f"{tag} mask", *mask, errs)
    if running:
        out["rm"], out["rv"] = (E.take_guarded(f"{tag} running", *t, errs)[0] for t in (rm, rv))
    z, dz, und = N.bn_check_fwd(tag, inp, out, relu, use_res, affine_on, dtype, errs, eps, momentum, run0, exact)
    return out, und


def _bn_bwd(ext, tag, inp, fwd, rm, use_dres, affine_on, dtype, ws, errs, exact=False):
    """One raw bn_bwd in ReLU mode ``rm`` (0 none, 1 from the y pointer, 2 recomputed, 3 saved bits) on the
    forward's stored statistics; the reference's dy_eff follows the same stored input."""
    x, dy = inp["x"], inp["dy"]
    rows, C = x.shape
    mean, inv = fwd["mean"].contiguous(), fwd["inv"].contiguous()
    und = None
    if rm == 0:
        g = dy.double()
    elif rm == 1:
        g = dy.double() * (fwd["y"].float() > 0)
    elif rm == 3:
        g = dy.double() * N.mask_bits(fwd["mask"], (rows, C))
    else:
        zero = torch.zeros((), dtype=torch.float64, device="cuda")
        w, b = (inp["w"], inp["b"]) if affine_on else (None, None)
        z2, _, dz2, _ = N.affine_fwd_ref(x, w, b, None, True, mean.double(), inv.double(), zero, zero, dtype)
        und = N.undecided(z2, dz2, tag, errs)
        g = dy.double() * (z2 > 0)
    dx, dres = _act(rows, C, dtype), _act(rows, C, dtype) if use_dres else None
    dw, db = _ch(C), _ch(C)
    yk, mk = (fwd["y"].contiguous() if rm == 1 else None), (fwd["mask"].contiguous() if rm == 3 else None)
    ext.bn_bwd(dy.data_ptr(), x.data_ptr(), _p(yk), _p(mk), _p(inp["w"]) if affine_on else 0,
               _p(inp["b"]) if affine_on else 0, mean.data_ptr(), inv.data_ptr(), dx[1].data_ptr(),
               dres[1].data_ptr() if use_dres else 0, dw[1].data_ptr(), db[1].data_ptr(), ws[1].data_ptr(), rows, C,
               int(rm != 0), _code(dtype), _st(), 0)
    _ws_check(tag, ws, errs)
    out = dict(dx=E.take_guarded(f"{tag} dx", *dx, errs), dw=E.take_guarded(f"{tag} dw", *dw, errs)[0],
               db=E.take_guarded(f"{tag} db", *db, errs)[0])
    if use_dres:
        out["dres"] = E.take_guarded(f"{tag} dres", *dres, errs)
    N.bn_check_bwd(tag, inp, out, mean, inv, g, affine_on, dtype, errs, und, exact)
    return out


BWD_OF = {"none": [(0, False)], "res": [(0, True)], "relu": [(2, True), (3, True), (1, False)],
          "relu_res": [(3, True), (1, True), (3, False)]}  # (3, False): the masked GradLink hand-over, no dres


def _bn_reference_only(inp, family, ratio, dtype, errs, modes, affine_on, eps=1e-5):
    """The CPU check that the float64 reference alone keeps every ReLU case of ``_bn_case`` inside the cap."""
    x = inp["x"]
    rows, C = x.shape
    mean, var, a1, a2 = N.stats_ref(x, 0)
    inv, dmean, dinv, _ = N.single_pass_bounds(N.bn_L(rows, C), mean, var, a1, a2, eps)
    w, b = (inp["w"], inp["b"]) if affine_on else (None, None)
    zero = torch.zeros((), dtype=torch.float64)
    for mode in modes:
        relu, use_res = MODES[mode]
        if not relu:
            continue
        tag = f"reference {family}{ratio} ({rows}, {C}) {mode}"
        z, _, dz, _ = N.affine_fwd_ref(x, w, b, inp["res"] if use_res else None, True, mean, inv, dmean, dinv, dtype)
        N.undecided(z, dz, tag, errs)
        if mode == "relu":  # RM 2 recomputes the decision from the stored float32 statistics
            z2, _, dz2, _ = N.affine_fwd_ref(x, w, b, None, True, mean.float().double(), inv.float().double(), zero,
                                             zero, dtype)
            N.undecided(z2, dz2, tag + " RM2", errs)


def _bn_case(ext, family, ratio, rows, C, dtype, errs, ws=None, modes=MODES, affine_on=True, running=True, seed=0):
    inp = N.rows_inputs(family, rows, C, dtype, ratio, seed)
    if ext is None:
        return _bn_reference_only(inp, family, ratio, dtype, errs, modes, affine_on)
    inp = _cuda(inp)
    ws = ws or _new_ws()
    exact = family == "integer"
    for mode in modes:
        relu, use_res = MODES[mode]
        tag = f"{family}{ratio} ({rows}, {C}) {mode}"
        fwd, _ = _bn_fwd(ext, tag, inp, relu, use_res, affine_on, running, dtype, ws, errs, exact)
        outs = {}
        for rm, use_dres in BWD_OF[mode]:
            outs[rm, use_dres] = _bn_bwd(ext, f"{tag} RM{rm}{' dres' if use_dres else ''}", inp, fwd, rm, use_dres,
                                         affine_on, dtype, ws, errs, exact)
        if mode == "relu":  # the recomputed mask is the saved one
            a, b = outs[2, True], outs[3, True]
            if not torch.equal(a["dres"], b["dres"]):
                errs.append(f"{tag}: RM 2 and RM 3 disagree on {int((a['dres'] != b['dres']).sum())} dres elements")
            if exact and not all(torch.equal(a[k], b[k]) for k in ("dx", "dw", "db")):
                errs.append(f"{tag}: RM 2 and RM 3 differ in the exact family")
        if exact and relu:
            want = inp["dy"] * (fwd["y"].float() > 0)
            for key, o in outs.items():
                if key[1] and not torch.equal(o["dres"], want.to(dtype)):
                    errs.append(f"{tag} RM{key[0]}: dres is not dy (y > 0) bit for bit")


# =============================================================================== GPU: BatchNorm

BN_SHAPES = [(1, 8), (37, 8), (4100, 8), (301, 24), (683, 96), (33, 1032), (50, 2040), (277, 2048)]


def _k(family, ratio, rows, C, **kw):
    return dict(family=family, ratio=ratio, rows=rows, C=C, **kw)


# group -> key -> the `_bn_case` calls of one test (each: bn_fwd_train in its modes, then bn_bwd in every ReLU mode
# that fits, dres present / absent). A CPU test walks the same table with the reference alone (the undecided cap).
BN_GROUPS = {
    # uniform inputs, affine and running statistics present
    "uniform": {f"{r}x{c}": [_k("uniform", 0, r, c)] for r, c in BN_SHAPES + [(126, 64), (64, 128)]},
    # w / b null (the kernels read a stand-in array), running statistics null / present
    "null": {f"{r}x{c}": [_k("uniform", 0, r, c, affine_on=False, running=False, seed=1),
                          _k("uniform", 0, r, c, modes=("relu_res",), affine_on=False, seed=1)]
             for r, c in [(37, 8), (301, 24), (277, 2048)]},
    # mean / std = ratio per channel: the kappa-scaled bounds hold (the ratios are printed)
    "offset": {str(ratio): [_k("offset", ratio, r, c, modes=_modes_of("offset", ratio, r, c))
                            for r, c in [(683, 96), (4100, 8)]] for ratio in (4, 32, 256)},
    # variance exactly 0; a constant channel at 1000, whose single-pass variance may come out negative
    "constant": {"all": [_k("constant", 0, 301, 24), _k("constant", 0, 64, 128),
                         _k("constant1000", 0, 64, 128, modes=("none", "res")),
                         _k("constant1000", 0, 683, 96, modes=("none", "res"))]},
    # sums below 2^24: save_mean exact, invstd / running statistics within 2 ulp, db equal, dres and the mask
    # bytes bit for bit, RM 2 == RM 3
    "integer": {f"{r}x{c}": [_k("integer", 0, r, c)]
                for r, c in [(64, 8), (8192, 8), (64, 24), (64, 1032), (64, 2048), (512, 2048), (128, 64)]},
}
BN_PARAMS = [(g, k, d) for g, keys in BN_GROUPS.items() for k in keys for d in DT
             if not (g == "offset" and k == "256" and d != torch.float32)]


@pytest.mark.parametrize("group,key,dtype", BN_PARAMS, ids=_ids(BN_PARAMS))
def test_bn_reference_within_cap_cpu(group, key, dtype):
    """The float64 reference alone leaves at most 0.1 % of every GPU case's elements undecided."""
    errs = []
    for kw in BN_GROUPS[group][key]:
        _bn_case(None, dtype=dtype, errs=errs, **kw)
    assert not errs, "\n".join(errs)


@gpu
@pytest.mark.parametrize("group,key,dtype", BN_PARAMS, ids=_ids(BN_PARAMS))
def test_bn_raw(gpu_ext, group, key, dtype):
    """bn_fwd_train and bn_bwd (all four ReLU modes, dres present / absent) over ``BN_GROUPS``."""
    errs = []
    for kw in BN_GROUPS[group][key]:
        _bn_case(gpu_ext, dtype=dtype, errs=errs, **kw)
    assert not errs, "\n".join(errs)


@gpu
def test_bn_workspace_sequence(gpu_ext):
    """C = 2048 -> 8 -> 1032 -> 24 on ONE workspace: a shard left non-zero in one layout would land inside
    the next call's reduction (and is looked for directly after every call)."""
    errs, ws = [], _new_ws()
    for rows, C in [(277, 2048), (4100, 8), (33, 1032), (301, 24), (512, 2048)]:
        _bn_case(gpu_ext, "integer" if rows == 512 else "uniform", 0, rows, C, torch.bfloat16, errs, ws=ws,
                 modes=("relu_res",))
    assert not errs, "\n".join(errs)


@gpu
@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
def test_bn_infer(gpu_ext, dtype):
    """Eval mode (invstd = rsqrt(running_var + eps) in the kernel) with running_var 0 and 1e-12 present."""
    errs = []
    for rows, C in [(37, 8), (301, 24), (50, 2040)]:
        inp = _cuda(N.rows_inputs("uniform", rows, C, dtype))
        rm = torch.linspace(-1, 1, C, device="cuda")
        rv = torch.linspace(0.25, 4, C, device="cuda")
        rv[0], rv[1] = 0.0, 1e-12
        eps = 1e-5
        inv = (rv.double() + eps).rsqrt()
        for mode, (relu, use_res) in MODES.items():
            y = _act(rows, C, dtype)
            gpu_ext.bn_fwd_infer(inp["x"].data_ptr(), y[1].data_ptr(), _p(inp["res"]) if use_res else 0,
                                 inp["w"].data_ptr(), inp["b"].data_ptr(), rm.data_ptr(), rv.data_ptr(), rows, C, eps,
                                 relu, _code(dtype), _st())
            _, yr, _, dy = N.affine_fwd_ref(inp["x"], inp["w"], inp["b"], inp["res"] if use_res else None, relu,
                                            rm.double(), inv, torch.zeros_like(inv), 5 * U32 * inv, dtype)
            tag = f"infer ({rows}, {C}) {mode}"
            E.check(f"{tag} y", E.take_guarded(tag, *y, errs), yr, dy, errs)
    assert not errs, "\n".join(errs)


@gpu
@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
def test_bn_stats_finalize_apply(gpu_ext, dtype):
    """bn_stats_finalize with its scale / shift outputs, then bn_apply on the stored statistics."""
    errs, ws = [], _new_ws()
    for rows, C in [(37, 8), (301, 24), (277, 2048)]:
        inp = _cuda(N.rows_inputs("uniform", rows, C, dtype))
        x, eps, mom = inp["x"], 1e-5, 0.25
        run0 = (torch.linspace(-1, 1, C, device="cuda"), torch.linspace(0.5, 2, C, device="cuda"))
        sm, si, sc, sh, rm, rv = _ch(C), _ch(C), _ch(C), _ch(C), _ch(C, run0[0]), _ch(C, run0[1])
        nbt = torch.tensor([0], dtype=torch.int64, device="cuda")
        gpu_ext.bn_stats_finalize(x.data_ptr(), inp["w"].data_ptr(), inp["b"].data_ptr(), rm[1].data_ptr(),
                                  rv[1].data_ptr(), sm[1].data_ptr(), si[1].data_ptr(), sc[1].data_ptr(),
                                  sh[1].data_ptr(), ws[1].data_ptr(), rows, C, mom, eps, 0, _code(dtype), _st(),
                                  nbt.data_ptr())
        tag = f"stats_finalize ({rows}, {C})"
        _ws_check(tag, ws, errs)
        assert int(nbt) == 1
        mean, var, a1, a2 = N.stats_ref(x, 0)
        inv, dmean, dinv, _ = N.single_pass_bounds(N.bn_L(rows, C), mean, var, a1, a2, eps)
        wd, bd = inp["w"].double(), inp["b"].double()
        scale = wd * inv
        dscale = wd.abs() * dinv + U32 * scale.abs()
        got = {k: E.take_guarded(f"{tag} {k}", *v, errs)[0] for k, v in
               dict(mean=sm, inv=si, scale=sc, shift=sh, rm=rm, rv=rv).items()}
        E.check(f"{tag} scale", got["scale"], scale, dscale + TINY, errs)
        E.check(f"{tag} shift", got["shift"], bd - mean * scale,
                scale.abs() * dmean + mean.abs() * dscale + dmean * dscale + 2 * U32 * ((mean * scale).abs() + bd.abs())
                + TINY, errs)
        # the statistics and running statistics under bn_check_fwd's bounds, y through bn_apply
        for mode, (relu, use_res) in MODES.items():
            y = _act(rows, C, dtype)
            mask = N.guarded_bytes(rows * C // 8, "cuda") if relu else None
            mean32, inv32 = got["mean"].contiguous(), got["inv"].contiguous()
            gpu_ext.bn_apply(x.data_ptr(), y[1].data_ptr(), _p(inp["res"]) if use_res else 0, inp["w"].data_ptr(),
                             inp["b"].data_ptr(), mean32.data_ptr(), inv32.data_ptr(), rows, C, relu,
                             mask[1].data_ptr() if mask else 0, _code(dtype), _st())
            out = dict(got, y=E.take_guarded(f"{tag} {mode} y", *y, errs))
            if mask:
                out["mask"] = N.take_bytes(f"{tag} {mode} mask", *mask, errs)
            N.bn_check_fwd(f"{tag} {mode}", inp, out, relu, use_res, True, dtype, errs, eps, mom, run0)
    assert not errs, "\n".join(errs)


def _stored_stats(x, eps=1e-5):
    """float32 (mean, invstd) of x as stored inputs of the apply / backward kernels."""
    mean, var, _, _ = N.stats_ref(x, 0)
    return mean.float().contiguous(), (var + eps).rsqrt().float().contiguous()


@gpu
@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("rows,C", [(1, 8), (37, 8), (301, 8), (1, 256), (3, 256), (131, 256), (5, 2048), (64, 2048)])
def test_bn_dual(gpu_ext, rows, C, dtype):
    """y = relu(BN_a(x) + BN_b(x2)) and its one-pass backward on stored statistics (nvec 1, odd, even)."""
    errs, ws, ws2 = [], _new_ws(), _new_ws()
    fam = "integer" if rows == 64 else "uniform"
    a, b = _cuda(N.rows_inputs(fam, rows, C, dtype)), _cuda(N.rows_inputs(fam, rows, C, dtype, seed=1))
    (m1, i1), (m2, i2) = _stored_stats(a["x"]), _stored_stats(b["x"])
    y, mask = _act(rows, C, dtype), N.guarded_bytes(rows * C // 8, "cuda")
    gpu_ext.bn_apply_dual(a["x"].data_ptr(), b["x"].data_ptr(), y[1].data_ptr(), a["w"].data_ptr(), a["b"].data_ptr(),
                          m1.data_ptr(), i1.data_ptr(), b["w"].data_ptr(), b["b"].data_ptr(), m2.data_ptr(),
                          i2.data_ptr(), rows, C, mask[1].data_ptr(), _code(dtype), _st())
    tag = f"dual ({rows}, {C})"
    zero = torch.zeros((), dtype=torch.float64, device="cuda")
    z1, _, dz1, _ = N.affine_fwd_ref(a["x"], a["w"], a["b"], None, False, m1.double(), i1.double(), zero, zero, dtype)
    z2, _, dz2, _ = N.affine_fwd_ref(b["x"], b["w"], b["b"], None, False, m2.double(), i2.double(), zero, zero, dtype)
    z = z1 + z2
    dz = dz1 + dz2 + 2 * U32 * z.abs()
    yk, mk = E.take_guarded(f"{tag} y", *y, errs), N.take_bytes(f"{tag} mask", *mask, errs)
    E.check(f"{tag} y", yk, z.clamp_min(0), dz + N.rt(dtype, z), errs)
    und = N.undecided(z, dz, tag, errs)
    N.check_mask(f"{tag} mask", mk, z, und, errs)
    if fam == "integer" and not torch.equal(mk, N.mask_bytes(yk.float() > 0)):
        errs.append(f"{tag}: mask bytes differ from the bits of y > 0")
    dx, dx2 = _act(rows, C, dtype), _act(rows, C, dtype)
    dw, db, dw2, db2 = _ch(C), _ch(C), _ch(C), _ch(C)
    mkc = mk.contiguous()
    gpu_ext.bn_bwd_dual(a["dy"].data_ptr(), mkc.data_ptr(), a["x"].data_ptr(), b["x"].data_ptr(), a["w"].data_ptr(),
                        m1.data_ptr(), i1.data_ptr(), b["w"].data_ptr(), m2.data_ptr(), i2.data_ptr(), dx[1].data_ptr(),
                        dx2[1].data_ptr(), dw[1].data_ptr(), db[1].data_ptr(), dw2[1].data_ptr(), db2[1].data_ptr(),
                        ws[1].data_ptr(), ws2[1].data_ptr(), rows, C, _code(dtype), _st())
    _ws_check(f"{tag} ws", ws, errs)
    _ws_check(f"{tag} ws2", ws2, errs)
    g = a["dy"].double() * N.mask_bits(mk, (rows, C))
    o1 = dict(dx=E.take_guarded("dx", *dx, errs), dw=E.take_guarded("dw", *dw, errs)[0],
              db=E.take_guarded("db", *db, errs)[0])
    o2 = dict(dx=E.take_guarded("dx2", *dx2, errs), dw=E.take_guarded("dw2", *dw2, errs)[0],
              db=E.take_guarded("db2", *db2, errs)[0])
    N.bn_check_bwd(f"{tag} bwd a", a, o1, m1, i1, g, True, dtype, errs, exact=fam == "integer")
    N.bn_check_bwd(f"{tag} bwd b", dict(b, dy=a["dy"]), o2, m2, i2, g, True, dtype, errs, exact=fam == "integer")
    assert not errs, "\n".join(errs)


@gpu
def test_bn_dual_refuses_non_fixed(gpu_ext):
    x = torch.zeros(4, 24, device="cuda", dtype=torch.bfloat16)
    f = torch.zeros(24, device="cuda")
    m = torch.zeros(12, device="cuda", dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="must divide 256"):
        gpu_ext.bn_apply_dual(x.data_ptr(), x.data_ptr(), x.data_ptr(), f.data_ptr(), f.data_ptr(), f.data_ptr(),
                              f.data_ptr(), f.data_ptr(), f.data_ptr(), f.data_ptr(), f.data_ptr(), 4, 24,
                              m.data_ptr(), _code(torch.bfloat16), _st())
    ws = torch.zeros(WS_FLOATS, device="cuda")
    with pytest.raises(RuntimeError, match="must divide 256"):
        gpu_ext.bn_bwd_dual(x.data_ptr(), m.data_ptr(), x.data_ptr(), x.data_ptr(), f.data_ptr(), f.data_ptr(),
                            f.data_ptr(), f.data_ptr(), f.data_ptr(), f.data_ptr(), x.data_ptr(), x.data_ptr(),
                            f.data_ptr(), f.data_ptr(), f.data_ptr(), f.data_ptr(), ws.data_ptr(), ws.data_ptr(), 4, 24,
                            _code(torch.bfloat16), _st())


@gpu
def test_bn_fp16_underflow(gpu_ext):
    """fp16 BatchNorm + residual + ReLU with positive pre-activations below 2^-25: y rounds to 0 while the
    mask bit is set; y > 0 implies the bit; a set bit with y == 0 only where the reference pre-activation is
    below fp16's smallest subnormal 2^-24; the backward follows the mask."""
    errs = []
    dtype, rows, C = torch.float16, 37, 24
    g = N._g("underflow")
    x = (torch.randint(-8, 9, (rows, C), generator=g).float() * 2.0 ** -10)  # |x| <= 2^-7: dz stays below 2^-26
    kind = torch.randint(0, 4, (rows, C), generator=g)
    res = torch.where(kind == 0, -x, torch.where(kind == 1, -x + 0.5, -x - 0.5))
    x = torch.where(kind == 3, torch.zeros_like(x), x)
    res = torch.where(kind == 3, torch.full_like(x, 2.0 ** -24), res)
    inp = _cuda(dict(x=x.to(dtype), res=res.to(dtype), dy=N._uni(g, (rows, C), -1, 1).to(dtype), w=torch.ones(C),
                     b=torch.full((C,), 2.0 ** -26)))
    assert torch.equal(inp["res"].float().cpu(), res) and torch.equal(inp["x"].float().cpu(), x)
    mean, inv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
    y, mask = _act(rows, C, dtype), N.guarded_bytes(rows * C // 8, "cuda")
    gpu_ext.bn_apply(inp["x"].data_ptr(), y[1].data_ptr(), inp["res"].data_ptr(), inp["w"].data_ptr(),
                     inp["b"].data_ptr(), mean.data_ptr(), inv.data_ptr(), rows, C, 1, mask[1].data_ptr(), _code(dtype),
                     _st())
    zero = torch.zeros((), dtype=torch.float64, device="cuda")
    z, yr, dz, dy = N.affine_fwd_ref(inp["x"], inp["w"], inp["b"], inp["res"], True, mean.double(), inv.double(), zero,
                                     zero, dtype)
    tiny = (z > 0) & (z < 2.0 ** -25)
    assert int(tiny.sum()) > rows * C // 8 and int(((z > 2.0 ** -24) & (z < 2.0 ** -23)).sum()) > rows * C // 8
    yk, mk = E.take_guarded("underflow y", *y, errs), N.take_bytes("underflow mask", *mask, errs)
    E.check("underflow y", yk, yr, dz + N.rt(dtype, yr), errs)
    bits, pos = N.mask_bits(mk, (rows, C)), yk.float() > 0
    und = N.undecided(z, dz, "underflow", errs)
    N.check_mask("underflow mask", mk, z, und, errs)
    assert bool((bits | ~pos).all()), "y > 0 without its mask bit"
    assert bool((~(bits & ~pos) | (z < 2.0 ** -24)).all()), "mask bit set, y == 0, pre-activation representable"
    assert bool((bits & ~pos & tiny).any())
    ws = _new_ws()
    fwd = dict(y=yk, mask=mk, mean=mean, inv=inv)
    out = _bn_bwd(gpu_ext, "underflow RM3 dres", inp, fwd, 3, True, True, dtype, ws, errs)
    if not torch.equal(out["dres"], inp["dy"] * bits):
        errs.append("underflow: dres does not follow the mask")
    assert not errs, "\n".join(errs)


@gpu
def test_bn_large(gpu_ext):
    """32 M elements (C = 256, bf16): more vectors than one round of resident workgroups takes at 4 per lane,
    so the elementwise grids are capped and every lane strides; the float64 reference runs on the GPU."""
    rows, C, dtype = 131072, 256, torch.bfloat16
    gen = torch.Generator(device="cuda").manual_seed(7)
    r = lambda lo, hi, *s: torch.rand(*s, device="cuda", generator=gen) * (hi - lo) + lo
    sgn = lambda *s: (torch.randint(0, 2, s, device="cuda", generator=gen) * 2 - 1).float()
    inp = dict(x=r(-2, 2, rows, C).to(dtype), res=r(-2, 2, rows, C).to(dtype), dy=r(-1, 1, rows, C).to(dtype),
               w=r(0.5, 1.5, C) * sgn(C), b=r(2.0 ** -4, 1, C) * sgn(C))
    errs, ws = [], _new_ws()
    fwd, _ = _bn_fwd(gpu_ext, "large relu_res", inp, 1, True, True, True, dtype, ws, errs)
    _bn_bwd(gpu_ext, "large RM3 dres", inp, fwd, 3, True, True, dtype, ws, errs)
    assert not errs, "\n".join(errs)


@gpu
def test_bn_wrappers(gpu_ext):
    """fused_batch_norm / FusedBatchNorm2d (4-D channels_last, 2-D, momentum=None, affine=False, eval with a
    running_var near 0, the masked GradLink hand-over), bn_from_stats(stats_ready=False) and dual_bn_relu,
    per element under the same bounds."""
    from fluxmpi_amd.ops import fused_block as fb
    from fluxmpi_amd.ops.batchnorm import FusedBatchNorm2d, GradLink, fused_batch_norm
    errs = []
    dtype = torch.bfloat16
    inp = _cuda(N.rows_inputs("uniform", 126, 64, dtype))
    nchw = lambda t: t.view(2, 7, 9, 64).permute(0, 3, 1, 2)  # rows are (n, h, w): a channels_last (2, 64, 7, 9)

    def module(**kw):
        bn = FusedBatchNorm2d(64, **kw).cuda()
        if bn.affine:
            with torch.no_grad():
                bn.weight.copy_(inp["w"]), bn.bias.copy_(inp["b"])
        return bn

    # momentum=None (cumulative average), relu + residual, masked GradLink
    bn = module(momentum=None)
    bn.num_batches_tracked.fill_(3)
    run0 = (bn.running_mean.clone(), bn.running_var.clone())
    x, res = nchw(inp["x"]).clone().requires_grad_(), nchw(inp["res"]).clone().requires_grad_()
    link = GradLink(masked=True)
    y = bn(x, relu=True, residual=res, link=link)
    assert int(bn.num_batches_tracked) == 4
    y.backward(nchw(inp["dy"]))
    dyk, mask = link.take()
    flat = lambda t: t.permute(0, 2, 3, 1).reshape(126, 64)
    out = dict(y=flat(y.detach()), rm=bn.running_mean, rv=bn.running_var, mask=mask)
    mean, var, a1, a2 = N.stats_ref(inp["x"], 0)
    inv, dmean, dinv, _ = N.single_pass_bounds(N.bn_L(126, 64), mean, var, a1, a2, bn.eps)
    z, yr, dz, dy = N.affine_fwd_ref(inp["x"], inp["w"], inp["b"], inp["res"], True, mean, inv, dmean, dinv, dtype)
    E.check("module y", out["y"], yr, dy, errs)
    und = N.undecided(z, dz, "module", errs)
    N.check_mask("module mask", mask, z, und, errs)
    E.check("module running_mean (momentum None)", bn.running_mean, 0.75 * run0[0].double() + 0.25 * mean,
            0.25 * dmean + 4 * U32 * (run0[0].abs() + mean.abs()) + TINY, errs)
    assert torch.equal(flat(dyk), inp["dy"]) and res.grad is None and x.grad is not None

    # affine=False, track_running_stats=False, 2-D input, ReLU (RM 2 in the backward)
    inp2 = _cuda(N.rows_inputs("uniform", 64, 128, torch.float16))
    bn2 = FusedBatchNorm2d(128, affine=False, track_running_stats=False).cuda()
    x2 = inp2["x"].clone().requires_grad_()
    y2 = fused_batch_norm(x2, None, None, None, None, True, 0.1, 1e-5, relu=True)
    assert torch.equal(y2, bn2(x2, relu=True))
    mean, var, a1, a2 = N.stats_ref(inp2["x"], 0)
    inv, dmean, dinv, _ = N.single_pass_bounds(N.bn_L(64, 128), mean, var, a1, a2, 1e-5)
    z, yr, dz, dy = N.affine_fwd_ref(inp2["x"], None, None, None, True, mean, inv, dmean, dinv, torch.float16)
    E.check("2-D null affine y", y2.detach(), yr, dy, errs)
    N.undecided(z, dz, "2-D null affine", errs)
    y2.backward(inp2["dy"])  # (the null-affine RM 2 backward is bounded per element in the raw tests)
    assert x2.grad.shape == x2.shape and bool(torch.isfinite(x2.grad).all())

    # eval mode, running_var near 0
    bn3 = module().eval()
    with torch.no_grad():
        bn3.running_var[0], bn3.running_var[1] = 0.0, 1e-12
        y3 = bn3(nchw(inp["x"]), relu=False)
    inv3 = (bn3.running_var.double() + bn3.eps).rsqrt()
    _, yr, _, dy = N.affine_fwd_ref(inp["x"], inp["w"], inp["b"], None, False, bn3.running_mean.double(), inv3,
                                    torch.zeros_like(inv3), 5 * U32 * inv3, dtype)
    E.check("eval y", flat(y3), yr, dy, errs)

    # bn_from_stats(stats_ready=False)
    bn4 = module()
    y4 = fb.bn_from_stats(nchw(inp["x"]).contiguous(memory_format=torch.channels_last), bn4, relu=True,
                          residual=nchw(inp["res"]).contiguous(memory_format=torch.channels_last), stats_ready=False)
    mean, var, a1, a2 = N.stats_ref(inp["x"], 0)
    inv, dmean, dinv, _ = N.single_pass_bounds(N.bn_L(126, 64), mean, var, a1, a2, bn4.eps)
    _, yr, _, dy = N.affine_fwd_ref(inp["x"], inp["w"], inp["b"], inp["res"], True, mean, inv, dmean, dinv, dtype)
    E.check("bn_from_stats y", flat(y4.detach()), yr, dy, errs)

    # dual_bn_relu
    bn5, bn6 = module(), module()
    c3 = nchw(inp["x"]).contiguous(memory_format=torch.channels_last)
    cds = nchw(inp["res"]).contiguous(memory_format=torch.channels_last)
    y5 = fb.dual_bn_relu(c3, bn5, cds, bn6, stats_ready=False)
    tot, dtot = 0, 0
    for t in (inp["x"], inp["res"]):
        mean, var, a1, a2 = N.stats_ref(t, 0)
        inv, dmean, dinv, _ = N.single_pass_bounds(N.bn_L(126, 64), mean, var, a1, a2, bn5.eps)
        z, _, dz, _ = N.affine_fwd_ref(t, inp["w"], inp["b"], None, False, mean, inv, dmean, dinv, dtype)
        tot, dtot = tot + z, dtot + dz
    E.check("dual_bn_relu y", flat(y5.detach()), tot.clamp_min(0), dtot + 2 * U32 * tot.abs() + N.rt(dtype, tot), errs)
    assert not errs, "\n".join(errs)


# =============================================================================== GPU: LayerNorm

def _ln_affine(inp, kind, dtype):
    """(w, b) as the kernel reads them and as the reference sees them: in the activation dtype, fp32, or
    absent (the wrappers' ones / zeros)."""
    D = inp["w"].numel()
    if kind == "none":
        return torch.ones(D, device="cuda"), torch.zeros(D, device="cuda"), None, None
    w, b = (inp["w"], inp["b"]) if kind == "f32" else (inp["w"].to(dtype), inp["b"].to(dtype))
    return w.contiguous(), b.contiguous(), w, b


def _ln_case(ext, family, ratio, rows, D, dtype, kind, errs, max_blocks=None, eps=1e-5):
    inp = _cuda(_ln_inputs(family, rows, D, dtype, ratio))
    w, b, wr, br = _ln_affine(inp, kind, dtype)
    exact = family == "integer"
    mb = max_blocks or min(N.ceil_div(rows, 4), 4096)
    blocks = []
    for add in (False, True):
        tag = f"ln {family}{ratio} ({rows}, {D}) {kind} add={add}"
        y, h = _act(rows, D, dtype), _act(rows, D, dtype) if add else None
        mean, rstd = (E.guarded(1, rows, rows + 8, torch.float32, "cuda") for _ in range(2))
        ext.layernorm_fwd(inp["x"].data_ptr(), inp["r"].data_ptr() if add else 0, h[1].data_ptr() if add else 0,
                          y[1].data_ptr(), w.data_ptr(), b.data_ptr(), mean[1].data_ptr(), rstd[1].data_ptr(), rows, D,
                          eps, _code(dtype), _code(w.dtype), _st())
        href = (inp["x"].float() + inp["r"].float()).to(dtype) if add else inp["x"]
        out = dict(y=E.take_guarded(f"{tag} y", *y, errs), mean=E.take_guarded(f"{tag} mean", *mean, errs)[0],
                   rstd=E.take_guarded(f"{tag} rstd", *rstd, errs)[0])
        if add:  # the stored h is the rounded x + r, bit for bit
            E.check(f"{tag} h", E.take_guarded(f"{tag} h", *h, errs), href.double(), None, errs)
        N.ln_check_fwd(tag, href, wr, br, out, dtype, errs, eps)
        m32, r32 = out["mean"].contiguous(), out["rstd"].contiguous()
        for dh, cs in ((False, False),) if not add else ((True, False), (True, True)):
            npart = 3 if cs else 2
            part, dx = E.guarded(mb, npart * D, npart * D, torch.float32, "cuda"), _act(rows, D, dtype)
            nb = ext.layernorm_bwd(inp["dy"].data_ptr(), href.data_ptr(), inp["r"].data_ptr() if dh else 0,
                                   m32.data_ptr(), r32.data_ptr(), w.data_ptr(), dx[1].data_ptr(), part[1].data_ptr(),
                                   mb, rows, D, _code(dtype), _code(w.dtype), _st(), cs)
            assert 1 <= nb <= min(mb, N.ceil_div(rows, 4)), nb
            blocks.append(nb)
            p = E.take_guarded(f"{tag} partials", *part, errs)
            if not bool(torch.isnan(p[nb:]).all()):
                errs.append(f"{tag}: partial rows past the {nb} launched blocks were written")
            sums = p[:nb].double().sum(0).view(npart, D)
            back = dict(dx=E.take_guarded(f"{tag} dx", *dx, errs), dw=sums[0], db=sums[1], cs=sums[2] if cs else None)
            N.ln_check_bwd(f"{tag} dh={dh} cs={cs}", inp["dy"], href, m32, r32, wr, inp["r"] if dh else None, back,
                           dtype, errs, exact)
    return blocks


LN_KINDS = ["act", "f32", "none"]


@gpu
@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("D", LN_D)
def test_ln_raw(gpu_ext, D, dtype):
    """layernorm_fwd / layernorm_bwd at every VPL variant: rows 1, 3, 5, 9 (and 50 under max_blocks = 2),
    the affine in the activation dtype / fp32 / absent, with and without the residual add and column sums."""
    errs = []
    i = LN_D.index(D) + DT.index(dtype)
    for j, rows in enumerate((1, 3, 5, 9)):
        _ln_case(gpu_ext, "uniform", 0, rows, D, dtype, LN_KINDS[(i + j) % 3], errs)
    nb = _ln_case(gpu_ext, "uniform", 0, 50, D, dtype, LN_KINDS[i % 3], errs, max_blocks=2)
    assert all(50 > 4 * b for b in nb)  # every wave walks several rows
    assert not errs, "\n".join(errs)


LN_FAMS = _with_dtypes([("offset", 4), ("offset", 32), ("offset", 256), ("constant", 0), ("integer", 0)])


@gpu
@pytest.mark.parametrize("family,ratio,dtype", LN_FAMS, ids=_ids(LN_FAMS))
def test_ln_families(gpu_ext, family, ratio, dtype):
    """Per-row offsets (the two-pass variance shows no kappa term: the same bounds hold), constant rows and
    the exact integer family (db equal to the integer sums)."""
    errs = []
    for rows, D in [(4, 64), (8, 520), (4, 768), (4, 4104), (4, 8192)]:
        _ln_case(gpu_ext, family, ratio, rows, D, dtype, "f32", errs)
    assert not errs, "\n".join(errs)


@gpu
@pytest.mark.parametrize("D", [8, 768])
def test_ln_rows_per_wave(gpu_ext, D):
    """Enough rows that each wave of the persistent grid walks more than one (checked against the block
    count the launcher returns)."""
    errs = []
    rows = 20000
    nb = _ln_case(gpu_ext, "uniform", 0, rows, D, torch.bfloat16, "act", errs)
    assert all(rows > 4 * b for b in nb), nb
    assert not errs, "\n".join(errs)


@gpu
def test_ln_wrappers(gpu_ext):
    """layer_norm, add_layer_norm and linear_add_layer_norm (the CS column-sum path) through autograd, on
    the statistics the nodes saved."""
    from fluxmpi_amd.ops.layernorm import add_layer_norm, layer_norm, linear_add_layer_norm
    errs = []
    dtype, rows, D = torch.bfloat16, 14, 1032
    inp = _cuda(_ln_inputs("uniform", rows, D, dtype))
    w, b = inp["w"].to(dtype).requires_grad_(), inp["b"].to(dtype).requires_grad_()

    def bwd_check(tag, node, h, dh, dx, dw, db, cs=None):
        saved = node.saved_tensors
        m32, r32 = saved[-2], saved[-1]
        r = N.ln_bwd_refs(inp["dy"], h, m32, r32, w.detach(), dh, dtype)
        E.check(f"{tag} dx", dx, r["dx"], r["ddx"], errs)
        E.check(f"{tag} dw", dw, r["dw"], r["ddw"] + N.rt(dtype, r["dw"]), errs)
        E.check(f"{tag} db", db, r["db"], r["ddb"] + N.rt(dtype, r["db"]), errs)
        if cs is not None:  # of the stored dx, rounded to the bias dtype
            sd = dx.double().sum(0)
            E.check(f"{tag} colsum", cs, sd, r["Lr"] * N.E23 * dx.double().abs().sum(0) + N.rt(dtype, sd) + TINY, errs)

    x = inp["x"].clone().requires_grad_()
    y = layer_norm(x, w, b)
    N.ln_check_fwd("layer_norm", inp["x"], w.detach(), b.detach(), dict(y=y.detach(), mean=y.grad_fn.saved_tensors[-2],
                                                                      rstd=y.grad_fn.saved_tensors[-1]), dtype, errs)
    node = y.grad_fn
    dx, dw, db = torch.autograd.grad(y, (x, w, b), inp["dy"], retain_graph=True)
    bwd_check("layer_norm", node, inp["x"], None, dx, dw, db)

    x, r = inp["x"].clone().requires_grad_(), inp["r"].clone().requires_grad_()
    h, y = add_layer_norm(x, r, w, b)
    href = (inp["x"].float() + inp["r"].float()).to(dtype)
    E.check("add_layer_norm h", h.detach(), href.double(), None, errs)
    node = y.grad_fn
    N.ln_check_fwd("add_layer_norm", href, w.detach(), b.detach(),
                   dict(y=y.detach(), mean=node.saved_tensors[-2], rstd=node.saved_tensors[-1]), dtype, errs)
    dx, dr, dw, db = torch.autograd.grad((h, y), (x, r, w, b), (inp["r"], inp["dy"]), retain_graph=True)
    assert torch.equal(dx, dr)
    bwd_check("add_layer_norm", node, href, inp["r"], dx, dw, db)

    g = N._g("ln-linear")
    a = (N._uni(g, (rows, 64), -1, 1)).to(dtype).cuda().requires_grad_()
    W = (N._uni(g, (D, 64), -0.1, 0.1)).to(dtype).cuda().requires_grad_()
    bias = (N._uni(g, (D,), -0.5, 0.5)).to(dtype).cuda().requires_grad_()
    x = inp["x"].clone().requires_grad_()
    h, y = linear_add_layer_norm(a, W, bias, x, w, b)
    node = y.grad_fn
    assert type(node).__name__.startswith("_LinearAddLayerNormFn"), type(node).__name__
    hs = h.detach()
    N.ln_check_fwd("linear_add_layer_norm", hs, w.detach(), b.detach(),
                   dict(y=y.detach(), mean=node.saved_tensors[-2], rstd=node.saved_tensors[-1]), dtype, errs)
    dx, dbias, dw, db = torch.autograd.grad((h, y), (x, bias, w, b), (inp["r"], inp["dy"]), retain_graph=True)
    bwd_check("linear_add_layer_norm", node, hs, inp["r"], dx, dw, db, cs=dbias)
    assert not errs, "\n".join(errs)


# =============================================================================== GPU: GroupNorm

GN_SHAPES = [(2, 8, 1, 1, 1), (2, 48, 3, 3, 8), (1, 64, 9, 9, 64), (2, 520, 3, 5, 5), (2, 2048, 2, 2, 64),
             (5, 24, 33, 31, 3), (3, 16, 5, 7, 4)]


# (add, relu, save h, extra elements between the samples of the out= slot)
GN_COMBOS = [(False, False, False, 0), (True, False, True, 0), (False, True, True, 64), (True, True, True, 0),
             (True, True, False, 64), (True, False, False, 0), (False, True, False, 0)]


def _gn_case(ext, family, ratio, n, c, hh, ww, g, dtype, errs, combos=None, affine_on=True, eps=1e-5):
    hw = hh * ww
    inp = _cuda(_gn_inputs(family, n, hw, c, g, dtype, ratio))
    w, b = (inp["w"], inp["b"]) if affine_on else (None, None)
    exact = family == "integer"
    for add, relu, saveh, stride in combos or GN_COMBOS:
        tag = f"gn {family}{ratio} ({n}, {c}, {hh}, {ww}, {g}) add={add} relu={relu} saveh={saveh} stride+{stride}"
        print(tag)
        y = E.guarded(n, hw * c, hw * c + stride, dtype, "cuda")  # the out= slot: sample i at i * (HW C + stride)
        h = _act(n, hw * c, dtype) if saveh else None
        mean, rstd = (E.guarded(1, n * g, n * g + 8, torch.float32, "cuda") for _ in range(2))
        ext.groupnorm_nhwc_fwd(inp["x"].data_ptr(), inp["a"].data_ptr() if add else 0, h[1].data_ptr() if saveh else 0,
                               y[1].data_ptr(), _p(w), _p(b), mean[1].data_ptr(), rstd[1].data_ptr(), n, hw, c, g, relu,
                               eps, _code(dtype), _st(), hw * c + stride if stride else 0)
        href = N.gn_h(inp["x"], inp["a"] if add else None, relu)
        out = dict(y=E.take_guarded(f"{tag} y", *y, errs).view(n, hw, c),
                   mean=E.take_guarded(f"{tag} mean", *mean, errs)[0].view(n, g),
                   rstd=E.take_guarded(f"{tag} rstd", *rstd, errs)[0].view(n, g))
        if saveh:
            E.check(f"{tag} h", E.take_guarded(f"{tag} h", *h, errs).view(n, hw, c), href.double(), None, errs)
        N.gn_check_fwd(tag, href, w, b, g, out, dtype, errs, eps)
        m32, r32 = out["mean"].contiguous(), out["rstd"].contiguous()
        dh, part = _act(n, hw * c, dtype), E.guarded(n, 2 * c, 2 * c, torch.float32, "cuda")
        ext.groupnorm_nhwc_bwd(inp["dy"].data_ptr(), href.data_ptr(), m32.data_ptr(), r32.data_ptr(), _p(w),
                               dh[1].data_ptr(), part[1].data_ptr(), n, hw, c, g, relu, _code(dtype), _st())
        back = dict(dh=E.take_guarded(f"{tag} dh", *dh, errs).view(n, hw, c),
                    part=E.take_guarded(f"{tag} part", *part, errs).view(n, 2, c))
        N.gn_check_bwd(tag, inp["dy"], href, m32, r32, w, g, relu, back, dtype, errs, exact)


@gpu
@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("n,c,hh,ww,g", GN_SHAPES)
def test_gn_raw(gpu_ext, n, c, hh, ww, g, dtype):
    """groupnorm_nhwc_fwd / _bwd: add / relu / save-h on and off, y in a strided out= slot, w / b null."""
    errs = []
    _gn_case(gpu_ext, "uniform", 0, n, c, hh, ww, g, dtype, errs)
    _gn_case(gpu_ext, "uniform", 0, n, c, hh, ww, g, dtype, errs, combos=[(True, True, True, 0)], affine_on=False)
    assert not errs, "\n".join(errs)


GN_FAMS = _with_dtypes([("offset", 4), ("offset", 32), ("offset", 256), ("constant", 0), ("integer", 0)])


@gpu
@pytest.mark.parametrize("family,ratio,dtype", GN_FAMS, ids=_ids(GN_FAMS))
def test_gn_families(gpu_ext, family, ratio, dtype):
    """Per-group offsets (positive, so they survive the ReLU: the kappa-scaled bounds), constant groups,
    the exact integer family."""
    errs = []
    shapes = [(2, 48, 2, 2, 8), (2, 2048, 2, 2, 64), (3, 16, 4, 7, 4)] if family == "integer" else GN_SHAPES[1:]
    for n, c, hh, ww, g in shapes:
        _gn_case(gpu_ext, family, ratio, n, c, hh, ww, g, dtype, errs,
                 combos=[(False, False, False, 0), (True, True, True, 0)])
    assert not errs, "\n".join(errs)


@gpu
@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
def test_gn_module(gpu_ext, dtype):
    """FusedGroupNorm through autograd (add + ReLU), on the statistics the node saved."""
    from fluxmpi_amd.ops.groupnorm import FusedGroupNorm
    errs = []
    n, c, hh, ww, g = 2, 48, 3, 3, 8
    inp = _cuda(_gn_inputs("uniform", n, hh * ww, c, g, dtype))
    nchw = lambda t: t.view(n, hh, ww, c).permute(0, 3, 1, 2)
    flat = lambda t: t.permute(0, 2, 3, 1).reshape(n, hh * ww, c)
    gn = FusedGroupNorm(g, c).cuda()
    with torch.no_grad():
        gn.weight.copy_(inp["w"]), gn.bias.copy_(inp["b"])
    x, a = nchw(inp["x"]).clone().requires_grad_(), nchw(inp["a"]).clone().requires_grad_()
    y = gn(x, add=a, relu=True)
    hs, m32, r32, _ = y.grad_fn.saved_tensors
    href = N.gn_h(inp["x"], inp["a"], True)
    E.check("module h", flat(hs), href.double(), None, errs)
    N.gn_check_fwd("module", href, inp["w"], inp["b"], g, dict(y=flat(y.detach()), mean=m32, rstd=r32), dtype, errs)
    dx, da, dw, db = torch.autograd.grad(y, (x, a, gn.weight, gn.bias), nchw(inp["dy"]))
    assert torch.equal(dx, da)
    rw, ddw, rb, ddb = N.gn_check_bwd("module", inp["dy"], href, m32, r32, inp["w"], g, True, dict(dh=flat(dx)), dtype,
                                      errs)
    for name, got, ref, bnd in (("dw", dw, rw, ddw), ("db", db, rb, ddb)):  # the wrapper sums the samples
        E.check(f"module {name}", got, ref.sum(0), bnd.sum(0) + n * N.E23 * ref.abs().sum(0) + TINY, errs)
    assert not errs, "\n".join(errs)


# =============================================================================== GPU: pool

POOL_SHAPES = [(2, 8, 7, 5, 3, 2, 1), (1, 16, 8, 8, 2, 2, 0), (2, 8, 9, 11, 3, 1, 1), (1, 8, 6, 6, 3, 3, 0),
               (1, 2048, 4, 4, 3, 2, 1), (1, 1024, 20, 20, 3, 2, 1)]


@gpu
@pytest.mark.parametrize("dtype,generic", [(torch.bfloat16, False), (torch.bfloat16, True), (torch.float16, False),
                                           (torch.float32, False)], ids=["bf16", "bf16-generic", "fp16", "fp32"])
@pytest.mark.parametrize("n,c,h,w,k,s,p", POOL_SHAPES)
def test_pool_exact(gpu_ext, monkeypatch, n, c, h, w, k, s, p, dtype, generic):
    """bn_relu_maxpool_fwd on exact inputs (a value grid with ties and blocked windows, signed power-of-two
    scales): y and idx EQUAL the first-max reference; maxpool_bwd with integer dy equals the scatter and
    conserves the gradient per channel."""
    if generic:
        monkeypatch.setenv("FLUXMPI_POOL_GENERIC", "1")
    else:
        monkeypatch.delenv("FLUXMPI_POOL_GENERIC", raising=False)
    assert (-(-k // s)) in (1, 2, 3)
    errs = []
    x, sc, sh = N.pool_inputs(n, c, h, w, dtype)
    oh, ow = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
    tag = f"pool ({n}, {c}, {h}, {w}, {k}, {s}, {p})"
    y, idx = _act(n * oh * ow, c, dtype), N.guarded_bytes(n * oh * ow * c, "cuda")
    xc, scc, shc = x.cuda(), sc.cuda(), sh.cuda()
    gpu_ext.bn_relu_maxpool_fwd(xc.data_ptr(), scc.data_ptr(), shc.data_ptr(), y[1].data_ptr(), idx[1].data_ptr(), n, h,
                                w, c, k, s, p, _code(dtype), _st())
    yk = E.take_guarded(f"{tag} y", *y, errs).view(n, oh, ow, c).cpu()
    ik = N.take_bytes(f"{tag} idx", *idx, errs).view(n, oh, ow, c).cpu()
    ir = N.pool_check(tag, yk, ik, x, sc, sh, k, s, p, errs)
    dy = torch.randint(-3, 4, (n, oh, ow, c), generator=N._g("pool-dy", n, c, h, w)).float().to(dtype)
    dz = _act(n * h * w, c, dtype)
    dyc, ikc = dy.cuda(), ir.to(torch.uint8).cuda()
    gpu_ext.maxpool_bwd(dyc.data_ptr(), ikc.data_ptr(), dz[1].data_ptr(), n, h, w, c, k, s, p, _code(dtype), _st())
    dzk = E.take_guarded(f"{tag} dz", *dz, errs).view(n, h, w, c).cpu()
    E.check(f"{tag} dz", dzk, N.pool_bwd_ref(dy, ir, h, w, k, s, p), None, errs)
    if not torch.equal(dzk.double().sum((0, 1, 2)), (dy.double() * (ir != 255)).sum((0, 1, 2))):
        errs.append(f"{tag}: sum dz != sum dy[idx != 0xFF] per channel")
    assert not errs, "\n".join(errs)


@gpu
@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
def test_pool_end_to_end(gpu_ext, dtype):
    """bn_relu_maxpool per element under the BatchNorm bounds (max over a window is 1-Lipschitz in the
    sup norm: the bound of a pooled element is the largest dz of its window, plus the output rounding)."""
    from fluxmpi_amd.ops.batchnorm import FusedBatchNorm2d
    from fluxmpi_amd.ops.pool import bn_relu_maxpool
    errs = []
    n, c, h, w = 2, 24, 9, 11
    inp = _cuda(N.rows_inputs("uniform", n * h * w, c, dtype))
    bn = FusedBatchNorm2d(c).cuda()
    with torch.no_grad():
        bn.weight.copy_(inp["w"]), bn.bias.copy_(inp["b"])
    x = inp["x"].view(n, h, w, c).permute(0, 3, 1, 2)
    y = bn_relu_maxpool(x, bn, 3, 2, 1)
    mean, var, a1, a2 = N.stats_ref(inp["x"], 0)
    inv, dmean, dinv, _ = N.single_pass_bounds(N.bn_L(n * h * w, c), mean, var, a1, a2, bn.eps)
    z, yr, dz, _ = N.affine_fwd_ref(inp["x"], inp["w"], inp["b"], None, True, mean, inv, dmean, dinv, dtype)
    img = lambda t: t.view(n, h, w, c).permute(0, 3, 1, 2)
    pr, pd = F.max_pool2d(img(yr), 3, 2, 1), F.max_pool2d(img(dz), 3, 2, 1)
    E.check("bn_relu_maxpool y", y.detach(), pr, pd + N.rt(dtype, pr), errs)
    assert not errs, "\n".join(errs)


@gpu
def test_pool_unsupported_geometry(gpu_ext):
    """K = 4, S = 1 (ceil(K / S) = 4): the backward kernel cannot run it, so the forward takes the reference
    composition and autograd completes (it used to run the forward kernel and raise in the backward)."""
    from fluxmpi_amd.ops.batchnorm import FusedBatchNorm2d
    from fluxmpi_amd.ops.pool import bn_relu_maxpool, supported
    x = torch.randn(2, 8, 9, 9, device="cuda").bfloat16().contiguous(memory_format=torch.channels_last)
    assert supported(x, 3, 2, 1) and not supported(x, 4, 1, 1) and not supported(x, 16, 8, 0)
    assert not supported(x[:, :, :2, :2], 3, 2, 0)  # empty output
    bn = FusedBatchNorm2d(8).cuda()
    xa = x.clone().requires_grad_()
    y = bn_relu_maxpool(xa, bn, 4, 1, 1)
    y.float().sum().backward()
    ref = F.max_pool2d(F.relu(F.batch_norm(x.float(), None, None, bn.weight, bn.bias, True, 0.1, bn.eps)), 4, 1, 1)
    torch.testing.assert_close(y.float(), ref, rtol=2.0 ** -7, atol=1e-6)
    assert xa.grad is not None and bool(torch.isfinite(xa.grad).all()) and int(bn.num_batches_tracked) == 1
