"""The MFMA GEMM and convolution kernels (gemm.hip, gemm_glds.hip, gemm_nt.hip, linbwd.hip,
wgrad256.hip, conv3x3n.hip, wgrad3x3n.hip), every launcher variant, per element against a float64
reference: derived componentwise bounds, exact (bit-for-bit as values) integer and gather inputs,
guard bands around every output that takes a leading dimension, and a CPU half that shows the bounds
are reachable and that planted defects trip the same checker.

Reference and bounds. Every operation is brought to ``C[i, j] = sum_k P[i, k] Q[j, k]`` (a 3x3
convolution through ``mfma_edges.im2col``: plain slices of the zero-padded image) and evaluated in
float64 on the bf16 operands upcast: ``R = P Q^T`` and ``A = |P| |Q|^T``. ``Kred`` is the reduction
length (K, 9 C, the rows of a weight gradient, 9 Cout of an input gradient). Assumptions: a product of
two bf16 values is exact in fp32; every fp32 addition, inside an MFMA or outside, errs by at most
2^-23 relatively (round to nearest or truncation). Then in ANY summation order, split-K partials and
atomics included, with 2^-8 bf16's unit roundoff and 1e-30 added to each bound and nothing else:

    fp32 output                            |got - R|       <= Kred 2^-23 A + 2^-24 |R|
    bf16 output, one rounding              |got - R|       <= 2^-8 |R| + Kred 2^-23 A
    residual epilogue bf16(bf16(C) + r)    |got - (R + r)| <= 2^-8 |R| + 2^-8 |R + r| + Kred 2^-23 A
    bias                                   R includes b, A includes |b|
    affine + ReLU prologue                 the operand is bf16(relu(fp32(fma(x, s, t)))) (one fp64 fma, as
                                           `_act` of test_gemm_gpu.py), fed to R and A as the operand
    statistics shards, EPI 2's db          against float64 sums of the kernel's OWN stored output:
                                           rows 2^-23 sum |y| (and likewise for y^2)
    EPI 2's dh = bf16(bf16(R) d)           2^-8 |R d| + |d| (2^-8 |R| + Kred 2^-23 A), d the stored derivative
    fp32 partials [splits, ...]            summed in float64 by the test, then the fp32 bound

No kernel needed a wider addition constant: everything here passes with 2^-23 on the MI355X.

The one measured constant is the fast GELU of EPI 1 (``GELU_C`` below): ``mfma_edges.gelu_emulated`` is
the formula of gelu_tanh.h / gemm_nt.hip's ``gelu_parts`` in float32 PyTorch, its worst
``|err| / (2^-8 |ref| + 2^-24)`` against float64 over all 65536 bf16 inputs was measured on the CPU
(``GELU_RATIO``), c = ceil(2 ratio), and a CPU test keeps the emulation within c / 2. That measurement
found the tanh derivative NaN for |x| >= 5e19 (``(1 - t^2) (1 + 3 k1 x^2)`` = 0 * inf once x^2 overflows,
16290 of the bf16 bit patterns); gelu_tanh.h now clamps the polynomial and the all-patterns test holds it.

Input families (``mfma_edges``; seeded, made on the CPU):
    uniform   U(-1, 1), the weight side scaled by Kred^-0.5
    cancel    adjacent reduction indices in pairs of equal weight and opposite operands, perturbed by
              2^-6 relatively: |R| << A, only the accumulation term of the bound is left
    ternary   both operands in {-1, 0, 1}, at most 256 (64 / 128 where a statistics epilogue or a residual
              needs the head room) non-zeros per row of the sparse side at seeded positions over the whole
              reduction range: every product, partial sum and result is an integer of magnitude <= 256,
              exact in fp32 in any order and in bf16, so the output must EQUAL the reference at every
              variant, split or not, and the statistics shards (sum y^2 < 2^24 asserted) equal too
    gather    P one-hot under pi(i) = (7 i + 3) mod K (11 where 7 divides K), Q distinct finite normal bf16
              bit patterns: the output equals the selected rows of Q. 3x3: output channel co takes tap
              co mod 9 of source channel pi(co), so y[n, co, h, w] = x[n, pi(co), h + dy, w + dx] with exact
              zeros on the border, all nine padding cases in one launch; the input gradient likewise with
              the flipped taps. EPI 1: M = N = K = 256, W = all 65536 bf16 bit patterns (non-finite ones
              made finite), x one-hot: every bf16 pre-activation reaches the epilogue exactly once.
    guard     every output that takes a leading dimension (ops.gemm.gemm, the gemm_nt / linear_bwd
              bindings, gemm_plain) lies at ldc = N + 8 (+ 16) inside a buffer of sentinel bit patterns,
              NaN inside; split-K workspaces handed to a binding are guarded the same way; a dense-only
              output (conv3x3, conv3x3_fwd / dgrad ``out=``) is pre-filled with NaN. Afterwards every
              sentinel is intact and no NaN is left.
"Equal" compares values (+0 and -0 identified: a float64 BLAS may start a sum of signed zeros either way).

Kernel / template variants, how the launchers select them, and the tests that reach them:

    gemm.hip  gemm_kernel<BM, BN, AK, BKM, NBUF, EX, CONV>  (engine 1; ops.gemm.gemm)
      BM / BN 64 or 128 (M, N >= 128)      GEMM_SHAPES: 64x64 (1, 8, .), 64x128 (127, 136, .), 128x64 (200, 72, .),
                                           128x128 (129, 192, .), (777, 136, .); partial tiles in every one
      AK, BKM = K-major, K-major           test_gemm_forward_layout[engine1-*]
                K-major, N-major           test_gemm_dgrad_layout
                M-major, N-major           test_gemm_wgrad_layout
                M-major, K-major           test_gemm_mmajor_a_kmajor_b (no wrapper uses it)
      NBUF 1, 2 (0 = the launcher's 2)     the nbuf0 / nbuf1 / nbuf2 ids of all of the above
      mode 0 bf16 / 1 statistics           plain / stats kinds; mode 3 partials at splits 1, 3, 7: f32_s*;
                                           mode 2 atomics: atomic_s3
      A affine (per k), B affine (per n)   affine kinds of the forward / weight-gradient layout tests
      EX (residual epilogue)               test_gemm_residual[engine1-*] (always double-buffered)
      CONV (implicit 3x3, stride 1)        test_gemm_implicit_3x3[engine1-*-stride1] (always double-buffered)
      K tails of 8, 24 and 40              K = 8, 24, 40, 72 and 520 = 16 * 32 + 8 in GEMM_SHAPES
    gemm_glds.hip  launch_glds<BM, BN, BK, ST, CONV, RES, AFF>  (engines 0, 2..9)
      engine 2 (auto): K <= 64 -> 32/2,    test_gemm_forward_layout[engine2-*]: K = 8 .. 64 and 72 / 520;
        else 32/3; conv / K >= 1024 -> 64/2  test_gemm_implicit_3x3[engine2-*] and [auto] (64/2 at C = 64, 32/3 at 32)
      engine 3: 32/3, 4: 32/4, 5: 64/2,    the engine3 .. engine6 and engine9 ids of test_gemm_forward_layout,
        6: 64/3, 9: 32/2                   test_gemm_residual, test_gemm_a_sub_gather, test_gemm_implicit_3x3
      engine 7 / 8: 256x128 tiles          the same tests at the six GEMM_SHAPES with M > 128 and N > 64 and the
        (32/3, 64/2; M > 128, N > 64)      (3, 9, 8, 64 -> 128) image; with a prologue affine (and for smaller
                                           shapes) the launcher falls to its 128-tile choice, which then runs
      BM / BN 64 or 128 (M, N > 64)        GEMM_SHAPES as above (65 rows take the 128 tile here)
      RES, AFF, statistics                 test_gemm_residual, the affine kinds (K <= 512: the launcher
                                           refuses a longer affine), the stats kinds
      a_sub (stride-2 row gather)          test_gemm_a_sub_gather at (3, 7, 5) and (2, 8, 8) images
      CONV, conv_s 1 and 2                 test_gemm_implicit_3x3 stride1 / stride2 ids
      not covered here: the BatchNorm-backward epilogue (bnb), res_mask / res_sub and the stride-2
      input-gradient classes (conv_s 16..19) belong to the normalisation / fused-block paths and
      test_s2_dgrad_gpu.py
    gemm_glds.hip  gemm_wgrad_kernel<BM, BN, BK, ST, MODE>  (ops.gemm.conv*_wgrad*)
      WGRAD_VARIANT 1 (32/3), 2 (64/2)     test_gemm_wgrad_v2[1-*], [2-*]; splits 1, 3, 7; XCD remap on and off
      MODE 0 plain, 2 b_sub,               conv1x1_wgrad_v2, conv1x1_wgrad_s2,
           1 im2col, 3 im2col stride 2     conv3x3_wgrad, conv3x3_wgrad_s2 inside test_gemm_wgrad_v2
      gemm_splitk_reduce to fp32 / bf16    the same test (fp32 and bf16 results)
    gemm_nt.hip  gemm_nt_kernel<EPI, BIAS, CONV, GF>
      EPI 0, BIAS 0 / 1 (fp32) / 2 (bf16)  test_gemm_nt_epi0[None / f32 / bf16 - split]
      EPI 1, GF 1 (tanh) / 0 (erf)         test_gemm_nt_gelu_all_bf16_inputs (BIAS 0), test_gemm_nt_epi1_bounds (BIAS 1, 2)
      EPI 2 (+ colpart), EPI 3 (shards)    test_gemm_nt_epi2_epi3_plain_ldc
      gemm_plain with ldc > N              the same test (ldc = N + 16)
      CONV with EPI 0 / 3 / 4              test_gemm_nt_conv3x3 at (4, 8, 8, 64 -> 256) and (256, 5, 7, 128 -> 256);
                                           test_gemm_nt_conv3x3_dgrad_residual (the flipped transposed filter)
      persistent tile stream               (256, 256, 128) one tile, (512, 256, 192) three k-tiles, (768, 512, 448)
                                           six tiles of seven k-tiles, multi_processor_count + 44 tiles at K = 128
      _set_split 0, 2, 8                   the split ids. The launcher never cuts an odd k-tile count or fewer than
                                           16 k-tiles, so at the two largest listed shapes (7 and 2 k-tiles) the
                                           setting is on and the tail runs whole; (768, 512, 1024) and the
                                           36-k-tile convolution ARE cut (EPI 0, 2, 3 and 4 under split)
    linbwd.hip  linbwd_kernel: job<false> (weight gradient), job<true> (input gradient)
      first 0 / 1, splits 1, 3, 7          test_linbwd (M = 256 .. 768: 8 .. 24 k-steps, the last split shorter)
    wgrad256.hip  wgrad256_kernel<32, 4>, <64, 2>, <32, 4, PRIO>, wgrad256h_kernel, wgrad256pp_kernel
      wgrad256_set_variant 0 .. 4          test_wgrad256[0] .. [4] (the function is bound); K = 8, 40, 264, 1000
    conv3x3n.hip  conv3x3n_kernel<C, CO, EPI>
      <64, 64, 0 / 3>, <128, 128, 0 / 3>   test_conv3x3n (forward with / without statistics; the input gradient
                                           runs EPI 0 on the flipped transposed filter)
      <128, 32, .>, <128, 16, .>           test_conv3x3n_tails[32], [16] (from the runtime slot count; GPU only)
    wgrad3x3n.hip  wgrad3x3n_kernel<C, TG, NWM, DEPTH, COB>
      C 64: variant 1 (8 waves), 0, 2      test_wgrad3x3n (variants 0, 1, 2, 4, 5 at every shape; 4 / 5 select the
      C 128: the same, and 4 / 5: COB 128  128-channel groups where C = 128 and Cout % 128 == 0, else fall to 0 / 1)

Wall time on the MI355X: the 200 GPU tests of this file 15.5 s, next to 93 s for the rest of the GPU suite
(108.8 s together, one run).
"""
import math

import pytest
import torch

from . import mfma_edges as E
from .mfma_edges import FAMILIES

gpu = pytest.mark.gpu

# Worst |err| / (2^-8 |ref| + 2^-24) of `mfma_edges.gelu_emulated` (float32 PyTorch, the header's
# formula, bf16-rounded like the stored outputs) against float64 over all 65536 bf16 inputs (CPU),
# and c = ceil(2 * ratio): (form, output) -> value. tanh: both worst cases sit near x = -4.6 .. -5,
# where 1 + tanh(u) cancels to a few fp32 ulps of 1; erf: the bf16 rounding of the output itself.
GELU_RATIO = {("tanh", "g"): 5.041, ("tanh", "d"): 28.189, ("erf", "g"): 0.974, ("erf", "d"): 0.993}
GELU_C = {("tanh", "g"): 11, ("tanh", "d"): 57, ("erf", "g"): 2, ("erf", "d"): 2}

# ---- shapes ---------------------------------------------------------------------------------
# gemm.hip / gemm_glds.hip (M, N, K): every M of {1, 63, 64, 65, 127, 129, 200, 777}, N of {8, 24, 64,
# 72, 136, 192} and K of {8, 24, 40, 64, 72, 520}; the last six have M > 128 and N > 64 (what engines
# 7 / 8 need for their 256x128 tiles) and carry every K and every N > 64 again
GEMM_SHAPES = [(1, 8, 520), (63, 24, 8), (64, 64, 24), (65, 72, 40), (127, 136, 64), (129, 192, 72),
               (200, 72, 520), (777, 136, 40), (200, 136, 8), (129, 72, 24), (777, 192, 64)]
ENGINES = [(1, 0), (1, 1), (1, 2)] + [(e, 0) for e in range(2, 10)]  # (engine, NBUF): NBUF acts in gemm.hip only
ENGINE_IDS = [f"engine{e}-nbuf{b}" for e, b in ENGINES]
# the weight-gradient layout of gemm.hip (M- / N-major operands): (rows = reduction, Cout, Cin)
WGRAD_SHAPES = [(1, 8, 8), (63, 24, 24), (64, 64, 40), (65, 72, 64), (127, 136, 72), (129, 192, 520),
                (200, 72, 136), (777, 136, 192)]
# (n, h, w, ci, co) of the a_sub / b_sub gathers and the implicit 3x3 (odd and even images)
IMG_1X1 = [(3, 7, 5, 32, 64), (2, 8, 8, 64, 128)]
IMG_3X3 = [(3, 7, 5, 32, 64), (2, 8, 8, 32, 64), (3, 7, 5, 64, 32), (3, 9, 8, 64, 128)]  # the last: M > 128, N > 64
NT_SHAPES = [(256, 256, 128), (512, 256, 192), (768, 512, 448)]  # + the ragged-round shape, from the device
NT_SPLIT_SHAPE = (768, 512, 1024)  # 16 k-tiles, even: the smallest shape the split tail really cuts
NT_CONV = [(4, 8, 8, 64, 256), (256, 5, 7, 128, 256)]  # (nimg, h, w, c, cout)
LINBWD_SHAPES = [(256, 256, 256), (512, 256, 768), (768, 512, 256)]
W256_SHAPES = [(256, 256), (512, 256)]
W256_K = (8, 40, 264, 1000)
CONVN_SHAPES = [(1, 64, 16, 16), (4, 64, 8, 8), (16, 64, 7, 16), (1, 64, 4, 64), (8, 128, 1, 32), (2, 128, 8, 16)]
W3N_SHAPES = [(n, c, co, h, w) for c, ws in ((64, (4, 28, 56)), (128, (4, 28))) for w in ws
              for (n, h, co) in ((1, 4, 64), (3, 8, 128), (1, 8, 128), (3, 4, 64))]
CUS_NOMINAL = 256  # the CPU half's stand-in for multi_processor_count


def _nt_ragged(cus):
    """More tiles than CUs and a ragged last round: cus + 44 tiles of 256 x 256 at K = 128."""
    return ((cus + 44) * 256, 256, 128)


def _aff(family, c):
    """(scale, shift) of the affine + ReLU prologue: random for the bounded families; (1, 0), a plain
    ReLU, for the exact ones (their operands stay integers / bit patterns)."""
    if family in E.EXACT:
        return torch.ones(c), torch.zeros(c)
    g = torch.Generator().manual_seed(c)
    return torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.5


def _act(x, aff, dim=1):
    """What the prologue feeds the MFMA (as `_act` of test_gemm_gpu.py): one fp64 fma, then fp32, ReLU, bf16."""
    if aff is None:
        return x
    s, t = (v.to(x.device).double().view([-1 if i == dim else 1 for i in range(x.dim())]) for v in aff)
    return torch.relu((x.double() * s + t).float()).bfloat16()


def _nhwc(x):
    return x.contiguous(memory_format=torch.channels_last)


def _t(x):
    """x^T in row-major storage with canonical strides (a [1, n] result of .contiguous() may keep stride 1)."""
    return torch.empty(x.shape[1], x.shape[0], dtype=x.dtype, device=x.device).copy_(x.t())


def _rows(y):
    """[n, c, h, w] -> [n h w, c]."""
    return y.permute(0, 2, 3, 1).reshape(-1, y.shape[1])


def _done(errs):
    assert not errs, "\n".join(errs[:20]) + (f"\n... and {len(errs) - 20} more" if len(errs) > 20 else "")


# ============================================================================ CPU half
# (a) a float32 evaluation, rounded where the kernels round, meets every bound and reproduces the
#     exact families; (b) planted defects make the same checker fail.

def _emulate_all(tag, family, p, q, kred, errs, res=None, d=None):
    r, a = E.ref_gemm(p, q)
    acc = p.float() @ q.float().t()
    E.check_out(f"{tag} bf16", family, E.rn_bf16(acc), r, a, kred, "bf16", errs)
    E.check_out(f"{tag} f32", family, acc, r, a, kred, "f32", errs)
    if res is not None:
        E.check_out(f"{tag} res", family, E.rn_bf16(E.rn_bf16(acc).float() + res.float()), r, a, kred, "bf16", errs, res)
    if d is not None:
        _check_dh(f"{tag} dh", family, E.rn_bf16(E.rn_bf16(acc).float() * d.float()), r, a, kred, d, errs)
    return r


def _check_dh(name, family, got, r, a, kred, d, errs):
    """EPI 2: dh = bf16(bf16(R) d): 2^-8 |R d| + |d| (2^-8 |R| + Kred 2^-23 A)."""
    dd = d.double()
    if family in E.EXACT:
        E.check(name, got, r * dd, None, errs)
    else:
        E.check(name, got, r * dd, E.U8 * (r * dd).abs() + dd.abs() * (E.U8 * r.abs() + kred * E.E23 * a) + E.TINY, errs)


def _residual(family, m, n):
    g = torch.Generator().manual_seed(m * 31 + n)
    if family in E.EXACT:
        return (torch.randint(0, 3, (m, n), generator=g) - 1).bfloat16()
    return (torch.rand(m, n, generator=g) * 2 - 1).bfloat16()


def _deriv(family, m, n):
    """A stored GELU derivative for EPI 2: signed halves and ones for the exact families (products exact)."""
    g = torch.Generator().manual_seed(m * 37 + n)
    if family in E.EXACT:  # (gather: signs only, a half of the smallest normal pattern would be subnormal)
        half = torch.randint(0, 2 if family == "ternary" else 1, (m, n), generator=g)
        return ((torch.randint(0, 2, (m, n), generator=g) * 2 - 1) * 0.5 ** half).bfloat16()
    return E.gelu_exact((torch.rand(m, n, generator=g) * 6 - 3).bfloat16(), "tanh")[1].bfloat16()


@pytest.mark.parametrize("family", FAMILIES)
def test_emulation_meets_bounds_gemm_cpu(family):
    errs = []
    for m, n, k in GEMM_SHAPES + NT_SHAPES + [NT_SPLIT_SHAPE, _nt_ragged(CUS_NOMINAL)]:
        p, q = E.gemm_inputs(family, m, n, k, nnz=128)
        extra = {} if family == "gather" else {"res": _residual(family, m, n)}
        if m % 256 == 0:
            extra["d"] = _deriv(family, m, n)
        _emulate_all(f"gemm {m}x{n}x{k}", family, p, q, k, errs, **extra)
    for rows, co, ci in WGRAD_SHAPES:
        p, q = E.gemm_inputs(family, co, ci, rows)
        _emulate_all(f"wgrad rows{rows} {co}x{ci}", family, p, q, rows, errs)
    for m, n, k in MK_SHAPES + [(n * ((h + 1) // 2) * ((w + 1) // 2), co, ci) for n, h, w, ci, co in IMG_1X1]:
        p, q = E.gemm_inputs(family, m, n, k)
        _emulate_all(f"gemm {m}x{n}x{k}", family, p, q, k, errs)
    for (mo, no) in W256_SHAPES:
        for k in W256_K:
            p, q = E.gemm_inputs(family, mo, no, k)
            _emulate_all(f"wgrad256 {mo}x{no} k{k}", family, p, q, k, errs)
    for m, n, k in LINBWD_SHAPES:
        dy, x, w = E.linbwd_inputs(family, m, n, k)
        _emulate_all(f"linbwd dx {m},{n},{k}", family, dy, w.t(), n, errs)
        _emulate_all(f"linbwd dw {m},{n},{k}", family, dy.t(), x.t(), m, errs)
    _done(errs)


@pytest.mark.parametrize("family", FAMILIES)
def test_emulation_meets_bounds_conv_cpu(family):
    """The convolutions through im2col (forward, input gradient, weight gradient, stride 2). The two
    conv3x3n tail shapes are derived from the device's slot count and exist on the GPU only."""
    errs = []
    fwd = ([(n, c, h, w, c) for n, c, h, w in CONVN_SHAPES] + [(n, c, h, w, co) for n, h, w, c, co in NT_CONV]
           + [(n, c, h, w, co) for n, h, w, c, co in IMG_3X3])
    for n, c, h, w, co in fwd:
        x, wt = E.conv_inputs(family, n, c, h, w, co, nnz=64)
        _emulate_all(f"conv fwd {n},{c},{h},{w}->{co}", family, E.im2col(x), E.taps(wt), 9 * c, errs)
        if (n, c, h, w) in CONVN_SHAPES or co == 256:
            dy, wt = E.conv_inputs(family, n, c, h, w, co, nnz=64, dgrad=True)
            _emulate_all(f"conv dgrad {n},{co},{h},{w}->{c}", family, E.im2col(dy), E.taps_t(wt), 9 * co, errs)
        if (n, h, w, c, co) in IMG_3X3:
            _emulate_all(f"conv s2 {n},{c},{h},{w}->{co}", family, E.im2col(x, 2), E.taps(wt), 9 * c, errs)
    for n, c, co, h, w in W3N_SHAPES:
        x, dy = _wgrad_conv_inputs(family, n, c, co, h, w)
        _emulate_all(f"wgrad3x3 {n},{c},{co},{h},{w}", family, _rows(dy).t(), E.im2col(x).t(), n * h * w, errs)
    for n, h, w, ci, co in IMG_1X1 + IMG_3X3:  # the b_sub gather and the implicit-im2col weight gradients
        x, dy = _wgrad_conv_inputs(family, n, ci, co, h, w, 2)
        _emulate_all(f"b_sub {n},{h},{w},{ci}->{co}", family, _rows(dy).t(), _rows(x[:, :, ::2, ::2]).t(), dy.numel() // co, errs)
        if (n, h, w, ci, co) in IMG_3X3:
            _emulate_all(f"wgrad s2 {n},{h},{w},{ci}->{co}", family, _rows(dy).t(), E.im2col(x, 2).t(), dy.numel() // co, errs)
            x, dy = _wgrad_conv_inputs(family, n, ci, co, h, w, 1)
            _emulate_all(f"wgrad s1 {n},{h},{w},{ci}->{co}", family, _rows(dy).t(), E.im2col(x).t(), dy.numel() // co, errs)
    _done(errs)


def test_gather_closed_forms_cpu():
    """The gather family's float64 reference IS the closed form: a GEMM output row i is Q row pi(i),
    y[n, co, h, w] = x[n, pi(co), h + dy, w + dx] with exact zeros on the border for tap co mod 9
    (all nine padding cases), and the same for the input gradient with the flipped taps."""
    p, q = E.gemm_inputs("gather", 200, 72, 520)
    assert torch.equal(E.ref_gemm(p, q)[0], q.double()[:, E.perm(200, 520)].t())
    n, c, h, w = 2, 64, 5, 7
    for dgrad in (False, True):
        x, wt = E.conv_inputs("gather", n, c, h, w, c, dgrad=dgrad)
        r = E.ref_gemm(E.im2col(x), E.taps_t(wt) if dgrad else E.taps(wt))[0].view(n, h, w, c)
        xp = torch.nn.functional.pad(x.double(), (1, 1, 1, 1))
        pi = E.perm(c, c)
        for o in range(c):
            dy, dx = (o % 9) // 3, o % 3
            assert torch.equal(r[..., o], xp[:, pi[o], dy:dy + h, dx:dx + w]), (dgrad, o)
        assert len(set(x.view(torch.int16).flatten().tolist())) == x.numel()  # distinct bit patterns


DEFECTS = ("zero_row_segment", "missing_ktile", "transposed_fragment", "truncation", "duplicated_split")


def test_planted_defects_fail_cpu():
    """At 1024 x 768 x 768 the clean float32 result passes and each planted defect fails the checker;
    a 3x3 tap that reads one pixel past the right border fails it too."""
    for family in ("uniform", "cancel"):
        p, q = E.gemm_inputs(family, 1024, 768, 768)
        r, a = E.ref_gemm(p, q)
        acc = p.float() @ q.float().t()
        errs = []
        E.check_out("clean", family, E.rn_bf16(acc), r, a, 768, "bf16", errs)
        _done(errs)
        for kind in DEFECTS:
            if kind == "truncation" and family == "cancel":
                continue  # |R| << A there: the output rounding is below the accumulation term by design
            errs = []
            E.check_out(kind, family, E.defect(kind, acc, p, q), r, a, 768, "bf16", errs)
            assert errs, f"{family}: planted defect {kind} passed the checker"
            print(errs[0])
    x, wt = E.conv_inputs("uniform", 4, 64, 8, 8, 64)
    r, a = E.ref_gemm(E.im2col(x), E.taps(wt))
    errs = []
    E.check_out("clean conv", "uniform", E.rn_bf16(E.im2col(x).float() @ E.taps(wt).float().t()), r, a, 576, "bf16", errs)
    _done(errs)
    E.check_out("shifted tap", "uniform", E.rn_bf16(E.shifted_tap_conv(x, wt)), r, a, 576, "bf16", errs)
    assert errs, "a tap shifted by one pixel at the border passed the checker"
    for family in E.EXACT:  # the exact families see a single wrong index
        p, q = E.gemm_inputs(family, 256, 256, 128)
        r, a = E.ref_gemm(p, q)
        errs = []
        E.check_out("t", family, E.defect("transposed_fragment", p.float() @ q.float().t(), p, q), r, a, 128, "bf16", errs)
        assert errs, family


@pytest.mark.parametrize("form", ["tanh", "erf"])
def test_gelu_emulation_within_half_c_cpu(form):
    """The float32 emulation of the fast GELU and its derivative over all finite bf16 inputs stays within
    c / 2 of float64 (finite everywhere: the derivative's x^2 factor is clamped, as in gelu_tanh.h)."""
    x = E.all_finite_bf16().reshape(-1)
    assert torch.isfinite(x.float()).all() and len(set(x.view(torch.int16).tolist())) == 65536 - 2 * 128
    for name, got, ref in zip("gd", E.gelu_emulated(x, form), E.gelu_exact(x, form)):
        assert torch.isfinite(got.float()).all(), (form, name)
        ratio = float(((got.double() - ref).abs() / E.gelu_bound(ref, 1)).max())
        print(f"{form} {name}: ratio {ratio:.3f} (c = {GELU_C[form, name]})")
        assert GELU_C[form, name] == math.ceil(2 * GELU_RATIO[form, name])
        assert ratio <= GELU_C[form, name] / 2


# ============================================================================ GPU: gemm.hip / gemm_glds.hip

def _gemm_case(errs, tag, family, m, n, k, engine, nbuf, *, ak=True, bk=True, kind="plain", a_aff=False,
               b_aff=False, splits=1, nnz=256):
    """One launch of ops.gemm.gemm on ``C = P Q^T`` in the given storage layout, output inside a guard
    band (ldc = N + 8), checked per element. kind: plain (bf16), stats, residual, f32 (mode 3 partials)."""
    from fluxmpi_amd.ops import gemm as G
    p, q = (t.cuda() for t in E.gemm_inputs(family, m, n, k, nnz=128 if kind == "residual" else nnz))
    aa = _aff(family, k) if a_aff else None   # per k on the K-major A (forward)
    ba = _aff(family, n) if b_aff else None   # per n on the N-major B (weight gradient)
    r, a = E.ref_gemm(_act(p, aa, 1), _act(q, ba, 0))
    sa = p if ak else _t(p)
    sb = q if bk else _t(q)
    ldc = n + 8
    kw = dict(M=m, N=n, K=k, lda=sa.shape[1], ldb=sb.shape[1], ldc=ldc, a_kmajor=ak, b_kmajor=bk, engine=engine,
              nbuf=nbuf, a_affine=None if aa is None else tuple(t.cuda() for t in aa),
              b_affine=None if ba is None else tuple(t.cuda() for t in ba))
    if kind in ("f32", "atomic"):  # mode 3: a [splits, M, ldc] workspace of partials; mode 2: atomics into a zeroed C
        s = G._actual_splits(k, splits)
        parts = s if kind == "f32" else 1
        buf, view = E.guarded(parts * m, n, ldc, torch.float32, "cuda", fill=float("nan") if kind == "f32" else 0.0)
        G.gemm(sa, sb, view, mode=3 if kind == "f32" else 2, splits=s, **kw)
        out = E.take_guarded(tag, buf, view, errs).view(parts, m, n).double().sum(0)
        E.check_out(tag, family, out, r, a, k, "f32", errs)
        return
    buf, view = E.guarded(m, n, ldc, torch.bfloat16, "cuda")
    res = stats = None
    if kind == "residual":
        res = torch.zeros(m, ldc, dtype=torch.bfloat16, device="cuda")[:, :n]
        res.copy_(_residual(family, m, n))
    if kind == "stats":
        stats = torch.zeros(G.SHARDS, 2, n, device="cuda")
    G.gemm(sa, sb, view, mode=1 if stats is not None else 0, stats=stats, residual=res, **kw)
    out = E.take_guarded(tag, buf, view, errs)
    E.check_out(tag, family, out, r, a, k, "bf16", errs, res)
    if stats is not None and family != "gather":
        E.check_colsums(tag, family, stats, out, errs)


def _admits(engine, m, n, k=0, aff=False):
    """Engines 7 / 8 take their 256x128 tiles only for M > 128 and N > 64; the LDS-DMA kernel stages a
    prologue affine of at most 512 channels (the launcher refuses more)."""
    return (engine not in (7, 8) or (m > 128 and n > 64)) and not (aff and engine >= 2 and k > 512)


@gpu
@pytest.mark.parametrize("kind", ["plain", "stats", "affine", "affine_stats"])
@pytest.mark.parametrize("engine,nbuf", ENGINES, ids=ENGINE_IDS)
def test_gemm_forward_layout(gpu_ext, engine, nbuf, kind):
    """Y = act(X) W^T, both operands K-major: every engine, plain / statistics epilogue, with and without
    the affine + ReLU prologue (engines 7 / 8 have no prologue variant: they run their 128-tile choice)."""
    errs = []
    for m, n, k in GEMM_SHAPES:
        if not _admits(engine, m, n, k, kind.startswith("affine")):
            continue
        for family in FAMILIES:
            _gemm_case(errs, f"{family} {m}x{n}x{k}", family, m, n, k, engine, nbuf, a_aff=kind.startswith("affine"),
                       kind="stats" if kind.endswith("stats") else "plain")
    _done(errs)


@gpu
@pytest.mark.parametrize("engine,nbuf", ENGINES, ids=ENGINE_IDS)
def test_gemm_residual(gpu_ext, engine, nbuf):
    """bf16(bf16(A B) + r): gemm.hip compiles it for the input-gradient layout (N-major B), the LDS-DMA
    engines for K-major B."""
    errs = []
    for m, n, k in GEMM_SHAPES:
        if not _admits(engine, m, n):
            continue
        for family in ("uniform", "cancel", "ternary"):
            _gemm_case(errs, f"{family} {m}x{n}x{k}", family, m, n, k, engine, nbuf, bk=engine != 1, kind="residual")
    _done(errs)


@gpu
@pytest.mark.parametrize("nbuf", [0, 1, 2])
def test_gemm_dgrad_layout(gpu_ext, nbuf):
    """dX = dY W with W N-major (transposed LDS reads of B), gemm.hip."""
    errs = []
    for m, n, k in GEMM_SHAPES:
        for family in FAMILIES:
            _gemm_case(errs, f"{family} {m}x{n}x{k}", family, m, n, k, 1, nbuf, bk=False)
    _done(errs)


MK_SHAPES = [(8, 24, 8), (24, 64, 24), (64, 72, 40), (72, 8, 64), (136, 520, 72), (192, 40, 520)]


@gpu
@pytest.mark.parametrize("nbuf", [0, 1, 2])
def test_gemm_mmajor_a_kmajor_b(gpu_ext, nbuf):
    """The fourth storage combination of gemm.hip (A M-major, B K-major), which only ops.gemm.gemm itself
    reaches: M and K multiples of 8."""
    errs = []
    for m, n, k in MK_SHAPES:
        for family in FAMILIES:
            _gemm_case(errs, f"{family} {m}x{n}x{k}", family, m, n, k, 1, nbuf, ak=False, bk=True)
    _done(errs)


@gpu
@pytest.mark.parametrize("kind", ["bf16", "f32_s1", "f32_s3", "f32_s7", "f32_s3_affine", "bf16_affine", "atomic_s3"])
@pytest.mark.parametrize("nbuf", [0, 1, 2])
def test_gemm_wgrad_layout(gpu_ext, nbuf, kind):
    """dW = dY^T act(X), both operands M- / N-major (transposed LDS reads of both), the reduction over
    the rows: bf16 store, fp32 split-K partials at 1, 3 and 7 splits (mode 3), fp32 atomics into a zeroed
    C (mode 2, which no wrapper uses), the affine + ReLU prologue on B."""
    errs = []
    for rows, co, ci in WGRAD_SHAPES:
        for family in FAMILIES:
            _gemm_case(errs, f"{family} rows{rows} {co}x{ci}", family, co, ci, rows, 1, nbuf, ak=False, bk=False,
                       kind=kind.split("_")[0] if "_s" in kind else "plain", b_aff=kind.endswith("affine"),
                       splits=int(kind.split("_s")[1][0]) if "_s" in kind else 1)
    _done(errs)


def _wgrad_conv_inputs(family, n, c, co, h, w, stride=1):
    """Image x [n, c, h, w] and output gradient dy [n, co, ho, wo] of a weight gradient, whose reduction
    runs over the output pixels: dy^T [co, pixels] is the P side of ``gemm_inputs`` (paired, sparse or one-hot
    along the pixels). The other operand is an im2col of x, which cannot be prescribed entry by entry, so x
    itself is drawn per family: uniform; nearly constant along each image row (cancel: horizontally
    adjacent pixels, the pairs of P, then see nearly equal rows); ternary; distinct bit patterns."""
    ho, wo = (h + stride - 1) // stride, (w + stride - 1) // stride
    px = n * ho * wo
    dyt, _ = E.gemm_inputs(family, co, 1, px, seed=c + h)
    g = E._gen("wgx", family, n, c, h, w)
    if family == "uniform":
        x = E._uni(g, n, c, h, w)
    elif family == "cancel":  # the image is constant over horizontal output-pixel pairs only approximately:
        x = E._uni(g, n, c, h, 1).expand(n, c, h, w) + 2.0 ** -6 * E._uni(g, n, c, h, w)
    elif family == "ternary":
        x = (torch.randint(0, 3, (n, c, h, w), generator=g) - 1).float()
    else:
        x = E.patterns(n, c, h, w).float()
    dy = dyt.float().t().reshape(n, ho, wo, co).permute(0, 3, 1, 2)
    return x.bfloat16().contiguous(), dy.bfloat16().contiguous()


@gpu
@pytest.mark.parametrize("engine", range(2, 10))
def test_gemm_a_sub_gather(gpu_ext, engine):
    """a_sub: the stride-2 1x1 convolution, A rows gathered from the even pixels (odd image sizes too),
    with the statistics epilogue."""
    from fluxmpi_amd.ops import gemm as G
    errs = []
    for n, h, w, ci, co in IMG_1X1:
        ho, wo = (h + 1) // 2, (w + 1) // 2
        m = n * ho * wo
        for family in FAMILIES:
            p, q = (t.cuda() for t in E.gemm_inputs(family, m, co, ci))
            x = (E.patterns(n, h, w, ci) if family == "gather" else torch.full((n, h, w, ci), 3.0).bfloat16()).cuda()
            x[:, ::2, ::2] = p.view(n, ho, wo, ci)  # the odd pixels hold values that no family produces
            r, a = E.ref_gemm(p, q)
            buf, view = E.guarded(m, co, co + 8, torch.bfloat16, "cuda")
            stats = torch.zeros(G.SHARDS, 2, co, device="cuda")
            G.gemm(x.view(-1, ci), q, view, M=m, N=co, K=ci, lda=ci, ldb=ci, ldc=co + 8, mode=1, stats=stats,
                   a_sub=(h, w), engine=engine)
            tag = f"{family} {n},{h},{w},{ci}->{co}"
            out = E.take_guarded(tag, buf, view, errs)
            E.check_out(tag, family, out, r, a, ci, "bf16", errs)
            if family != "gather":
                E.check_colsums(tag, family, stats, out, errs)
    _done(errs)


CONV_ENGINES = [(e, b, s) for s in (1, 2) for e, b in [(0, 0)] + ENGINES if not (s == 2 and e == 1)]


@gpu
@pytest.mark.parametrize("engine,nbuf,stride", CONV_ENGINES, ids=[f"engine{e}-nbuf{b}-stride{s}" for e, b, s in CONV_ENGINES])
def test_gemm_implicit_3x3(gpu_ext, engine, nbuf, stride):
    """The implicit 3x3 / pad 1 convolution at stride 1 (every engine; gemm.hip's CONV kernel for engine
    1) and stride 2 (gemm_glds.hip only: no engine 1), with statistics; stride 1 also behind the
    affine + ReLU prologue (the zero padding stays zero)."""
    from fluxmpi_amd.ops import gemm as G
    errs = []
    for n, h, w, c, co in IMG_3X3:
        ho, wo = (h + stride - 1) // stride, (w + stride - 1) // stride
        m = n * ho * wo
        if not _admits(engine, m, co):
            continue
        for family in FAMILIES:
            for aff in ((False, True) if stride == 1 and engine not in (7, 8) else (False,)):
                x, wt = (t.cuda() for t in E.conv_inputs(family, n, c, h, w, co, nnz=64))
                af = _aff(family, c) if aff else None
                r, a = E.ref_gemm(E.im2col(_act(x, af, 1), stride), E.taps(wt))
                buf, view = E.guarded(m, co, co + 8, torch.bfloat16, "cuda")
                stats = torch.zeros(G.SHARDS, 2, co, device="cuda")
                G.gemm(_rows(x).contiguous(), E.taps(wt).contiguous(), view, M=m, N=co, K=9 * c, lda=c, ldb=9 * c,
                       ldc=co + 8, mode=1, stats=stats, conv=(h, w, c), conv_stride=stride, engine=engine, nbuf=nbuf,
                       a_affine=None if af is None else tuple(t.cuda() for t in af))
                tag = f"{family} {n},{c},{h},{w}->{co} aff{int(aff)}"
                out = E.take_guarded(tag, buf, view, errs)
                E.check_out(tag, family, out, r, a, 9 * c, "bf16", errs)
                if family != "gather":
                    E.check_colsums(tag, family, stats, out, errs)
    _done(errs)


@gpu
@pytest.mark.parametrize("remap", [True, False], ids=["remap", "dispatch_order"])
@pytest.mark.parametrize("splits", [1, 3, 7])
@pytest.mark.parametrize("variant", [1, 2])
def test_gemm_wgrad_v2(gpu_ext, variant, splits, remap, monkeypatch):
    """gemm_glds.hip's weight-gradient kernel (WGRAD_VARIANT 1 and 2) at 1, 3 and 7 splits: the plain
    dY^T X, the b_sub stride-2 gather, and the implicit im2col B at stride 1 and 2; fp32 and bf16 out."""
    from fluxmpi_amd.ops import gemm as G
    monkeypatch.setattr(G, "WGRAD_VARIANT", variant)
    monkeypatch.setattr(G, "WGRAD_REMAP", remap)
    errs = []
    for rows, co, ci in WGRAD_SHAPES:
        for family in FAMILIES:
            p, q = (t.cuda() for t in E.gemm_inputs(family, co, ci, rows))
            r, a = E.ref_gemm(p, q)
            for dt in (torch.float32, torch.bfloat16):
                dw = G.conv1x1_wgrad_v2(_t(p), _t(q), out_dtype=dt, splits=splits)
                E.check_out(f"{family} rows{rows} {co}x{ci} {dt}", family, dw, r, a, rows,
                            "f32" if dt == torch.float32 else "bf16", errs)
    for n, h, w, ci, co in IMG_1X1 + IMG_3X3:
        for family in FAMILIES:
            x, dy = (t.cuda() for t in _wgrad_conv_inputs(family, n, ci, co, h, w, 2))
            xs = x[:, :, ::2, ::2]
            r, a = E.ref_gemm(_rows(dy).t(), _rows(xs).t())
            dw = G.conv1x1_wgrad_s2(_rows(dy).contiguous(), _nhwc(x), out_dtype=torch.float32, splits=splits)
            E.check_out(f"{family} b_sub {n},{h},{w},{ci}->{co}", family, dw, r, a, dy.numel() // co, "f32", errs)
    for n, h, w, ci, co in IMG_3X3:
        for stride in (1, 2):
            for family in FAMILIES:
                x, dy = (t.cuda() for t in _wgrad_conv_inputs(family, n, ci, co, h, w, stride))
                r, a = E.ref_gemm(_rows(dy).t(), E.im2col(x, stride).t())
                fn = G.conv3x3_wgrad if stride == 1 else G.conv3x3_wgrad_s2
                dw = fn(_nhwc(dy), _nhwc(x), splits=splits)  # [co, ci, 3, 3] bf16
                E.check_out(f"{family} 3x3 s{stride} {n},{h},{w},{ci}->{co}", family, E.taps(dw), r, a, dy.numel() // co,
                            "bf16", errs)
    _done(errs)


# ============================================================================ GPU: gemm_nt.hip

@pytest.fixture
def nt_split():
    from fluxmpi_amd.ops import gemm_nt as G
    prev = G.get_split()
    yield G._set_split
    G._set_split(prev)


def _nt(epi, p, q, errs, tag, bias=None, h=None, stats=None):
    """gemm_nt through its binding, every output in a guard band (ldc = N + 8). Returns the outputs."""
    from fluxmpi_amd.ops import _ext
    from fluxmpi_amd.ops.gelu import _sync
    C = _ext.get(required=True)
    m, k = p.shape
    n = q.shape[0]
    ldc = n + 8
    buf, view = E.guarded(m, n, ldc, torch.bfloat16, "cuda")
    buf2, view2 = E.guarded(m, n, ldc, torch.bfloat16, "cuda") if epi == 1 else (None, None)
    part = None
    if epi == 2:
        rows = C.gemm_nt_colpart_rows(m)
        pbuf, part = E.guarded(rows, n, n, torch.float32, "cuda")
        hb = torch.zeros(m, ldc, device="cuda", dtype=torch.bfloat16)  # the derivative is laid out as C
        hb[:, :n] = h
        h = hb
    if epi == 1:
        _sync(C)
    s = torch.cuda.current_stream().cuda_stream
    if epi == 3:
        C.gemm_nt_stats(p.data_ptr(), q.data_ptr(), view.data_ptr(), stats.data_ptr(), k, k, ldc, m, n, k, s)
    else:
        C.gemm_nt(p.data_ptr(), q.data_ptr(), view.data_ptr(), view2.data_ptr() if epi == 1 else 0,
                  bias.data_ptr() if bias is not None else 0, int(bias is not None and bias.dtype == torch.float32),
                  h.data_ptr() if epi == 2 else 0, part.data_ptr() if epi == 2 else 0, k, k, ldc, m, n, k, epi, s)
    out = [E.take_guarded(tag, buf, view, errs)]
    if epi == 1:
        out.append(E.take_guarded(tag + " c2", buf2, view2, errs))
    if epi == 2:
        out.append(E.take_guarded(tag + " colpart", pbuf, part, errs))
    return out


_NT_CACHE = {}


def _nt_inputs(family, m, n, k):
    key = (family, m, n, k)
    if key not in _NT_CACHE:
        p, q = (t.cuda() for t in E.gemm_inputs(family, m, n, k, nnz=64))
        _NT_CACHE[key] = (p, q) + E.ref_gemm(p, q)
    return _NT_CACHE[key]


def _nt_shapes():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return NT_SHAPES + [_nt_ragged(cus)]


def _bias(kind, family, n):
    if kind is None:
        return None
    g = torch.Generator().manual_seed(n)
    b = (torch.randint(0, 3, (n,), generator=g) - 1).float() if family in E.EXACT else torch.randn(n, generator=g) * 0.5
    return b.to(torch.float32 if kind == "f32" else torch.bfloat16).cuda()


def _nt_epi0(errs, tag, family, m, n, k, bias_kind):
    p, q, r, a = _nt_inputs(family, m, n, k)
    b = _bias(bias_kind, family, n)
    if family == "gather" and b is not None:
        return  # a bias on bit patterns is an addition, not a move: the bounded families cover it
    rb = r if b is None else r + b.double()
    ab = a if b is None else a + b.double().abs()
    (y,) = _nt(0, p, q, errs, tag, bias=b)
    E.check_out(tag, family, y, rb, ab, k, "bf16", errs)


@gpu
@pytest.mark.parametrize("split", [0, 2, 8])
@pytest.mark.parametrize("bias", [None, "f32", "bf16"])
def test_gemm_nt_epi0(gpu_ext, nt_split, bias, split):
    """EPI 0 (+ bias absent / fp32 / bf16) at every shape; with the split tail requested the two largest
    listed shapes (7 and 2 k-tiles: the launcher never cuts an odd or short K) and the one it does cut."""
    nt_split(split)
    errs = []
    shapes = _nt_shapes() if split == 0 else _nt_shapes()[-2:] + [NT_SPLIT_SHAPE]
    for m, n, k in shapes:
        for family in FAMILIES:
            _nt_epi0(errs, f"{family} {m}x{n}x{k} bias {bias} split {split}", family, m, n, k, bias)
    _done(errs)


@gpu
@pytest.mark.parametrize("split", [0, 2, 8])
def test_gemm_nt_epi2_epi3_plain_ldc(gpu_ext, nt_split, split):
    """EPI 2 (dh = bf16(dx) gelu'(h) and the bias-gradient partials), EPI 3 (statistics shards) and
    gemm_plain with ldc > N, unsplit and under the split tail."""
    from fluxmpi_amd.ops import gemm as GM
    from fluxmpi_amd.ops import gemm_nt as G
    nt_split(split)
    errs = []
    shapes = _nt_shapes() if split == 0 else _nt_shapes()[-2:] + [NT_SPLIT_SHAPE]
    for m, n, k in shapes:
        for family in FAMILIES:
            p, q, r, a = _nt_inputs(family, m, n, k)
            tag = f"{family} {m}x{n}x{k} split {split}"
            d = _deriv(family, m, n).cuda()
            dh, part = _nt(2, p, q, errs, tag + " EPI2", h=d)
            _check_dh(tag + " dh", family, dh, r, a, k, d, errs)
            if family != "gather":
                E.check_colsums(tag + " db", family, part, dh, errs, squares=False)
            stats = torch.zeros(GM.SHARDS, 2, n, device="cuda")
            (y,) = _nt(3, p, q, errs, tag + " EPI3", stats=stats)
            E.check_out(tag + " EPI3", family, y, r, a, k, "bf16", errs)
            if family != "gather":
                E.check_colsums(tag + " EPI3", family, stats, y, errs)
            buf, view = E.guarded(m, n, n + 16, torch.bfloat16, "cuda")
            G.gemm_plain(p, q, view)
            E.check_out(tag + " gemm_plain", family, E.take_guarded(tag, buf, view, errs), r, a, k, "bf16", errs)
    _done(errs)


@gpu
@pytest.mark.parametrize("bias", ["f32", "bf16"])
@pytest.mark.parametrize("form", ["tanh", "erf"])
def test_gemm_nt_epi1_bounds(gpu_ext, form, bias):
    """EPI 1 at every shape: both outputs are functions of h = bf16(x W^T + b), which is not stored; they
    must equal the GELU (within the measured c) of SOME bf16 h inside the EPI 0 bound, so both are checked
    against the float64 GELU of the nearest-rounded reference with the bound's slack propagated through
    the largest slope (|gelu'| <= 1.13, |gelu''| <= 0.8, each times 1 + c 2^-8 for the move of the
    relative term: 1.2 and 1.0)."""
    from fluxmpi_amd.ops import gelu as GL
    old = GL.FORM
    GL.set_form(form)
    try:
        errs = []
        for m, n, k in _nt_shapes():
            for family in ("uniform", "cancel", "ternary"):
                p, q, r, a = _nt_inputs(family, m, n, k)
                b = _bias(bias, family, n)
                rb, ab = r + b.double(), a + b.double().abs()
                d, g = _nt(1, p, q, errs, f"{family} {m}x{n}x{k}", bias=b)
                slack = E.bound(rb, ab, k, "bf16") if family not in E.EXACT else torch.zeros_like(rb)
                h = rb.bfloat16() if family in E.EXACT else rb
                rg, rd = E.gelu_exact(h, form)
                E.check(f"{family} {m}x{n}x{k} gelu", g, rg, E.gelu_bound(rg, GELU_C[form, "g"]) + 1.2 * slack, errs)
                E.check(f"{family} {m}x{n}x{k} gelu'", d, rd, E.gelu_bound(rd, GELU_C[form, "d"]) + 1.0 * slack, errs)
        _done(errs)
    finally:
        GL.set_form(old)


@gpu
@pytest.mark.parametrize("form", ["tanh", "erf"])
def test_gemm_nt_gelu_all_bf16_inputs(gpu_ext, form):
    """M = N = K = 256, one-hot x rows, W all 65536 bf16 bit patterns (non-finite ones made finite): every
    bf16 pre-activation reaches the EPI 1 epilogue exactly once; gelu and gelu' against float64."""
    from fluxmpi_amd.ops import gelu as GL
    old = GL.FORM
    GL.set_form(form)
    try:
        w = E.all_finite_bf16().cuda()  # [n, k]
        x = torch.zeros(256, 256)
        x[torch.arange(256), E.perm(256, 256)] = 1.0
        x = x.bfloat16().cuda()
        h = w[:, E.perm(256, 256).cuda()].t().contiguous()  # h[i, j] = w[j, pi(i)]
        errs = []
        (y,) = _nt(0, x, w, errs, "EPI 0")
        E.check("pre-activation", y, h.double(), None, errs)
        d, g = _nt(1, x, w, errs, "EPI 1")
        rg, rd = E.gelu_exact(h, form)
        E.check("gelu", g, rg, E.gelu_bound(rg, GELU_C[form, "g"]), errs)
        E.check("gelu'", d, rd, E.gelu_bound(rd, GELU_C[form, "d"]), errs)
        _done(errs)
    finally:
        GL.set_form(old)


@gpu
@pytest.mark.parametrize("split", [0, 2, 8])
@pytest.mark.parametrize("nimg,h,w,c,co", NT_CONV)
def test_gemm_nt_conv3x3(gpu_ext, nt_split, monkeypatch, nimg, h, w, c, co, split):
    """conv3x3 on the 256x256 kernel: plain, with statistics (EPI 3) and with a residual (EPI 4),
    MIN_TILES / MIN_K zeroed."""
    from fluxmpi_amd.ops import gemm as GM
    from fluxmpi_amd.ops import gemm_nt as G
    monkeypatch.setattr(G, "MIN_TILES", 0)
    monkeypatch.setattr(G, "MIN_K", 0)
    monkeypatch.setattr(G, "CONV", True)
    nt_split(split)
    m = nimg * h * w
    errs = []
    for family in FAMILIES:
        x, wt = (t.cuda() for t in E.conv_inputs(family, nimg, c, h, w, co, nnz=64))
        xs, tp = _nhwc(x), E.taps(wt).contiguous()
        assert G.conv_ok(m, c, co, xs, tp)
        r, a = E.ref_gemm(E.im2col(x), tp)
        for with_stats in (False, True):
            y = torch.full((m, co), float("nan"), device="cuda", dtype=torch.bfloat16)
            stats = torch.zeros(GM.SHARDS, 2, co, device="cuda") if with_stats else None
            G.conv3x3(xs, tp, y, stats)
            tag = f"{family} fwd stats{int(with_stats)}"
            E.check_out(tag, family, y, r, a, 9 * c, "bf16", errs)
            if with_stats and family != "gather":
                E.check_colsums(tag, family, stats, y, errs)
        if family != "gather":  # EPI 4: bf16(bf16(conv) + r)
            res = _residual(family, m, co).cuda()
            yr = torch.full((m, co), float("nan"), device="cuda", dtype=torch.bfloat16)
            G.conv3x3(xs, tp, yr, residual=res)
            E.check_out(f"{family} fwd + residual", family, yr, r, a, 9 * c, "bf16", errs, res)
            if not torch.equal(yr, (y.float() + res.float()).bfloat16()):
                errs.append(f"{family}: EPI 4 is not bf16(EPI 0 + r)")
    _done(errs)


@gpu
@pytest.mark.parametrize("split", [0, 8])
def test_gemm_nt_conv3x3_dgrad_residual(gpu_ext, nt_split, split):
    """The input gradient on the same kernel (the flipped transposed filter as B), plain and with the
    residual summand (EPI 4), at (256, 5, 7, 256 -> 256): 9 * 256 / 64 = 36 k-tiles, which the split cuts."""
    from fluxmpi_amd.ops import gemm_nt as G
    nt_split(split)
    nimg, h, w, c, co = 256, 5, 7, 256, 256
    m = nimg * h * w
    errs = []
    for family in FAMILIES:
        dy, wt = (t.cuda() for t in E.conv_inputs(family, nimg, c, h, w, co, nnz=64, dgrad=True))
        tp = E.taps_t(wt).contiguous()
        r, a = E.ref_gemm(E.im2col(dy), tp)
        dx = torch.full((m, c), float("nan"), device="cuda", dtype=torch.bfloat16)
        G.conv3x3(_nhwc(dy), tp, dx)
        E.check_out(f"{family} dgrad", family, dx, r, a, 9 * co, "bf16", errs)
        if family != "gather":
            res = _residual(family, m, c).cuda()
            dxr = torch.full((m, c), float("nan"), device="cuda", dtype=torch.bfloat16)
            G.conv3x3(_nhwc(dy), tp, dxr, residual=res)
            E.check_out(f"{family} dgrad + residual", family, dxr, r, a, 9 * co, "bf16", errs, res)
            if not torch.equal(dxr, (dx.float() + res.float()).bfloat16()):
                errs.append(f"{family}: EPI 4 is not bf16(EPI 0 + r)")
    _done(errs)


# ============================================================================ GPU: linbwd.hip, wgrad256.hip

@gpu
@pytest.mark.parametrize("splits,first", [(1, 0), (1, 1), (3, 0), (3, 1), (7, 0), (7, 1)])
@pytest.mark.parametrize("m,n,k", LINBWD_SHAPES)
def test_linbwd(gpu_ext, m, n, k, splits, first):
    """dx (bf16, lddx = K + 8 inside a guard band) and the weight gradient's fp32 partials (guarded
    workspace; 3 and 7 splits leave the last one shorter) of one launch, both grid orders."""
    C = gpu_ext
    errs = []
    for family in FAMILIES:
        dy, x, w = (t.cuda() for t in E.linbwd_inputs(family, m, n, k))
        s = C.linear_bwd_splits(m, n, k, splits)
        lddx = k + 8
        buf, dx = E.guarded(m, k, lddx, torch.bfloat16, "cuda")
        wbuf, ws = E.guarded(s * n, k, k, torch.float32, "cuda")
        C.linear_bwd(dy.data_ptr(), x.data_ptr(), w.data_ptr(), dx.data_ptr(), ws.data_ptr(), m, n, k, n, k, k, lddx,
                     splits, first, torch.cuda.current_stream().cuda_stream)
        r, a = E.ref_gemm(dy, w.t())
        E.check_out(f"{family} dx", family, E.take_guarded("dx", buf, dx, errs), r, a, n, "bf16", errs)
        r, a = E.ref_gemm(dy.t(), x.t())
        dw = E.take_guarded("ws", wbuf, ws, errs).view(s, n, k).double().sum(0)
        E.check_out(f"{family} dw", family, dw, r, a, m, "f32", errs)
    _done(errs)


@pytest.fixture
def w256_variant(gpu_ext):
    yield gpu_ext.wgrad256_set_variant
    gpu_ext.wgrad256_set_variant(4)


@gpu
@pytest.mark.parametrize("variant", range(5))
def test_wgrad256(gpu_ext, w256_variant, variant):
    """C [M, N] = A^T B on 256 x 256 tiles, every pipeline variant, reductions of 8, 40, 264 and 1000 rows
    (partial and sub-tile k-steps) at 1 and 3 splits; fp32 partials in a guarded workspace."""
    C = gpu_ext
    w256_variant(variant)
    errs = []
    for mo, no in W256_SHAPES:
        for k in W256_K:
            for family in FAMILIES:
                p, q = (t.cuda() for t in E.gemm_inputs(family, mo, no, k))
                r, a = E.ref_gemm(p, q)
                at, bt = _t(p), _t(q)
                assert C.wgrad256_supported(mo, no, k, mo, no)
                for splits in (1, 3):
                    s = C.wgrad256_actual_splits(k, splits)
                    buf, ws = E.guarded(s * mo, no, no, torch.float32, "cuda")
                    C.gemm_wgrad256(at.data_ptr(), bt.data_ptr(), ws.data_ptr(), mo, no, mo, no, k, splits,
                                    torch.cuda.current_stream().cuda_stream)
                    tag = f"{family} {mo}x{no} k{k} splits{splits}"
                    out = E.take_guarded(tag, buf, ws, errs).view(s, mo, no).double().sum(0)
                    E.check_out(tag, family, out, r, a, k, "f32", errs)
    _done(errs)


# ============================================================================ GPU: conv3x3n.hip, wgrad3x3n.hip

def _convn_case(errs, n, c, h, w):
    from fluxmpi_amd.ops import gemm as G
    m = n * h * w
    for family in FAMILIES:
        x, wt = (t.cuda() for t in E.conv_inputs(family, n, c, h, w, c, nnz=64))
        xs, wc = _nhwc(x), _nhwc(wt)
        assert G.conv_n_ok(m, c, c, h, w, xs, E.taps(wt).contiguous(), xs)
        r, a = E.ref_gemm(E.im2col(x), E.taps(wt))
        outs = []
        for with_stats in (False, True):
            y = torch.full((n, h, w, c), float("nan"), device="cuda", dtype=torch.bfloat16).permute(0, 3, 1, 2)
            stats = torch.zeros(G.SHARDS, 2, c, device="cuda") if with_stats else None
            G.conv3x3_fwd(xs, wc, stats=stats, out=y)
            tag = f"{family} {n},{c},{h},{w} fwd stats{int(with_stats)}"
            E.check_out(tag, family, _rows(y), r, a, 9 * c, "bf16", errs)
            if with_stats and family != "gather":
                E.check_colsums(tag, family, stats, _rows(y), errs)
            outs.append(y)
        if not torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)):
            errs.append(f"{family} {n},{c},{h},{w}: the statistics epilogue changed the output")
        dy, wt = (t.cuda() for t in E.conv_inputs(family, n, c, h, w, c, nnz=64, dgrad=True))
        wc = _nhwc(wt)
        G.note_filter(wc)
        dx = torch.full((n, h, w, c), float("nan"), device="cuda", dtype=torch.bfloat16).permute(0, 3, 1, 2)
        G.conv3x3_dgrad(_nhwc(dy), wc, out=dx)
        r, a = E.ref_gemm(E.im2col(dy), E.taps_t(wt))
        E.check_out(f"{family} {n},{c},{h},{w} dgrad", family, _rows(dx), r, a, 9 * c, "bf16", errs)


@gpu
@pytest.mark.parametrize("n,c,h,w", CONVN_SHAPES)
def test_conv3x3n(gpu_ext, n, c, h, w):
    """Forward with and without statistics and the input gradient, C = 64 and 128: tiles that span image
    rows and images, the widest W, H = 1."""
    errs = []
    _convn_case(errs, n, c, h, w)
    _done(errs)


@gpu
@pytest.mark.parametrize("tail_co", [32, 16])
def test_conv3x3n_tails(gpu_ext, tail_co):
    """The 32- and 16-output-channel tail workgroups of the 128-channel kernel, shapes derived from the
    runtime slot count as test_conv3x3n_tail_split derives them (one 16 x 16 image = one tile)."""
    slots = gpu_ext.conv3x3n_slots128()
    rem = slots // 8 + 2 if tail_co == 32 else max(1, slots // 16)
    assert (rem * 8 > slots) == (tail_co == 32) and rem * 4 <= slots
    errs = []
    _convn_case(errs, slots + rem, 128, 16, 16)
    _done(errs)


@gpu
@pytest.mark.parametrize("n,c,co,h,w", W3N_SHAPES)
def test_wgrad3x3n(gpu_ext, n, c, co, h, w):
    """Both wave counts (variant 1: 8 waves, 0: 4) plus the two-deep (2) and 128-channel-group (4, 5) forms,
    one and several splits: the fp32 partials in a guarded workspace and the bf16 result of the public entry."""
    from fluxmpi_amd.ops import gemm as G
    C = gpu_ext
    errs = []
    for family in FAMILIES:
        x, dy = (t.cuda() for t in _wgrad_conv_inputs(family, n, c, co, h, w))
        xs, dys = _nhwc(x), _nhwc(dy)
        assert G.wgrad3x3n_ok(tuple(x.shape), co)
        r, a = E.ref_gemm(_rows(dy).t(), E.im2col(x).t())
        for variant in (0, 1, 2, 4, 5):
            for want in (1, 3):
                s = C.wgrad3x3n_splits(n, h, want)
                buf, ws = E.guarded(s * co, 9 * c, 9 * c, torch.float32, "cuda")
                C.wgrad3x3n(dys.data_ptr(), xs.data_ptr(), ws.data_ptr(), n, h, w, c, co, want, variant,
                            torch.cuda.current_stream().cuda_stream)
                tag = f"{family} variant {variant} splits {s}"
                out = E.take_guarded(tag, buf, ws, errs).view(s, co, 9 * c).double().sum(0)
                E.check_out(tag, family, out, r, a, n * h * w, "f32", errs)
            dw = G.conv3x3_wgrad_n(dys, xs, variant, 7)
            E.check_out(f"{family} variant {variant} bf16", family, E.taps(dw), r, a, n * h * w, "bf16", errs)
    _done(errs)
