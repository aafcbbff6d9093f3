"""The one-pass backward of conv3 (1x1, 64 -> 256) -> bn3 (+ residual, ReLU): ``gemm_bf16`` mode 4
(csrc/kernels/conv3bn3_bwd.hip), ``bn_bwd`` without a dx, and the autograd node built on them.

The kernel forms bn3's input gradient dx3 in registers with the dx pass's own arithmetic (bn_dx.h) and
feeds d_a2 = dx3 . W and dW = dx3^T . a2 from it. The unfused dx pass run from the SAME finished sums
(``bn_bwd`` with a dx, or ``bn_sync_bwd_dx`` without a count: the same kernel from given sums) stores
that dx3, so it is the exact bf16 operand of the float64 references R = dx3 . W, dx3^T . a2 and of
their absolute-value companions A (``mfma_edges.ref_gemm``), and the derived bounds of
test_mfma_edges_gpu.py apply unchanged: d_a2 within ``bound(R, A, 256, "bf16")``, the filter gradient
within ``bound(R, A, P, "bf16")``, per element. A dx3 element that is not bit-identical shows as a
bound failure (one bf16 ulp of one term is of the order of the whole accumulation term).

Exact cases (ternary / gather families): BatchNorm weight +-2 and invstd 1/2 give a = +-1, and
finished sums of zero give b = -+0, d = 0, so dx3 = +-dy_eff exactly; every product and partial sum is
then a small integer (gather: one bit pattern, or signed powers of two), the d_a2 must EQUAL the
reference and so must the filter gradient, reduced to fp32.

Outputs lie in NaN-filled buffers between sentinel rows (``mfma_edges.guarded``): a row written out of
range or left unwritten shows. Shapes: 49 pixels (less than a tile), 392 (full tiles and a partial
one), 6272 (a multiple of the tile), 31360 (more tiles than resident workgroups: the persistent loop
wraps unevenly); one case launches more workgroups than tiles (the idle ones store zero slabs).
"""
import pytest
import torch

from . import mfma_edges as E

pytestmark = pytest.mark.gpu

CO, CI = 256, 64
BF16, F32 = 9, 7
SHAPES = [(1, 7, 7), (2, 14, 14), (8, 28, 28), (40, 28, 28)]


def _st():
    return torch.cuda.current_stream().cuda_stream


def _inputs(family, P, seed, mask_mode="random"):
    """dy [P, 256], a2 [P, 64], W [256, 64] (``mfma_edges.linbwd_inputs``), x3, the mask bytes and the
    BatchNorm vectors, on the GPU."""
    if family == "cancel" and P % 2:  # the family pairs rows: build one row more and drop it
        dy, a2, w = E.linbwd_inputs(family, P + 1, CO, CI, seed)
        dy, a2 = dy[:P].contiguous(), a2[:P].contiguous()
    else:
        dy, a2, w = E.linbwd_inputs(family, P, CO, CI, seed)
    g = torch.Generator().manual_seed(1000 + seed + P)
    x3 = (torch.rand(P, CO, generator=g) * 4 - 2).bfloat16()
    if mask_mode == "random":
        mask = torch.randint(0, 256, (P * CO // 8,), generator=g).to(torch.uint8)
    else:
        mask = torch.full((P * CO // 8,), 255 if mask_mode == "ones" else 0, dtype=torch.uint8)
    sign = (torch.randint(0, 2, (CO,), generator=g) * 2 - 1).float()
    if family in E.EXACT:
        bw, mean, inv = 2 * sign, torch.full((CO,), 0.5), torch.full((CO,), 0.5)
    else:
        bw = sign * (0.5 + torch.rand(CO, generator=g))
        mean, inv = torch.rand(CO, generator=g) - 0.5, 0.5 + 1.5 * torch.rand(CO, generator=g)
    return [t.cuda() for t in (dy, a2, w, x3, mask, bw, mean, inv)]


def _dx3_from_sums(C, dy, x3, mask, bw, mean, inv, sums):
    """The unfused dx pass (bn_bwd's dx kernel) from given finished sums [sum dy_eff | sum dy_eff xhat]."""
    P = dy.shape[0]
    dx3 = torch.full_like(dy, float("nan"))
    zero = torch.zeros(CO, device=dy.device)
    C.bn_sync_bwd_dx(dy.data_ptr(), x3.data_ptr(), 0, mask.data_ptr(), bw.data_ptr(), zero.data_ptr(),
                     mean.data_ptr(), inv.data_ptr(), sums.data_ptr(), 0, 0, dx3.data_ptr(), 0, P, CO, 1, BF16, _st())
    return dx3


def _fused(C, dy, x3, mask, bw, mean, inv, sum_dy, sum_dy_xhat, a2, w, slabs, errs, name):
    """gemm_bf16 mode 4 into guarded outputs; returns (d_a2 [P, 64] bf16, slabs [s, 256 * 64] fp32)."""
    from fluxmpi_amd.ops.gemm import gemm
    P = dy.shape[0]
    obuf, oview = E.guarded(P, CI, CI, torch.bfloat16, dy.device)
    sbuf, sview = E.guarded(slabs, CO * CI, CO * CI, torch.float32, dy.device)
    gemm(dy, w, oview, M=P, N=CI, K=CO, lda=CO, ldb=CI, ldc=CI, a_kmajor=True, b_kmajor=False, mode=4,
         splits=slabs, a_affine=(sum_dy, sum_dy_xhat), stats=sview, residual=a2,
         bn_bwd=(x3, bw, None, mean, inv, mask, 3))
    torch.cuda.synchronize()
    return E.take_guarded(f"{name} d_a2", obuf, oview, errs), E.take_guarded(f"{name} slabs", sbuf, sview, errs)


def _reduce(C, part, dtype):
    out = torch.full((CO, CI), float("nan"), device=part.device, dtype=dtype)
    ws = part.clone()  # the reduce may write intermediate levels in place
    C.gemm_splitk_reduce(ws.data_ptr(), part.shape[0], CO * CI, out.data_ptr(), BF16 if dtype == torch.bfloat16 else F32,
                         _st())
    return out


def _refs(dx3, w, a2):
    """(R, A) of d_a2 = dx3 . W and of dW = dx3^T . a2, float64, from the stored bf16 dx3."""
    return E.ref_gemm(dx3, w.t()), E.ref_gemm(dx3.t(), a2.t())


@pytest.mark.parametrize("family", ["uniform", "cancel"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_against_unfused_path(gpu_ext, shape, family):
    """Check 1: bn_bwd with a dx, conv1x1_dgrad and the present weight gradient on the same inputs; dx3
    of that path is the exact operand of the float64 references that bound the fused outputs."""
    from fluxmpi_amd.ops import fused_block as fb
    from fluxmpi_amd.ops import gemm as G
    C = gpu_ext
    P = shape[0] * shape[1] * shape[2]
    dy, a2, w, x3, mask, bw, mean, inv = _inputs(family, P, 1)
    zero = torch.zeros(CO, device="cuda")
    dx3 = torch.full_like(dy, float("nan"))
    sum_dxh, sum_dy = torch.empty(CO, device="cuda"), torch.empty(CO, device="cuda")
    ws = torch.zeros(64 * 2 * 2048, device="cuda")
    C.bn_bwd(dy.data_ptr(), x3.data_ptr(), 0, mask.data_ptr(), bw.data_ptr(), zero.data_ptr(), mean.data_ptr(),
             inv.data_ptr(), dx3.data_ptr(), 0, sum_dxh.data_ptr(), sum_dy.data_ptr(), ws.data_ptr(), P, CO, 1, BF16,
             _st(), 0)
    da_u = G.conv1x1_dgrad(dx3, w)
    dw_u = G.conv1x1_wgrad_v2(dx3, a2, out_dtype=torch.bfloat16)
    errs = []
    slabs = fb.conv3bn3_slabs(P, dy.device)
    da, part = _fused(C, dy, x3, mask, bw, mean, inv, sum_dy, sum_dxh, a2, w, slabs, errs, "fused")
    dw = _reduce(C, part, torch.bfloat16)
    (ra, aa), (rw, aw) = _refs(dx3, w, a2)
    assert bool(torch.isfinite(dx3.float()).all())
    E.check("fused d_a2", da, ra, E.bound(ra, aa, CO, "bf16"), errs)
    E.check("fused dW", dw, rw, E.bound(rw, aw, P, "bf16"), errs)
    E.check("unfused d_a2", da_u, ra, E.bound(ra, aa, CO, "bf16"), errs)
    E.check("unfused dW", dw_u, rw, E.bound(rw, aw, P, "bf16"), errs)
    assert not errs, "\n".join(errs)


@pytest.mark.parametrize("mask_mode", ["zeros", "ones"])
def test_mask_all_zero_all_one(gpu_ext, mask_mode):
    """All-zero mask: dy_eff = 0 everywhere, dx3 = b x + d; all-one: dy_eff = dy. More workgroups than
    tiles on the way: the idle ones must store zero slabs."""
    C = gpu_ext
    P = 2 * 14 * 14
    dy, a2, w, x3, mask, bw, mean, inv = _inputs("uniform", P, 2, mask_mode)
    g = torch.Generator().manual_seed(7)
    sums = (torch.rand(2 * CO, generator=g) * 8 - 4).cuda()  # any finished sums: the dx pass takes them as given
    dx3 = _dx3_from_sums(C, dy, x3, mask, bw, mean, inv, sums)
    errs = []
    da, part = _fused(C, dy, x3, mask, bw, mean, inv, sums[:CO], sums[CO:], a2, w, 20, errs, mask_mode)
    (ra, aa), (rw, aw) = _refs(dx3, w, a2)
    E.check("d_a2", da, ra, E.bound(ra, aa, CO, "bf16"), errs)
    E.check("dW", _reduce(C, part, torch.bfloat16), rw, E.bound(rw, aw, P, "bf16"), errs)
    tiles = -(-P // 32)
    E.check("idle slabs", part[tiles:], torch.zeros_like(part[tiles:]).double(), None, errs)
    assert not errs, "\n".join(errs)


@pytest.mark.parametrize("family", E.EXACT)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_exact_families(gpu_ext, shape, family):
    """Check 2: a = +-1, b = -+0, d = 0, so dx3 = +-dy_eff and both products are exact."""
    from fluxmpi_amd.ops import fused_block as fb
    C = gpu_ext
    P = shape[0] * shape[1] * shape[2]
    dy, a2, w, x3, mask, bw, mean, inv = _inputs(family, P, 3)
    sums = torch.zeros(2 * CO, device="cuda")
    bits = ((mask.view(P, CO // 8, 1) >> torch.arange(8, device="cuda", dtype=torch.uint8)) & 1).view(P, CO)
    dx3_ref = (dy.double() * bits.double() * (bw * inv).double()).bfloat16()
    errs = []
    dx3 = _dx3_from_sums(C, dy, x3, mask, bw, mean, inv, sums)
    E.check("unfused dx3", dx3, dx3_ref.double(), None, errs)
    da, part = _fused(C, dy, x3, mask, bw, mean, inv, sums[:CO], sums[CO:], a2, w, fb.conv3bn3_slabs(P, dy.device),
                      errs, family)
    (ra, _), (rw, aw) = _refs(dx3_ref, w, a2)
    assert float(aw.max()) < 2 ** 24
    E.check("d_a2", da, ra.bfloat16().double(), None, errs)
    assert bool((ra.bfloat16().double() == ra).all()), "the reference itself must be exact in bf16"
    E.check("dW", _reduce(C, part, torch.float32), rw, None, errs)
    assert not errs, "\n".join(errs)


def test_bn_bwd_without_dx(gpu_ext):
    """bn_bwd(dx = null): reduce and finalize only. The sums are fp32 sums of P terms in some order:
    within (P + 4) 2^-23 sum |term| of float64 (4: the rounding of xhat's two operations and the fma)."""
    C = gpu_ext
    P = 8 * 28 * 28
    dy, _, _, x3, mask, bw, mean, inv = _inputs("uniform", P, 4)
    zero = torch.zeros(CO, device="cuda")
    sum_dxh, sum_dy = torch.full((CO,), float("nan"), device="cuda"), torch.full((CO,), float("nan"), device="cuda")
    ws = torch.zeros(64 * 2 * 2048, device="cuda")
    C.bn_bwd(dy.data_ptr(), x3.data_ptr(), 0, mask.data_ptr(), bw.data_ptr(), zero.data_ptr(), mean.data_ptr(),
             inv.data_ptr(), 0, 0, sum_dxh.data_ptr(), sum_dy.data_ptr(), ws.data_ptr(), P, CO, 1, BF16, _st(), 0)
    torch.cuda.synchronize()
    bits = ((mask.view(P, CO // 8, 1) >> torch.arange(8, device="cuda", dtype=torch.uint8)) & 1).view(P, CO)
    g = dy.double() * bits.double()
    t = g * ((x3.double() - mean.double()) * inv.double())
    errs = []
    E.check("sum dy_eff", sum_dy, g.sum(0), (P + 4) * E.E23 * g.abs().sum(0) + E.TINY, errs)
    E.check("sum dy_eff xhat", sum_dxh, t.sum(0), (P + 4) * E.E23 * t.abs().sum(0) + E.TINY, errs)
    assert float(ws.abs().max()) == 0.0, "the finalize leaves the workspace zeroed"
    assert not errs, "\n".join(errs)


def test_bn_bwd_without_dx_rejects_dres(gpu_ext):
    """dres is written by the dx pass: asking for it without a dx is an error, raised before any launch."""
    C = gpu_ext
    P = 49
    dy, _, _, x3, mask, bw, mean, inv = _inputs("uniform", P, 4)
    zero = torch.zeros(CO, device="cuda")
    sum_dxh, sum_dy = torch.zeros(CO, device="cuda"), torch.zeros(CO, device="cuda")
    dres = torch.zeros_like(dy)
    ws = torch.zeros(64 * 2 * 2048, device="cuda")
    with pytest.raises(RuntimeError, match="without a dx"):
        C.bn_bwd(dy.data_ptr(), x3.data_ptr(), 0, mask.data_ptr(), bw.data_ptr(), zero.data_ptr(), mean.data_ptr(),
                 inv.data_ptr(), 0, dres.data_ptr(), sum_dxh.data_ptr(), sum_dy.data_ptr(), ws.data_ptr(), P, CO, 1, BF16,
                 _st(), 0)
    torch.cuda.synchronize()
    assert float(dres.float().abs().max()) == 0.0 and float(ws.abs().max()) == 0.0


def _block(seed):
    from fluxmpi_amd.models.resnet import Bottleneck
    torch.manual_seed(seed)
    blk = Bottleneck(256, 64, conv_impl="hybrid").cuda().to(torch.bfloat16).to(memory_format=torch.channels_last)
    for bn in (blk.bn1, blk.bn2, blk.bn3):
        bn.float()
        with torch.no_grad():
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.uniform_(-0.2, 0.2)
    return blk.train()


def _forward(blk, x0, on, monkeypatch):
    from fluxmpi_amd.ops import fused_block as fb
    monkeypatch.setattr(fb, "CONV3BN3", on)
    x = x0.clone().requires_grad_(True)
    # the block input is a non-leaf, as in a network: conv1's dgrad epilogue completes its gradient
    return x, blk(x * 1)


def _up(t, cls):
    """Up the block's main path from ``t`` (every node there saves its input first) to the tensor that
    the autograd node ``cls`` produced."""
    while not type(t.grad_fn).__name__.startswith(cls):
        t = t.grad_fn.saved_tensors[0]
    return t


def _nhwc(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _bits(mask, P):
    return ((mask.view(P, CO // 8, 1) >> torch.arange(8, device=mask.device, dtype=torch.uint8)) & 1).view(P, CO)


def _check_input_grad(name, gx, dc1, w1, dy, mask, errs):
    """The block input's gradient = dc1 . W1 + dy * mask (conv1's input-gradient GEMM, K = 64, with the
    (dy, mask) the bn3 node handed over added in its epilogue), from the run's own dc1: the derived
    bound of a bf16 GEMM with a residual epilogue (``bound(..., "res")``)."""
    P = dc1.shape[0] * dc1.shape[2] * dc1.shape[3]
    r, a = E.ref_gemm(_nhwc(dc1), w1.reshape(CI, CO).t())
    res = _nhwc(dy).double() * _bits(mask, P).double()
    E.check(name, _nhwc(gx), r + res, E.bound(r, a, CI, "res", res=res), errs)


def test_autograd_identity_block(gpu_ext, monkeypatch):
    """Check 3: one stage-1 identity bottleneck (N = 2, 56 x 56), switch on against switch off, per
    element with the bounds of check 1.

    Two forwards do not compute the same function: the BatchNorm statistics come from float atomics, so
    mean / invstd differ in the last place from run to run (in ONE mode already) and single ReLU bits
    with them. So both modes run their backward from ONE forward's saved tensors: the block is run with
    the switch on, its backward is the node's; then the switch-off backward of conv3 -> bn3 (``_bn_bwd``
    with a dx, ``conv1x1_dgrad``, the weight gradient, the masked (dy, mask) hand-over) runs on the
    tensors that forward saved, and its d_a2 goes down the same graph to the block input.

    Per element, in both modes: d_a2 within ``bound(R, A, 256, "bf16")`` and conv3's filter gradient
    within ``bound(R, A, P, "bf16")`` of the float64 references from the mode's own bf16 dx3 (on: what
    the dx pass stores from the node's finished sums); bn3's parameter gradients within the bound of
    test_bn_bwd_without_dx of float64 sums over the saved tensors; the block input's gradient within
    the residual-epilogue bound of dc1 . W1 + dy * mask, dc1 the run's own gradient of conv1's output
    (this is where a wrong row or bit of the handed-over (dy, mask) shows). On against off directly:
    within the sum of the two modes' bounds plus the distance of their references.

    The parameter gradients of conv1, conv2, bn1 and bn2 come from kernels that this node does not
    touch, applied to d_a2; check 1 derives no bound for how d_a2's rounding travels through them. They
    are compared with a second, switch-off forward + backward in the 2-norm only (2^-7: two bf16
    roundings), as is everything else, as a whole-block cross-check beside the per-element ones."""
    from fluxmpi_amd.ops import fused_block as fb
    from fluxmpi_amd.ops import gemm as G
    C = gpu_ext
    blk = _block(0)
    g = torch.Generator().manual_seed(5)
    x0 = torch.randn(2, 256, 56, 56, generator=g).bfloat16().cuda().contiguous(memory_format=torch.channels_last)
    dy = torch.randn(2, 256, 56, 56, generator=g).bfloat16().cuda().contiguous(memory_format=torch.channels_last)
    P = 2 * 56 * 56
    x, out = _forward(blk, x0, True, monkeypatch)
    node = out.grad_fn
    assert type(node).__name__.startswith("_Conv3BN3"), type(node).__name__
    a2g, weight, c3, mask, w32, b32, mean, inv = node.saved_tensors
    c1 = _up(a2g, "_Conv1x1Hybrid")
    w1 = blk.conv1.weight.detach()
    seen = {}
    a2g.register_hook(lambda t: seen.__setitem__("d_a2", t.clone()))
    c1.register_hook(lambda t: seen.__setitem__("dc1", t.clone()))
    a2, weight, c3 = a2g.detach(), weight.detach(), c3.detach()
    w2d = weight.reshape(CO, CI)

    # ---- switch on: the node's own backward
    out.backward(dy, retain_graph=True)
    torch.cuda.synchronize()
    gx_on, gp_on = x.grad.clone(), {n: p.grad.clone() for n, p in blk.named_parameters()}
    da_on, dc1_on = seen.pop("d_a2"), seen.pop("dc1")
    sums = torch.cat([gp_on["bn3.bias"].float(), gp_on["bn3.weight"].float()]).contiguous()
    dx3_on = _dx3_from_sums(C, _nhwc(dy), _nhwc(c3), mask, w32, mean, inv, sums)

    # ---- switch off, from the same saved tensors: what _BNFromStats and _Conv1x1Hybrid run backward
    dx3_off, _, dbw_off, dbb_off = fb._bn_bwd(dy, c3, mask, w32, b32, mean, inv, True, False)
    da_off = G.conv1x1_dgrad(_nhwc(dx3_off), w2d)
    dw_off = G.conv1x1_wgrad_v2(_nhwc(dx3_off), _nhwc(a2), out_dtype=torch.bfloat16)
    node.link.grad = (dy, mask)  # the masked hand-over of _BNFromStats.backward
    gx_off, = torch.autograd.grad(a2g, [x], grad_outputs=da_off.view(2, 56, 56, CI).permute(0, 3, 1, 2),
                                  retain_graph=True)
    torch.cuda.synchronize()
    dc1_off = seen.pop("dc1")

    errs = []
    (ra, aa), (rw, aw) = _refs(dx3_on, w2d, _nhwc(a2))
    (ra_f, aa_f), (rw_f, aw_f) = _refs(_nhwc(dx3_off), w2d, _nhwc(a2))
    ba, bw_, ba_f, bw_f = (E.bound(ra, aa, CO, "bf16"), E.bound(rw, aw, P, "bf16"), E.bound(ra_f, aa_f, CO, "bf16"),
                           E.bound(rw_f, aw_f, P, "bf16"))
    dw_on = gp_on["conv3.weight"].reshape(CO, CI)
    E.check("on d_a2", _nhwc(da_on), ra, ba, errs)
    E.check("off d_a2", da_off, ra_f, ba_f, errs)
    E.check("on vs off d_a2", _nhwc(da_on), da_off.double(), ba + ba_f + (ra - ra_f).abs(), errs)
    E.check("on conv3 filter", dw_on, rw, bw_, errs)
    E.check("off conv3 filter", dw_off, rw_f, bw_f, errs)
    E.check("on vs off conv3 filter", dw_on, dw_off.double(), bw_ + bw_f + (rw - rw_f).abs(), errs)
    gd = _nhwc(dy).double() * _bits(mask, P).double()
    td = gd * ((_nhwc(c3).double() - mean.double()) * inv.double())
    bb, bt = (P + 4) * E.E23 * gd.abs().sum(0) + E.TINY, (P + 4) * E.E23 * td.abs().sum(0) + E.TINY
    E.check("on bn3.bias", gp_on["bn3.bias"], gd.sum(0), bb, errs)
    E.check("off bn3.bias", dbb_off, gd.sum(0), bb, errs)
    E.check("on vs off bn3.bias", gp_on["bn3.bias"], dbb_off.double(), 2 * bb, errs)
    E.check("on bn3.weight", gp_on["bn3.weight"], td.sum(0), bt, errs)
    E.check("off bn3.weight", dbw_off, td.sum(0), bt, errs)
    E.check("on vs off bn3.weight", gp_on["bn3.weight"], dbw_off.double(), 2 * bt, errs)
    _check_input_grad("on block input", gx_on, dc1_on, w1, dy, mask, errs)
    _check_input_grad("off block input", gx_off, dc1_off, w1, dy, mask, errs)

    # ---- a second forward with the switch off: the whole block in the 2-norm
    for p in blk.parameters():
        p.grad = None
    x2, out2 = _forward(blk, x0, False, monkeypatch)
    assert not type(out2.grad_fn).__name__.startswith("_Conv3BN3")
    out2.backward(dy)
    torch.cuda.synchronize()
    pairs = {n: (gp_on[n], p.grad) for n, p in blk.named_parameters()}
    pairs["input"] = (gx_on, x2.grad)
    for n, (a, b) in pairs.items():
        rel = float((a.double() - b.double()).norm() / b.double().norm())
        print(f"{n}: on vs a switch-off run, relative 2-norm difference {rel:.3e}")
        if not rel <= 2.0 ** -7:
            errs.append(f"{n}: on vs a switch-off run differ by {rel:.3e} of the norm")
    assert not errs, "\n".join(errs)


