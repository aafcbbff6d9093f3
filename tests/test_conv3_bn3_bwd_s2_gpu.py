"""The one-pass backward of conv3 (1x1, 128 -> 512) -> bn3 (+ residual, ReLU) of a stage-2 identity block:
``gemm_bf16`` mode 4 with (N, K) = (128, 512) (csrc/kernels/conv3bn3_s2_bwd.hip) and the autograd node on it.

The checks are those of test_conv3_bn3_bwd_gpu.py (read its docstring) with CO = 512, CI = 128: the unfused dx
pass run from the SAME finished sums stores the dx3 that the kernel forms in registers, so it is the exact
bf16 operand of the float64 references R = dx3 . W, dx3^T . a2 and of their absolute-value companions A
(``mfma_edges.ref_gemm``): d_a2 within ``bound(R, A, 512, "bf16")``, the reduced filter gradient within
``bound(R, A, P, "bf16")``, per element. Exact families (ternary / gather): BatchNorm weight +-2, invstd 1/2
and finished sums of zero give dx3 = +-dy_eff, every product and partial sum a small integer (gather: one bit
pattern of W per d_a2 row, signed powers of two in a2), so d_a2 and the fp32-reduced filter gradient must EQUAL
the reference. No gather check is left out: at these pixel counts (none equals 512) a2 holds powers of two, and
W's 3e38 bit patterns only ever meet one non-zero term per sum, so nothing overflows fp32.

Outputs lie in NaN-filled buffers between sentinel rows (``mfma_edges.guarded``). The slab count (= workgroups)
is passed explicitly, so no case depends on the device's compute units: 49 pixels (two tiles, the second
partial) on one workgroup; 392 (full tiles and a partial one) with one tile per workgroup, with 7 workgroups
(several tiles each) and with more workgroups than tiles (the idle ones store zero slabs); 6272 on 64; 8624 on
256 (270 tiles: the persistent loop wraps unevenly).
"""
import pytest
import torch

from . import mfma_edges as E

pytestmark = pytest.mark.gpu

CO, CI = 512, 128
TILE = 32
BF16, F32 = 9, 7
# (N, H, W), slabs
CASES = [((1, 7, 7), 1), ((2, 14, 14), 13), ((2, 14, 14), 7), ((8, 28, 28), 64), ((11, 28, 28), 256)]
IDS = ["x".join(map(str, s)) + f"-s{n}" for s, n in CASES]


def _st():
    return torch.cuda.current_stream().cuda_stream


def _inputs(family, P, seed, mask_mode="random"):
    """dy [P, 512], a2 [P, 128], W [512, 128] (``mfma_edges.linbwd_inputs``), x3, the mask bytes and the
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


def _launch(dy, x3, mask, bw, mean, inv, sum_dy, sum_dy_xhat, a2, w, out, part, slabs, n=CI, k=CO):
    from fluxmpi_amd.ops.gemm import gemm
    gemm(dy, w, out, M=dy.shape[0], N=n, K=k, lda=k, ldb=n, ldc=n, a_kmajor=True, b_kmajor=False, mode=4,
         splits=slabs, a_affine=(sum_dy, sum_dy_xhat), stats=part, residual=a2,
         bn_bwd=(x3, bw, None, mean, inv, mask, 3))


def _fused(dy, x3, mask, bw, mean, inv, sum_dy, sum_dy_xhat, a2, w, slabs, errs, name):
    """gemm_bf16 mode 4 into guarded outputs; returns (d_a2 [P, 128] bf16, slabs [s, 512 * 128] fp32)."""
    P = dy.shape[0]
    obuf, oview = E.guarded(P, CI, CI, torch.bfloat16, dy.device)
    sbuf, sview = E.guarded(slabs, CO * CI, CO * CI, torch.float32, dy.device)
    _launch(dy, x3, mask, bw, mean, inv, sum_dy, sum_dy_xhat, a2, w, oview, sview, slabs)
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
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_against_unfused_path(gpu_ext, case, family):
    """bn_bwd with a dx on the same inputs: its dx3 (from the sums it finished itself) is the exact operand
    of the float64 references that bound the fused outputs."""
    C = gpu_ext
    shape, slabs = case
    P = shape[0] * shape[1] * shape[2]
    dy, a2, w, x3, mask, bw, mean, inv = _inputs(family, P, 1)
    zero = torch.zeros(CO, device="cuda")
    dx3 = torch.full_like(dy, float("nan"))
    sum_dxh, sum_dy = torch.empty(CO, device="cuda"), torch.empty(CO, device="cuda")
    ws = torch.zeros(64 * 2 * 2048, device="cuda")
    C.bn_bwd(dy.data_ptr(), x3.data_ptr(), 0, mask.data_ptr(), bw.data_ptr(), zero.data_ptr(), mean.data_ptr(),
             inv.data_ptr(), dx3.data_ptr(), 0, sum_dxh.data_ptr(), sum_dy.data_ptr(), ws.data_ptr(), P, CO, 1, BF16,
             _st(), 0)
    errs = []
    da, part = _fused(dy, x3, mask, bw, mean, inv, sum_dy, sum_dxh, a2, w, slabs, errs, "fused")
    dw = _reduce(C, part, torch.bfloat16)
    (ra, aa), (rw, aw) = _refs(dx3, w, a2)
    assert bool(torch.isfinite(dx3.float()).all())
    E.check("fused d_a2", da, ra, E.bound(ra, aa, CO, "bf16"), errs)
    E.check("fused dW", dw, rw, E.bound(rw, aw, P, "bf16"), errs)
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
    da, part = _fused(dy, x3, mask, bw, mean, inv, sums[:CO], sums[CO:], a2, w, 20, errs, mask_mode)
    (ra, aa), (rw, aw) = _refs(dx3, w, a2)
    E.check("d_a2", da, ra, E.bound(ra, aa, CO, "bf16"), errs)
    E.check("dW", _reduce(C, part, torch.bfloat16), rw, E.bound(rw, aw, P, "bf16"), errs)
    tiles = -(-P // TILE)
    assert tiles < 20
    E.check("idle slabs", part[tiles:], torch.zeros_like(part[tiles:]).double(), None, errs)
    assert not errs, "\n".join(errs)


@pytest.mark.parametrize("family", E.EXACT)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_exact_families(gpu_ext, case, family):
    """a = +-1, b = -+0, d = 0, so dx3 = +-dy_eff and both products are exact."""
    C = gpu_ext
    shape, slabs = case
    P = shape[0] * shape[1] * shape[2]
    dy, a2, w, x3, mask, bw, mean, inv = _inputs(family, P, 3)
    sums = torch.zeros(2 * CO, device="cuda")
    bits = ((mask.view(P, CO // 8, 1) >> torch.arange(8, device="cuda", dtype=torch.uint8)) & 1).view(P, CO)
    dx3_ref = (dy.double() * bits.double() * (bw * inv).double()).bfloat16()
    errs = []
    dx3 = _dx3_from_sums(C, dy, x3, mask, bw, mean, inv, sums)
    E.check("unfused dx3", dx3, dx3_ref.double(), None, errs)
    da, part = _fused(dy, x3, mask, bw, mean, inv, sums[:CO], sums[CO:], a2, w, slabs, errs, family)
    (ra, _), (rw, aw) = _refs(dx3_ref, w, a2)
    assert float(aw.max()) < 2 ** 24
    E.check("d_a2", da, ra.bfloat16().double(), None, errs)
    assert bool((ra.bfloat16().double() == ra).all()), "the reference itself must be exact in bf16"
    E.check("dW", _reduce(C, part, torch.float32), rw, None, errs)
    assert not errs, "\n".join(errs)


def test_deterministic(gpu_ext):
    """Two launches on the same inputs: bit-equal d_a2 and slabs (plain stores, nothing between workgroups)."""
    P = 11 * 28 * 28
    dy, a2, w, x3, mask, bw, mean, inv = _inputs("uniform", P, 5)
    g = torch.Generator().manual_seed(9)
    sums = (torch.rand(2 * CO, generator=g) * 8 - 4).cuda()
    errs, runs = [], []
    for i in range(2):
        da, part = _fused(dy, x3, mask, bw, mean, inv, sums[:CO], sums[CO:], a2, w, 256, errs, f"run {i}")
        runs.append((da.view(torch.int16), part.view(torch.int32)))
    assert not errs, "\n".join(errs)
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_guards(gpu_ext):
    """Mode 4 takes (N, K) = (64, 256) and (128, 512) only, 16-byte aligned operands and 1 <= splits <= 65535:
    anything else raises before a launch (the outputs keep their fill)."""
    P = 49
    dy, a2, w, x3, mask, bw, mean, inv = _inputs("uniform", P, 6)
    sums = torch.zeros(2 * CO, device="cuda")
    out = torch.full((P, CI), 7.0, device="cuda", dtype=torch.bfloat16)
    part = torch.full((2, CO * CI), 7.0, device="cuda")
    args = (dy, x3, mask, bw, mean, inv, sums[:CO], sums[CO:], a2, w, out, part)
    for n, k in ((128, 256), (64, 512), (256, 1024), (128, 384)):
        with pytest.raises(RuntimeError, match="mode 4"):
            _launch(*args, 2, n=n, k=k)
    for splits in (0, -1, 65536):
        with pytest.raises(RuntimeError, match="splits"):
            _launch(*args, splits)
    off = torch.zeros(P * CI + 8, device="cuda", dtype=torch.bfloat16)[1:1 + P * CI].view(P, CI)  # 2 bytes off
    with pytest.raises(RuntimeError, match="aligned"):
        _launch(dy, x3, mask, bw, mean, inv, sums[:CO], sums[CO:], off, w, out, part, 2)
    with pytest.raises(RuntimeError, match="aligned"):
        _launch(dy, x3, mask, bw, mean, inv, sums[:CO], sums[CO:], a2, w, off, part, 2)
    torch.cuda.synchronize()
    assert bool((out.float() == 7.0).all()) and bool((part == 7.0).all())


def _block(seed):
    from fluxmpi_amd.models.resnet import Bottleneck
    torch.manual_seed(seed)
    blk = Bottleneck(CO, CI, conv_impl="hybrid").cuda().to(torch.bfloat16).to(memory_format=torch.channels_last)
    for bn in (blk.bn1, blk.bn2, blk.bn3):
        bn.float()
        with torch.no_grad():
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.uniform_(-0.2, 0.2)
    return blk.train()


def _forward(blk, x0, switch, monkeypatch):
    from fluxmpi_amd.ops import fused_block as fb
    monkeypatch.setattr(fb, "CONV3BN3", switch)
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
    """The block input's gradient = dc1 . W1 + dy * mask (conv1's input-gradient GEMM, K = 128, with the
    (dy, mask) the bn3 node handed over through the GradLink added in its epilogue), from the run's own dc1:
    the derived bound of a bf16 GEMM with a residual epilogue (``bound(..., "res")``)."""
    P = dc1.shape[0] * dc1.shape[2] * dc1.shape[3]
    r, a = E.ref_gemm(_nhwc(dc1), w1.reshape(CI, CO).t())
    res = _nhwc(dy).double() * _bits(mask, P).double()
    E.check(name, _nhwc(gx), r + res, E.bound(r, a, CI, "res", res=res), errs)


def test_autograd_identity_block(gpu_ext, monkeypatch):
    """One stage-2 identity bottleneck at (21, 512, 28, 28), 16 464 pixels (above the 64-pixels-per-compute-
    unit gate up to 257 compute units), switch at 2 against switch at 1 from ONE forward's saved tensors (two
    forwards differ in single ReLU bits: see test_conv3_bn3_bwd_gpu.py). At 2 the node's own backward runs; at
    1 what ``_BNFromStats`` and ``_Conv1x1Hybrid`` run backward (``_bn_bwd`` with a dx, ``conv1x1_dgrad``, the
    weight gradient, the masked (dy, mask) hand-over) runs on the tensors that forward saved, and its d_a2 goes
    down the same graph to the block input.

    Per element, in both modes: d_a2 within ``bound(R, A, 512, "bf16")`` and conv3's filter gradient within
    ``bound(R, A, P, "bf16")`` of the float64 references from the mode's own bf16 dx3; bn3's parameter
    gradients within (P + 4) 2^-23 sum |term| of float64 sums over the saved tensors; the block input's
    gradient (the GradLink path) within the residual-epilogue bound of dc1 . W1 + dy * mask. 2 against 1
    directly: within the sum of the two modes' bounds plus the distance of their references. A second forward
    with the switch at 1 must not build the node."""
    from fluxmpi_amd.ops import fused_block as fb
    from fluxmpi_amd.ops import gemm as G
    C = gpu_ext
    n, hw = 21, 28
    P = n * hw * hw
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if P < 64 * cus:
        pytest.skip(f"the 128 -> 512 gate of this device ({64 * cus} pixels) is above the case's {P}")
    blk = _block(0)
    g = torch.Generator().manual_seed(5)
    x0 = torch.randn(n, CO, hw, hw, generator=g).bfloat16().cuda().contiguous(memory_format=torch.channels_last)
    dy = torch.randn(n, CO, hw, hw, generator=g).bfloat16().cuda().contiguous(memory_format=torch.channels_last)
    x, out = _forward(blk, x0, 2, monkeypatch)
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

    # ---- switch at 2: the node's own backward
    out.backward(dy, retain_graph=True)
    torch.cuda.synchronize()
    gx_on, gp_on = x.grad.clone(), {k: p.grad.clone() for k, p in blk.named_parameters()}
    da_on, dc1_on = seen.pop("d_a2"), seen.pop("dc1")
    sums = torch.cat([gp_on["bn3.bias"].float(), gp_on["bn3.weight"].float()]).contiguous()
    dx3_on = _dx3_from_sums(C, _nhwc(dy), _nhwc(c3), mask, w32, mean, inv, sums)

    # ---- switch at 1, from the same saved tensors
    dx3_off, _, dbw_off, dbb_off = fb._bn_bwd(dy, c3, mask, w32, b32, mean, inv, True, False)
    da_off = G.conv1x1_dgrad(_nhwc(dx3_off), w2d)
    dw_off = G.conv1x1_wgrad_v2(_nhwc(dx3_off), _nhwc(a2), out_dtype=torch.bfloat16)
    node.link.grad = (dy, mask)  # the masked hand-over of _BNFromStats.backward
    gx_off, = torch.autograd.grad(a2g, [x], grad_outputs=da_off.view(n, hw, hw, CI).permute(0, 3, 1, 2),
                                  retain_graph=True)
    torch.cuda.synchronize()
    dc1_off = seen.pop("dc1")

    errs = []
    (ra, aa), (rw, aw) = _refs(dx3_on, w2d, _nhwc(a2))
    (ra_f, aa_f), (rw_f, aw_f) = _refs(_nhwc(dx3_off), w2d, _nhwc(a2))
    ba, bw_, ba_f, bw_f = (E.bound(ra, aa, CO, "bf16"), E.bound(rw, aw, P, "bf16"), E.bound(ra_f, aa_f, CO, "bf16"),
                           E.bound(rw_f, aw_f, P, "bf16"))
    dw_on = gp_on["conv3.weight"].reshape(CO, CI)
    E.check("2 d_a2", _nhwc(da_on), ra, ba, errs)
    E.check("1 d_a2", da_off, ra_f, ba_f, errs)
    E.check("2 vs 1 d_a2", _nhwc(da_on), da_off.double(), ba + ba_f + (ra - ra_f).abs(), errs)
    E.check("2 conv3 filter", dw_on, rw, bw_, errs)
    E.check("1 conv3 filter", dw_off, rw_f, bw_f, errs)
    E.check("2 vs 1 conv3 filter", dw_on, dw_off.double(), bw_ + bw_f + (rw - rw_f).abs(), errs)
    gd = _nhwc(dy).double() * _bits(mask, P).double()
    td = gd * ((_nhwc(c3).double() - mean.double()) * inv.double())
    bb, bt = (P + 4) * E.E23 * gd.abs().sum(0) + E.TINY, (P + 4) * E.E23 * td.abs().sum(0) + E.TINY
    E.check("2 bn3.bias", gp_on["bn3.bias"], gd.sum(0), bb, errs)
    E.check("1 bn3.bias", dbb_off, gd.sum(0), bb, errs)
    E.check("2 vs 1 bn3.bias", gp_on["bn3.bias"], dbb_off.double(), 2 * bb, errs)
    E.check("2 bn3.weight", gp_on["bn3.weight"], td.sum(0), bt, errs)
    E.check("1 bn3.weight", dbw_off, td.sum(0), bt, errs)
    E.check("2 vs 1 bn3.weight", gp_on["bn3.weight"], dbw_off.double(), 2 * bt, errs)
    _check_input_grad("2 block input", gx_on, dc1_on, w1, dy, mask, errs)
    _check_input_grad("1 block input", gx_off, dc1_off, w1, dy, mask, errs)

    # ---- the switch at 1 keeps this block on the unfused nodes
    _, out2 = _forward(blk, x0, 1, monkeypatch)
    assert not type(out2.grad_fn).__name__.startswith("_Conv3BN3"), type(out2.grad_fn).__name__
    assert not errs, "\n".join(errs)
