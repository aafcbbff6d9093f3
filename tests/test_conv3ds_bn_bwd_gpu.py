"""The one-pass backward around the dual BatchNorm of a stage-1 downsample block,
out = relu(bn3(conv3(a2)) + bn_ds(conv_ds(x))): ``conv3ds_bwd`` (csrc/kernels/conv3ds_bwd.hip),
``bn_bwd_dual`` without a dx, and the autograd node built on them.

The kernel forms both BatchNorms' input gradients dx3 and dx_ds in registers with the dx pass's own
arithmetic (bn_dx.h) and feeds d_a2 = dx3 . W3, dW3 = dx3^T . a2, d_xside = dx_ds . W_ds and
dW_ds = dx_ds^T . x from them. Per branch, the single-branch dx pass run from the SAME finished sums
(``bn_sync_bwd_dx`` without a count, same dy and mask) stores that dx, so it is the exact bf16 operand
of the float64 references and of their absolute-value companions (``mfma_edges.ref_gemm``), and the
derived bounds of test_mfma_edges_gpu.py apply unchanged: d_a2 and d_xside within
``bound(R, A, 256, "bf16")``, both filter gradients after the reduce within ``bound(R, A, P, "bf16")``,
per element. (The dual dx pass stores the same bits: checked on the way.)

Exact cases (ternary / gather families): BatchNorm weight +-2 and invstd 1/2 with zero sums give
dx = +-dy_eff, every product and partial sum is a small integer (or one bit pattern, or signed powers of
two), and all four outputs must EQUAL the reference.

The two branches never share an operand: different statistics, sums, c3 / c_ds, a2 / x and filters in
every test, so a swapped branch fails everywhere (test_distinct_branches shows that it would).
Outputs lie in NaN-filled buffers between sentinel rows (``mfma_edges.guarded``). Shapes: 49 pixels
(less than a tile), 392 (full tiles and a partial one), 6272 (a multiple of the tile), 31360 (980 tiles
over one workgroup per compute unit: the persistent loop wraps unevenly); the mask tests launch more
workgroups than tiles (the idle ones store zero slabs in both slab sets).
"""
import pytest
import torch

from . import mfma_edges as E
from . import norm_edges as N

pytestmark = pytest.mark.gpu

CO, CI = 256, 64
BF16, F32 = 9, 7
SHAPES = [(1, 7, 7), (2, 14, 14), (8, 28, 28), (40, 28, 28)]


def _st():
    return torch.cuda.current_stream().cuda_stream


def _X():
    from fluxmpi_amd.ops import _ext
    return _ext.get(required=True)


def _branch(family, P, seed, flip):
    """One branch's (act [P, 64], W [256, 64], c [P, 256], bn weight, mean, invstd) and the dy that
    ``mfma_edges.linbwd_inputs`` makes with them (the first branch's is the block's dy)."""
    if family == "cancel" and P % 2:  # the family pairs rows: build one row more and drop it
        dy, act, w = E.linbwd_inputs(family, P + 1, CO, CI, seed)
        dy, act = dy[:P].contiguous(), act[:P].contiguous()
    else:
        dy, act, w = E.linbwd_inputs(family, P, CO, CI, seed)
    if flip:  # the second branch's filter: other rows even where the family's filter ignores the seed
        w = w.flip(0).contiguous()
    g = torch.Generator().manual_seed(1000 + seed + P)
    c = (torch.rand(P, CO, generator=g) * 4 - 2).bfloat16()
    sign = (torch.randint(0, 2, (CO,), generator=g) * 2 - 1).float()
    if family in E.EXACT:
        bw, mean, inv = 2 * sign, torch.full((CO,), 0.5), torch.full((CO,), 0.5)
    else:
        bw = sign * (0.5 + torch.rand(CO, generator=g))
        mean, inv = torch.rand(CO, generator=g) - 0.5, 0.5 + 1.5 * torch.rand(CO, generator=g)
    return dy, dict(act=act.cuda(), w=w.cuda(), c=c.cuda(), bw=bw.cuda(), mean=mean.cuda(), inv=inv.cuda())


def _inputs(family, P, seed, mask_mode="random"):
    """dy [P, 256], the mask bytes and the two branches (conv3 / bn3, downsample), on the GPU."""
    dy, b0 = _branch(family, P, seed, False)
    _, b1 = _branch(family, P, seed + 100, True)
    g = torch.Generator().manual_seed(77 + seed + P)
    if mask_mode == "random":
        mask = torch.randint(0, 256, (P * CO // 8,), generator=g).to(torch.uint8)
    else:
        mask = torch.full((P * CO // 8,), 255 if mask_mode == "ones" else 0, dtype=torch.uint8)
    assert not torch.equal(b0["w"], b1["w"]) and not torch.equal(b0["act"], b1["act"])
    return dy.cuda(), mask.cuda(), (b0, b1)


def _bits(mask, P):
    return ((mask.view(P, CO // 8, 1) >> torch.arange(8, device=mask.device, dtype=torch.uint8)) & 1).view(P, CO)


def _dx_from_sums(C, dy, mask, b, sums):
    """The single-branch dx pass from given finished sums [sum dy_eff | sum dy_eff xhat]."""
    P = dy.shape[0]
    dx = torch.full_like(dy, float("nan"))
    zero = torch.zeros(CO, device=dy.device)
    C.bn_sync_bwd_dx(dy.data_ptr(), b["c"].data_ptr(), 0, mask.data_ptr(), b["bw"].data_ptr(), zero.data_ptr(),
                     b["mean"].data_ptr(), b["inv"].data_ptr(), sums.data_ptr(), 0, 0, dx.data_ptr(), 0, P, CO, 1, BF16,
                     _st())
    return dx


def _fused(dy, mask, br, sums, slabs, errs, name):
    """conv3ds_bwd into guarded outputs: [(d_a [P, 64] bf16, slabs [s, 256 * 64] fp32)] per branch."""
    P = dy.shape[0]
    o = [E.guarded(P, CI, CI, torch.bfloat16, dy.device) for _ in range(2)]
    s = [E.guarded(slabs, CO * CI, CO * CI, torch.float32, dy.device) for _ in range(2)]
    b0, b1 = br
    _X().conv3ds_bwd(dy.data_ptr(), mask.data_ptr(), b0["c"].data_ptr(), b1["c"].data_ptr(), b0["bw"].data_ptr(),
                     b0["mean"].data_ptr(), b0["inv"].data_ptr(), sums[0][:CO].data_ptr(), sums[0][CO:].data_ptr(),
                     b1["bw"].data_ptr(), b1["mean"].data_ptr(), b1["inv"].data_ptr(), sums[1][:CO].data_ptr(),
                     sums[1][CO:].data_ptr(), b0["act"].data_ptr(), b1["act"].data_ptr(), b0["w"].data_ptr(),
                     b1["w"].data_ptr(), o[0][1].data_ptr(), o[1][1].data_ptr(), s[0][1].data_ptr(), s[1][1].data_ptr(),
                     P, slabs, _st())
    torch.cuda.synchronize()
    return [(E.take_guarded(f"{name} d_a[{i}]", *o[i], errs), E.take_guarded(f"{name} slabs[{i}]", *s[i], errs))
            for i in range(2)]


def _reduce(C, part, dtype):
    out = torch.full((CO, CI), float("nan"), device=part.device, dtype=dtype)
    ws = part.clone()  # the reduce may write intermediate levels in place
    C.gemm_splitk_reduce(ws.data_ptr(), part.shape[0], CO * CI, out.data_ptr(), BF16 if dtype == torch.bfloat16 else F32,
                         _st())
    return out


def _refs(dx, w, act):
    """(R, A) of d_a = dx . W and of dW = dx^T . act, float64, from the stored bf16 dx."""
    return E.ref_gemm(dx, w.t()), E.ref_gemm(dx.t(), act.t())


def _check_branches(C, name, got, dxs, br, P, errs):
    for i, ((da, part), dx, b) in enumerate(zip(got, dxs, br)):
        (ra, aa), (rw, aw) = _refs(dx, b["w"], b["act"])
        E.check(f"{name} d_a[{i}]", da, ra, E.bound(ra, aa, CO, "bf16"), errs)
        E.check(f"{name} dW[{i}]", _reduce(C, part, torch.bfloat16), rw, E.bound(rw, aw, P, "bf16"), errs)


@pytest.mark.parametrize("family", ["uniform", "cancel"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_against_dx_passes(gpu_ext, shape, family):
    """The sums come from bn_bwd_dual itself (with a dx); the single-branch dx pass from those sums stores
    the operands of the references, and the dual dx pass must have stored the same bits."""
    from fluxmpi_amd.ops import fused_block as fb
    C = gpu_ext
    P = shape[0] * shape[1] * shape[2]
    dy, mask, br = _inputs(family, P, 1)
    b0, b1 = br
    dxd = [torch.full_like(dy, float("nan")) for _ in range(2)]
    dw, db, dw2, db2 = (torch.empty(CO, device="cuda") for _ in range(4))
    ws, ws2 = torch.zeros(64 * 2 * 2048, device="cuda"), torch.zeros(64 * 2 * 2048, device="cuda")
    C.bn_bwd_dual(dy.data_ptr(), mask.data_ptr(), b0["c"].data_ptr(), b1["c"].data_ptr(), b0["bw"].data_ptr(),
                  b0["mean"].data_ptr(), b0["inv"].data_ptr(), b1["bw"].data_ptr(), b1["mean"].data_ptr(),
                  b1["inv"].data_ptr(), dxd[0].data_ptr(), dxd[1].data_ptr(), dw.data_ptr(), db.data_ptr(),
                  dw2.data_ptr(), db2.data_ptr(), ws.data_ptr(), ws2.data_ptr(), P, CO, BF16, _st())
    sums = [torch.cat([db, dw]).contiguous(), torch.cat([db2, dw2]).contiguous()]
    dxs = [_dx_from_sums(C, dy, mask, b, s) for b, s in zip(br, sums)]
    errs = []
    for i in range(2):
        assert bool(torch.isfinite(dxs[i].float()).all())
        if not torch.equal(dxd[i].view(torch.int16), dxs[i].view(torch.int16)):
            errs.append(f"dual dx pass, branch {i}: not the bits of the single-branch dx pass")
    got = _fused(dy, mask, br, sums, fb.conv3ds_slabs(P, dy.device), errs, "fused")
    _check_branches(C, "fused", got, dxs, br, P, errs)
    assert not errs, "\n".join(errs)


@pytest.mark.parametrize("mask_mode", ["zeros", "ones"])
def test_mask_all_zero_all_one(gpu_ext, mask_mode):
    """All-zero mask: dy_eff = 0 everywhere, dx = b x + d; all-one: dy_eff = dy. More workgroups than
    tiles on the way: the idle ones must store zero slabs in both slab sets."""
    C = gpu_ext
    P = 2 * 14 * 14
    dy, mask, br = _inputs("uniform", P, 2, mask_mode)
    g = torch.Generator().manual_seed(7)
    # any finished sums, other ones per branch: the dx pass takes them as given
    sums = [(torch.rand(2 * CO, generator=g) * 8 - 4).cuda() for _ in range(2)]
    dxs = [_dx_from_sums(C, dy, mask, b, s) for b, s in zip(br, sums)]
    errs = []
    got = _fused(dy, mask, br, sums, 20, errs, mask_mode)
    _check_branches(C, mask_mode, got, dxs, br, P, errs)
    tiles = -(-P // 32)
    assert tiles < 20
    for i in range(2):
        idle = got[i][1][tiles:]
        E.check(f"idle slabs[{i}]", idle, torch.zeros_like(idle).double(), None, errs)
    assert not errs, "\n".join(errs)


@pytest.mark.parametrize("family", E.EXACT)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_exact_families(gpu_ext, shape, family):
    """a = +-1, b = -+0, d = 0 in both branches (other signs per branch), so dx = +-dy_eff and all four
    products are exact."""
    from fluxmpi_amd.ops import fused_block as fb
    C = gpu_ext
    P = shape[0] * shape[1] * shape[2]
    dy, mask, br = _inputs(family, P, 3)
    sums = [torch.zeros(2 * CO, device="cuda") for _ in range(2)]
    bits = _bits(mask, P)
    errs = []
    refs = []
    for i, b in enumerate(br):
        ref = (dy.double() * bits.double() * (b["bw"] * b["inv"]).double()).bfloat16()
        E.check(f"single-branch dx[{i}]", _dx_from_sums(C, dy, mask, b, sums[i]), ref.double(), None, errs)
        refs.append(ref)
    got = _fused(dy, mask, br, sums, fb.conv3ds_slabs(P, dy.device), errs, family)
    for i, ((da, part), ref, b) in enumerate(zip(got, refs, br)):
        (ra, _), (rw, aw) = _refs(ref, b["w"], b["act"])
        assert float(aw.max()) < 2 ** 24
        assert bool((ra.bfloat16().double() == ra).all()), "the reference itself must be exact in bf16"
        E.check(f"d_a[{i}]", da, ra, None, errs)
        E.check(f"dW[{i}]", _reduce(C, part, torch.float32), rw, None, errs)
    assert not errs, "\n".join(errs)


def test_distinct_branches(gpu_ext):
    """Different statistics, sums, inputs and filters per branch: each output is within its own branch's
    bound, and far outside the other branch's (so the inputs do tell a swapped branch)."""
    C = gpu_ext
    P = 2 * 14 * 14
    dy, mask, br = _inputs("uniform", P, 5)
    g = torch.Generator().manual_seed(11)
    sums = [(torch.rand(2 * CO, generator=g) * 8 - 4).cuda() for _ in range(2)]
    dxs = [_dx_from_sums(C, dy, mask, b, s) for b, s in zip(br, sums)]
    errs = []
    got = _fused(dy, mask, br, sums, 13, errs, "distinct")
    _check_branches(C, "distinct", got, dxs, br, P, errs)
    assert not errs, "\n".join(errs)
    swapped = []
    _check_branches(C, "swapped", got[::-1], dxs, br, P, swapped)
    assert len(swapped) == 4, "every output must tell its branch:\n" + "\n".join(swapped)


def _dual(C, dy, mask, br, P, dx, dx2):
    dw, db, dw2, db2 = (torch.full((CO,), float("nan"), device="cuda") for _ in range(4))
    ws, ws2 = torch.zeros(64 * 2 * 2048, device="cuda"), torch.zeros(64 * 2 * 2048, device="cuda")
    b0, b1 = br
    C.bn_bwd_dual(dy.data_ptr(), mask.data_ptr(), b0["c"].data_ptr(), b1["c"].data_ptr(), b0["bw"].data_ptr(),
                  b0["mean"].data_ptr(), b0["inv"].data_ptr(), b1["bw"].data_ptr(), b1["mean"].data_ptr(),
                  b1["inv"].data_ptr(), dx, dx2, dw.data_ptr(), db.data_ptr(), dw2.data_ptr(), db2.data_ptr(),
                  ws.data_ptr(), ws2.data_ptr(), P, CO, BF16, _st())
    torch.cuda.synchronize()
    return (dw, db, dw2, db2), (ws, ws2)


def test_bn_bwd_dual_without_dx(gpu_ext):
    """bn_bwd_dual(dx = dx2 = null): reduce and finalize only. The four sums are within the bounds the dual
    tests of test_norm_edges_gpu.py use (``norm_edges.bn_bwd_ref``: L 2^-23 sum |term|) of float64, as are
    those of the call with a dx, and the two calls agree within twice that (float atomics reorder)."""
    C = gpu_ext
    P = 8 * 28 * 28
    dy, mask, br = _inputs("uniform", P, 4)
    none, wss = _dual(C, dy, mask, br, P, 0, 0)
    dx, dx2 = torch.empty_like(dy), torch.empty_like(dy)
    full, _ = _dual(C, dy, mask, br, P, dx.data_ptr(), dx2.data_ptr())
    g = dy.double() * _bits(mask, P).double()
    errs = []
    for i, b in enumerate(br):
        r = N.bn_bwd_ref(dict(x=b["c"], dy=dy, w=b["bw"]), b["mean"], b["inv"], g, True, torch.bfloat16)
        for what, j, ref, bnd in (("dw", 0, r["dw"], r["ddw"]), ("db", 1, r["db"], r["ddb"])):
            E.check(f"null dx: {what}[{i}]", none[2 * i + j], ref, bnd, errs)
            E.check(f"with dx: {what}[{i}]", full[2 * i + j], ref, bnd, errs)
            E.check(f"null vs with dx: {what}[{i}]", none[2 * i + j], full[2 * i + j].double(), 2 * bnd, errs)
    assert all(float(w.abs().max()) == 0.0 for w in wss), "the finalize leaves both workspaces zeroed"
    assert not errs, "\n".join(errs)


def test_bn_bwd_dual_rejects_one_null_dx(gpu_ext):
    """Both dx or neither: one null pointer is an error, raised before any launch."""
    C = gpu_ext
    P = 49
    dy, mask, br = _inputs("uniform", P, 4)
    dx = torch.zeros_like(dy)
    for args in ((dx.data_ptr(), 0), (0, dx.data_ptr())):
        with pytest.raises(RuntimeError, match="or neither"):
            _dual(C, dy, mask, br, P, *args)
    torch.cuda.synchronize()
    assert float(dx.float().abs().max()) == 0.0


def test_host_checks(gpu_ext):
    """A misaligned pointer, a missing one and a slab count out of range raise before any launch."""
    P = 49
    dy, mask, br = _inputs("uniform", P, 4)
    sums = [torch.zeros(2 * CO, device="cuda") for _ in range(2)]
    out = torch.zeros(P + 1, CI, device="cuda", dtype=torch.bfloat16)
    part = torch.zeros(2, 2, CO * CI, device="cuda")
    b0, b1 = br

    def call(d_a2, slabs, a2=b0["act"].data_ptr()):
        _X().conv3ds_bwd(dy.data_ptr(), mask.data_ptr(), b0["c"].data_ptr(), b1["c"].data_ptr(), b0["bw"].data_ptr(),
                         b0["mean"].data_ptr(), b0["inv"].data_ptr(), sums[0][:CO].data_ptr(), sums[0][CO:].data_ptr(),
                         b1["bw"].data_ptr(), b1["mean"].data_ptr(), b1["inv"].data_ptr(), sums[1][:CO].data_ptr(),
                         sums[1][CO:].data_ptr(), a2, b1["act"].data_ptr(), b0["w"].data_ptr(), b1["w"].data_ptr(),
                         d_a2, out.data_ptr(), part[0].data_ptr(), part[1].data_ptr(), P, slabs, _st())

    with pytest.raises(RuntimeError, match="16-byte aligned"):
        call(out.data_ptr() + 8, 2)
    with pytest.raises(RuntimeError, match="all required"):
        call(out.data_ptr(), 2, a2=0)
    for slabs in (0, 65536):
        with pytest.raises(RuntimeError, match="slabs"):
            call(out.data_ptr(), slabs)
    torch.cuda.synchronize()
    assert float(out.float().abs().max()) == 0.0 and float(part.abs().max()) == 0.0


# ------------------------------------------------------------------------------- the autograd node

def _block(seed):
    from fluxmpi_amd.models.resnet import Bottleneck, _norm, conv1x1
    torch.manual_seed(seed)
    # layer1.0 as ResNet._make builds it: 64 -> 64 -> 256 with the 64 -> 256 stride-1 downsample
    down = torch.nn.Sequential(conv1x1(CI, CO, 1, "miopen"), _norm(CO, "fused"))
    blk = Bottleneck(CI, CI, 1, down, "hybrid").cuda().to(torch.bfloat16).to(memory_format=torch.channels_last)
    for bn in (blk.bn1, blk.bn2, blk.bn3, blk.downsample[1]):
        bn.float()
        with torch.no_grad():
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.uniform_(-0.2, 0.2)
    return blk.train()


def _up(t, cls):
    """Up the block's main path from ``t`` (every node there saves its input first) to the tensor that
    the autograd node ``cls`` produced."""
    while not type(t.grad_fn).__name__.startswith(cls):
        t = t.grad_fn.saved_tensors[0]
    return t


def _nhwc(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _input_grad_ref(dc1, w1, dxds, wds):
    """The block input's gradient = dc1 . W1 + dx_ds . W_ds from a path's own dc1 and bf16 dx_ds: float64
    reference and bound. The side summand is a bf16 GEMM result (``bound(.., 256, "bf16")``, b2); it is added
    in conv1's input-gradient epilogue (``bound(.., 64, "res")``) or, without a link, by autograd to the
    bf16 result of that GEMM (b1, then one bf16 rounding of the sum): the bound below covers both."""
    r1, a1 = E.ref_gemm(_nhwc(dc1), w1.reshape(CI, CI).t())
    r2, a2 = E.ref_gemm(dxds, wds.t())
    b2 = E.bound(r2, a2, CO, "bf16")
    return r1 + r2, E.bound(r1, a1, CI, "res", res=r2) + (1 + E.U8) * b2 + E.U8 * E.bound(r1, a1, CI, "bf16")


@pytest.mark.parametrize("form", [2, 1], ids=["dual", "two-launch"])
@pytest.mark.parametrize("linked", [True, False], ids=["link", "nolink"])
def test_autograd_downsample_block(gpu_ext, monkeypatch, linked, form):
    """A layer1.0-shaped block (N = 2, 14 x 14), switch on against switch off from ONE forward's saved
    tensors (two forwards differ in single ReLU bits: see test_conv3_bn3_bwd_gpu.py). On: the node's own
    backward. Off: what ``_DualBN``, ``_Conv1x1Hybrid`` and ``_Conv1x1Downsample`` run backward
    (``bn_bwd_dual`` with a dx, two input-gradient GEMMs, two weight gradients), on the saved tensors; its
    d_a2 goes down the same graph to the block input, its side gradient through the link (or is added).

    Per element, each path against the float64 references from its own bf16 operands within the derived
    bounds, and on against off within the sum of the two paths' bounds plus the distance of their
    references: d_a2, both filter gradients, the four BatchNorm parameter gradients and the block input's
    gradient after conv1's epilogue. With a link, ``link.delivered`` is true."""
    from fluxmpi_amd.ops import fused_block as fb
    from fluxmpi_amd.ops import gemm as G
    C = gpu_ext
    monkeypatch.setattr(fb, "CONV3DS", form)
    seen = {}

    class Rec(fb.SideGradLink):  # records what the node offers
        __slots__ = ()

        def offer(self, g):
            seen["side"] = g
            return super().offer(g)

    monkeypatch.setattr(fb, "SideGradLink", Rec if linked else (lambda: None))
    blk = _block(0)
    g = torch.Generator().manual_seed(5)
    n, h = 2, 14
    P = n * h * h
    x0 = torch.randn(n, CI, h, h, generator=g).bfloat16().cuda().contiguous(memory_format=torch.channels_last)
    dy = torch.randn(n, CO, h, h, generator=g).bfloat16().cuda().contiguous(memory_format=torch.channels_last)
    xl = x0.clone().requires_grad_(True)
    x = xl * 1  # the block input is a non-leaf, as in a network
    out = blk(x)
    node = out.grad_fn
    assert type(node).__name__.startswith("_Conv3DsBN"), type(node).__name__
    a2g, w3, xs, wds, c3, cds, mask, w32, mean, inv, w232, mean2, inv2 = node.saved_tensors
    link = node.link
    assert (link is not None) == linked
    c1 = _up(a2g, "_Conv1x1Hybrid")
    w1 = blk.conv1.weight.detach()
    a2g.register_hook(lambda t: seen.__setitem__("d_a2", t.clone()))
    c1.register_hook(lambda t: seen.__setitem__("dc1", t.clone()))
    a2, w3d, xd, wdsd = _nhwc(a2g.detach()), w3.detach().reshape(CO, CI), _nhwc(xs.detach()), wds.detach().reshape(CO, CI)
    dy2, c32, cds2 = _nhwc(dy), _nhwc(c3.detach()), _nhwc(cds.detach())
    br = (dict(c=c32, bw=w32, mean=mean, inv=inv, act=a2, w=w3d), dict(c=cds2, bw=w232, mean=mean2, inv=inv2, act=xd, w=wdsd))

    # ---- switch on: the node's own backward
    out.backward(dy, retain_graph=True)
    torch.cuda.synchronize()
    gx_on, gp_on = xl.grad.clone(), {k: p.grad.clone() for k, p in blk.named_parameters()}
    da_on, dc1_on = seen.pop("d_a2"), seen.pop("dc1")
    if linked:
        assert link.delivered, "conv1's dgrad epilogue did not take the side gradient"
        seen.pop("side")
    names = (("bn3.weight", "bn3.bias"), ("downsample.1.weight", "downsample.1.bias"))
    sums_on = [torch.cat([gp_on[nb].float(), gp_on[nw].float()]).contiguous() for nw, nb in names]
    dxs_on = [_dx_from_sums(C, dy2, mask, b, s) for b, s in zip(br, sums_on)]

    # ---- switch off, from the same saved tensors
    dxs_off = [torch.empty_like(dy2), torch.empty_like(dy2)]
    (dw_o, db_o, dw2_o, db2_o), _ = _dual(C, dy2, mask, br, P, dxs_off[0].data_ptr(), dxs_off[1].data_ptr())
    da_off = [G.conv1x1_dgrad(dxs_off[i], br[i]["w"]) for i in range(2)]
    dwt_off = [G.conv1x1_wgrad_v2(dxs_off[i], br[i]["act"], out_dtype=torch.bfloat16) for i in range(2)]
    side_off = da_off[1].view(n, h, h, CI).permute(0, 3, 1, 2)
    if linked:
        link.closed = False
        assert link.offer(side_off)
    gx_off, = torch.autograd.grad(a2g, [xl], grad_outputs=da_off[0].view(n, h, h, CI).permute(0, 3, 1, 2),
                                  retain_graph=True)
    if not linked:
        gx_off = gx_off + side_off
    torch.cuda.synchronize()
    dc1_off = seen.pop("dc1")

    errs = []
    dwt_on = [gp_on["conv3.weight"].reshape(CO, CI), gp_on["downsample.0.weight"].reshape(CO, CI)]
    for i, tag in enumerate(("conv3", "downsample")):
        (ra, aa), (rw, aw) = _refs(dxs_on[i], br[i]["w"], br[i]["act"])
        (ra_f, aa_f), (rw_f, aw_f) = _refs(dxs_off[i], br[i]["w"], br[i]["act"])
        ba, bw_, ba_f, bw_f = (E.bound(ra, aa, CO, "bf16"), E.bound(rw, aw, P, "bf16"), E.bound(ra_f, aa_f, CO, "bf16"),
                               E.bound(rw_f, aw_f, P, "bf16"))
        if i == 0:
            E.check("on d_a2", _nhwc(da_on), ra, ba, errs)
            E.check("on vs off d_a2", _nhwc(da_on), da_off[0].double(), ba + ba_f + (ra - ra_f).abs(), errs)
        E.check(f"off {tag} input gradient", da_off[i], ra_f, ba_f, errs)
        E.check(f"on {tag} filter", dwt_on[i], rw, bw_, errs)
        E.check(f"off {tag} filter", dwt_off[i], rw_f, bw_f, errs)
        E.check(f"on vs off {tag} filter", dwt_on[i], dwt_off[i].double(), bw_ + bw_f + (rw - rw_f).abs(), errs)
    gd = dy2.double() * _bits(mask, P).double()
    for i, (offs, (nw, nb)) in enumerate(zip(((dw_o, db_o), (dw2_o, db2_o)), names)):
        r = N.bn_bwd_ref(dict(x=br[i]["c"], dy=dy2, w=br[i]["bw"]), br[i]["mean"], br[i]["inv"], gd, True, torch.bfloat16)
        for name, off, ref, bnd in ((nw, offs[0], r["dw"], r["ddw"]), (nb, offs[1], r["db"], r["ddb"])):
            E.check(f"on {name}", gp_on[name], ref, bnd, errs)
            E.check(f"off {name}", off, ref, bnd, errs)
            E.check(f"on vs off {name}", gp_on[name], off.double(), 2 * bnd, errs)
    r_on, b_on = _input_grad_ref(dc1_on, w1, dxs_on[1], wdsd)
    r_off, b_off = _input_grad_ref(dc1_off, w1, dxs_off[1], wdsd)
    E.check("on block input", _nhwc(gx_on), r_on, b_on, errs)
    E.check("off block input", _nhwc(gx_off), r_off, b_off, errs)
    E.check("on vs off block input", _nhwc(gx_on), _nhwc(gx_off).double(), b_on + b_off + (r_on - r_off).abs(), errs)
    assert not errs, "\n".join(errs)


def test_switch_off_takes_the_unfused_path(gpu_ext, monkeypatch):
    """FLUXMPI_CONV3DS=0: the block runs the dual BatchNorm node as before."""
    from fluxmpi_amd.ops import fused_block as fb
    monkeypatch.setattr(fb, "CONV3DS", 0)
    blk = _block(1)
    x = torch.randn(2, CI, 14, 14).bfloat16().cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    out = blk(x * 1)
    assert type(out.grad_fn).__name__.startswith("_DualBN"), type(out.grad_fn).__name__
    out.backward(torch.ones_like(out))
    torch.cuda.synchronize()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad.float()).all()) for p in blk.parameters())
