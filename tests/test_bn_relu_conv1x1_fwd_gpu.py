"""bn2 apply + ReLU + conv3 forward in one kernel (csrc/kernels/bn_relu_conv1x1_fwd.hip) and the autograd
node built on it (``fused_block.bn_relu_conv3``), for (Cin, Cout) = (64, 256) and (128, 512).

Kernel level, through the entry point (no gate): a2 must EQUAL what ``bn_apply`` stores from the same
(w, b, mean, invstd), bit for bit (NaN where both are NaN cannot occur: the inputs are finite). That bf16
a2 is the exact operand of the float64 reference R = a2 . W^T and its absolute-value companion A
(``mfma_edges.ref_gemm``), so c3 lies within ``bound(R, A, Cin, "bf16")`` per element (uniform, cancel) or
EQUALS R (ternary, gather), and the statistics shards hold the column sums and sums of squares of the
kernel's own stored c3 (``check_colsums``: ternary exact; not for gather, whose bit patterns reach 3e38, so
that their squares and column sums leave fp32 in any kernel: ``stem_edges`` leaves them out for the same
reason; the guard band around the shards is checked there too).

scale / shift are handed to the kernel as ``bn_stats_finalize`` computes them: scale = w * invstd in fp32,
shift = fmaf(-mean, scale, b). The fmaf is formed here in float64 (the product is exact there) and rounded
to fp32: the same value unless the float64 sum lands on an fp32 rounding boundary, which the seeded inputs
do not (the EQUAL check on a2 would show it).

Exact families: BatchNorm weight +-2, invstd 1/2, mean 1/2 and bias +-1/2 give scale = +-1 and
shift = fmaf(-1/2, +-1, +-1/2) = 0; c2 = scale * (2 T - 1) for the family's 0 / 1 operand T, so a2 = T
exactly and every zero of T went through the ReLU. ternary rows carry 8 non-zeros: c3 is an integer of
magnitude <= 8 and the sums of 31 360 squares stay below 2^24.

Outputs lie in NaN-filled buffers between sentinel rows (``mfma_edges.guarded``), the shards in a zeroed
one: a row written out of range or left unwritten shows. Shapes: 49 pixels (one tile and a partial one),
392, 6272 and 31 360 (980 tiles over at most 512 workgroups and more: the persistent loop wraps unevenly).

Node level: a stage-1 identity block, the stage-1 downsample block (N = 6, 56 x 56) and a stage-2 block
(N = 24, 28 x 28), 18 816 pixels each (above the gate of 64 x compute units), switch on and off from the
same inputs.
"""
import pytest
import torch

from . import mfma_edges as E

pytestmark = pytest.mark.gpu

BF16 = 9
PAIRS = [(64, 256), (128, 512)]
PIXELS = [49, 392, 6272, 31360]
SHARDS = 64


def _st():
    return torch.cuda.current_stream().cuda_stream


def _entry():
    from fluxmpi_amd.ops import _ext
    return _ext.get(required=True)


def _inputs(family, P, ci, co, seed):
    """c2 [P, ci], W [co, ci] (bf16) and the BatchNorm vectors (w, b, mean, inv) (fp32), on the GPU."""
    t, w = E.gemm_inputs(family, P, co, ci, seed, nnz=8)
    g = torch.Generator().manual_seed(4000 + seed + P + ci)
    sign = (torch.randint(0, 2, (ci,), generator=g) * 2 - 1).float()
    if family in E.EXACT:
        t = t.float().abs()  # the 0 / 1 operand T = a2
        c2 = (sign * (2 * t - 1)).bfloat16()
        bw, bb, mean, inv = 2 * sign, 0.5 * sign, torch.full((ci,), 0.5), torch.full((ci,), 0.5)
    else:
        c2 = t
        bw = sign * (0.5 + torch.rand(ci, generator=g))
        bb = torch.rand(ci, generator=g) - 0.5
        mean, inv = 0.5 * torch.rand(ci, generator=g) - 0.25, 0.5 + 1.5 * torch.rand(ci, generator=g)
    return [v.cuda() for v in (c2, w, bw, bb, mean, inv)]


def _affine(bw, bb, mean, inv):
    """(scale, shift) of bn_finalize_fwd_kernel: w * invstd, fmaf(-mean, scale, b)."""
    scale = bw * inv
    shift = (bb.double() - mean.double() * scale.double()).float()
    return scale.contiguous(), shift.contiguous()


def _bn_apply(C, c2, bw, bb, mean, inv):
    y = torch.full_like(c2, float("nan"))
    C.bn_apply(c2.data_ptr(), y.data_ptr(), 0, bw.data_ptr(), bb.data_ptr(), mean.data_ptr(), inv.data_ptr(),
               c2.shape[0], c2.shape[1], 1, 0, BF16, _st())
    return y


def _fused(c2, scale, shift, w, errs, name):
    """The entry point into guarded outputs; returns (a2 [P, ci], c3 [P, co], shards [64, 2, co])."""
    P, ci = c2.shape
    co = w.shape[0]
    abuf, aview = E.guarded(P, ci, ci, torch.bfloat16, c2.device)
    cbuf, cview = E.guarded(P, co, co, torch.bfloat16, c2.device)
    sbuf, sview = E.guarded(SHARDS, 2 * co, 2 * co, torch.float32, c2.device, fill=0.0)
    _entry().bn_relu_conv1x1_fwd(c2.data_ptr(), scale.data_ptr(), shift.data_ptr(), w.data_ptr(), aview.data_ptr(),
                                 cview.data_ptr(), sview.data_ptr(), P, ci, co, _st())
    torch.cuda.synchronize()
    return (E.take_guarded(f"{name} a2", abuf, aview, errs), E.take_guarded(f"{name} c3", cbuf, cview, errs),
            E.take_guarded(f"{name} shards", sbuf, sview, errs).view(SHARDS, 2, co))


def _bits_equal(name, got, ref, errs):
    bad = got.view(torch.int16) != ref.view(torch.int16)
    if bool(bad.any()):
        i = tuple(int(j) for j in torch.nonzero(bad)[0])
        errs.append(f"{name}: {int(bad.sum())} of {got.numel()} differ in bits; first at {i}: got "
                    f"{float(got[i]):.9g} ref {float(ref[i]):.9g}")


@pytest.mark.parametrize("family", E.FAMILIES)
@pytest.mark.parametrize("P", PIXELS)
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}to{p[1]}")
def test_kernel(gpu_ext, pair, P, family):
    C = gpu_ext
    ci, co = pair
    c2, w, bw, bb, mean, inv = _inputs(family, P, ci, co, 1)
    scale, shift = _affine(bw, bb, mean, inv)
    a2_ref = _bn_apply(C, c2, bw, bb, mean, inv)
    errs = []
    a2, c3, shards = _fused(c2, scale, shift, w, errs, family)
    assert bool(torch.isfinite(a2_ref.float()).all())
    _bits_equal("a2 vs bn_apply", a2, a2_ref, errs)
    if family in E.EXACT:
        assert float(scale.abs().min()) == 1.0 and float(scale.abs().max()) == 1.0 and float(shift.abs().max()) == 0.0
        t = E.gemm_inputs(family, P, co, ci, 1, nnz=8)[0].float().abs().cuda()
        E.check("a2 vs the 0 / 1 operand", a2, t.double(), None, errs)
    r, a = E.ref_gemm(a2_ref, w)
    if family in E.EXACT:
        assert bool((r.bfloat16().double() == r).all()), "the reference itself must be exact in bf16"
    E.check_out("c3", family, c3, r, a, ci, "bf16", errs)
    if family != "gather":  # (its bit patterns reach 3e38: their squares and column sums overflow fp32 in any kernel)
        E.check_colsums("shards", family, shards, c3, errs)
    assert not errs, "\n".join(errs)


def test_rejects_other_shapes(gpu_ext):
    """Other channel pairs, a misaligned pointer and an empty batch are errors raised before any launch."""
    c2, w, bw, bb, mean, inv = _inputs("uniform", 49, 64, 256, 2)
    scale, shift = _affine(bw, bb, mean, inv)
    a2, c3 = torch.zeros_like(c2), torch.zeros(49, 256, device="cuda", dtype=torch.bfloat16)
    ws = torch.zeros(SHARDS * 2 * 256, device="cuda")
    args = [c2.data_ptr(), scale.data_ptr(), shift.data_ptr(), w.data_ptr(), a2.data_ptr(), c3.data_ptr(), ws.data_ptr()]
    fn = _entry().bn_relu_conv1x1_fwd
    for P, ci, co in ((49, 64, 512), (49, 256, 1024), (0, 64, 256)):
        with pytest.raises(RuntimeError, match="needs"):
            fn(*args, P, ci, co, _st())
    with pytest.raises(RuntimeError, match="aligned"):
        fn(args[0] + 2, *args[1:], 48, 64, 256, _st())
    with pytest.raises(RuntimeError, match="required"):
        fn(*args[:4], 0, *args[5:], 49, 64, 256, _st())
    torch.cuda.synchronize()
    assert float(a2.float().abs().max()) == 0.0 and float(c3.float().abs().max()) == 0.0 and float(ws.abs().max()) == 0.0


# ------------------------------------------------------------------------------- node level

def _block(kind, seed):
    from fluxmpi_amd.models.resnet import Bottleneck, _norm, conv1x1
    torch.manual_seed(seed)
    if kind == "identity1":
        blk, shape = Bottleneck(256, 64, conv_impl="hybrid"), (6, 256, 56, 56)
    elif kind == "downsample1":
        down = torch.nn.Sequential(conv1x1(64, 256, 1, "miopen"), _norm(256, "fused"))
        blk, shape = Bottleneck(64, 64, 1, down, "hybrid"), (6, 64, 56, 56)
    else:
        blk, shape = Bottleneck(512, 128, conv_impl="hybrid"), (24, 512, 28, 28)
    blk = blk.cuda().to(torch.bfloat16).to(memory_format=torch.channels_last)
    for bn in [m for m in blk.modules() if hasattr(m, "running_mean")]:
        bn.float()
        with torch.no_grad():
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.uniform_(-0.2, 0.2)
    return blk.train(), shape


def _ours(monkeypatch, blk, shape):
    """conv3's forward counts as 'ours' for the shape (what ``conv1x1_forward_is_ours`` would measure on
    a quiet device): the precondition of the fused path, fixed here so that both arms run the same nodes."""
    from fluxmpi_amd.ops import fused_block as fb
    n, _, h, w = shape
    ci, co = blk.conv3.weight.shape[1], blk.conv3.weight.shape[0]
    monkeypatch.setitem(fb._FWD1_CHOICE, ((n, ci, h, w), co), True)


def _run(blk, x0, dy, on, monkeypatch):
    """Forward + backward with the switch ``on``; returns what the comparison needs."""
    from fluxmpi_amd.ops import fused_block as fb
    monkeypatch.setattr(fb, "BN2CONV3", on)
    for p in blk.parameters():
        p.grad = None
    x = x0.clone().requires_grad_(True)
    out = blk(x * 1)  # the block input is a non-leaf, as in a network
    node = out.grad_fn
    name = type(node).__name__
    if name.startswith("_Conv3BN3"):
        a2, c3 = node.saved_tensors[0], node.saved_tensors[2]
    elif name.startswith("_Conv3DsBN"):
        a2, c3 = node.saved_tensors[0], node.saved_tensors[4]
    else:
        assert name.startswith("_BNFromStats") or name.startswith("_DualBN"), name
        c3 = node.saved_tensors[0]
        assert type(c3.grad_fn).__name__.startswith("_Conv1x1Hybrid"), type(c3.grad_fn).__name__
        a2 = c3.grad_fn.saved_tensors[0]
    bn2 = a2.grad_fn
    assert type(bn2).__name__.startswith("_BN2Conv3" if on else "_BNFromStats"), type(bn2).__name__
    c2 = bn2.saved_tensors[0]
    # saved by both nodes in this order after c2 (the unfused node keeps a None mask in between)
    w32, b32, mean, inv = [t for t in bn2.saved_tensors[1:] if t is not None][:4]
    seen = {}
    c2.register_hook(lambda t: seen.__setitem__("dc2", t.clone()))
    out.backward(dy)
    torch.cuda.synchronize()
    grads = {n: p.grad.clone() for n, p in blk.named_parameters()}
    grads["input"], grads["c2"] = x.grad.clone(), seen["dc2"]
    return dict(out=out.detach(), a2=a2.detach(), c3=c3.detach(), c2=c2.detach(), bn=(w32, b32, mean, inv), grads=grads)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


@pytest.mark.parametrize("kind", ["identity1", "downsample1", "identity2"])
def test_node(gpu_ext, monkeypatch, kind):
    """Switch on and off from the same inputs. In each arm a2 EQUALS ``bn_apply`` of the arm's own c2 and
    saved statistics and c3 lies within ``bound(R, A, Cin, "bf16")`` of the float64 product of that a2.
    Between the arms the statistics differ in the last place (float atomics), and single ReLU bits with them,
    so they are compared as the existing block tests compare two forwards: the block output and the gradients
    of the block input, of c2, of bn2's weight and bias, of W3 and of every other parameter within 2^-7 of
    the norm (two bf16 roundings)."""
    C = gpu_ext
    blk, shape = _block(kind, 0)
    _ours(monkeypatch, blk, shape)
    g = torch.Generator().manual_seed(11)
    x0 = torch.randn(*shape, generator=g).bfloat16().cuda().contiguous(memory_format=torch.channels_last)
    n, _, h, w = shape
    dy = torch.randn(n, blk.conv3.weight.shape[0], h, w, generator=g).bfloat16().cuda().contiguous(
        memory_format=torch.channels_last)
    ci = blk.conv3.weight.shape[1]
    w3 = blk.conv3.weight.detach().reshape(-1, ci)
    errs = []
    runs = {}
    for on in (True, False):
        tag = "on" if on else "off"
        r = runs[on] = _run(blk, x0, dy, on, monkeypatch)
        a2_ref = _bn_apply(C, _nhwc(r["c2"]).contiguous(), *r["bn"])
        _bits_equal(f"{tag} a2 vs bn_apply", _nhwc(r["a2"]), a2_ref, errs)
        ref, mag = E.ref_gemm(a2_ref, w3)
        E.check(f"{tag} c3", _nhwc(r["c3"]), ref, E.bound(ref, mag, ci, "bf16"), errs)
    pairs = {name: (runs[True]["grads"][name], runs[False]["grads"][name]) for name in runs[True]["grads"]}
    pairs["output"] = (runs[True]["out"], runs[False]["out"])
    for name, (a, b) in pairs.items():
        rel = float((a.double() - b.double()).norm() / b.double().norm())
        print(f"{name}: on vs off, relative 2-norm difference {rel:.3e}")
        if not rel <= 2.0 ** -7:
            errs.append(f"{name}: on vs off differ by {rel:.3e} of the norm")
    assert not errs, "\n".join(errs)


def test_gate(gpu_ext, monkeypatch):
    """Without gradients, in eval mode and below 64 x compute-unit pixels the block issues the unfused
    launches; above the gate in training mode it issues the fused kernel once."""
    from fluxmpi_amd.ops import fused_block as fb
    blk, shape = _block("identity1", 1)
    _ours(monkeypatch, blk, shape)
    calls = []
    real = fb.launch_apply_conv1x1
    monkeypatch.setattr(fb, "launch_apply_conv1x1", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    g = torch.Generator().manual_seed(12)
    x = torch.randn(*shape, generator=g).bfloat16().cuda().contiguous(memory_format=torch.channels_last)
    blk(x.clone().requires_grad_(True))
    assert len(calls) == 1
    with torch.no_grad():
        blk(x)
    blk.eval()
    blk(x.clone().requires_grad_(True))
    blk.train()
    cus = torch.cuda.get_device_properties(x.device).multi_processor_count
    small = x[:1]  # 3136 pixels
    assert small.shape[0] * 56 * 56 < 64 * cus
    monkeypatch.setitem(fb._FWD1_CHOICE, ((1, 64, 56, 56), 256), True)
    out = blk(small.clone().requires_grad_(True))
    a2 = out.grad_fn.saved_tensors[0]
    assert type(a2.grad_fn).__name__.startswith("_BNFromStats"), type(a2.grad_fn).__name__
    torch.cuda.synchronize()
    assert len(calls) == 1
