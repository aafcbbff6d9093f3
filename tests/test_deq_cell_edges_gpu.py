"""The fused DEQ cell kernels (deq_cell.hip: deq_cell_fwd_kernel, deq_cell_vjp_kernel, deq_adjoint_check_kernel)
per element against float64 references: the forward stage by stage from the kernel's own stored state, the
VJP against the float64 chain under a bound composed by absolute-value propagation, exact cases that must be
EQUAL, guard bands around every output, the launcher's refusals, and a CPU half that shows a float32
evaluation in the kernels' summation order meets every bound, reproduces every exact case and that planted
defects trip the same checkers. ``deq_cell_edges``' docstring writes out every bound term.

Input families (seeded, made on the CPU; ``conv_inputs`` per convolution):
    uniform   z, W1, W2 as ``mfma_edges``; x in [-2, 2), affine w in +-[0.5, 1.5), |b| in [2^-4, 1)
    cancel    adjacent channel pairs cancel under equal weights: only the accumulation term is left
    ternary   h1 is an integer of magnitude <= 256: EQUAL; the later stages by their bounds
    gather    stage 1 only: h1 EQUALS the selected bit patterns, all nine padding cases and every
              pixel-block-to-row mapping in one launch
    chain     gather filters, z in {+-1, +-2, +-4}, GN1 bias 0: h1 and h2 EQUAL (a1 reproduced in float32)
    offset    x shifted by 4 and 32 standard deviations: GN2's E[h^2] - mean^2 cancellation (kappa)
    VJP       uniform, cancel (u and filters), offset 4 / 32 on the supplied h_k; exact (integers, EQUAL,
              with ``grad``: u_new, ss_part and deq_adjoint_check EQUAL too); zero W1 (out = d3, checked with
              ``gn_check_bwd`` directly); centre-tap identity filters (both convolutions exact)
    guard     out, out32 (row stride H W C + 8), out_slot (row stride H W C + 16), h1 .. h3 and the six
              statistics lie inside sentinel bands, NaN inside: no sentinel touched, no NaN left

Shapes (N, H, W) at 48 channels and the code paths they reach (asserted in ``test_shapes_reach_paths_cpu``):
    (1, 1, 16) (3, 16, 1) (3, 2, 8) (3, 4, 4)   one pixel block: waves 1 .. 7 own nothing (L.ok[i] false
                                                everywhere); H = 1 / W = 1: every tap but the row / column is halo
    (3, 3, 16)                                  3 blocks, one per image row
    (3, 8, 8) (3, 5, 16) (2, 16, 16)            4, 5, 16 blocks: partly idle waves; blocks of two rows at W = 8
    (3, 16, 7)                                  7 blocks, W does not divide 16: every block straddles rows
    (3, 12, 12)                                 9 blocks: wave 0 owns two, blocks straddle rows
    (2, 28, 28)                                 49 blocks, the production shape (wave 0 owns 7, the others 6)
    (2, 28, 32) (2, 8, 112)                     56 blocks: nothing idle; the widest supported row
    (300, 4, 4)                                 more workgroups than CUs
    G in {1, 2, 3, 4, 6, 8, 12, 16} at (3, 16, 7) and (2, 28, 28), {1, 8, 16} elsewhere; cpg = 3 at G = 16: a
    group boundary inside a lane's four channels. eps 1e-5, and 2^-6 in ``test_fwd_eps_forwarded``.
    Refusals (``test_refusals``, and on the host alone ``test_refusals_before_any_launch_cpu``): H W = 196, 912;
    (112, 8) and (4, 224) (56 blocks, over 160 KB of LDS, sizes
    from the documented formula); G = 24, 5; C = 64; a misaligned pointer; (8, 112) and (7, 128) are taken.
    Variants: null w / b, keep=False, two launches bit-identical, ``cell_forward`` / ``cell_vjp`` /
    ``ResidualCell.adjoint_step`` against the raw calls, a state from the fused and from the unfused forward,
    an ``out`` that aliases grad or a state tensor (raw: raises; wrapper: a fresh tensor).

Kernel / launcher changes this file needed: the launchers compared the LDS size with 160 KB only once, for the
constant they request, so (112, 8) and (4, 224) went on to the launch, asking for more dynamic LDS than that; both now refuse such a
shape before any launch, as ``deq_cell_supported`` does. ``deq_cell_vjp`` parks d3 in ``out`` and reads grad
and h1 .. h3 afterwards; it refused only ``out == u`` and now refuses any overlap of ``out`` with its inputs
(``cell_vjp`` takes a fresh tensor instead). No kernel arithmetic changed.

Measured on the MI355X (one run of this file), worst |err| / bound over every shape, group count and family:
    forward   h1 0.938 (uniform / offset; cancel 0.136: |R| << A there), mean1 .. mean3 0.050 / 0.038 / 0.049,
              rstd1 .. rstd3 0.223 (cancel) / 0.079 / 0.070, h2 0.854 (offset; uniform 0.600, ternary 0.398),
              h3 0.995, out 0.995; out32, out_slot, keep=False, null affine, the wrappers and the second launch
              bit-identical; ternary / gather / chain h1 and chain h2 EQUAL
    VJP       d3 alone (zero W1) 0.995, identity filters 0.532, the full chain uniform 0.206, cancel 0.184,
              offset 4 / 32 0.070 / 0.066, a state from the fused / unfused forward 0.008; the exact case, its
              ss_part and deq_adjoint_check EQUAL
A stage whose bound is its own output rounding (h1, h3, out, d3) sits just under 1, as a correctly rounded store
must. h2 and the full VJP chain sit lower because their bounds carry the propagated term (up to 432 roundings of
the previous stage added in absolute value, signed in reality): expected, and not tightened by fit. The sharp VJP
criteria are therefore the exact case, d3 alone and the identity filters; the CPU half shows that a GroupNorm
backward reading the wrong h passes the full-chain bound (its h-dependent part is O(M^-1/2)) and fails the
identity-filter one 12.6-fold. No kernel exceeded a derived bound and no bound was changed after the first run.
Wall time: the 159 GPU tests of this file 10.1 s run alone, next to 134 s for the rest of the GPU suite
(144.4 s together, one run); the CPU half's 79 tests 12 s.
"""

import pytest
import torch

from . import deq_cell_edges as D
from . import mfma_edges as E
from . import norm_edges as NE
from .deq_cell_edges import BF, C

gpu = pytest.mark.gpu

SHAPES = [(1, 1, 16), (3, 16, 1), (3, 2, 8), (3, 4, 4), (3, 3, 16), (3, 8, 8), (3, 16, 7), (3, 5, 16), (3, 12, 12),
          (2, 16, 16), (2, 28, 28), (2, 28, 32), (2, 8, 112), (300, 4, 4)]
ALL_G = ((3, 16, 7), (2, 28, 28))
CASES = [(s, G) for s in SHAPES for G in (D.GROUPS if s in ALL_G else (1, 8, 16))]
CASE_IDS = [f"{n}x{h}x{w}-G{G}" for (n, h, w), G in CASES]
EXACT_CASES = [(s, G) for s, G in CASES if s[1] >= 3 and s[2] >= 3 and s[0] <= 3]
EXACT_IDS = [f"{n}x{h}x{w}-G{G}" for (n, h, w), G in EXACT_CASES]
FWD_FAMILIES = [("uniform", 0), ("cancel", 0), ("ternary", 0), ("gather", 0), ("chain", 0), ("offset", 4), ("offset", 32)]
VJP_FAMILIES = [("uniform", 0), ("cancel", 0), ("offset", 4), ("offset", 32)]
EPS = 1e-5
EPS_OTHER = 2.0 ** -6  # float32-representable, 1562 x 1e-5
REFUSED_HW = [(14, 14), (24, 38), (112, 8), (4, 224)]
EXACT_SEEDS = (0, 1, 2)


def _done(errs):
    assert not errs, "\n".join(errs[:20]) + (f"\n... and {len(errs) - 20} more" if len(errs) > 20 else "")


# =============================================================================== CPU half

def test_lds_arithmetic_cpu():
    """The refusal predicate from the documented formula: the two 56-block shapes over 160 KB, the two under."""
    assert D.lds_bytes(28, 28) == 30 * (30 * 48 + 32) * 2 + 44544 + 4032
    assert D.lds_bytes(112, 8) == 165312 and D.lds_bytes(4, 224) == 179136          # > 163840
    assert D.lds_bytes(8, 112) == 158656 and D.lds_bytes(7, 128) == 161472          # <= 163840
    for H, W in ((112, 8), (4, 224), (8, 112), (7, 128)):
        assert H * W == 896 and H * W // 16 == 56
    assert not D.supported_ref(112, 8, 48, 8) and not D.supported_ref(4, 224, 48, 8)
    assert D.supported_ref(8, 112, 48, 8) and D.supported_ref(7, 128, 48, 8)
    assert not D.supported_ref(14, 14, 48, 8) and 14 * 14 == 196 and 196 % 16 != 0
    assert not D.supported_ref(24, 38, 48, 8) and 24 * 38 == 912 and 912 % 16 == 0 and 912 // 16 == 57
    assert not D.supported_ref(28, 28, 48, 24) and not D.supported_ref(28, 28, 48, 5)
    assert not D.supported_ref(28, 28, 64, 8)
    assert all(D.supported_ref(h, w, 48, G) for (_, h, w), G in CASES)


def test_refusals_before_any_launch_cpu():
    """The predicate and both launchers on the host alone: every refusal is raised from the argument checks,
    before the first HIP call, so it reads the same on a machine without a GPU (the pointers are never
    dereferenced). The GPU half repeats this next to real buffers."""
    try:
        import fluxmpi_amd._C as ext
    except ImportError:
        pytest.skip("fluxmpi_amd._C is not built")
    assert ext.deq_cell_supported(8, 112, 48, 8) and ext.deq_cell_supported(7, 128, 48, 8)
    assert all(ext.deq_cell_supported(h, w, 48, G) == D.supported_ref(h, w, 48, G)
               for h in (1, 2, 4, 7, 8, 16, 28, 112) for w in (1, 4, 7, 8, 16, 28, 32, 112, 128) for G in range(1, 26))
    for H, W, ch, G in [(H, W, 48, 8) for H, W in REFUSED_HW] + [(28, 28, 48, 24), (28, 28, 48, 5), (28, 28, 64, 8)]:
        assert not ext.deq_cell_supported(H, W, ch, G) and not D.supported_ref(H, W, ch, G)
    if torch.cuda.is_available():
        return  # made-up pointers stay away from a real device: test_refusals / test_vjp_refuses_aliased_out
    p, q, o = 1 << 20, 2 << 20, 3 << 20

    def fwd(H, W, ch, G, z=p):
        ext.deq_cell_fwd(z, p, q, q, [0, 0, 0], [0, 0, 0], o, 0, 0, [0, 0, 0], [0, 0, 0], [0, 0, 0], 1, H, W, ch, G, EPS, 0, 0)

    def vjp(H, W, ch, G, u=p, out=o, h=(p, p, p), grad=0, part=0):
        ext.deq_cell_vjp(u, list(h), q, q, [q, q, q], [q, q, q], [q, q, q], out, grad, part, 1, H, W, ch, G, 0)

    for H, W, ch, G in [(H, W, 48, 8) for H, W in REFUSED_HW] + [(28, 28, 48, 24), (28, 28, 48, 5), (28, 28, 64, 8)]:
        for call in (fwd, vjp):
            with pytest.raises(RuntimeError, match="deq_cell"):
                call(H, W, ch, G)
    for H, W in ((112, 8), (4, 224)):
        for call in (fwd, vjp):
            with pytest.raises(RuntimeError, match="does not fit in LDS"):
                call(H, W, 48, 8)
    for call in (fwd, vjp):
        with pytest.raises(RuntimeError, match="16-byte aligned"):
            call(4, 4, 48, 8, p + 2)
    act = 4 * 4 * 48 * 2
    for kw in (dict(out=p), dict(h=(p, o, p)), dict(grad=o, part=q), dict(out=p + act - 16), dict(h=(p, p, o + act - 16))):
        with pytest.raises(RuntimeError, match="alias"):
            vjp(4, 4, 48, 8, **kw)


def test_shapes_reach_paths_cpu():
    """The chosen shapes reach the paths they are listed for."""
    blocks = {s: s[1] * s[2] // 16 for s in SHAPES}
    assert [blocks[s] for s in SHAPES] == [1, 1, 1, 1, 3, 4, 7, 5, 9, 16, 49, 56, 56, 1]
    owned = lambda nb, w: len(range(w, nb, 8))           # pixel blocks of wave w
    assert owned(1, 0) == 1 and all(owned(1, w) == 0 for w in range(1, 8))
    assert owned(9, 0) == 2 and owned(9, 1) == 1 and owned(49, 0) == 7 and owned(49, 1) == 6
    assert all(owned(56, w) == 7 for w in range(8))
    assert 16 % 7 != 0 and all((16 * b) // 7 != (16 * b + 15) // 7 for b in range(7))   # every block straddles rows
    assert 16 % 12 != 0 and 16 // 8 == 2
    assert 300 > 256
    assert 48 // 16 == 3 and any((4 * q) // 3 != (4 * q + 3) // 3 for q in range(12))   # a group boundary in a lane
    assert D.cell_L(16) == 22 and D.cell_L(1) == 67
    assert EPS_OTHER / EPS >= 1000 and float(torch.tensor(EPS_OTHER, dtype=torch.float32)) == EPS_OTHER


def _cpu_groups(shape):
    return D.GROUPS if shape == (3, 16, 7) else (1, 8, 16)


@pytest.mark.parametrize("shape", SHAPES, ids=[f"{n}x{h}x{w}" for n, h, w in SHAPES])
def test_emulation_fwd_meets_bounds_cpu(shape):
    n, h, w = min(shape[0], 5), shape[1], shape[2]
    errs = []
    for G in _cpu_groups(shape):
        for family, ratio in FWD_FAMILIES:
            if family == "gather" and G != 8:
                continue  # stage 1 does not depend on G
            inp = D.fwd_inputs(family, n, h, w, ratio=ratio, null_affine=family == "cancel")
            out = D.emulate_fwd(inp, G, EPS)
            D.check_fwd(f"cpu fwd {family}{ratio} {shape} G{G}", inp, out, G, EPS, errs)
    _done(errs)


@pytest.mark.parametrize("shape", SHAPES, ids=[f"{n}x{h}x{w}" for n, h, w in SHAPES])
def test_emulation_vjp_meets_bounds_cpu(shape):
    n, h, w = min(shape[0], 5), shape[1], shape[2]
    errs = []
    for G in _cpu_groups(shape):
        for family, ratio in VJP_FAMILIES:
            inp = D.vjp_inputs(family, n, h, w, G, ratio=ratio)
            D.check_vjp(f"cpu vjp {family}{ratio} {shape} G{G}", inp, D.emulate_vjp(inp, G)[0], G, errs)
    for filt in ("zero_w1", "identity"):
        inp = D.vjp_inputs("uniform", n, h, w, 8, filt=filt)
        got = D.emulate_vjp(inp, 8)[0]
        D.check_vjp(f"cpu vjp {filt} {shape}", inp, got, 8, errs)
        if filt == "zero_w1":
            NE.gn_check_bwd(f"cpu vjp d3 {shape}", inp["u"], inp["h"][2], inp["mean"][2], inp["rstd"][2], inp["gw"][2], 8,
                            True, dict(dh=got), BF, errs, Lpx=D.L_PX)
    _done(errs)


@pytest.mark.parametrize("shape,G", EXACT_CASES, ids=EXACT_IDS)
def test_vjp_exact_structure_cpu(shape, G):
    """The exact case is exact: the sums vanish, every rounding point holds a bf16-exact value, every tap of
    W1^T is hit over the seeds, and the float32 emulation reproduces the chain."""
    n, h, w = shape
    hit = torch.zeros(9, dtype=torch.bool)
    for seed in EXACT_SEEDS:
        inp = D.vjp_exact_inputs(n, h, w, G, seed)
        ref, ss = D.vjp_exact_asserts(inp, G)
        hit |= (inp["t1t"].float().view(C, 9, C) != 0).any(2).any(0)
        assert int((inp["t1t"] != 0).sum(1).max()) <= 4
        got, ss_e = D.emulate_vjp(inp, G)
        errs = []
        E.check(f"cpu exact {shape} G{G} seed{seed}", got, ref, None, errs)
        E.check("ss", ss_e, ss, None, errs)
        _done(errs)
    assert bool(hit.all())
    assert bool((inp["h"][0][0, 0].float() <= 0).any()) and bool((inp["h"][0][0, 0].float() > 0).sum() > 40)
    assert bool((inp["h"][2].float() < 0).any()) and bool((inp["h"][2].float() > 0).any())


FWD_DEFECTS = {"ktail": ("uniform", (3, 8, 8), 8), "shifted_tap": ("uniform", (3, 8, 8), 8),
               "lost_block": ("uniform", (2, 28, 28), 8), "neighbour_group": ("uniform", (3, 16, 7), 16),
               "truncation": ("uniform", (3, 8, 8), 8)}


@pytest.mark.parametrize("defect", list(FWD_DEFECTS) + ["h3_for_stage2", "truncation_vjp", "ktail_gather"])
def test_planted_defect_fails_cpu(defect):
    def run(on):
        errs = []
        if defect == "h3_for_stage2":  # the h-dependent part of a GroupNorm backward is C h with C = O(M^-1/2):
            # below the propagated bound of a 432-term convolution, far above it where the convolutions are exact
            inp = D.vjp_inputs("uniform", 3, 8, 8, 8, filt="identity")
            D.check_vjp(defect, inp, D.emulate_vjp(inp, 8, defect if on else None)[0], 8, errs)
        elif defect == "truncation_vjp":  # seen where one rounding is observable: out = d3 under a zero W1
            inp = D.vjp_inputs("uniform", 3, 8, 8, 8, filt="zero_w1")
            got = D.emulate_vjp(inp, 8, "truncation" if on else None)[0]
            NE.gn_check_bwd(defect, inp["u"], inp["h"][2], inp["mean"][2], inp["rstd"][2], inp["gw"][2], 8, True,
                            dict(dh=got), BF, errs, Lpx=D.L_PX)
        elif defect == "ktail_gather":  # an exact family sees one dropped term wherever it lands
            inp = D.fwd_inputs("ternary", 3, 8, 8)
            D.check_fwd(defect, inp, D.emulate_fwd(inp, 8, EPS, "ktail" if on else None), 8, EPS, errs)
        else:
            family, (n, h, w), G = FWD_DEFECTS[defect]
            inp = D.fwd_inputs(family, n, h, w)
            D.check_fwd(defect, inp, D.emulate_fwd(inp, G, EPS, defect if on else None), G, EPS, errs)
        return errs

    _done(run(False))
    errs = run(True)
    print("\n".join(errs))
    assert errs, f"the checkers did not notice the planted defect {defect}"


# =============================================================================== GPU: plumbing

def _st():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return 0 if t is None else t.data_ptr()


def _cuda(ts):
    return [None if t is None else t.cuda() for t in ts]


def _take(name, pair, errs, shape=None):
    t = E.take_guarded(name, pair[0], pair[1], errs).cpu()
    return t if shape is None else t.reshape(shape)


def _fwd(ext, tag, inp, N, G, eps, errs, keep=True, slot=False, o32=True):
    """One raw forward inside guard bands: dict(h, mean, rstd, out[, out32]) on the CPU."""
    H, W = inp["H"], inp["W"]
    HW, nel = H * W, H * W * C
    z, x, t1, t2 = _cuda([inp["z"], inp["x"], inp["t1"], inp["t2"]])
    gw, gb = _cuda(inp["gw"]), _cuda(inp["gb"])
    ob = E.guarded(N, nel, nel + (16 if slot else 0), BF, "cuda")
    of = E.guarded(N, nel, nel + 8, torch.float32, "cuda") if o32 else None
    hs = [E.guarded(N, nel, nel, BF, "cuda") for _ in range(3)] if keep else []
    ms = [E.guarded(1, N * G, N * G + 8, torch.float32, "cuda") for _ in range(6)] if keep else []
    hp = [h[1].data_ptr() for h in hs] if keep else [0, 0, 0]
    mp = [m[1].data_ptr() for m in ms[:3]] if keep else [0, 0, 0]
    rp = [m[1].data_ptr() for m in ms[3:]] if keep else [0, 0, 0]
    ext.deq_cell_fwd(z.data_ptr(), x.data_ptr(), t1.data_ptr(), t2.data_ptr(), [_p(t) for t in gw], [_p(t) for t in gb],
                     ob[1].data_ptr(), of[1].data_ptr() if o32 else 0, nel + 8 if o32 else 0, hp, mp, rp,
                     N, H, W, C, G, eps, _st(), nel + 16 if slot else 0)
    torch.cuda.synchronize()
    out = dict(out=_take(f"{tag} out", ob, errs, (N, HW, C)))
    if o32:
        out["out32"] = _take(f"{tag} out32", of, errs, (N, HW, C))
    if keep:
        out["h"] = [_take(f"{tag} h{k + 1}", hs[k], errs, (N, HW, C)) for k in range(3)]
        out["mean"] = [_take(f"{tag} mean{k + 1}", ms[k], errs, (N, G)) for k in range(3)]
        out["rstd"] = [_take(f"{tag} rstd{k + 1}", ms[3 + k], errs, (N, G)) for k in range(3)]
    return out


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def _same(name, a, b, errs):
    if not torch.equal(_bits(a), _bits(b)):
        errs.append(f"{name}: {int((_bits(a) != _bits(b)).sum())} elements differ in their bits")


def _vjp(ext, tag, inp, N, G, errs, out_ptr=None):
    """One raw VJP inside guard bands: (out [N, HW, C], ss_part [N] or None) on the CPU."""
    H, W = inp["H"], inp["W"]
    nel = H * W * C
    u, t2t, t1t, grad = _cuda([inp["u"], inp["t2t"], inp["t1t"], inp["grad"]])
    hs, gw, mean, rstd = _cuda(inp["h"]), _cuda(inp["gw"]), _cuda(inp["mean"]), _cuda(inp["rstd"])
    ob = E.guarded(N, nel, nel, BF, "cuda")
    pt = E.guarded(1, N, N + 8, torch.float32, "cuda") if grad is not None else None
    ext.deq_cell_vjp(u.data_ptr(), [t.data_ptr() for t in hs], t2t.data_ptr(), t1t.data_ptr(), [_p(t) for t in gw],
                     [t.data_ptr() for t in mean], [t.data_ptr() for t in rstd], ob[1].data_ptr(), _p(grad),
                     pt[1].data_ptr() if pt else 0, N, H, W, C, G, _st())
    torch.cuda.synchronize()
    return (_take(f"{tag} out", ob, errs, (N, H * W, C)),
            _take(f"{tag} ss_part", pt, errs, (N,)) if pt else None)


def _img(r, H, W):
    """rows -> the 4-D channels_last view the wrappers take."""
    return r.view(r.shape[0], H, W, C).permute(0, 3, 1, 2)


def _cell(inp, G, w1=None, w2=None):
    """A ``ResidualCell`` carrying the inputs' filters and (bf16-representable) affine parameters."""
    from fluxmpi_amd.models.deq import ResidualCell
    cell = ResidualCell(C, groups=G).cuda().to(BF).to(memory_format=torch.channels_last)
    with torch.no_grad():
        cell.conv1.weight.copy_(inp["w1"] if w1 is None else w1)
        cell.conv2.weight.copy_(inp["w2"] if w2 is None else w2)
        for k, m in enumerate((cell.n1, cell.n2, cell.n3)):
            m.weight.copy_(inp["gw"][k])
            if inp.get("gb") is not None:
                m.bias.copy_(inp["gb"][k])
    return cell


def _bf16_affine(inp):
    for key in ("gw", "gb"):
        if inp.get(key) is not None:
            inp[key] = [t.to(BF).float() for t in inp[key]]
    return inp


# =============================================================================== GPU: refusals

@gpu
def test_refusals(gpu_ext):
    """``deq_cell_supported`` is false and both launchers raise before any launch; the LDS sizes come from
    the documented formula, not from the extension."""
    ext = gpu_ext
    big = torch.zeros(1024 * 64 + 16, dtype=BF, device="cuda")       # larger than any refused sample
    f = torch.ones(64, device="cuda")
    st = torch.ones(64, device="cuda")
    flt = torch.zeros(64 * 9 * 64, dtype=BF, device="cuda")
    outb = torch.zeros_like(big)
    p = big.data_ptr()

    def fwd(H, W, ch, G, z=p):
        ext.deq_cell_fwd(z, p, flt.data_ptr(), flt.data_ptr(), [0, 0, 0], [0, 0, 0], outb.data_ptr(), 0, 0, [0, 0, 0],
                         [0, 0, 0], [0, 0, 0], 1, H, W, ch, G, EPS, _st(), 0)

    def vjp(H, W, ch, G, u=p):
        ext.deq_cell_vjp(u, [p, p, p], flt.data_ptr(), flt.data_ptr(), [f.data_ptr()] * 3, [st.data_ptr()] * 3,
                         [st.data_ptr()] * 3, outb.data_ptr(), 0, 0, 1, H, W, ch, G, _st())

    refused = [(H, W, 48, 8) for H, W in REFUSED_HW] + [(28, 28, 48, 24), (28, 28, 48, 5), (28, 28, 64, 8)]
    for H, W, ch, G in refused:
        assert not D.supported_ref(H, W, ch, G)
        assert not ext.deq_cell_supported(H, W, ch, G), (H, W, ch, G)
        for call in (fwd, vjp):
            with pytest.raises(RuntimeError, match="deq_cell"):
                call(H, W, ch, G)
    for H, W in ((112, 8), (4, 224)):
        assert D.lds_bytes(H, W) > D.LDS_LIMIT
        for call in (fwd, vjp):
            with pytest.raises(RuntimeError, match="does not fit in LDS"):
                call(H, W, 48, 8)
    for call in (fwd, vjp):
        with pytest.raises(RuntimeError, match="16-byte aligned"):
            call(4, 4, 48, 8, p + 2)
    for H, W in ((8, 112), (7, 128)):
        assert D.lds_bytes(H, W) <= D.LDS_LIMIT and ext.deq_cell_supported(H, W, 48, 8)
    for (_, h, w), G in CASES:
        assert ext.deq_cell_supported(h, w, 48, G)
    torch.cuda.synchronize()
    assert not bool(outb.any())  # nothing ran


# =============================================================================== GPU: forward

@gpu
@pytest.mark.parametrize("shape,G", CASES, ids=CASE_IDS)
def test_fwd(gpu_ext, shape, G):
    n, h, w = shape
    errs = []
    for family, ratio in FWD_FAMILIES:
        if family == "gather" and G not in (1, 8):
            continue  # stage 1 does not depend on G
        tag = f"fwd {family}{ratio} {shape} G{G}"
        inp = D.fwd_inputs(family, n, h, w, ratio=ratio, null_affine=family == "cancel")
        out = _fwd(gpu_ext, tag, inp, n, G, EPS, errs)
        D.check_fwd(tag, inp, out, G, EPS, errs)
        if family == "gather":
            continue
        E.check(f"{tag} out32", out["out32"], out["out"].double(), None, errs)
        slot = _fwd(gpu_ext, f"{tag} slot", inp, n, G, EPS, errs, keep=False, slot=True, o32=False)
        _same(f"{tag} out_slot / keep=False", slot["out"], out["out"], errs)
    _done(errs)


@gpu
def test_fwd_eps_forwarded(gpu_ext):
    """eps = 2^-6: rstd and everything after it follow the eps that was passed (at 1e-5 these bounds fail)."""
    errs = []
    for (n, h, w), G in (((3, 16, 7), 16), ((2, 28, 28), 8)):
        inp = D.fwd_inputs("uniform", n, h, w)
        out = _fwd(gpu_ext, "eps", inp, n, G, EPS_OTHER, errs)
        D.check_fwd(f"fwd eps {h}x{w}", inp, out, G, EPS_OTHER, errs)
        wrong = []
        D.check_fwd("wrong eps", inp, out, G, EPS, wrong)
        assert wrong, "the checker cannot tell eps = 2^-6 from 1e-5"
    _done(errs)


@gpu
@pytest.mark.parametrize("shape,G", [((3, 16, 7), 16), ((3, 12, 12), 8), ((2, 28, 28), 8)], ids=["16x7", "12x12", "28x28"])
def test_fwd_variants(gpu_ext, shape, G):
    """Null w / b equal ones / zeros, two launches are bit-identical, ``cell_forward`` equals the raw call."""
    from fluxmpi_amd.ops import deq_cell
    n, h, w = shape
    errs = []
    inp = _bf16_affine(D.fwd_inputs("uniform", n, h, w))
    a = _fwd(gpu_ext, "a", inp, n, G, EPS, errs)
    b = _fwd(gpu_ext, "b", inp, n, G, EPS, errs)
    null = dict(inp, gw=[None] * 3, gb=[None] * 3)
    ones = dict(inp, gw=[torch.ones(C)] * 3, gb=[torch.zeros(C)] * 3)
    c, d = _fwd(gpu_ext, "null", null, n, G, EPS, errs), _fwd(gpu_ext, "ones", ones, n, G, EPS, errs)
    D.check_fwd("fwd null affine", null, c, G, EPS, errs)
    for key in ("out", "out32"):
        _same(f"two launches {key}", a[key], b[key], errs)
        _same(f"null affine {key}", c[key], d[key], errs)
    for key in ("h", "mean", "rstd"):
        for k in range(3):
            _same(f"two launches {key}{k + 1}", a[key][k], b[key][k], errs)
            _same(f"null affine {key}{k + 1}", c[key][k], d[key][k], errs)
    cell = _cell(inp, G)
    z4, x4 = _img(inp["z"].cuda(), h, w), _img(inp["x"].cuda(), h, w)
    assert deq_cell.supported(cell, z4)
    o4, state = deq_cell.cell_forward(cell, z4, x4, keep=True)
    r = lambda t: t.permute(0, 2, 3, 1).reshape(n, h * w, C).cpu()
    _same("cell_forward out", r(o4), a["out"], errs)
    for k in range(3):
        hk, mk, rk, wk = state[1 + k]
        _same(f"cell_forward h{k + 1}", r(hk), a["h"][k], errs)
        _same(f"cell_forward mean{k + 1}", mk.cpu(), a["mean"][k], errs)
        _same(f"cell_forward rstd{k + 1}", rk.cpu(), a["rstd"][k], errs)
        _same(f"cell_forward w{k + 1}", wk.cpu(), inp["gw"][k], errs)
    o2, _ = cell.forward_state(z4, x4)
    _same("forward_state out", r(o2), a["out"], errs)
    _done(errs)


# =============================================================================== GPU: VJP

@gpu
@pytest.mark.parametrize("shape,G", CASES, ids=CASE_IDS)
def test_vjp(gpu_ext, shape, G):
    n, h, w = shape
    errs = []
    for family, ratio in VJP_FAMILIES:
        tag = f"vjp {family}{ratio} {shape} G{G}"
        inp = D.vjp_inputs(family, n, h, w, G, ratio=ratio)
        got, _ = _vjp(gpu_ext, tag, inp, n, G, errs)
        D.check_vjp(tag, inp, got, G, errs)
    # stage isolation: a zero W1 makes the output d3 exactly (``gn_check_bwd`` directly); centre-tap identity
    # filters make both convolutions exact, so the bound is a few bf16 roundings
    inp = D.vjp_inputs("uniform", n, h, w, G, filt="zero_w1")
    got, _ = _vjp(gpu_ext, "zero_w1", inp, n, G, errs)
    NE.gn_check_bwd(f"vjp d3 {shape} G{G}", inp["u"], inp["h"][2], inp["mean"][2], inp["rstd"][2], inp["gw"][2], G, True,
                    dict(dh=got), BF, errs, Lpx=D.L_PX)
    inp = D.vjp_inputs("uniform", n, h, w, G, filt="identity")
    got, _ = _vjp(gpu_ext, "identity", inp, n, G, errs)
    D.check_vjp(f"vjp identity {shape} G{G}", inp, got, G, errs)
    _done(errs)


@gpu
@pytest.mark.parametrize("shape,G", EXACT_CASES, ids=EXACT_IDS)
def test_vjp_exact(gpu_ext, shape, G):
    """The integer case: u_new EQUALS the float64 chain and ss_part[n] the integer sum (u_new - u)^2."""
    n, h, w = shape
    errs = []
    for seed in EXACT_SEEDS:
        inp = D.vjp_exact_inputs(n, h, w, G, seed, with_grad=seed != 1)
        ref, ss = D.vjp_exact_asserts(inp, G)
        got, part = _vjp(gpu_ext, f"exact seed{seed}", inp, n, G, errs)
        E.check(f"vjp exact {shape} G{G} seed{seed}", got, ref, None, errs)
        if ss is not None:
            E.check(f"vjp exact ss_part {shape} G{G} seed{seed}", part, ss, None, errs)
    _done(errs)


@gpu
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_adjoint_check_exact(gpu_ext, n):
    """Integer partials: the total is EQUAL, the flag is 1 at thresh2 == ss and 0 one float32 below."""
    from fluxmpi_amd.ops import deq_cell
    g = E._gen("adjoint_check", n)
    part = torch.randint(0, 4000, (n,), generator=g).float()
    total = float(part.double().sum())
    assert total < 2 ** 24
    flag = torch.full((1,), -1.0, device="cuda")
    ss = deq_cell.adjoint_check(part.cuda(), torch.tensor(total, device="cuda"), flag)
    assert float(ss) == total and float(flag) == 1.0
    below = torch.nextafter(torch.tensor(total), torch.tensor(0.0))
    ss = deq_cell.adjoint_check(part.cuda(), below.cuda(), flag)
    assert float(ss) == total and float(flag) == 0.0 and float(below) < total


def _state4(inp, h, w):
    """The wrappers' state tuple on the GPU from a helper state."""
    n = inp["u"].shape[0]
    hs, gw, mean, rstd = _cuda(inp["h"]), _cuda(inp["gw"]), _cuda(inp["mean"]), _cuda(inp["rstd"])
    return ((n, C, h, w),) + tuple((_img(hs[k], h, w), mean[k], rstd[k], gw[k]) for k in range(3))


@gpu
@pytest.mark.parametrize("shape,G", [((3, 16, 7), 16), ((2, 28, 28), 8)], ids=["16x7", "28x28"])
def test_vjp_wrappers(gpu_ext, shape, G):
    """``cell_vjp`` and ``ResidualCell.adjoint_step`` equal the raw call bit for bit (``filter_t``'s flipped
    layout); two launches are bit-identical."""
    from fluxmpi_amd.ops import deq_cell
    n, h, w = shape
    errs = []
    inp = D.vjp_inputs("uniform", n, h, w, G)
    g = E._gen("wrappers", n, h, w)
    inp_g = dict(inp, grad=NE._uni(g, (n, h * w, C), -1, 1).to(BF))
    a, _ = _vjp(gpu_ext, "a", inp, n, G, errs)
    b, _ = _vjp(gpu_ext, "b", inp, n, G, errs)
    _same("two launches", a, b, errs)
    ag, part = _vjp(gpu_ext, "grad", inp_g, n, G, errs)
    cell = _cell(inp, G)
    state = _state4(inp, h, w)
    u4, g4 = _img(inp["u"].cuda(), h, w), _img(inp_g["grad"].cuda(), h, w)
    assert deq_cell.supported(cell, u4)
    r = lambda t: t.permute(0, 2, 3, 1).reshape(n, h * w, C).cpu()
    _same("cell_vjp", r(deq_cell.cell_vjp(cell, state, u4)), a, errs)
    _same("ResidualCell.vjp", r(cell.vjp(state, u4)), a, errs)
    flag = torch.full((1,), -1.0, device="cuda")
    un, ss = cell.adjoint_step(state, u4, g4, torch.tensor(1e30, device="cuda"), flag)
    _same("adjoint_step u_new", r(un), ag, errs)
    ref_ss = ((ag.double() - inp["u"].double()) ** 2).sum((1, 2))
    E.check("ss_part", part, ref_ss, (h * w * C + 20) * E.E23 * ref_ss + E.TINY, errs)
    assert float(flag) == 1.0 and abs(float(ss) - float(part.double().sum())) <= n * E.E23 * float(part.double().sum())
    _done(errs)


@gpu
def test_vjp_state_from_forward(gpu_ext, monkeypatch):
    """A state from the fused forward and the same state from the unfused 5-launch forward both satisfy the
    VJP's bounds."""
    from fluxmpi_amd.ops import deq_cell
    n, h, w, G = 2, 28, 28, 8
    errs = []
    fi = _bf16_affine(D.fwd_inputs("uniform", n, h, w))
    cell = _cell(fi, G)
    z4, x4 = _img(fi["z"].cuda(), h, w), _img(fi["x"].cuda(), h, w)
    u = D.vjp_inputs("uniform", n, h, w, G)["u"]
    r = lambda t: t.permute(0, 2, 3, 1).reshape(n, h * w, C).cpu()
    for fused in (True, False):
        monkeypatch.setattr(deq_cell, "ENABLED", fused)
        if not fused:
            assert cell.manual_ok(z4)
        _, state = cell.forward_state(z4, x4)
        monkeypatch.setattr(deq_cell, "ENABLED", True)
        inp = dict(family="uniform", H=h, W=w, u=u, grad=None, t2t=E.taps_t(fi["w2"]).contiguous(),
                   t1t=E.taps_t(fi["w1"]).contiguous(), h=[r(state[1 + k][0]) for k in range(3)],
                   mean=[state[1 + k][1].cpu() for k in range(3)], rstd=[state[1 + k][2].cpu() for k in range(3)],
                   gw=[state[1 + k][3].cpu() for k in range(3)])
        got, _ = _vjp(gpu_ext, f"state fused={fused}", inp, n, G, errs)
        D.check_vjp(f"vjp state fused={fused}", inp, got, G, errs)
        _same(f"cell_vjp fused={fused}", r(deq_cell.cell_vjp(cell, state, _img(u.cuda(), h, w))), got, errs)
    _done(errs)


@gpu
def test_vjp_refuses_aliased_out(gpu_ext):
    """``out`` parks d3 while grad and h1 .. h3 are still to be read: the launcher raises on any overlap."""
    n, h, w, G = 3, 8, 8, 8
    inp = D.vjp_inputs("uniform", n, h, w, G)
    u, t2t, t1t = _cuda([inp["u"], inp["t2t"], inp["t1t"]])
    grad = torch.zeros_like(u)
    part = torch.zeros(n, device="cuda")
    hs, gw, mean, rstd = _cuda(inp["h"]), _cuda(inp["gw"]), _cuda(inp["mean"]), _cuda(inp["rstd"])
    keep = [t.clone() for t in hs + [grad, u]]

    def call(out_ptr):
        gpu_ext.deq_cell_vjp(u.data_ptr(), [t.data_ptr() for t in hs], t2t.data_ptr(), t1t.data_ptr(),
                             [t.data_ptr() for t in gw], [t.data_ptr() for t in mean], [t.data_ptr() for t in rstd],
                             out_ptr, grad.data_ptr(), part.data_ptr(), n, h, w, C, G, _st())

    for t in [u, grad] + hs:
        with pytest.raises(RuntimeError, match="alias"):
            call(t.data_ptr())
    with pytest.raises(RuntimeError, match="alias"):
        call(hs[1].data_ptr() + 16 * C * 2)  # a partial overlap
    torch.cuda.synchronize()
    for a, b in zip(hs + [grad, u], keep):
        assert torch.equal(_bits(a), _bits(b))


@gpu
def test_cell_vjp_fresh_out_when_aliased(gpu_ext):
    """``cell_vjp`` writes a fresh tensor when the offered ``out`` is u, grad or a state tensor."""
    from fluxmpi_amd.ops import deq_cell
    n, h, w, G = 3, 8, 8, 8
    errs = []
    inp = D.vjp_inputs("uniform", n, h, w, G)
    cell = _cell(inp, G)
    state = _state4(inp, h, w)
    u4 = _img(inp["u"].cuda(), h, w)
    g4 = _img(NE._uni(E._gen("fresh"), (n, h * w, C), -1, 1).to(BF).cuda(), h, w)
    good = torch.empty_like(u4)
    ref, ref_part = deq_cell.cell_vjp(cell, state, u4, grad=g4, out=good)
    assert ref.data_ptr() == good.data_ptr()
    for name, t in [("u", u4), ("grad", g4)] + [(f"h{k + 1}", state[1 + k][0]) for k in range(3)]:
        before = t.clone()
        o, part = deq_cell.cell_vjp(cell, state, u4, grad=g4, out=t)
        assert o.data_ptr() != t.data_ptr(), name
        _same(f"out={name}: operand unchanged", t, before, errs)
        _same(f"out={name}: result", o, ref, errs)
        _same(f"out={name}: ss_part", part, ref_part, errs)
    _done(errs)
