"""The two front-end kernels (stem.hip: the ResNet-50 7x7/2 convolution with its BatchNorm statistics and the
one-pass stem backward; conv_c3.hip: the CIFAR DEQ stem's 3-channel 3x3 forward and filter gradient) per
element against float64 references: derived componentwise bounds, exact integer / one-hot families, guard
bands around every output, the persistent loops at the trip counts training runs them at, and a CPU half
that shows the bounds are reachable and that planted defects trip the same checker. Inputs, references and
emulations live in ``stem_edges``; ``bound``, ``check``, ``check_out``, ``check_colsums``, the guard bands,
``patterns`` and ``rn_bf16`` are ``mfma_edges``'.

Assumptions, as in test_mfma_edges_gpu.py: a product of two bf16 values is exact in fp32; every fp32 addition
or fma (MFMA, fdot2, plain code) errs by at most 2^-23 relatively, in any order; u = 2^-8 is bf16's unit
roundoff; 1e-30 is added to every bound and nothing else. No kernel needed a wider constant.

stem_fwd   y = bf16(conv7x7/2(x, w)) and the statistics shards [64][2][64]
    reference   float64 on the bf16 operands through the packed-K im2col of the kernel header: A [pixels, 256]
                by ``ops.stem.emulate_conv``'s gather lifted to float64 (``stem_edges.im2col``), W' [64, 256] with
                NATURAL channel rows (``pack_nat``; the kernel's operand is ``pack_filter``, rows permuted, so the
                permutation and the packing are under test), R = A W'^T, |A| |W'|^T
    y           |y - R| <= u |R| + 256 2^-23 (|A| |W'|^T)            (Kred = 256 packed k)
    shards      summed in float64, against float64 sums of the kernel's OWN stored y and y^2:
                rows 2^-23 sum |y| and rows 2^-23 sum y^2, rows = 12544 n
    families    uniform (filter scaled by 147^-0.5); cancel (channels 0 / 1 opposite up to 2^-6 under equal
                weights: |R| << A); ternary (x, w in {-1, 0, 1}, 96 non-zero taps per filter: |y| <= 96 <= 256 and
                sum y^2 < 2^24 per channel, both asserted; y and both statistics EQUAL the reference); gather
                (three launches; in launch j channel co holds a single 1.0 at flat (ci, ky, kx) tap 64 j + co, none
                from 147 on; x = distinct finite normal bf16 bit patterns; y[n, oy, ox, co] must equal
                x[n, ci, 2 oy + ky - 3, 2 ox + kx - 3], exact zeros outside: all 147 taps, every border of every
                row group; the CPU half shows the reference IS that closed form)
    guards      y inside a sentinel buffer (NaN inside, guard rows on both sides), the shards between guard bands
    max_blocks  (the one source change: a host-side cap of the persistent grid, 0 = the resident workgroups)
                (n, max_blocks) = (1, 0) 14 workgroups of one row group; (1, 1) one workgroup walks all 14, both
                halo buffers reused six times; (1, 4) 4, 4, 4, 2 groups; (2, 3) 10 groups per workgroup, the
                walk crosses from image 0 to image 1; (2, 5) 6, 6, 6, 6, 4; (3, 0) the default grid. The number
                of workgroups is asserted from the non-zero shards. Every family runs the first three, uniform
                and ternary all six. max_blocks < 0 raises.
    pad_c3_to_c4  bit-equal channels 0 .. 2 and a zero channel 3, bf16 and fp16, 35 pixels
    pack_filter   composed with the row permutation it puts each real tap exactly once: implied by the gather
                family (every tap comes out of exactly the channel that holds it, in natural channel order)

stem_bwd   the raw binding on synthetic operands (c, dp, idx, mean, inv, w fed directly, so idx covers what a
           real pool rarely produces)
    reference   dz[n, oy, ox, ch] = sum of dp[n, py, px, ch] over the pooled windows covering the pixel whose idx
                equals (oy - 2 py + 1) * 3 + (ox - 2 px + 1) (0xFF selects nothing; positions outside the image are
                never generated), as one float64 scatter. |dp| in [2^-4, 1] or small integers: a sum of at most
                four terms is exact in fp32 (asserted: the fp32 scatter equals the float64 one), so rn_bf16(dz) is
                the kernel's dz bit for bit. G1 = A^T rn_bf16(dz), G2 = A^T c, G3 = colsum(A) over all 256 packed
                k (the pseudo-taps and channel 3, which holds data here, included), sdz = sum dz,
                sdzx = sum dz (c inv - mean inv).
    1 part      summed over blocks in float64: pixels 2^-23 (|.|^T |A|) + 2^-24 |R|, pixels = 12544 n
    2 db_bn     pixels 2^-23 sum |dz|
      dw_bn     xhat = fma(c, inv, fl(-mean inv)) carries two roundings, each at most 2^-23 (|c inv| + |mean inv|);
                the sum of fma(dz, xhat, .) over the pixels then errs by pixels 2^-23 sum |dz xhat|:
                pixels 2^-23 sum |dz xhat| + 2 2^-23 sum |dz| (|c inv| + |mean inv|)
    3 dwp       against sc g1 + cb g2 + cd g3 in float64 on the kernel's OWN part, dw_bn, db_bn (sc = w inv,
                k2 = db_bn / pixels, k3 = dw_bn / pixels, cb = -sc inv k3, cd = sc (mean inv k3 - k2)). Roundings:
                sc 1; 1 / pixels 1; k2, k3 2 each; cb 5; cd 7 relative to cdm = |sc| (|mean inv k3| + |k2|) >= |cd|
                (its two terms may cancel); cd g3 1; two fmas 2: at most 10 on any term. The fp32 sum of the
                blocks' partials: blocks 2^-23 sum_b |part_b|.
                10 2^-23 (|sc g1| + |cb g2| + cdm |g3|) + blocks 2^-23 (|sc| sum_b |p1| + |cb| sum_b |p2| + cdm sum_b |p3|)
    4 dW        unpack_grad(dwp) against the filter gradient of the float64 dC = sc (rn_bf16(dz) - xhat k3 - k2),
                k2, k3 from the unrounded dz (evaluated as sc G1 + cb G2 + cd G3 with the float64 coefficients; the
                CPU half shows that this is conv2d_weight(x, dC)). The three terms' bounds added, in term
                magnitudes (with the batch's own statistics R itself cancels):
                |sc| B(G1) + |cb| B(G2) + cdm B(G3)                                      check 1's bounds
                + |sc inv| (B(dw_bn) / pixels) |G2| + |sc| (|mean inv| B(dw_bn) + B(db_bn)) / pixels |G3|    check 2's
                + 10 2^-23 (|sc G1| + |cb G2| + cdm |G3|) + blocks 2^-23 (|sc| A1 + |cb| A2 + cdm A3)        check 3's
    5 .. 7      the BatchNorm workspace all zero after every call, inside guard bands; part pre-filled with NaN, none
                left in blocks * stem_part_floats() floats, guards intact; dwp, dw_bn, db_bn pre-filled with NaN
    families    uniform (mean / inv the batch's own statistics of c at n = 1, arbitrary at n = 2, 3)
                integer (x, c, dp in {-2 .. 2}, idx uniform over {0 .. 8, 0xFF}, mean 0, inv 1, w 1: every sum an
                    integer below 2^24, asserted; summed G1, G2, G3, db_bn, dw_bn EQUAL at every grid)
                overlap (idx = (8, 6, 2, 0)[(py & 1) * 2 + (px & 1)]: every conv pixel (odd, odd) with py, px even is
                    chosen by all four of its windows, all four visits fire; integers, exact)
                blocked (idx all 0xFF: G1, db_bn, dw_bn exactly zero, G2 and G3 as ever)
                gather (idx 0xFF but one (window, position) per channel with dp = 1: G1[:, ch] EQUALS the 256-entry
                    im2col row of that channel's pixel, bit patterns of x and zeros (4096 distinct ones, exponents
                    2^-7 .. 2^8: G2 and G3 sum the operand over all pixels, which the full exponent range of
                    ``patterns`` would overflow in fp32, in the kernel as anywhere); db_bn = 1; the 64 pixels of
                    ``stem_edges.gather_pixels``: corners, edge mid-points, ox = 111 (two_w false) and 109, pooled
                    row 55, both rows and parities of several row pairs, either window of an odd coordinate)
                w = null equals w = ones bit for bit
    grids       (n, blocks) = (1, 1) 56 row pairs in one workgroup; (1, 5) 12, 12, 12, 12, 8; (1, 56) one each;
                (1, 40) two each, blocks 28 .. 39 idle and still writing zero partials; (2, 3) 38 each, the image
                boundary inside block 1; (3, stem_bwd_blocks(3)). integer and uniform at all, the rest at the
                first two. blocks = 0 and blocks > stem_bwd_blocks(n) raise.

conv_c3.hip   raw conv_c3_fwd / conv_c3_wgrad and ops.conv_small.conv3x3_small
    reference   R = P Q^T, P = plain slices of the zero-padded image with columns in (kh, kw, ci) order
    forward     u |R| + 28 2^-23 A      (14 fdot2 of two products each)
    gradient    the [blocks][Cout][27] fp32 partials summed in float64: pixels 2^-23 A + 2^-24 |R|; through
                conv3x3_small(...).backward one more u |R| for the bf16 store
    families    uniform, cancel, ternary (EQUAL), gather (forward: channel co holds a 1.0 at tap co mod 27; gradient:
                dy one-hot per channel at pixel 0, 1, the last two, and both sides of every 256 / 512 boundary, so
                dW[co] equals that pixel's window of bit patterns)
    shapes      (N, H, W, stride, Cout): (1, 1, 1, 1, 128) one pixel; (1, 2, 2, 2, 128) one pixel at stride 2;
                (3, 7, 9, 1, 256) 189 pixels, odd, pairs straddling rows and images; (1, 16, 16, 1, 128) 256 exactly;
                (1, 1, 257, 1, 128) H = 1; (1, 257, 1, 1, 128) W = 1; (2, 16, 16, 1, 128) 512 exactly;
                (1, 19, 27, 1, 128) 513: the last gradient workgroup holds one pixel; (5, 17, 13, 2, 384) stride 2,
                odd, three column blocks; (2, 8, 6, 2, 128) stride 2, even
    guards      y and part NaN-filled inside guard bands; stride 3, Cout 64 and Cout 192 raise from both entries

CPU half: the float64 im2col references equal F.conv2d / conv2d_weight; a float32 evaluation of each kernel's
formulas (sequential over the reduction; per-block partials, then the combine) meets every bound and
reproduces the exact families; each planted defect trips the checker (a tap shifted by one; a border tap not
zeroed; the second window column dropped at pooled column 55 / at all columns; a stale stage; a halo row off
by one in the second conv row of a pair; G3 from half the k-steps; an idle block's partial unwritten; cd
with the wrong sign; conv_c3: the unpaired last pixel counted twice, k-pair 13's high half not zero, i.e.
repeating k = 26 on both sides; and ``mfma_edges.defect``'s missing k-tile, transposed fragment and truncation
on the forward's GEMM).

Measured on the MI355X (one run of the whole suite), worst |err| / bound per kernel:
    stem_fwd        y 0.973 (uniform, n = 2, max_blocks = 3); shards: sum 2.0e-6, sum of squares 1.4e-4
    stem_bwd part   G1 5.4e-5, G2 9.5e-4, G3 5.5e-4
    BN sums         db_bn 0 (these dz are multiples of 2^-11 and their sums stay below 2^13: exact in any order),
                    dw_bn 4.0e-4
    combine         dwp against its own partials 0.19; dW against the float64 filter gradient 0.026
    conv_c3         forward 0.994 raw / 0.995 through conv3x3_small; filter gradient partials 0.018, through the
                    wrapper's bf16 store 0.988
A ratio just under 1 is what a correctly rounded bf16 store gives (u |R| dominates those bounds); the fp32 sums
sit far below 1 because their bounds grow with the number of additions (12544 n pixels) while fp32 rounding
errors largely cancel. Every exact family came out equal at every grid; no guard element was touched; no
kernel needed a constant wider than 2^-23, and no defect was found. Wall time: the 63 GPU tests of this file
4.2 s, next to 126 s for the rest of the GPU suite (130.0 s together); the 17 CPU tests take 15 s without a GPU.
"""
import pytest
import torch
import torch.nn.functional as F

from . import mfma_edges as E
from . import stem_edges as T

gpu = pytest.mark.gpu
_CACHE = {}


def _done(errs):
    assert not errs, "\n".join(errs[:20]) + (f"\n... and {len(errs) - 20} more" if len(errs) > 20 else "")


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _fwd_case(family, n, launch=0):
    """(x4, w, R, A) of one forward input set, shared by every max_blocks."""
    def make():
        x, w = T.fwd_inputs(family, n, launch)
        x4 = T.to_x4(x)
        return (x4, w) + T.fwd_reference(x4, w)
    return _cached(("fwd", family, n, launch), make)


def _bwd_case(family, n):
    def make():
        inp = T.bwd_inputs(family, n)
        return inp, T.bwd_reference(inp)
    return _cached(("bwd", family, n), make)


def _fwd_families(case):
    return T.FWD_FAMILIES if case in T.FWD_CASES[:3] else ("uniform", "ternary")


# ============================================================================ CPU half

def test_packed_layout_matches_ops_cpu():
    """``stem_edges``' k decomposition is ``ops.stem``'s: the same real taps, and im2col / pack_nat reproduce
    emulate_conv (the definition of A) to float32 accuracy."""
    from fluxmpi_amd.ops import stem as S
    dy, dx, c = T.k_offsets()
    real = T.real_taps()
    for k in range(T.KK):
        t = S._k_tap(k)
        want = t if (t is not None and t[0] < 3) else None
        got = (int(c[k]), int(dy[k]) + 3, int(dx[k]) + 3) if bool(real[k]) else None
        assert got == want, k
    assert int(real.sum()) == 147
    x4, w, r, _ = _fwd_case("uniform", 1)
    emu = S.emulate_conv(x4[..., :3].permute(0, 3, 1, 2), w)  # [1, 64, 112, 112] fp32
    assert float((emu.permute(0, 2, 3, 1).reshape(-1, 64).double() - r).abs().max()) < 1e-4


def test_references_equal_torch_cpu():
    """The float64 im2col references equal F.conv2d (stride 2, padding 3, 224 x 224) and conv2d_weight of the
    float64 dC, and conv_c3's equal F.conv2d / conv2d_weight at every shape."""
    x4, w, r, _ = _fwd_case("uniform", 1)
    x = x4[..., :3].permute(0, 3, 1, 2).double()
    want = F.conv2d(x, w.double(), stride=2, padding=3).permute(0, 2, 3, 1).reshape(-1, 64)
    assert float((r - want).abs().max()) < 1e-12
    for stats in (True, False):
        inp = T.bwd_inputs("uniform", 1, true_stats=stats)
        ref = T.bwd_reference(inp)
        sc, cb, cd, _ = T.coefficients(inp["w"], inp["mean"], inp["inv"], ref["sdzx"], ref["sdz"], ref["pix"])
        packed = (sc * ref["G1"] + cb * ref["G2"] + cd * ref["G3"].view(-1, 1)).t().contiguous()
        iv, m = inp["inv"].double(), inp["mean"].double()
        xhat = inp["c"].double().view(-1, 64) * iv - m * iv
        dC = sc * (ref["dzb"] - xhat * (ref["sdzx"] / ref["pix"]) - ref["sdz"] / ref["pix"])
        dC = dC.view(1, 112, 112, 64).permute(0, 3, 1, 2)
        x3 = inp["x4"][..., :3].permute(0, 3, 1, 2).double()
        dw = torch.nn.grad.conv2d_weight(x3, (64, 3, 7, 7), dC, stride=2, padding=3)
        scale = float(dw.abs().max())
        assert float((T.unpack_nat(packed) - dw).abs().max()) < 1e-11 * max(scale, 1.0), stats
        if stats:  # the batch's own statistics: sum dC = sum dC xhat = 0 up to the bf16 rounding of dz
            assert float(dC.sum((0, 2, 3)).abs().max()) < 1e-2 * float(dC.abs().sum((0, 2, 3)).max())
    for n, h, wd, s, co in T.C3_SHAPES:
        x, wt = T.c3_fwd_inputs("uniform", n, h, wd, s, co)
        _, _, r, _ = T.c3_fwd_reference(x, wt, s)
        want = F.conv2d(x.double(), wt.double(), stride=s, padding=1)
        assert float((r - T.c3_rows(want)).abs().max()) < 1e-12
        x, dy = T.c3_wgrad_inputs("uniform", n, h, wd, s, co)
        r, _ = T.c3_wgrad_reference(x, dy, s)
        want = torch.nn.grad.conv2d_weight(x.double(), (co, 3, 3, 3), dy.double(), stride=s, padding=1)
        assert float((r - E.taps(want)).abs().max()) < 1e-10


def test_gather_closed_forms_cpu():
    """The gather families' references ARE the closed forms. Forward: launch j, channel co = tap 64 j + co:
    y[n, oy, ox, co] = x[n, ci, 2 oy + ky - 3, 2 ox + kx - 3], zero outside (all 147 taps). Backward:
    G1[:, ch] = the im2col row of channel ch's pixel, db_bn's reference = 1."""
    seen = set()
    for j in range(3):
        x4, w, r, _ = _fwd_case("gather", 1, j)
        xp = F.pad(x4[0, :, :, :3].double().permute(2, 0, 1), (3, 3, 3, 3))
        r = r.view(112, 112, 64)
        for co in range(64):
            t = 64 * j + co
            if t >= 147:
                assert not bool(r[..., co].any())
                continue
            ci, ky, kx = t // 49, (t % 49) // 7, t % 7
            assert torch.equal(r[..., co], xp[ci, ky:ky + 223:2, kx:kx + 223:2]), (j, co)
            seen.add(t)
    assert len(seen) == 147
    for n in (1, 2):
        inp = T.bwd_inputs("gather", n)
        ref = T.bwd_reference(inp)
        rows = ref["arow"].view(n, 112, 112, 256)
        px = T.gather_pixels()
        assert len(set(px)) == 64
        for must in [(0, 0), (0, 111), (111, 0), (111, 111), (0, 56), (56, 0), (111, 56), (56, 111)]:
            assert must in px
        assert any(ox == 111 for _, ox in px) and any(oy >= 109 for oy, _ in px)
        for ch, (oy, ox) in enumerate(px):
            assert torch.equal(ref["G1"][:, ch], rows[ch % n, oy, ox]), ch
        assert torch.equal(ref["sdz"], torch.ones(64, dtype=torch.float64))


@pytest.mark.parametrize("family", T.FWD_FAMILIES)
def test_fwd_emulation_meets_bounds_cpu(family):
    errs = []
    cases = [(1, 0), (1, 1), (1, 4)] + ([(2, 3)] if family in ("uniform", "ternary") else [])
    for n, mb in cases:
        for launch in (range(3) if family == "gather" else (0,)):
            if family == "gather" and mb != 1:
                continue  # y does not depend on the grid in the emulation: one launch set suffices
            x4, w, r, a = _fwd_case(family, n, launch)
            y, shards = T.fwd_emulate(x4, w, mb)
            if family == "ternary":
                assert float(r.abs().max()) <= 256
            T.fwd_check(f"cpu fwd {family} n{n} mb{mb} l{launch}", family, y, shards, r, a, errs)
    _done(errs)


@pytest.mark.parametrize("family", T.BWD_FAMILIES)
def test_bwd_emulation_meets_bounds_cpu(family):
    errs = []
    grids = [(1, 5), (1, 40)] + ([(2, 3)] if family in ("uniform", "integer") else [])
    for n, blocks in grids:
        inp, ref = _bwd_case(family, n)
        out = T.bwd_emulate(inp, blocks)
        T.bwd_check(f"cpu bwd {family} n{n} b{blocks}", family, inp, ref, out, blocks, errs)
    if family == "uniform":  # w = null is w = ones
        inp, ref = _bwd_case(family, 1)
        a = T.bwd_emulate(dict(inp, w=None), 5)["dwp"]
        b = T.bwd_emulate(dict(inp, w=torch.ones(64)), 5)["dwp"]
        assert torch.equal(a, b)
    _done(errs)


def test_planted_defects_fail_cpu():
    """Each planted defect makes the checker that passes the clean emulation fail, one assertion each."""
    dy, dx, c = T.k_offsets()
    k_in = int(torch.nonzero(T.real_taps() & (dx == 0) & (dy == 0))[0])   # an interior real tap
    k_left = int(torch.nonzero(T.real_taps() & (dx == -3) & (dy == 0))[0])  # a tap that leaves the image at ox = 0, 1
    for family in ("uniform", "gather"):
        launches = range(3) if family == "gather" else (0,)
        for kw in (dict(shift_k=k_in), dict(raw_border_k=k_left)):
            tripped = []
            for launch in launches:
                x4, w, r, a = _fwd_case(family, 1, launch)
                y = E.rn_bf16(T.im2col(x4, torch.float32, **kw) @ T.pack_nat(w, torch.float32).t())
                T.fwd_check("d", family, y, None, r, a, tripped)
            assert tripped, f"forward {family}: planted defect {kw} passed the checker"
            print(tripped[0])
    x4, w, r, a = _fwd_case("uniform", 1)  # mfma_edges' GEMM defects on the forward's A W'^T
    p, q = T.im2col(x4, torch.float32), T.pack_nat(w, torch.float32)
    for kind in ("missing_ktile", "transposed_fragment", "truncation"):
        errs = []
        E.check_out(kind, "uniform", E.defect(kind, p @ q.t(), p, q), r, a, T.KK, "bf16", errs)
        assert errs, f"forward: planted defect {kind} passed the checker"
    for family in ("uniform", "integer"):
        inp, ref = _bwd_case(family, 1)
        for kind in T.BWD_DEFECTS:
            blocks = 40 if kind == "idle_unwritten" else 5
            errs = []
            T.bwd_check("d", family, inp, ref, T.bwd_emulate(inp, blocks, kind), blocks, errs)
            assert errs, f"backward {family}: planted defect {kind} passed the checker"
            print(kind, errs[0])
    n, h, wd, s, co = T.C3_SHAPES[2]  # 189 pixels: the last one is unpaired
    for family in ("uniform", "ternary"):
        x, dy_ = T.c3_wgrad_inputs(family, n, h, wd, s, co)
        r, a = T.c3_wgrad_reference(x, dy_, s)
        errs = []
        T.c3_check_wgrad("d", family, T.c3_wgrad_emulate(x, dy_, s, "last_twice").double().sum(0), r, a, 189, errs)
        assert errs, f"conv_c3 {family}: the unpaired last pixel counted twice passed the checker"
        x, wt = T.c3_fwd_inputs(family, n, h, wd, s, co)
        _, _, r, a = T.c3_fwd_reference(x, wt, s)
        errs = []
        E.check_out("d", family, T.c3_fwd_emulate(x, wt, s, "pair13"), r, a, 28, "bf16", errs)
        assert errs, f"conv_c3 {family}: a non-zero high half of k-pair 13 passed the checker"


@pytest.mark.parametrize("family", E.FAMILIES)
def test_conv_c3_emulation_meets_bounds_cpu(family):
    errs = []
    for n, h, wd, s, co in T.C3_SHAPES:
        tag = f"cpu c3 {family} {(n, h, wd, s, co)}"
        x, wt = T.c3_fwd_inputs(family, n, h, wd, s, co)
        _, _, r, a = T.c3_fwd_reference(x, wt, s)
        E.check_out(tag + " fwd", family, T.c3_fwd_emulate(x, wt, s), r, a, 28, "bf16", errs)
        x, dy = T.c3_wgrad_inputs(family, n, h, wd, s, co)
        r, a = T.c3_wgrad_reference(x, dy, s)
        part = T.c3_wgrad_emulate(x, dy, s)
        px = dy.numel() // co
        T.c3_check_wgrad(tag + " wgrad", family, part.double().sum(0), r, a, px, errs)
        T.c3_check_wgrad(tag + " wgrad bf16", family, E.rn_bf16(part.sum(0)), r, a, px, errs, bf16_store=True)
        if family == "gather":  # dW[co] is the chosen pixel's window
            sel = T.c3_gather_pixels(px)
            win = E.im2col(x, s).double()
            assert {0, px - 1} <= set(sel) and all(b in sel for b in (255, 256, 511, 512) if b < px)
            for o in range(co):
                assert torch.equal(r[o], win[sel[o % len(sel)]]), o
    _done(errs)


# ============================================================================ GPU: stem_fwd

def _stream():
    return torch.cuda.current_stream().cuda_stream


def _run_stem_fwd(ext, tag, x4, w, n, max_blocks, errs):
    from fluxmpi_amd.ops import stem as S
    xd, wp = x4.cuda(), S.pack_filter(w.cuda())
    ybuf, y = E.guarded(n * T.PIX, 64, 64, torch.bfloat16, "cuda")
    sbuf, st = E.guarded(128, 64, 64, torch.float32, "cuda", fill=0.0)
    ext.stem_fwd(xd.data_ptr(), wp.data_ptr(), y.data_ptr(), st.data_ptr(), n, _stream(), max_blocks)
    torch.cuda.synchronize()
    return (E.take_guarded(tag + " y", ybuf, y, errs).cpu(),
            E.take_guarded(tag + " stats", sbuf, st, errs).view(64, 2, 64).cpu())


FWD_PARAMS = [(f, c) for c in T.FWD_CASES for f in _fwd_families(c)]


@gpu
@pytest.mark.parametrize("family,case", FWD_PARAMS, ids=[f"{f}-n{c[0]}-mb{c[1]}" for f, c in FWD_PARAMS])
def test_stem_fwd(gpu_ext, family, case):
    n, mb = case
    errs = []
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for launch in (range(3) if family == "gather" else (0,)):
        x4, w, r, a = _fwd_case(family, n, launch)
        if family == "ternary":
            assert float(r.abs().max()) <= 256
        tag = f"fwd {family} n{n} mb{mb} l{launch}"
        y, shards = _run_stem_fwd(gpu_ext, tag, x4, w, n, mb, errs)
        T.fwd_check(tag, family, y, shards, r, a, errs)
        if family in ("uniform", "ternary"):  # one shard per workgroup: the grid is what the case says
            used = int((shards[:, 1].abs().sum(1) > 0).sum())
            assert used == T.fwd_grid(n, mb, cus)[0], (used, T.fwd_grid(n, mb, cus))
    _done(errs)


@gpu
def test_stem_fwd_negative_max_blocks_raises(gpu_ext):
    x4, w, _, _ = _fwd_case("uniform", 1)
    with pytest.raises(Exception, match="max_blocks"):
        _run_stem_fwd(gpu_ext, "neg", x4, w, 1, -1, [])


@gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_pad_c3_to_c4_exact(gpu_ext, dtype):
    """35 pixels (no multiple of 64): channels 0 .. 2 bit-equal, channel 3 zero bits."""
    from fluxmpi_amd.ops.pool import pad_c3_to_c4
    x = E.patterns(1, 5, 7, 3).view(torch.int16).view(dtype).cuda().permute(0, 3, 1, 2)
    y = pad_c3_to_c4(x).permute(0, 2, 3, 1)
    assert y.shape == (1, 5, 7, 4) and y.is_contiguous()
    assert torch.equal(y[..., :3].contiguous().view(torch.int16), x.permute(0, 2, 3, 1).contiguous().view(torch.int16))
    assert int(y[..., 3].contiguous().view(torch.int16).abs().max()) == 0


# ============================================================================ GPU: stem_bwd

def _run_stem_bwd(ext, tag, inp, blocks, errs, w="own"):
    n = inp["n"]
    assert ext.stem_part_floats() == T.PART
    d = {k: inp[k].cuda() for k in ("x4", "c", "dp", "idx", "mean", "inv")}
    wt = inp["w"] if w == "own" else w
    wd = wt.cuda() if wt is not None else None
    pbuf, part = E.guarded(blocks, T.PART, T.PART, torch.float32, "cuda")
    sbuf, ws = E.guarded(128, 64, 64, torch.float32, "cuda", fill=0.0)
    obuf, ob = E.guarded(2, 64, 64, torch.float32, "cuda")
    dbuf, dwp = E.guarded(64, 256, 256, torch.float32, "cuda")
    ext.stem_bwd(d["x4"].data_ptr(), d["c"].data_ptr(), d["dp"].data_ptr(), d["idx"].data_ptr(),
                 wd.data_ptr() if wd is not None else 0, d["mean"].data_ptr(), d["inv"].data_ptr(), part.data_ptr(),
                 blocks, ws.data_ptr(), ob[0].data_ptr(), ob[1].data_ptr(), dwp.data_ptr(), n, _stream())
    torch.cuda.synchronize()
    out = dict(part=E.take_guarded(tag + " part", pbuf, part, errs).cpu(),
               dwp=E.take_guarded(tag + " dwp", dbuf, dwp, errs).cpu())
    o = E.take_guarded(tag + " bn sums", obuf, ob, errs).cpu()
    out["dw_bn"], out["db_bn"] = o[0], o[1]
    left = E.take_guarded(tag + " workspace", sbuf, ws, errs)
    if int(torch.count_nonzero(left)):
        errs.append(f"{tag}: {int(torch.count_nonzero(left))} workspace floats left non-zero")
    return out


def _bwd_grid(ext, gi):
    return T.bwd_grids(ext.stem_bwd_blocks(3))[gi]


BWD_PARAMS = [(f, gi) for gi in range(6) for f in T.BWD_FAMILIES if gi < 2 or f in ("uniform", "integer")]


@gpu
@pytest.mark.parametrize("family,gi", BWD_PARAMS, ids=[f"{f}-grid{gi}" for f, gi in BWD_PARAMS])
def test_stem_bwd(gpu_ext, family, gi):
    n, blocks = _bwd_grid(gpu_ext, gi)
    assert 1 <= blocks <= gpu_ext.stem_bwd_blocks(n), "the grid of this case needs a workgroup per row pair"
    inp, ref = _bwd_case(family, n)
    errs = []
    tag = f"bwd {family} n{n} b{blocks}"
    out = _run_stem_bwd(gpu_ext, tag, inp, blocks, errs)
    for k in ("dwp", "dw_bn", "db_bn"):
        if not bool(torch.isfinite(out[k]).all()):
            errs.append(f"{tag} {k}: not fully written")
    T.bwd_check(tag, family, inp, ref, out, blocks, errs)
    _done(errs)


@gpu
@pytest.mark.parametrize("gi", [0, 1])
def test_stem_bwd_null_w_is_ones(gpu_ext, gi):
    n, blocks = _bwd_grid(gpu_ext, gi)
    inp, _ = _bwd_case("uniform", n)
    errs = []
    a = _run_stem_bwd(gpu_ext, "null w", inp, blocks, errs, w=None)
    b = _run_stem_bwd(gpu_ext, "ones w", inp, blocks, errs, w=torch.ones(64))
    _done(errs)
    assert torch.equal(a["dwp"].view(torch.int32), b["dwp"].view(torch.int32))
    assert torch.equal(a["part"].view(torch.int32), b["part"].view(torch.int32))


@gpu
def test_stem_bwd_bad_grid_raises(gpu_ext):
    inp, _ = _bwd_case("uniform", 1)
    for blocks in (0, gpu_ext.stem_bwd_blocks(1) + 1):
        with pytest.raises(Exception, match="grid"):
            _raw_bad_bwd(gpu_ext, inp, blocks)  # refused before any buffer is touched (which have room anyway)


def _raw_bad_bwd(ext, inp, blocks):
    d = {k: inp[k].cuda() for k in ("x4", "c", "dp", "idx", "mean", "inv")}
    part = torch.zeros(max(blocks, 1) * T.PART, device="cuda")
    ws, o, dwp = torch.zeros(128 * 64, device="cuda"), torch.zeros(2, 64, device="cuda"), torch.zeros(64, 256, device="cuda")
    ext.stem_bwd(d["x4"].data_ptr(), d["c"].data_ptr(), d["dp"].data_ptr(), d["idx"].data_ptr(), 0,
                 d["mean"].data_ptr(), d["inv"].data_ptr(), part.data_ptr(), blocks, ws.data_ptr(), o[0].data_ptr(),
                 o[1].data_ptr(), dwp.data_ptr(), 1, _stream())


# ============================================================================ GPU: conv_c3.hip

C3_IDS = ["x".join(map(str, s)) for s in T.C3_SHAPES]


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


@gpu
@pytest.mark.parametrize("shape", T.C3_SHAPES, ids=C3_IDS)
def test_conv_c3_raw(gpu_ext, shape):
    """conv_c3_fwd and conv_c3_wgrad through their bindings, every family, outputs in guard bands."""
    from fluxmpi_amd.ops.conv_small import _filter_pairs
    n, h, wd, s, co = shape
    ho, wo = T.c3_out(h, wd, s)
    px = n * ho * wo
    assert gpu_ext.conv_c3_supported(n, h, wd, s, co)
    blocks = gpu_ext.conv_c3_wgrad_blocks(n, h, wd, s)
    assert blocks == T.ceil_div(px, T.C3_WG_PX)
    errs = []
    for family in E.FAMILIES:
        tag = f"c3 {family} {shape}"
        x, wt = T.c3_fwd_inputs(family, n, h, wd, s, co)
        _, _, r, a = T.c3_fwd_reference(x, wt, s)
        xd, pairs = _nhwc(x).cuda(), _filter_pairs(wt.cuda()).contiguous()
        ybuf, y = E.guarded(px, co, co, torch.bfloat16, "cuda")
        gpu_ext.conv_c3_fwd(xd.data_ptr(), pairs.data_ptr(), y.data_ptr(), n, h, wd, s, co, _stream())
        torch.cuda.synchronize()
        E.check_out(tag + " fwd", family, E.take_guarded(tag + " y", ybuf, y, errs).cpu(), r, a, 28, "bf16", errs)
        x, dy = T.c3_wgrad_inputs(family, n, h, wd, s, co)
        r, a = T.c3_wgrad_reference(x, dy, s)
        xd, dyd = _nhwc(x).cuda(), _nhwc(dy).cuda()
        pbuf, part = E.guarded(blocks * co, 27, 27, torch.float32, "cuda")
        gpu_ext.conv_c3_wgrad(xd.data_ptr(), dyd.data_ptr(), part.data_ptr(), n, h, wd, s, co, _stream())
        torch.cuda.synchronize()
        got = E.take_guarded(tag + " part", pbuf, part, errs).cpu().view(blocks, co, 27)
        if not bool(torch.isfinite(got).all()):
            errs.append(f"{tag} part: not fully written")
            continue
        T.c3_check_wgrad(tag + " wgrad", family, got.double().sum(0), r, a, px, errs)
    _done(errs)


@gpu
@pytest.mark.parametrize("shape", T.C3_SHAPES, ids=C3_IDS)
def test_conv_c3_wrapper(gpu_ext, shape):
    """conv3x3_small and its backward (the bf16 filter gradient: one more u |R|)."""
    from fluxmpi_amd.ops.conv_small import _native, conv3x3_small
    n, h, wd, s, co = shape
    px = n * T.c3_out(h, wd, s)[0] * T.c3_out(h, wd, s)[1]
    errs = []
    for family in E.FAMILIES:
        tag = f"c3 wrapper {family} {shape}"
        x, dy = T.c3_wgrad_inputs(family, n, h, wd, s, co)
        _, wt = T.c3_fwd_inputs(family, n, h, wd, s, co)
        conv = torch.nn.Conv2d(3, co, 3, stride=s, padding=1, bias=False).cuda().bfloat16()
        conv = conv.to(memory_format=torch.channels_last)
        with torch.no_grad():
            conv.weight.copy_(wt)
        xd = x.cuda().contiguous(memory_format=torch.channels_last)
        assert _native(xd, conv.weight, s, 1) is not None
        y = conv3x3_small(xd, conv)
        _, _, r, a = T.c3_fwd_reference(x, wt, s)
        if family != "gather":  # (the gather filter of the forward belongs to the other image: bounded families suffice)
            E.check_out(tag + " fwd", family, T.c3_rows(y.detach()).cpu(), r, a, 28, "bf16", errs)
        y.backward(dy.cuda().contiguous(memory_format=torch.channels_last))
        r, a = T.c3_wgrad_reference(x, dy, s)
        T.c3_check_wgrad(tag + " dW", family, E.taps(conv.weight.grad).cpu(), r, a, px, errs, bf16_store=True)
    _done(errs)


@gpu
def test_conv_c3_refusals(gpu_ext):
    x = torch.zeros(1, 8, 8, 3, device="cuda", dtype=torch.bfloat16)
    big = torch.zeros(1 << 16, device="cuda", dtype=torch.float32)
    for s, co in ((3, 128), (1, 64), (1, 192)):
        assert not gpu_ext.conv_c3_supported(1, 8, 8, s, co)
        with pytest.raises(Exception, match="unsupported"):
            gpu_ext.conv_c3_fwd(x.data_ptr(), big.data_ptr(), big.data_ptr(), 1, 8, 8, s, co, _stream())
        with pytest.raises(Exception, match="unsupported"):
            gpu_ext.conv_c3_wgrad(x.data_ptr(), big.data_ptr(), big.data_ptr(), 1, 8, 8, s, co, _stream())
