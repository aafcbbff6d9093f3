"""The Anderson solver kernels (anderson.hip: gram_kernel, mix_kernel, solve_kernel, adjoint_step_kernel) against
float64 references under derived bounds, exact cases that must be EQUAL, NaN padding and guard bands around
every buffer, every layout argument, the launchers' refusals, and a CPU half that shows a float32 evaluation in
the kernels' summation order meets every bound with room, reproduces every exact case, and that planted defects
trip the same checkers. ``anderson_edges``' docstring writes out every bound term.

Input families (seeded, made on the CPU):
    gauss       the inputs of ``test_deq.py``: X, F normal (mix: alpha normal; solve: rows of F = X + 0.1 randn)
    converging  F = X + 2^-10 randn, X of order 1: a solve near its fixed point
    collinear   difference rows = one base row + 2^-10 noise: a Gram matrix of nearly rank one
    scaled      row norms fall by 2^-20 from the oldest to the newest (solve: the largest entry 2^13 lam, see
                ``solve_rows``: below u of it lam is lost in fp32 and the last pivot is 0)
    cancel      gram: odd rows (w, -w, ..), even rows (w, w, ..): odd x even sums cancel; mix: weights of
                +-1000 that sum to 1; solve: rows in +- pairs up to noise
    exact       gram, mix and the adjoint's "int": integers, EQUAL (``anderson_edges``)
    solve only  identity (2^k I, lam 0), tie (2^k (I + J): equal candidates in the pivot columns, two launches
                bit-identical), below1 / above1 (different pivot sequences, ``test_solve_pivot_sequences_cpu``);
                every family as synthetic partials over 1 and 3 chunks at lam 1e-4 and 1e-8, and the partials
                of a real Gram launch once (``test_gram_to_solve_handover``)

Shapes and the paths they reach are asserted in ``test_shapes_reach_paths_cpu``. Gram / mix d: 4 (one lane), 36
(9 lanes, bf16 rows 8-byte aligned), 1024 (one full pass), 1028 (one lane twice), 4100 (auto chunks 2), 37632 with
raw chunks 8 (the production chunk4 1176); raw chunks 1, 3 (last chunk one vector short), 1025 (chunk4 1), 1030
(five empty chunks, EQUAL 0) at d 4100; bsz 1, 3, 300; n 1 .. 8 with every last (all-fresh) and every fr
(one-fresh); one padded layout per kernel and dtype pair. Solve bsz 1, 63, 64, 65, 1000, 1024, and 1025 through the
wrapper's composition. Mix: every slot x beta {1, 0.8, 0.5} x z {none, bf16, fp16, fp32} at d 4100. adjoint_step:
8 (1, 255, 256, 257, 4097) elements, blocks 1, 2, auto, auto + 3, three dtypes, both layouts through the wrapper,
and 8 (4 * 256 * 1024 + 1) bf16 elements past the wrapper's 1024-block cap.

What changed in the launchers and the wrapper: ``anderson_gram`` divided by ``chunks`` without checking it
(``chunks = 0``: an integer division by zero in the caller's process) and launched with ``bsz < 1``; neither it
nor ``anderson_mix`` checked that the rows 0 .. n-1 fit inside ``batch_stride`` (``check_layout`` does now, for
both). ``ops.anderson.mix(z_dtype=float32)`` on a bf16 history returned the bf16 row; it now returns the
unrounded fp32 mix through the float z instantiation, as the CPU composition does. No kernel arithmetic changed,
and the tests found no kernel defect.

One deviation from the plan of this file: 2^k I with lam = 0 was expected to give alpha = 1 / n bit for bit
whenever n is a power of two. That holds at n = 1 and 2 (asserted). At n = 4 and 8 partial pivoting passes through
the pivots 1, 2, 3, so 1 / 3 is rounded, and a correctly rounded fp32 elimination (the emulation) ends one unit in
the last place off (0.249999985); those cases go by the backward-error bound. Measured on the MI355X (figures,
65 systems each): n = 2: 0 of 130 entries differ from 1 / n; n = 4: 52 of 260, the emulation's 52, by 1.49e-8;
n = 8: 260 of 520 (the emulation, which has no fma, 117), by at most 1.49e-8.

Measured on the MI355X (one run of this file; no bound was changed after it, none was exceeded), worst
|err| / bound over every shape, n, last / fr and dtype pair:
    gram      per-chunk partials: gauss 0.146, converging 0.104, collinear 0.118, scaled 0.143, cancel 0.119; the
              wrapper's totals 0.086 .. 0.104; exact: every partial, total and fn EQUAL; stored G EQUAL in every
              launch that stores one (12960 launches in all); unused slots and the five empty chunks EQUAL 0
    solve     |H a - e0| / bound: gauss 0.051, converging 0.040, collinear 0.045, scaled 0.057, cancel 0.058,
              identity 0.012, tie 0.020, below1 0.023, above1 0.031, the Gram hand-over 0.025, the wrapper at
              3 / 1024 / 1025 0.009 / 0.022 / 0.023; res 0.070 .. 0.127; n = 1 and 2^k I at n = 2 EQUAL; two
              launches bit-identical (tie included)
    mix       the fp32 row 0.50 (0.497: a single product's rounding is half of its E), a bf16 row or a bf16 /
              fp16 z 0.995 .. 0.998 (one correctly rounded store sits just under 1); exact EQUAL; z ==
              X[:, slot].to(z), z == X[:, slot] and X[:, slot] == bf16(z) bit for bit; nothing else touched
    adjoint   per-block partials: gauss 0.032, converging 0.044; ss 0.015 / 0.027; u_new EQUAL in fp32, bf16 and
              fp16; int: every partial, ss and the flag at thresh2 == ss EQUAL, the 8.4 M-element case included
The CPU half (fp32 emulation, not the GPU): gram 0.146, solve 0.062 (res 0.116), mix 0.447 before the store,
adjoint 0.044; every exact case reproduced. Planted defects, factor over the bound (CPU half): drop_vec 4.7e3,
last_chunk 1.6e5, stale 7.4e4, pidx 4.0e4 (gauss; 24 collinear, 22 scaled), fn_row0 7.1e4, row_stride_d reads
the NaN padding (non-finite), trunc: 9918 stored-G elements differ / 1.9 on the mixed row, swap_beta 3.4e6,
alpha_n8 4.3e6, swap_y 3.6e5, no_pivot 31 (scaled), unrounded 2.4e4. ``test_deq.py``'s forward-error test
(2e-3) passes pidx and no_pivot on ``scaled`` at lam 1e-4, which the residual criterion fails
(``test_solve_forward_error_is_blind_cpu``).
Wall time (one run each): this file's 74 GPU tests 18.2 s alone; the GPU suite 181.4 s with it, 177.0 s without
(the parent's tests); the CPU half's 48 tests 32 s.
"""

import pytest
import torch

from . import anderson_edges as A
from . import mfma_edges as E
from .anderson_edges import BF, F32, HF, KOUT, KP, Layout

gpu = pytest.mark.gpu

PAIRS = [(F32, F32), (BF, BF), (BF, F32), (F32, BF)]  # (F dtype, history dtype); the second is production
PAIR_IDS = ["f32-f32", "bf16-bf16", "bf16-f32", "f32-bf16"]
NAME = {F32: "f32", BF: "bf16", HF: "f16", None: "none"}
# (bsz, d, raw chunks or None for the launcher's own choice, padded)
GRAM_SHAPES = [(3, 4, None, False), (3, 36, None, True), (1, 1024, None, False), (3, 1028, None, False),
               (3, 4100, None, True), (2, 4100, 1, False), (2, 4100, 3, True), (2, 4100, 1025, False),
               (2, 4100, 1030, False), (300, 36, None, False), (2, 37632, 8, False)]
MIX_SHAPES = [(3, 4, False), (3, 36, True), (1, 1024, False), (3, 1028, False), (3, 4100, True), (300, 36, False),
              (2, 37632, False)]
MIX_FAMILIES = ("gauss", "cancel", "exact")
SOLVE_BSZ = (1, 63, 64, 65, 1000, 1024)
ADJ_SIZES = (8, 8 * 255, 8 * 256, 8 * 257, 8 * (4 * 1024 + 1))
ADJ_BIG = 8 * (4 * 256 * 1024 + 1)
ZS = (None, BF, HF, F32)
HALF = 0.5


def _done(errs):
    assert not errs, "\n".join(errs[:20]) + (f"\n... and {len(errs) - 20} more" if len(errs) > 20 else "")


def _shapes_for(fdt, hdt):
    """Every shape for fp32 and the production pair; d = 36 and d = 4100 for the mixed pairs."""
    return [s for s in GRAM_SHAPES if fdt == hdt or s[1] in (36, 4100)]


def _chunks(s):
    return s[2] if s[2] is not None else A.gram_chunks_ref(s[0], s[1])


def _cpu_worst(since):
    """The CPU half's criterion: no emulation ratio recorded since ``since`` above one half."""
    bad = {k: v for k, v in A.WORST.items() if k[0] == "cpu" and v > HALF and since.get(k, -1.0) < v}
    assert not bad, f"emulation above {HALF} of a bound: {bad}"


# =============================================================================== CPU half

def test_dtype_codes_cpu():
    from fluxmpi_amd.ops.multi_tensor import DTYPE_CODE
    assert all(DTYPE_CODE[t] == c for t, c in A.CODE.items())


def test_shapes_reach_paths_cpu():
    """The chosen shapes reach the paths they are listed for."""
    geo = {s: A.gram_geometry(s[1], _chunks(s)) for s in GRAM_SHAPES}
    assert geo[(3, 4, None, False)][:3] == (1, 1, 1)                       # one lane
    assert geo[(3, 36, None, True)][:3] == (9, 1, 9) and 36 % 8 != 0 and (36 + 4) % 8 == 0 and 36 * 2 % 16 != 0
    assert geo[(1, 1024, None, False)][:3] == (256, 1, 256)                # exactly one full pass
    assert geo[(3, 1028, None, False)][:3] == (257, 2, 257)                # one lane goes round twice
    assert _chunks((3, 4100, None, True)) == 2 and geo[(3, 4100, None, True)] == (513, 3, 512, 0)
    assert geo[(2, 4100, 1, False)] == (1025, 5, 1025, 0)
    assert geo[(2, 4100, 3, True)] == (342, 2, 341, 0)                     # the last chunk one vector short
    assert geo[(2, 4100, 1025, False)] == (1, 1, 1, 0)                     # chunk4 = 1
    assert geo[(2, 4100, 1030, False)] == (1, 1, 1, 5)                     # five trailing empty chunks
    assert (1030 - 1) * 1 >= 1025
    assert geo[(2, 37632, 8, False)] == (1176, 5, 1176, 0) and 1176 % 256 != 0   # production chunk, last pass partial
    assert A.gram_chunks_ref(256, 37632) == 8 and A.gram_chunks_ref(3, 36) == 1
    assert 300 > 256                                                       # more workgroups than CUs
    assert A.gram_chunk_L(37632, 8) == 19 and A.gram_total_L(37632, 8) == 26
    lay = Layout(3, 36, True)
    assert (lay.rs, lay.bs) == (40, 8 * 40 + 8) and Layout(3, 36).bs == 8 * 36
    # solve: 1 .. 16 waves, a partial wave, full waves; 1024 = 16 full waves in the one workgroup
    assert [A.ceil_div(b, 64) for b in SOLVE_BSZ] == [1, 1, 1, 2, 16, 16] and 1024 % 64 == 0 and 1000 % 64 != 0
    # adjoint: one vector; a partial wave set; one full pass; one lane twice; past 4 vectors per lane
    assert [A.adjoint_blocks_ref(n) for n in ADJ_SIZES] == [1, 1, 1, 1, 5]
    assert [A.adjoint_K(n, 1) for n in ADJ_SIZES] == [1, 1, 1, 2, 17]
    assert A.adjoint_K(ADJ_SIZES[4], 5) == 4 and A.adjoint_K(ADJ_SIZES[4], 8) == 3 and A.adjoint_K(8, 4) == 1
    assert A.ceil_div(ADJ_BIG // 8, 1024) == 1025 and A.adjoint_blocks_ref(ADJ_BIG) == 1024 and A.adjoint_K(ADJ_BIG, 1024) == 5
    assert ADJ_BIG < 2 ** 24                                               # the integer case's ss stays exact
    try:
        import fluxmpi_amd._C as ext
    except ImportError:
        return
    for s in GRAM_SHAPES:
        assert ext.anderson_gram_chunks(s[0], s[1]) == A.gram_chunks_ref(s[0], s[1])
    for n in ADJ_SIZES + (ADJ_BIG,):
        assert ext.adjoint_step_blocks(n) == A.adjoint_blocks_ref(n)


def _emu_gram_case(tag, key, family, fdt, hdt, shape, ns, errs, defect=None, total_defect=None, stale=None):
    """The emulation's launches of one shape against the references: all-fresh (with G) and one-fresh."""
    bsz, d, _, padded = shape
    chunks = _chunks(shape)
    lay = Layout(bsz, d, padded)
    X, F = A.gram_inputs(family, bsz, d, fdt, hdt)
    refs = A.gram_refs(X, F, hdt, chunks)
    Lc = A.gram_chunk_L(d, chunks)
    exact = family == "exact"
    for n in ns:
        Xb, Fb = lay.place(X, hdt, n), lay.place(F, fdt, n)
        want_G = lay.place(refs["gs"], hdt, n)
        for last in sorted({0, n // 2, n - 1}):
            for one in (False, True):
                Gb = torch.full((lay.numel,), A.NAN, dtype=hdt)
                if one:
                    Gb = want_G.clone()
                    lay.view(Gb)[:, last] = A.NAN if stale is None else stale[:, last].to(hdt)
                part, Gn = A.emu_gram(lay, Xb, Fb, Gb, n, last, chunks, one, defect)
                ref, mag, nfs = A.gram_expected(refs, n, last, one)
                t = f"{tag} n{n} last{last} {'one' if one else 'all'}"
                A.check_sums(key + ("part",), f"{t} part", part, ref, mag, nfs, Lc, exact, errs)
                tot = A.sum_chunks(part, total_defect)
                A.check_sums(key + ("total",), f"{t} total", tot, ref.sum(1), mag.sum(1), nfs, Lc + chunks - 1, exact, errs)
                A.same_bits(f"{t} stored G", Gn, want_G, errs)


@pytest.mark.parametrize("family", A.GRAM_FAMILIES)
def test_emulation_gram_cpu(family):
    since = dict(A.WORST)
    errs = []
    for (fdt, hdt), pid in zip(PAIRS, PAIR_IDS):
        for shape in _shapes_for(fdt, hdt):
            if fdt != hdt and shape[1] != 36:
                continue  # the mixed pairs' d = 4100 shapes are left to the GPU half (the emulation's cost)
            ns = (3, 8) if shape[2] in (1025, 1030) or shape[0] == 300 else (1, 2, 3, 5, 8)
            _emu_gram_case(f"cpu gram {family} {pid} {shape}", ("cpu", "gram", family), family, fdt, hdt, shape, ns, errs)
    _done(errs)
    _cpu_worst(since)


SOLVE_CASES = [(f, lam) for f in A.SOLVE_FAMILIES for lam in A.solve_partials(f, 2, 1, 1)[1]]
SOLVE_IDS = [f"{f}-{lam:g}" for f, lam in SOLVE_CASES]


def _solve_exact(family, n, lam, alpha, tag, errs):
    """2^k I with lam = 0: alpha EQUALS 1 / n at n = 1 and 2. At n = 4 and 8 the elimination passes through the
    pivots 1, 2, 3 (or their multiples), 1 / 3 is rounded and a correctly rounded fp32 elimination ends one
    unit in the last place from 1 / n (0.249999985 in the emulation): those go by the bound."""
    if family == "identity" and n in (1, 2):
        E.check(f"{tag} alpha == 1 / n", alpha, torch.full(alpha.shape, 1.0 / n, dtype=torch.float64), None, errs)


@pytest.mark.parametrize("family,lam", SOLVE_CASES, ids=SOLVE_IDS)
def test_emulation_solve_cpu(family, lam):
    """The fp32, no-fma emulation meets the backward-error criterion and the residual bound at half; every float64
    pivot is non-zero and the emulation finite (the criterion's condition) for every input the GPU half uses."""
    since = dict(A.WORST)
    errs = []
    for n in range(1, 9):
        for chunks in (1, 3):
            part, _ = A.solve_partials(family, n, 130, chunks, lam=lam)
            for bsz in (1, 65, 130):
                last = (n - 1) if bsz != 65 else n // 2
                alpha, res = A.emu_solve(part[:bsz], n, last, lam)
                assert bool(torch.isfinite(alpha).all()) and bool(torch.isfinite(res).all())
                tag = f"cpu solve {family} lam{lam:g} n{n} chunks{chunks} bsz{bsz}"
                el = A.solve_check(("cpu", "solve", "alpha", family), tag, part[:bsz], n, lam, alpha, errs)
                assert bool((el["pivots"] != 0).all()) and bool(torch.isfinite(el["x"]).all()), tag
                rr, rb = A.res_ref(part[:bsz], last, n)
                A.check(("cpu", "solve", "res", family), f"{tag} res", res, rr, rb, errs)
                _solve_exact(family, n, lam, alpha, tag, errs)
    _done(errs)
    _cpu_worst(since)


def test_solve_pivot_sequences_cpu():
    """Gram entries below 1 keep row 0's |1| as the pivot of column 1; entries above 1 move it; the tie family has
    equal candidates in a pivot column and the float64 elimination takes the first."""
    n = 4
    lo = A.eliminate(A.build_H(A.solve_partials("below1", n, 8, 1)[0].double().sum(1), n, 1e-4))
    hi = A.eliminate(A.build_H(A.solve_partials("above1", n, 8, 1)[0].double().sum(1), n, 1e-4))
    assert bool((lo["piv"][:, 0] == 1).all()) and bool((hi["piv"][:, 0] == 1).all())   # H[0][0] = 0: always row 1
    assert bool((lo["piv"][:, 1] == 1).all()), lo["piv"]          # after the swap row 0 sits at position 1: it stays
    assert bool((hi["piv"][:, 1] != 1).all()), hi["piv"]
    assert not torch.equal(lo["piv"], hi["piv"])
    H = A.build_H(A.solve_partials("tie", n, 8, 1)[0].double().sum(1), n, 0.0)
    assert bool((H[:, 1:, 0] == 1).all())                                              # column 0: n equal candidates
    work = H.clone()
    work[:, [0, 1]] = work[:, [1, 0]]
    work[:, 2:] -= work[:, 0:1]
    col = work[:, 1:, 1].abs()
    ties = (col == col.max(1, keepdim=True)[0]).sum(1)
    big = torch.arange(8) % 5 - 2 >= 0                                                 # 2^k >= 1: a tie in column 1 too
    assert bool((ties[big] >= 2).all()) and bool((ties[~big] == 1).all()) and int(big.sum()) >= 3
    el = A.eliminate(H)
    assert bool((el["piv"][:, 0] == 1).all())                                          # the first of n equal candidates
    assert bool((el["piv"][:, 1] == 1 + torch.argmax(col, 1)).all())


@pytest.mark.parametrize("family", MIX_FAMILIES)
def test_emulation_mix_cpu(family):
    since = dict(A.WORST)
    errs = []
    for (fdt, hdt), pid in zip(PAIRS, PAIR_IDS):
        for bsz, d, padded in MIX_SHAPES[:5]:
            lay = Layout(bsz, d, padded)
            X, F, alpha = A.mix_inputs(family, bsz, d, fdt, hdt)
            for k, (n, slot, beta, zdt) in enumerate(_mix_combos(family, full=d == 36)):
                Xb, Fb = lay.place(X, hdt, n), lay.place(F, fdt, n)
                Xa, z, o = A.emu_mix(lay, Xb, Fb, alpha, n, slot, beta, zdt)
                tag = f"cpu mix {family} {pid} {bsz}x{d} n{n} slot{slot} beta{beta} z{NAME[zdt]}"
                # one half of B_o for the fp32 value; a bound that is one correctly rounded store (a bf16 row,
                # a bf16 or fp16 z) is met just under 1 by construction, so the stores are held to their bounds
                ref, Bo = A.mix_ref(X, F, alpha, n, beta)
                A.check(("cpu", "mix", family, "o"), f"{tag} o", o, ref, None if family == "exact" else Bo, errs)
                _mix_after(("emu", "mix", family), tag, lay, X, F, alpha, n, slot, beta, hdt, zdt, Xb, Xa, z, family == "exact", errs)
    _done(errs)
    _cpu_worst(since)


def _mix_combos(family, full):
    """(n, slot, beta, z dtype): every slot x beta x z once with n cycling (``full``), or every n once."""
    betas = (1.0, 0.5, 0.5) if family == "exact" else (1.0, 0.8, 0.5)
    if full:
        return [(1 + (slot + bi + zi) % 8, slot, betas[bi], ZS[zi]) for slot in range(8) for bi in range(3) for zi in range(4)]
    return [(n, (n + 2) % 8, betas[n % 3], ZS[n % 4]) for n in range(1, 9)]


def _mix_after(key, tag, lay, X, F, alpha, n, slot, beta, hdt, zdt, Xb, Xa, z, exact, errs):
    """One launch's buffers: the written row and z by their bounds and EQUAL relations, everything else untouched."""
    row = lay.view(Xa)[:, slot].clone()
    want = Xb.clone()
    lay.view(want)[:, slot] = row
    A.same_bits(f"{tag} X outside the slot", Xa, want, errs)
    A.check_mix(key, tag, X, F, alpha, n, slot, beta, hdt, zdt, row, z, exact, errs)


@pytest.mark.parametrize("family", ("gauss", "converging", "int"))
def test_emulation_adjoint_cpu(family):
    since = dict(A.WORST)
    errs = []
    for dtype in (F32, BF, HF):
        for n in ADJ_SIZES:
            v, g, u = A.adjoint_inputs(family, n, dtype)
            auto = A.adjoint_blocks_ref(n)
            for blocks in (1, 2, auto, auto + 3):
                un, part = A.emu_adjoint(v, g, u, blocks)
                tag = f"cpu adjoint {family} {NAME[dtype]} n{n} blocks{blocks}"
                ref_p = A.check_adjoint(("cpu", "adjoint", "part", family), tag, v, g, u, blocks, un, part, family == "int", errs)
                tot = A.emu_adjoint_total(part).reshape(1)
                A.check(("cpu", "adjoint", "ss", family), f"{tag} ss", tot, ref_p.sum().reshape(1),
                        None if family == "int" else torch.tensor([A.ss_bound(ref_p, n, blocks)], dtype=torch.float64), errs)
    _done(errs)
    _cpu_worst(since)


GRAM_DEFECT_SHAPE = (3, 4100, 3, True)
DEFECTS = ("drop_vec", "last_chunk", "stale", "pidx", "fn_row0", "row_stride_d", "trunc_gram", "trunc_mix", "swap_beta",
           "alpha_n8", "swap_y", "no_pivot", "unrounded")


def _defect_errs(defect, on):
    errs = []
    key = ("defect", defect)
    if defect in ("drop_vec", "last_chunk", "stale", "fn_row0", "row_stride_d", "trunc_gram"):
        fdt, hdt = (BF, BF) if defect == "trunc_gram" else (F32, F32)
        stale = A.gram_refs(*A.gram_inputs("gauss", 3, 4100, fdt, hdt, seed=1), hdt, 1)["gs"] if defect == "stale" else None
        _emu_gram_case(defect, key, "gauss", fdt, hdt, GRAM_DEFECT_SHAPE, (3, 8), errs,
                       defect={"trunc_gram": "trunc"}.get(defect, defect) if on and defect not in ("last_chunk", "stale") else
                       ("stale" if on and defect == "stale" else None),
                       total_defect="last_chunk" if on and defect == "last_chunk" else None, stale=stale)
    elif defect in ("pidx", "swap_y", "no_pivot"):
        for family in ("gauss", "scaled", "collinear"):
            part, _ = A.solve_partials(family, 8, 65, 3)
            alpha, _ = A.emu_solve(part, 8, 7, 1e-4, defect if on else None)
            A.solve_check(key, f"{defect} {family}", part, 8, 1e-4, alpha, errs)
    elif defect in ("trunc_mix", "swap_beta", "alpha_n8", "row_stride_d_mix"):
        hdt = BF if defect == "trunc_mix" else F32
        lay = Layout(3, 36, True)
        X, F, alpha = A.mix_inputs("gauss", 3, 36, F32, hdt)
        n, slot, beta, zdt = 3, 5, 0.8, BF
        Xb, Fb = lay.place(X, hdt, n), lay.place(F, F32, n)
        Xa, z, _ = A.emu_mix(lay, Xb, Fb, alpha, n, slot, beta, zdt, {"trunc_mix": "trunc"}.get(defect, defect) if on else None)
        _mix_after(key, defect, lay, X, F, alpha, n, slot, beta, hdt, zdt, Xb, Xa, z, False, errs)
    elif defect == "unrounded":
        v, g, u = A.adjoint_inputs("converging", 8 * 257, BF)
        un, part = A.emu_adjoint(v, g, u, 2, defect if on else None)
        A.check_adjoint(key, defect, v, g, u, 2, un, part, False, errs)
    else:
        raise ValueError(defect)
    return errs


@pytest.mark.parametrize("defect", DEFECTS)
def test_planted_defect_fails_cpu(defect):
    _done(_defect_errs(defect, False))
    errs = _defect_errs(defect, True)
    print("\n".join(errs))
    assert errs, f"the checkers did not notice the planted defect {defect}"


def test_solve_forward_error_is_blind_cpu():
    """``test_deq.py``'s forward-error test (2e-3, relative and absolute) against the backward-error criterion on
    the ``scaled`` family: which of the solve defects the former passes and the latter fails."""
    table = {}
    for defect in (None, "pidx", "swap_y", "no_pivot"):
        for lam in (1e-4, 1e-8):
            part, _ = A.solve_partials("scaled", 8, 65, 1, lam=lam)
            alpha, _ = A.emu_solve(part, 8, 7, lam, defect)
            want = A.solve_forward(part, 8, lam)
            fwd = (alpha.double() - want).abs()
            fwd_ok = bool((fwd <= 2e-3 + 2e-3 * want.abs()).all())
            errs = []
            A.solve_check(("defect", "fwd", str(defect)), f"{defect} lam{lam:g}", part, 8, lam, alpha, errs)
            print(f"{defect} lam {lam:g}: forward error {float(fwd.max()):.3g}, forward test {'passes' if fwd_ok else 'fails'}, "
                  f"residual criterion {'fails' if errs else 'passes'}")
            table[(defect, lam)] = (fwd_ok, not errs)
    assert table == FORWARD_VS_RESIDUAL, table


# (defect, lam) -> (the forward test passes, the residual criterion passes), from the fp32 emulation on ``scaled``.
# At lam 1e-4 the wrong pair index and the missing pivoting pass the forward test and fail the criterion. At lam
# 1e-8 the family's Gram entries are 2^13 lam, the one wrong entry is below the rounding of the border of ones in
# both tests, and elimination without pivoting has the sound emulation's forward error (6.3e-4): no test of alpha
# alone can see either there, and the Gram tests see the first.
FORWARD_VS_RESIDUAL = {(None, 1e-4): (True, True), (None, 1e-8): (True, True),
                       ("pidx", 1e-4): (True, False), ("pidx", 1e-8): (True, True),
                       ("swap_y", 1e-4): (False, False), ("swap_y", 1e-8): (False, False),
                       ("no_pivot", 1e-4): (True, False), ("no_pivot", 1e-8): (True, True)}


def test_mix_composition_cpu():
    """The CPU composition of ``ops.anderson.mix`` returns a tensor of ``z_dtype`` for every (history, z) pair:
    the stored row for None (and fp32 on fp32), otherwise the fp32 mix rounded once."""
    from fluxmpi_amd.ops import anderson as AO
    errs = []
    for hdt in (F32, BF):
        for zdt in ZS:
            X, F, alpha = A.mix_inputs("gauss", 3, 36, F32, hdt)
            Xh = X.to(hdt)
            z = AO.mix(Xh, F, alpha[:, :3], 5, 0.8, zdt)
            assert z.dtype == (hdt if zdt is None else zdt) and z.shape == (3, 36), (hdt, zdt, z.dtype)
            ref, Bo = A.mix_ref(X, F, alpha, 3, 0.8)
            # the composition's operations are the kernel's (n products and additions in bmm, the products with
            # beta and c, one sum), but its c is fl32(1 - 0.8) where the reference's is fl32(1 - fl32(0.8)),
            # 1.25 u apart: one E more on the same magnitudes
            Bo = Bo * (3 + 3) / (3 + 2)
            bnd = Bo if z.dtype == F32 else Bo + A.rt(z.dtype, ref) + A.UT[z.dtype] * Bo
            E.check(f"composition {NAME[hdt]} z {NAME[zdt]}", z, ref, bnd, errs)
            if zdt is None or (zdt == F32 and hdt == F32):
                assert z.data_ptr() == Xh[:, 5].data_ptr()
            else:
                assert z.data_ptr() != Xh[:, 5].data_ptr()
            if zdt == F32:  # the stored row is the returned fp32 value rounded once to the history's type
                A.same_bits("X[:, slot] == hdt(z)", Xh[:, 5], z.to(hdt), errs)
    _done(errs)


def _refusal_calls(ext, p, q, o, st):
    """(match, call) pairs: every one is refused by the argument checks of the launchers."""
    lay = Layout(2, 36, True)

    def gram(n=3, last=0, chunks=1, bsz=2, d=36, rs=lay.rs, bs=lay.bs, X=p, G=0, fdt=7, hdt=7):
        return lambda: ext.anderson_gram(X, q, fdt, G, 0, o, bsz, d, rs, bs, n, last, chunks, st, hdt)

    def mix(n=3, slot=0, bsz=2, d=36, rs=lay.rs, bs=lay.bs, X=p, z=0, zdt=7, fdt=7, hdt=7):
        return lambda: ext.anderson_mix(X, q, fdt, o, z, zdt, bsz, d, rs, bs, n, slot, 0.5, st, hdt)

    def solve(chunks=1, bsz=2, n=3, last=0):
        return lambda: ext.anderson_solve(p, chunks, bsz, n, last, 1e-4, o, 0, st)

    def adj(blocks=1, n=64, v=p, dt=7):
        return lambda: ext.adjoint_step(v, q, q, o, o, blocks, n, dt, st)

    return [
        ("chunks >= 1", gram(chunks=0)), ("chunks >= 1", gram(chunks=-3)),
        ("1 <= bsz", gram(bsz=0)), ("1 <= bsz", gram(bsz=-1)), ("bsz", gram(bsz=65536)),
        ("do not fit", gram(n=8, bs=7 * lay.rs + 32)), ("do not fit", gram(n=3, bs=2 * lay.rs + 32)),
        ("do not fit", gram(n=2, rs=1 << 40, bs=1 << 40)),
        ("do not fit", mix(n=8, bs=7 * lay.rs + 32)), ("do not fit", mix(n=3, bs=2 * lay.rs + 32)),
        ("slot out of range", mix(slot=8)), ("slot out of range", mix(slot=-1)),
        ("1 <= n <= 8", gram(n=0)), ("1 <= n <= 8", gram(n=9)), ("1 <= n <= 8", mix(n=0)), ("1 <= n <= 8", mix(n=9)),
        ("multiples of 4", gram(d=38)), ("multiples of 4", gram(rs=42)), ("multiples of 4", gram(bs=8 * 40 + 6)),
        ("multiples of 4", gram(rs=32)), ("multiples of 4", mix(d=38)),
        ("16-byte aligned", gram(X=p + 4)), ("16-byte aligned", gram(G=p + 8)), ("16-byte aligned", mix(X=p + 4)),
        ("8-byte aligned", mix(z=p + 4, zdt=9)),
        ("last row out of range", gram(n=3, last=3)), ("last row out of range", gram(last=-1)),
        ("fp32 or bf16", gram(fdt=6)), ("fp32 or bf16", gram(hdt=6)), ("fp32 or bf16", mix(fdt=6)), ("fp32 or bf16", mix(hdt=8)),
        ("unsupported z dtype", mix(z=p, zdt=8)),
        ("anderson_solve", solve(chunks=0)), ("anderson_solve", solve(bsz=0)), ("anderson_solve", solve(bsz=1025)),
        ("anderson_solve", solve(n=9)), ("anderson_solve", solve(last=3)),
        ("adjoint_step", adj(blocks=0)), ("adjoint_step", adj(n=60)), ("16-byte aligned", adj(v=p + 8)),
        ("adjoint_step", adj(dt=8)),
    ]


def test_refusals_before_any_launch_cpu():
    """The launchers on the host alone: every refusal is raised from the argument checks, before the first HIP
    call, so it reads the same on a machine without a GPU (the pointers are never dereferenced). The GPU half
    repeats this next to real buffers."""
    try:
        import fluxmpi_amd._C as ext
    except ImportError:
        pytest.skip("fluxmpi_amd._C is not built")
    if torch.cuda.is_available():
        return  # made-up pointers stay away from a real device: test_refusals
    for match, call in _refusal_calls(ext, 1 << 20, 2 << 20, 3 << 20, 0):
        with pytest.raises(RuntimeError, match=match):
            call()


# =============================================================================== GPU: plumbing

def _st():
    return torch.cuda.current_stream().cuda_stream


def _gram_raw(ext, lay, Xg, Fg, Gg, fdt, hdt, n, last, chunks, mask, tag, errs):
    part = A.banded(lay.bsz * chunks * KOUT, F32, "cuda")
    ext.anderson_gram(lay.ptr(Xg), lay.ptr(Fg), A.CODE[fdt], 0 if Gg is None else lay.ptr(Gg), mask, part[1].data_ptr(),
                      lay.bsz, lay.d, lay.rs, lay.bs, n, last, chunks, _st(), A.CODE[hdt])
    return A.take_banded(f"{tag} part", part, errs).view(lay.bsz, chunks, KOUT)


def _solve_raw(ext, part_g, n, last, lam, tag, errs, want_res=True):
    bsz, chunks = part_g.shape[:2]
    alpha = A.banded(bsz * n, F32, "cuda")
    res = A.banded(1, F32, "cuda")
    ext.anderson_solve(part_g.data_ptr(), chunks, bsz, n, last, float(lam), alpha[1].data_ptr(),
                       res[1].data_ptr() if want_res else 0, _st())
    return A.take_banded(f"{tag} alpha", alpha, errs).view(bsz, n), A.take_banded(f"{tag} res", res, errs)


def _packed(H, n):
    out = torch.zeros(H.shape[0], KOUT, dtype=H.dtype)
    for i, j in A.pairs(n):
        out[:, A.pidx(i, j, n)] = H[:, i, j]
    return out


# =============================================================================== GPU: refusals

@gpu
def test_refusals(gpu_ext):
    """Every refusal next to real buffers; nothing ran: the output stays as it was."""
    big = torch.zeros(1 << 16, device="cuda")
    src = torch.zeros(1 << 16, device="cuda")
    out = torch.full((1 << 16,), 7.0, device="cuda")
    for match, call in _refusal_calls(gpu_ext, big.data_ptr(), src.data_ptr(), out.data_ptr(), _st()):
        with pytest.raises(RuntimeError, match=match):
            call()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and not bool(big.any())


# =============================================================================== GPU: gram

@gpu
@pytest.mark.parametrize("fdt,hdt", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("family", A.GRAM_FAMILIES)
def test_gram(gpu_ext, family, fdt, hdt):
    """Raw launches with explicit chunks, every n, every last (all-fresh) and every fr (one-fresh), NaN everywhere
    a kernel must not read, per-chunk partials by their bounds, the stored G EQUAL, then the wrapper's totals."""
    from fluxmpi_amd.ops import anderson as AO
    errs = []
    exact = family == "exact"
    pid = PAIR_IDS[PAIRS.index((fdt, hdt))]
    key = ("gpu", "gram", family, pid)
    for shape in _shapes_for(fdt, hdt):
        bsz, d, raw, padded = shape
        chunks = _chunks(shape)
        lay = Layout(bsz, d, padded)
        X, F = A.gram_inputs(family, bsz, d, fdt, hdt)
        refs = A.gram_refs(X, F, hdt, chunks)
        Lc = A.gram_chunk_L(d, chunks)
        for n in range(1, 9):
            Xc, Fc = lay.place(X, hdt, n), lay.place(F, fdt, n)
            Xg, Fg, want_G = Xc.cuda(), Fc.cuda(), lay.place(refs["gs"], hdt, n).cuda()
            for last in range(n):
                for one in (False, True):
                    t = f"gram {family} {pid} {shape} n{n} last{last} {'one' if one else 'all'}"
                    if one:
                        Gg = want_G.clone()
                        lay.view(Gg)[:, last] = A.NAN
                    else:  # without a G buffer once per n
                        Gg = None if last == n - 1 and n % 2 == 0 else torch.full_like(want_G, A.NAN)
                    part = _gram_raw(gpu_ext, lay, Xg, Fg, Gg, fdt, hdt, n, last, chunks, (1 << last) if one else (1 << n) - 1, t, errs)
                    ref, mag, nfs = A.gram_expected(refs, n, last, one)
                    A.check_sums(key + ("part",), f"{t} part", part, ref, mag, nfs, Lc, exact, errs)
                    if Gg is not None:
                        A.same_bits(f"{t} stored G", Gg, want_G, errs)
            A.same_bits(f"gram {shape} n{n} X untouched", Xg.cpu(), Xc, errs)
            A.same_bits(f"gram {shape} n{n} F untouched", Fg.cpu(), Fc, errs)
            if raw is None and n in (3, 8):  # the wrapper on the same strided buffers: totals of the auto chunks
                last = n - 1
                ref, mag, nfs = A.gram_expected(refs, n, last, False)
                H, fn = AO.gram(lay.view(Xg), lay.view(Fg), n, last)
                if not torch.equal(H, H.transpose(1, 2)):
                    errs.append(f"wrapper {shape} n{n}: H is not symmetric")
                tot = _packed(H.cpu(), n)
                tot[:, KP] = fn.cpu()
                A.check_sums(key + ("total",), f"wrapper gram {family} {pid} {shape} n{n}", tot, ref.sum(1), mag.sum(1), nfs,
                             Lc + chunks - 1, exact, errs)
                Gg = want_G.clone()
                lay.view(Gg)[:, last] = A.NAN
                H1, fn1 = AO.gram(lay.view(Xg), lay.view(Fg), n, last, lay.view(Gg), (last,))
                ref, mag, nfs = A.gram_expected(refs, n, last, True)
                tot = _packed(H1.cpu(), n)
                tot[:, KP] = fn1.cpu()
                A.check_sums(key + ("total",), f"wrapper gram one-fresh {family} {pid} {shape} n{n}", tot, ref.sum(1), mag.sum(1),
                             nfs, Lc + chunks - 1, exact, errs)
                A.same_bits(f"wrapper {shape} n{n} stored G", Gg, want_G, errs)
    print("\n".join(A.worst_lines()))
    _done(errs)


# =============================================================================== GPU: solve

@gpu
@pytest.mark.parametrize("family,lam", SOLVE_CASES, ids=SOLVE_IDS)
def test_solve(gpu_ext, family, lam):
    """``anderson_solve`` on partials the test writes itself: the backward-error criterion, the residual, the exact
    cases, two launches bit-identical."""
    errs = []
    for n in range(1, 9):
        for chunks in (1, 3):
            full, _ = A.solve_partials(family, n, 1024, chunks, lam=lam)
            for bsz in SOLVE_BSZ:
                part = full[:bsz].contiguous()
                pg = part.cuda()
                last = n - 1 if bsz != 65 else n // 2
                tag = f"solve {family} lam{lam:g} n{n} chunks{chunks} bsz{bsz}"
                alpha, res = _solve_raw(gpu_ext, pg, n, last, lam, tag, errs)
                A.solve_check(("gpu", "solve", "alpha", family), tag, part, n, lam, alpha, errs)
                rr, rb = A.res_ref(part, last, n)
                A.check(("gpu", "solve", "res", family), f"{tag} res", res, rr, rb, errs)
                _solve_exact(family, n, lam, alpha, tag, errs)
                if bsz in (65, 1024):
                    again, res2 = _solve_raw(gpu_ext, pg, n, last, lam, tag, errs, want_res=False)
                    A.same_bits(f"{tag} two launches", again, alpha, errs)
                    if not bool(torch.isnan(res2).all()):
                        errs.append(f"{tag}: res written although not asked for")
    print("\n".join(A.worst_lines()))
    _done(errs)


@gpu
@pytest.mark.parametrize("fdt,hdt", PAIRS[:2], ids=PAIR_IDS[:2])
def test_gram_to_solve_handover(gpu_ext, fdt, hdt):
    """The partials of a real Gram launch ([bsz][chunks][37], slot 36) straight into the solve; then the wrapper
    ``gram_solve`` at 3, 1024 and, through the PyTorch composition, 1025 against the same criterion."""
    from fluxmpi_amd.ops import anderson as AO
    errs = []
    bsz, d, chunks, n, last, lam = 65, 4100, 3, 5, 2, 1e-4
    lay = Layout(bsz, d, True)
    X, F = A.gram_inputs("collinear", bsz, d, fdt, hdt)
    Xg, Fg = lay.place(X, hdt, n).cuda(), lay.place(F, fdt, n).cuda()
    part = torch.full((bsz, chunks, KOUT), A.NAN, device="cuda")
    gpu_ext.anderson_gram(lay.ptr(Xg), lay.ptr(Fg), A.CODE[fdt], 0, 0, part.data_ptr(), bsz, d, lay.rs, lay.bs, n, last,
                          chunks, _st(), A.CODE[hdt])
    alpha, res = _solve_raw(gpu_ext, part, n, last, lam, "handover", errs)
    pc = part.cpu()
    A.solve_check(("gpu", "solve", "alpha", "handover"), "handover", pc, n, lam, alpha, errs)
    rr, rb = A.res_ref(pc, last, n)
    A.check(("gpu", "solve", "res", "handover"), "handover res", res, rr, rb, errs)
    refs = A.gram_refs(X, F, hdt, chunks)
    ref, mag, nfs = A.gram_expected(refs, n, last, False)
    A.check_sums(("gpu", "gram", "handover", "part"), "handover part", pc, ref, mag, nfs, A.gram_chunk_L(d, chunks), False, errs)
    for b in (3, 1024, 1025):
        dd = 36
        X, F = A.gram_inputs("collinear", b, dd, fdt, hdt)
        Xg, Fg = X.to(hdt).cuda(), F.to(fdt).cuda()
        G = torch.full_like(Xg, A.NAN)
        a, r = AO.gram_solve(Xg, Fg, n, last, G, tuple(range(n)), lam, True)
        H, fn = AO.gram(Xg, Fg, n, last)   # the same deterministic launch: the Gram the solve saw (b <= 1024)
        pk = _packed(H.cpu(), n)
        pk[:, KP] = fn.cpu()
        pk = pk[:, None]
        # 1025: the composition forms its own fp32 Gram (the subtraction, dd products and dd additions in an
        # order of PyTorch's: dd + 2 operations) where the supplied one is the kernel's (1 + L_c): their distance
        # goes to dH; its residual adds the batch in an order of PyTorch's (at most b - 1 additions)
        extra = (dd + 2 + 1 + A.gram_chunk_L(dd, 1)) * A.E23 if b == 1025 else 0.0
        A.solve_check(("gpu", "solve", "alpha", f"wrapper{b}"), f"gram_solve bsz{b}", pk, n, lam, a.cpu(), errs, extra=extra)
        rr, rb = A.res_ref(pk, last, n)
        A.check(("gpu", "solve", "res", f"wrapper{b}"), f"gram_solve bsz{b} res", r.cpu().reshape(1), rr,
                rb + ((extra + b * A.E23) * rr if b == 1025 else 0.0), errs)
        assert a.shape == (b, n) and a.dtype == F32
    print("\n".join(A.worst_lines()))
    _done(errs)


# =============================================================================== GPU: mix

@gpu
@pytest.mark.parametrize("fdt,hdt", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("family", MIX_FAMILIES)
def test_mix(gpu_ext, family, fdt, hdt):
    """Raw ``anderson_mix`` (the float z instantiation included): every slot, beta and z dtype, NaN wherever the
    kernel must not read, the written row and z by bound and by their EQUAL relations, nothing else touched."""
    errs = []
    pid = PAIR_IDS[PAIRS.index((fdt, hdt))]
    for bsz, d, padded in MIX_SHAPES:
        if fdt != hdt and d not in (36, 4100):
            continue
        lay = Layout(bsz, d, padded)
        X, F, alpha = A.mix_inputs(family, bsz, d, fdt, hdt)
        for n, slot, beta, zdt in _mix_combos(family, full=d == 4100):
            Xb, Fb = lay.place(X, hdt, n), lay.place(F, fdt, n)
            Xg, Fg = Xb.cuda(), Fb.cuda()
            ag = A.banded(bsz * n, F32, "cuda")
            ag[1].copy_(alpha[:, :n].reshape(-1))
            zb = A.banded(bsz * d, zdt, "cuda") if zdt is not None else None
            tag = f"mix {family} {pid} {bsz}x{d} n{n} slot{slot} beta{beta} z{NAME[zdt]}"
            gpu_ext.anderson_mix(lay.ptr(Xg), lay.ptr(Fg), A.CODE[fdt], ag[1].data_ptr(), zb[1].data_ptr() if zb else 0,
                                 A.CODE[zdt] if zb else 7, bsz, d, lay.rs, lay.bs, n, slot, beta, _st(), A.CODE[hdt])
            z = A.take_banded(f"{tag} z", zb, errs).view(bsz, d) if zb else None
            _mix_after(("gpu", "mix", family, pid), tag, lay, X, F, alpha, n, slot, beta, hdt, zdt, Xb, Xg.cpu(), z,
                       family == "exact", errs)
            A.same_bits(f"{tag} F untouched", Fg.cpu(), Fb, errs)
    print("\n".join(A.worst_lines()))
    _done(errs)


@gpu
@pytest.mark.parametrize("hdt", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("zdt", ZS, ids=[NAME[z] for z in ZS])
def test_mix_wrapper_returns_z_dtype(gpu_ext, hdt, zdt):
    """``ops.anderson.mix`` returns a tensor of ``z_dtype`` for all eight (history, z) pairs, equal to the raw
    launch's, and the GPU path agrees with the CPU composition on dtype and on aliasing."""
    from fluxmpi_amd.ops import anderson as AO
    errs = []
    bsz, d, n, slot, beta = 3, 4100, 5, 6, 0.8
    X, F, alpha = A.mix_inputs("gauss", bsz, d, hdt, hdt)
    Xg, Fg = X.to(hdt).cuda(), F.to(hdt).cuda()
    Xc = X.to(hdt)
    z = AO.mix(Xg, Fg, alpha[:, :n].cuda(), slot, beta, zdt)
    zc = AO.mix(Xc, F.to(hdt), alpha[:, :n], slot, beta, zdt)
    assert z.dtype == zc.dtype == (hdt if zdt is None else zdt) and z.shape == zc.shape == (bsz, d)
    alias = zdt is None or (zdt == F32 and hdt == F32)
    assert (z.data_ptr() == Xg[:, slot].data_ptr()) == alias and (zc.data_ptr() == Xc[:, slot].data_ptr()) == alias
    A.check_mix(("gpu", "mix", "wrapper", NAME[hdt]), f"wrapper {NAME[hdt]} z {NAME[zdt]}", X, F, alpha, n, slot, beta, hdt,
                z.dtype, Xg[:, slot].cpu(), z.cpu(), False, errs)
    _done(errs)


# =============================================================================== GPU: adjoint_step

def _adjoint_raw(ext, v, g, u, blocks, tag, errs):
    vg, gg, ug = v.cuda(), g.cuda(), u.cuda()
    un = A.banded(v.numel(), v.dtype, "cuda")
    part = A.banded(blocks, F32, "cuda")
    ext.adjoint_step(vg.data_ptr(), gg.data_ptr(), ug.data_ptr(), un[1].data_ptr(), part[1].data_ptr(), blocks, v.numel(),
                     A.CODE[v.dtype], _st())
    return A.take_banded(f"{tag} u_new", un, errs), A.take_banded(f"{tag} part", part, errs), part[1]


@gpu
@pytest.mark.parametrize("dtype", [F32, BF, HF], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("family", ("gauss", "converging", "int"))
def test_adjoint_step(gpu_ext, family, dtype):
    """Raw ``adjoint_step`` with explicit blocks (1, 2, the wrapper's, 3 more: idle blocks store 0): u_new EQUAL,
    per-block partials by their bound (integers EQUAL); then the wrapper, contiguous and channels_last, with
    the flag on either side of the exact value."""
    from fluxmpi_amd.ops import anderson as AO
    from fluxmpi_amd.ops import deq_cell
    errs = []
    exact = family == "int"
    for n in ADJ_SIZES:
        v, g, u = A.adjoint_inputs(family, n, dtype)
        auto = gpu_ext.adjoint_step_blocks(n)
        for blocks in (1, 2, auto, auto + 3):
            tag = f"adjoint {family} {NAME[dtype]} n{n} blocks{blocks}"
            un, part, part_g = _adjoint_raw(gpu_ext, v, g, u, blocks, tag, errs)
            ref_p = A.check_adjoint(("gpu", "adjoint", "part", family, NAME[dtype]), tag, v, g, u, blocks, un, part, exact, errs)
            total = float(ref_p.sum())
            flag = torch.full((1,), -1.0, device="cuda")
            if exact:  # thresh2 == ss exactly: the flag is 1; one float below: 0
                ss = deq_cell.adjoint_check(part_g, torch.tensor(total, device="cuda"), flag)
                ok = float(ss) == total and float(flag) == 1.0
                if total > 0:
                    below = torch.nextafter(torch.tensor(total), torch.tensor(0.0)).cuda()
                    deq_cell.adjoint_check(part_g, below, flag)
                    ok = ok and float(flag) == 0.0
                if not ok:
                    errs.append(f"{tag}: integer ss {float(ss)} != {total} or a wrong flag")
    for shape, cl in (((3, 16, 5, 8), False), ((3, 16, 5, 8), True), ((2, 48, 28, 28), True)):
        n = 1
        for s in shape:
            n *= s
        mf = torch.channels_last if cl else torch.contiguous_format
        v, g, u = (t.view(shape).contiguous(memory_format=mf) for t in A.adjoint_inputs(family, n, dtype, seed=1))
        flat = lambda t: t.permute(0, 2, 3, 1).reshape(-1) if cl else t.reshape(-1)
        blocks = gpu_ext.adjoint_step_blocks(n)
        ref_un, ref_p = A.adjoint_ref(flat(v), flat(g), flat(u), blocks)
        total, bnd = float(ref_p.sum()), A.ss_bound(ref_p, n, blocks)
        tag = f"wrapper adjoint {family} {NAME[dtype]} {shape} cl{cl}"
        un, ss = AO.adjoint_step(v.cuda(), g.cuda(), u.cuda())
        assert un.stride() == v.stride() and un.dtype == dtype
        A.same_bits(f"{tag} u_new", flat(un.cpu()), ref_un, errs)
        A.check(("gpu", "adjoint", "ss", family, NAME[dtype]), f"{tag} ss", ss.cpu().reshape(1), torch.tensor([total], dtype=torch.float64),
                None if exact else torch.tensor([bnd], dtype=torch.float64), errs)
        # the flag's launch sums the partials itself: its own ss, from a call whose threshold cannot matter
        flag = torch.full((1,), -1.0, device="cuda")
        own = AO.adjoint_step(v.cuda(), g.cuda(), u.cuda(), thresh2=torch.tensor(float("inf"), device="cuda"), flag=flag)[1].clone()
        A.check(("gpu", "adjoint", "ss", family, NAME[dtype]), f"{tag} ss (flag launch)", own.cpu().reshape(1),
                torch.tensor([total], dtype=torch.float64), None if exact else torch.tensor([bnd], dtype=torch.float64), errs)
        if float(flag) != 1.0:
            errs.append(f"{tag}: flag {float(flag)} at an infinite threshold")
        for name, t2, want in (("above", total + 2 * bnd, 1.0), ("below", total - 2 * bnd, 0.0), ("own", None, 1.0),
                               ("one float below own", "below", 0.0)):
            if t2 is None:
                th = own.clone()
            elif isinstance(t2, str):
                th = torch.nextafter(own, torch.zeros_like(own))
            else:
                th = torch.tensor(t2, device="cuda", dtype=torch.float32)
                # the float32 threshold must itself lie on the intended side of ref +- bound
                assert (float(th) >= total + bnd) if want else (float(th) < total - bnd), (name, float(th), total, bnd)
            flag = torch.full((1,), -1.0, device="cuda")
            un2, ss2 = AO.adjoint_step(v.cuda(), g.cuda(), u.cuda(), thresh2=th, flag=flag)
            if float(flag) != want or float(ss2) != float(own):
                errs.append(f"{tag}: flag {float(flag)} at the threshold {name} (ss {float(ss2)}, thresh2 {float(th)})")
    print("\n".join(A.worst_lines()))
    _done(errs)


@gpu
def test_adjoint_step_past_the_block_cap(gpu_ext):
    """8 (4 * 256 * 1024 + 1) bf16 integers: the wrapper's count of 1025 blocks is capped at 1024, so lanes go
    round a fifth time; u_new, every partial and ss EQUAL; the flag is 1 at thresh2 == ss."""
    from fluxmpi_amd.ops import anderson as AO
    from fluxmpi_amd.ops import deq_cell
    errs = []
    n = ADJ_BIG
    v, g, u = A.adjoint_inputs("int", n, BF)
    blocks = gpu_ext.adjoint_step_blocks(n)
    assert blocks == 1024
    un, part, part_g = _adjoint_raw(gpu_ext, v, g, u, blocks, "big", errs)
    ref_p = A.check_adjoint(("gpu", "adjoint", "part", "int", "big"), "big", v, g, u, blocks, un, part, True, errs)
    total = float(ref_p.sum())
    flag = torch.full((1,), -1.0, device="cuda")
    un2, ss = AO.adjoint_step(v.cuda(), g.cuda(), u.cuda(), thresh2=torch.tensor(total, device="cuda"), flag=flag)
    assert float(ss) == total and float(flag) == 1.0 and total > 2 ** 22
    A.same_bits("big wrapper u_new", un2.cpu(), un, errs)
    ss3 = deq_cell.adjoint_check(part_g, torch.nextafter(torch.tensor(total), torch.tensor(0.0)).cuda(), flag)
    assert float(ss3) == total and float(flag) == 0.0
    _done(errs)
