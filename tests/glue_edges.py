"""Inputs, references, bounds, float32 emulations in the kernels' summation order and planted defects shared by
``test_glue_edges_gpu.py`` (plain helper module: no fixtures, no tests, nothing read from the extension).

The glue kernels: ``mt_copy`` / ``mt_fill`` / ``mt_sumsq`` (multi_tensor.hip), ``gemm_splitk_reduce`` / ``_seg``
(gemm.hip: splitk_reduce_kernel, colreduce_kernel, sumall_kernel), ``colsum`` / ``gelu_fwd`` / ``gelu_bwd_bias``
(gelu.hip), ``transpose_bf16`` (gemm_nt.hip) and ``transpose_filters`` (gemm_glds.hip: xpose_taps_kernel).

Criteria (E = 2^-23 covers one fp32 addition or fma, rounded or truncated; u_T the unit roundoff of the stored type):
    mt_copy    one IEEE multiply in the product type, one round-to-nearest-even conversion: EQUAL bit for bit. The
               product type is fp64 when the source or the destination is fp64 (the caller's double), else fp32 (the
               scale rounded once to fp32).
    mt_fill    EQUAL: the double on fp64 leaves, else the value rounded once to fp32 and then to the leaf's type.
    mt_sumsq   |got - sum x^2| <= L E sum x^2 + 1e-30, L = 32 + 6 + 3 + B: a lane's 32 fmas over an 8192-element chunk
               (either path), the wave's 6 levels, the 3 additions of the 4 wave totals (the first lands on zero), one
               atomic per workgroup of the call. Every term is non-negative, so sum x^2 is its own magnitude.
    reduce     |got - r| <= S E sum_s |ws| + u_T |r| + 1e-30: no path adds a column more than S times.
    colsum     per workgroup: rpw E sum |x| + 1e-30 over its rows; the total through ``mfma_edges.check_colsums``.
    gelu_fwd   ``gelu_bound_t``: c (u_T |ref| + 2^-24), c from ``GELU_C`` (measured on the emulation, never the device).
    gelu_bwd   |dh - dy d| <= |dy| c32 E (|d| + 1) + u_T |dy d| + SUB_T + 1e-30 (d = gelu' in float64).
    transposes EQUAL as int16.
Exact families (integers, sums below 2^24 and, for a bf16 store, at most 256) must be EQUAL on every path.
"""
import math

import torch

from fluxmpi_amd.ops.multi_tensor import align_elems, aligned_offsets

from . import mfma_edges as E
from .norm_edges import SUB, UT

BF, HF, F32, F64 = torch.bfloat16, torch.float16, torch.float32, torch.float64
DTYPES = (BF, HF, F32, F64)
NAME = {BF: "bf16", HF: "f16", F32: "f32", F64: "f64"}
CODE = {F32: 7, BF: 9, HF: 6, F64: 8}
BITS = {BF: torch.int16, HF: torch.int16, F32: torch.int32, F64: torch.int64}
SENT = {BF: 0x5A5A, HF: 0x5A5A, F32: 0x5A5A5A5A, F64: 0x5A5A5A5A5A5A5A5A}
E23 = E.E23
TINY = E.TINY
NAN = float("nan")
WORST = {}  # (half, kernel, family) -> worst |err| / bound seen


def _gen(*key):
    return E._gen("glue", *key)


def ceil_div(a, b):
    return -(-a // b)


def record(key, ratio):
    WORST[key] = max(WORST.get(key, 0.0), float(ratio))


def bits_of(t):
    return t.contiguous().view(BITS[t.dtype])


def same_bits(name, got, want, errs):
    """Two tensors equal bit for bit (+-0 and subnormals count)."""
    if got.shape != want.shape or got.dtype != want.dtype:
        errs.append(f"{name}: {tuple(got.shape)} {got.dtype} != {tuple(want.shape)} {want.dtype}")
        return
    bad = bits_of(got) != bits_of(want)
    if bool(bad.any()):
        i = int(torch.nonzero(bad.reshape(-1))[0])
        errs.append(f"{name}: {int(bad.sum())} of {got.numel()} differ in bits; first at {i}: got "
                    f"{float(got.reshape(-1)[i]):.17g} want {float(want.reshape(-1)[i]):.17g}")


def check(key, name, got, ref, bnd, errs):
    """``mfma_edges.check`` that also records the worst ratio under ``key``."""
    got = got.double()
    if bnd is not None and got.shape == ref.shape and bool(torch.isfinite(got).all()):
        record(key, ((got - ref).abs() / bnd).max() if got.numel() else 0.0)
    E.check(name, got, ref, bnd, errs)


def factor(got, ref, bnd):
    """Worst |err| / bound (inf for a non-finite value): by how much a planted defect fails."""
    got = got.double()
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    return float(((got - ref).abs() / bnd).max())


# =============================================================================== mt_copy / mt_fill

MT_CHUNK, MT_VEC, MT_THREADS, MT_MAXT = 8192, 8, 256, 40
LENS = (1, 7, 8, 9, 0, 8191, 8192, 8193, 2 * 8192 + 11)  # the empty leaf in the middle is skipped
SCALES = (1.0, 0.5, -3.0, 2.0 ** -20, 1.0 / 3.0)  # 1 / 3 is also 1 / world at world = 3
PAIRS = [(a, b) for a in DTYPES for b in DTYPES if not (a == F64 and b in (BF, HF))]
REFUSED = [(F64, BF), (F64, HF)]
FILL_VALUES = (0.0, -0.0, -1.0, 0.25, 0.1, 1e-40, 70000.0, float("inf"))
GROUP_COUNTS = (41, 81)


def group_lens(count):
    return [1 + i % 9 for i in range(count)]


def product_type(tin, tout):
    return F64 if F64 in (tin, tout) else F32


def copy_ref(src, tout, scale):
    """One multiply in the product type, one rounding to ``tout``."""
    wide = product_type(src.dtype, tout)
    return (src.to(wide) * torch.tensor(scale, dtype=wide)).to(tout)


def fill_ref(n, dtype, value):
    if dtype == F64:
        return torch.full((n,), value, dtype=F64)
    return torch.full((n,), value, dtype=F32).to(dtype)


class Flat:
    """Leaves inside one buffer of sentinel bit patterns: 64 bytes of sentinels, then ``off`` elements (0: every
    leaf 16-byte aligned, 1: none), the leaves at ``aligned_offsets``, 64 bytes after. The padding between the
    leaves is sentinels too, so a store past a leaf shows."""

    def __init__(self, numels, dtype, off=0):
        self.numels, self.dtype, self.off = list(numels), dtype, off
        a = align_elems(dtype)
        offs, total = aligned_offsets(self.numels, dtype)
        self.starts = [a + off + o for o in offs]
        self.total = a + off + total + a

    def buffer(self, leaves=None, fill=NAN):
        buf = torch.full((self.total,), SENT[self.dtype], dtype=BITS[self.dtype]).view(self.dtype)
        for i, (s, n) in enumerate(zip(self.starts, self.numels)):
            buf[s:s + n] = fill if leaves is None else leaves[i].to(self.dtype)
        return buf

    def ptrs(self, buf):
        es = buf.element_size()
        return [buf.data_ptr() + s * es for s in self.starts]

    def leaves(self, buf):
        return [buf[s:s + n] for s, n in zip(self.starts, self.numels)]

    def aligned(self, i):
        return self.starts[i] * torch.empty((), dtype=self.dtype).element_size() % 16 == 0


def _mant_bits(dt):
    return int(round(-math.log2(torch.finfo(dt).eps)))


def copy_values(tin, tout, n, seed=0):
    """``n`` finite values of ``tin``: first +-0, +-largest finite, +-smallest normal, +-smallest and +-largest
    subnormal of ``tin``; then normals over the whole exponent range of the narrower-ranged of the two types and
    down through its subnormals (so products land on ``tout``'s subnormals), every fifth one, where ``tin`` is the
    more precise, set exactly half way between two neighbours of ``tout`` (a rounding tie at scales 2^k)."""
    g = _gen("copy", NAME[tin], NAME[tout], n, seed)
    fi, fo = torch.finfo(tin), torch.finfo(tout)
    fn = fi if fi.max <= fo.max else fo
    nb = _mant_bits(tin if fi.max <= fo.max else tout)
    emax, emin = int(math.floor(math.log2(fn.max))), int(round(math.log2(fn.smallest_normal))) - nb - 2
    e = torch.randint(emin, emax + 1, (n,), generator=g)
    m = torch.rand(n, generator=g, dtype=F64)
    sign = (torch.randint(0, 2, (n,), generator=g) * 2 - 1).double()
    v = (sign * (1 + m) * torch.pow(torch.tensor(2.0, dtype=F64), e.double())).clamp(-fi.max, fi.max).to(tin)
    if _mant_bits(tin) > _mant_bits(tout):
        t = v.to(tout)
        up = (bits_of(t) + 1).view(tout)
        ok = torch.isfinite(t.double()) & torch.isfinite(up.double())
        mid = ((t.double() + up.double()) / 2).clamp(-fi.max, fi.max).to(tin)
        pick = ok & (torch.arange(n) % 5 == 0)
        v = torch.where(pick, mid, v)
    sn, eps = fi.smallest_normal, fi.eps
    special = torch.tensor([0.0, -0.0, fi.max, -fi.max, sn, -sn, sn * eps, -sn * eps, sn * (1 - eps), -sn * (1 - eps)],
                           dtype=F64).to(tin)
    k = min(n, special.numel())
    v[:k] = special[:k]
    assert bool(torch.isfinite(v.double()).all())
    return v


def split(stream, numels):
    out, at = [], 0
    for n in numels:
        out.append(stream[at:at + n])
        at += n
    return out


def index_leaves(count, dtype):
    """Leaf i of 1 + i % 9 elements holds (i + 1) 2^(j - 4): no two leaves agree at any position, exact in bf16
    (i + 1 <= 81 < 2^8) and still exact after a scale of 1/2."""
    return [((i + 1) * 2.0 ** (torch.arange(n, dtype=F64) - 4)).to(dtype) for i, n in enumerate(group_lens(count))]


def mt_launches(numels):
    """(tensors, workgroups) of each launch ``for_each_group`` makes: empty leaves skipped, at most 40 per launch."""
    live = [n for n in numels if n > 0]
    return [(len(live[i:i + MT_MAXT]), sum(ceil_div(n, MT_CHUNK) for n in live[i:i + MT_MAXT]))
            for i in range(0, len(live), MT_MAXT)]


def mt_chunks(n, vector):
    """Per workgroup of a leaf of n elements: (full 8-vectors taken by the vector loop, scalar-tail elements)."""
    out = []
    for c in range(ceil_div(n, MT_CHUNK)):
        m = min(MT_CHUNK, n - c * MT_CHUNK)
        out.append((m // MT_VEC, m % MT_VEC) if vector else (0, m))
    return out


def trunc_to(x32, dtype):
    """fp32 -> bf16 / fp16 toward zero (a planted defect)."""
    r = x32.to(dtype)
    over = r.float().abs() > x32.abs()
    down = (bits_of(r) - 1).view(dtype)
    return torch.where(over, down, r)


def emu_copy(src_flat, src_buf, dst_flat, dst_buf, scale, defect=None):
    """The launches of mt_copy_kernel replayed over two ``Flat`` buffers, chunk by chunk (vector loop, then the
    scalar tail; the scalar loop when either side is unaligned), with one planted defect."""
    tout = dst_flat.dtype
    live = [i for i, n in enumerate(src_flat.numels) if n > 0]
    out = dst_buf.clone()
    for g0 in range(0, len(live), MT_MAXT):
        group = live[g0:g0 + MT_MAXT]
        for k, i in enumerate(group):
            n = src_flat.numels[i]
            s0, d0 = src_flat.starts[i], dst_flat.starts[i]
            vector = src_flat.aligned(i) and dst_flat.aligned(i)
            if defect == "leaf40_from_leaf0" and g0 > 0 and k == 0:
                s0 = src_flat.starts[live[0]]  # the second launch's first leaf reads the first launch's
            for c, (nvec, tail) in enumerate(mt_chunks(n, vector)):
                base = c * MT_CHUNK
                if defect == "start_off_by_chunk" and k == len(group) - 1 and c > 0:
                    base -= MT_CHUNK  # the last leaf's later workgroups land one chunk early
                lo, hi = base, base + nvec * MT_VEC + tail
                if defect == "drop_last_vector" and nvec > 0 and c == 0:
                    hi_v = base + (nvec - 1) * MT_VEC
                    x = src_buf[s0 + lo:s0 + hi_v]
                    out[d0 + lo:d0 + hi_v] = copy_ref(x, tout, scale)
                    lo = base + nvec * MT_VEC
                if defect == "drop_tail" and vector:
                    hi = base + nvec * MT_VEC
                if defect == "one_past_end" and base + MT_CHUNK >= n:
                    hi += 1
                x = src_buf[s0 + lo:s0 + hi]
                if defect == "scale_twice":
                    y = copy_ref(copy_ref(x, product_type(x.dtype, tout), scale), tout, scale)
                elif defect == "fp32_product":
                    y = (x.float() * torch.tensor(scale, dtype=F32)).to(tout)
                elif defect == "truncating_store":
                    y = trunc_to(x.float() * torch.tensor(scale, dtype=F32), tout)
                else:
                    y = copy_ref(x, tout, scale)
                out[d0 + lo:d0 + hi] = y
    return out


# =============================================================================== mt_sumsq

SUMSQ_FAMILIES = ("uniform", "huge", "tiny", "exact")
SUMSQ_DTYPES = (BF, HF, F32)


def sumsq_inputs(family, dtype, numels, seed=0):
    """Leaves of one family. tiny: squares near fp32's underflow (bf16 / fp32: |x| in 2^-63 .. 2^-60; fp16 has no
    such values: its subnormals). exact: integers in -3 .. 3 (sum x^2 <= 9 n < 2^24)."""
    g = _gen("sumsq", family, NAME[dtype], sum(numels), seed)
    n = sum(numels)
    if family == "uniform":
        v = torch.rand(n, generator=g) * 2 - 1
    elif family == "huge":
        v = torch.rand(n, generator=g) * 2 - 1
        v[(7 * n) // 11] = 30000.0
    elif family == "tiny":
        v = (torch.rand(n, generator=g) * 2 - 1) * (2.0 ** -14 if dtype == HF else 2.0 ** -60)
    elif family == "exact":
        v = (torch.randint(0, 7, (n,), generator=g) - 3).float()
    else:
        raise ValueError(family)
    return split(v.to(dtype), numels)


def sumsq_blocks(numels):
    return sum(ceil_div(n, MT_CHUNK) for n in numels)


def sumsq_L(numels):
    return 32 + 6 + 3 + sumsq_blocks(numels)


def sumsq_ref(leaves):
    return sum(float((t.double() ** 2).sum()) for t in leaves)


def sumsq_bound(ref, numels):
    return sumsq_L(numels) * E23 * ref + TINY


def _fma32(a, b, c):
    """fmaf on float32 tensors: the product of two fp32 values is exact in float64; one rounding to fp32 (the
    float64 addition before it can differ from the single rounding only in a tie's last place)."""
    return (a.double() * b.double() + c.double()).float()


def wave_sum_emulated(v):
    """wave_sum_dpp of common.h over the last axis (64 lanes) in fp32: quad_perm [1,0,3,2], [2,3,0,1], row_ror:4,
    row_ror:8 within 16-lane rows, then (row0 + row1) + (row2 + row3)."""
    lanes = torch.arange(64)
    row, l = lanes // 16 * 16, lanes % 16
    for src in (lanes ^ 1, lanes ^ 2, row + (l - 4) % 16, row + (l - 8) % 16):
        v = v + v[..., src]
    return (v[..., 0] + v[..., 16]) + (v[..., 32] + v[..., 48])


def emu_sumsq(leaves, aligned=True, defect=None):
    """mt_sumsq_kernel in fp32: every lane's fmas in its own order (vector loop k = 0 .. 3, j = 0 .. 7, then the
    tail; or the scalar loop), the wave tree, the four wave totals in order, the workgroups' atomics ascending."""
    out = torch.zeros((), dtype=F32)
    for t in leaves:
        n = t.numel()
        x = t.float()
        for c, (nvec, tail) in enumerate(mt_chunks(n, aligned)):
            base = c * MT_CHUNK
            m = nvec * MT_VEC + tail
            idx = torch.full((MT_THREADS, 64), -1, dtype=torch.int64)  # [lane, step] -> element of the chunk
            steps = 0
            if nvec:
                vv = torch.arange(nvec)
                if defect == "drop_last_vector":
                    vv = vv[:-1]
                lane, k = vv % MT_THREADS, vv // MT_THREADS
                for j in range(MT_VEC):
                    idx[lane, k * MT_VEC + j] = vv * MT_VEC + j
                steps = 32
            rest = torch.arange(nvec * MT_VEC, m)
            if defect == "drop_tail" and aligned:
                rest = rest[:0]
            if rest.numel():
                r = rest - nvec * MT_VEC
                idx[r % MT_THREADS, steps + r // MT_THREADS] = rest
            acc = torch.zeros(MT_THREADS, dtype=F32)
            xc = torch.cat([x[base:base + m], torch.zeros(1)])  # index -1: a zero term (acc unchanged)
            for s in range(64):
                col = idx[:, s]
                if bool((col >= 0).any()):
                    f = xc[col]
                    acc = _fma32(f, f, acc)
            w = wave_sum_emulated(acc.view(4, 64))
            s = torch.zeros((), dtype=F32)
            for k in range(4):
                s = s + w[k]
            out = out + s
    return out


# =============================================================================== gemm_splitk_reduce(_seg)

RED_GROUP, RED_THREADS, COL_V, COL_PH, COL_MAX_S = 16, 256, 8, 32, 2048
RED_FAMILIES = ("uniform", "cancel", "exact")
FINAL_CASES = [(S, n) for S in (1, 2, 5, 16) for n in (4, 36, 1, 6, 37)]
SUMALL_CASES = [(S, 1) for S in (17, 256, 257, 5000)]
COL_CASES = [(S, n) for S in (17, 32, 33, 128, 129, 2048) for n in (4, 28, 32, 36)]
TREE_CASES = [(S, n) for S in (17, 300) for n in (6, 37)] + [(S, n) for S in (2049, 5000) for n in (4, 36)]
TREE_BIG = (4100, 4 * 256 * 9)
SEG_CASES = [(4, 12), (12, 12), (12, 32), (12, 36), (16, 12), (16, 32), (16, 36), (16, 44)]  # (seg, n): <= 3 segments
SEG_S = (5, 33, 2049)  # final, column and tree path


def reduce_path(S, n):
    """The launcher's choice: ("final",), ("sumall",), ("col",) or ("tree", levels before the final kernel)."""
    cs = max(S, 1)
    if cs > RED_GROUP and n == 1:
        return ("sumall",)
    if RED_GROUP < cs <= COL_MAX_S and n % 4 == 0 and n > 0:
        return ("col",)
    levels = 0
    while cs > RED_GROUP:
        cs = ceil_div(cs, RED_GROUP)
        levels += 1
    return ("tree", levels) if levels else ("final",)


def reduce_tree_grid(S, n):
    """(gx, groups) of the first tree level: about 2048 workgroups in all."""
    groups = ceil_div(S, RED_GROUP)
    return max(1, min(ceil_div(n // 4, RED_THREADS), ceil_div(2048, groups))), groups


def reduce_inputs(family, S, n, bf16_out=False, seed=0):
    """fp32 partials [S, n]. cancel: rows in +- pairs plus 2^-10 noise. exact: ternary rows, non-zero on the lattice
    (s + 7 c) % m == 0 with m chosen so a column holds at most 200 non-zeros (sum |ws| <= 256 for a bf16 store)."""
    g = _gen("reduce", family, S, n, seed)
    if family == "uniform":
        return torch.rand(S, n, generator=g) * 2 - 1
    if family == "cancel":
        u = torch.rand(ceil_div(S, 2), n, generator=g) * 2 - 1
        w = torch.zeros(S, n)
        w[0::2] = u[:ceil_div(S, 2)]
        w[1::2] = -u[:S // 2]
        return w + 2.0 ** -10 * (torch.rand(S, n, generator=g) * 2 - 1)
    if family == "exact":
        m = ceil_div(S, 200)
        s, c = torch.arange(S).view(S, 1), torch.arange(n).view(1, n)
        sign = (torch.randint(0, 2, (S, n), generator=g) * 2 - 1).float()
        return torch.where((s + 7 * c) % m == 0, sign, torch.zeros(S, n))
    raise ValueError(family)


def reduce_ref(ws):
    wd = ws.double()
    return wd.sum(0), wd.abs().sum(0)


def reduce_bound(r, a, S, tout):
    return S * E23 * a + UT[tout] * r.abs() + TINY


def _seq_sum(rows):
    """rows[0] + rows[1] + ... in fp32, in order."""
    acc = rows[0].clone()
    for i in range(1, rows.shape[0]):
        acc = acc + rows[i]
    return acc


def emu_reduce(ws, tout, defect=None):
    """The path ``reduce_path`` names, in fp32 and in the kernel's order; rounded to ``tout``."""
    S, n = ws.shape
    path = reduce_path(S, n)
    if path[0] == "sumall":
        col = ws[:, 0]
        pad = torch.cat([col, torch.zeros(ceil_div(S, RED_THREADS) * RED_THREADS - S)]).view(-1, RED_THREADS)
        acc = _seq_sum(torch.cat([torch.zeros(1, RED_THREADS), pad]))  # lane t: ws[t], ws[t + 256], ...
        w = wave_sum_emulated(acc.view(4, 64))
        return _seq_sum(torch.cat([torch.zeros(1), w]).view(5, 1)).to(tout)
    if path[0] == "col":
        acc = torch.zeros(COL_PH, n)
        for ph in range(COL_PH):
            rows = ws[ph::COL_PH]
            if defect == "skip_unroll_row" and ph == 0 and rows.shape[0] > 4:
                rows = torch.cat([rows[:4], rows[5:]])  # the row after the 4-row unroll is lost (S = 129: row 128)
            if rows.shape[0]:
                acc[ph] = _seq_sum(torch.cat([torch.zeros(1, n), rows]))
        w = COL_PH // 2
        while w:
            acc[:w] = acc[:w] + acc[w:2 * w]
            w //= 2
        out = acc[0].clone()
        if defect == "clamped_column_stored" and n >= 8:  # a clamped lane's copy of the last float4 lands on its neighbour
            out[-8:-4] = out[-4:]
        return out.to(tout)
    cur = ws
    while cur.shape[0] > RED_GROUP:
        groups = ceil_div(cur.shape[0], RED_GROUP)
        nxt = torch.stack([_seq_sum(cur[g * RED_GROUP:(g + 1) * RED_GROUP]) for g in range(groups)])
        if defect == "last_group_twice":
            nxt[-1] = nxt[-1] + _seq_sum(cur[(groups - 1) * RED_GROUP:])
            defect = None
        cur = nxt
    return _seq_sum(cur).to(tout)


def seg_split(row, seg):
    """The reduced row cut into the <= 3 outputs of ``gemm_splitk_reduce_seg``."""
    return [row[k * seg:min((k + 1) * seg, row.numel())] for k in range(ceil_div(row.numel(), seg))]


# =============================================================================== colsum

COLSUM_N = (8, 24, 512, 2048, 2056, 8192)
COLSUM_DTYPES = (BF, HF, F32)
COLSUM_FAMILIES = ("uniform", "ternary")


def colsum_geometry(N):
    """(V, R, threads) of colsum's launch."""
    V = N // 8
    R = max(1, 256 // V)
    return V, R, V * R


def colsum_rows(N):
    R = colsum_geometry(N)[1]
    return sorted({r for r in (1, 3, R - 1, R, 4 * R, 4 * R + 1, 1000) if r >= 1})


def colsum_blocks_ref(rows):
    return max(1, min(1024, rows // 64))


def gelu_blocks_ref(rows):
    return max(1, min(1024, rows // 32))


def colsum_block_choices(rows, auto):
    return sorted({1, 2, auto, rows + 3})


def colsum_inputs(family, rows, N, dtype, seed=0):
    g = _gen("colsum", family, rows, N, seed)
    if family == "uniform":
        return (torch.rand(rows, N, generator=g) * 2 - 1).to(dtype)
    return (torch.randint(0, 3, (rows, N), generator=g) - 1).float().to(dtype)  # |sum| <= rows <= 1024 < 2^24


def block_ranges(rows, blocks, floor=False):
    """Rows [b rpw, min((b + 1) rpw, rows)) of each workgroup, rpw = ceil(rows / blocks) (``floor``: a defect)."""
    rpw = max(1, rows // blocks) if floor else ceil_div(rows, blocks)
    return rpw, [(min(b * rpw, rows), min((b + 1) * rpw, rows)) for b in range(blocks)]


def range_sums(x, ranges):
    """float64 (sum, sum |.|) of the rows of each range: [blocks, N] each."""
    xd = x.double()
    out = torch.zeros(2, len(ranges), x.shape[1], dtype=F64)
    for b, (lo, hi) in enumerate(ranges):  # each range summed on its own: a difference of prefix sums would cancel
        if hi > lo:
            out[0, b], out[1, b] = xd[lo:hi].sum(0), xd[lo:hi].abs().sum(0)
    return out[0], out[1]


def check_partials(key, name, part, x, blocks, exact, errs, floor=False):
    """Each workgroup's partial row against the float64 sum over its own rows (empty workgroups: EQUAL 0)."""
    rpw, ranges = block_ranges(x.shape[0], blocks, floor)
    ref, mag = range_sums(x, ranges)
    if exact:
        assert float(mag.max()) < 2 ** 24
        E.check(f"{name} partials", part, ref, None, errs)
        return
    check(key, f"{name} partials", part, ref, rpw * E23 * mag + TINY, errs)
    empty = torch.tensor([lo >= hi for lo, hi in ranges])
    if bool(empty.any()):
        E.check(f"{name} empty workgroups", part[empty], torch.zeros_like(ref[empty]), None, errs)


def emu_colsum(x, blocks, defect=None):
    """colsum_kernel in fp32: lane (cv, ph) adds rows r0 + ph, r0 + ph + R, ... in order, then the phases 0 .. R - 1
    are added in order from zero."""
    rows, N = x.shape
    R = colsum_geometry(N)[1]
    rpw, ranges = block_ranges(rows, blocks, floor=defect == "rpw_floor")
    xf = x.float()
    out = torch.zeros(blocks, N)
    for b, (lo, hi) in enumerate(ranges):
        s = torch.zeros(N)
        for ph in range(R - 1 if defect == "drop_last_phase" else R):
            seg = xf[lo + ph:hi:R]
            if seg.shape[0]:
                s = s + _seq_sum(torch.cat([torch.zeros(1, N), seg]))
        out[b] = s
    return out


# =============================================================================== gelu_fwd / gelu_bwd_bias

FORMS = ("tanh", "erf")
GELU_DTYPES = (BF, HF)
# measured on the CPU from mfma_edges.gelu_emulated over every finite input of the type against float64
# (test_gelu_constants_cpu keeps them): the fp16 store of g, ratio to u_T |g| + 2^-24; the unrounded fp32
# derivative, ratio to 2^-23 (|d| + 1), the larger of the bf16 and the fp16 input sets. c = ceil(2 ratio): the
# device's exp2 / rcp are 1 ulp where the emulation's are correctly rounded.
GELU_RATIO = {("tanh", "g16"): 6.087, ("erf", "g16"): 1.179, ("tanh", "d32"): 16.409, ("erf", "d32"): 1.634}
GELU_C = {("tanh", "g16"): 13, ("erf", "g16"): 3, ("tanh", "d32"): 33, ("erf", "d32"): 4}
GELU_FWD_VECS = (1, 255, 256, 257, 1023, 1024, 1025)
GELU_FWD_BIG = 8 * (4 * 4096 * 256 + 1)
GELU_BWD_N = (512, 1024, 8192)
GELU_BWD_ROWS = (1, 3, 4, 5, 37, 130)


def all_finite_f16():
    """All 65536 fp16 bit patterns as a [256, 256] matrix, the 2048 non-finite ones replaced by the pattern with the
    exponent field lowered by one (63488 distinct finite patterns), as ``mfma_edges.all_finite_bf16``."""
    bits = torch.arange(65536, dtype=torch.int64)
    bits = torch.where((bits >> 10) & 0x1F == 0x1F, bits - 1024, bits)
    bits = torch.where(bits >= 32768, bits - 65536, bits).to(torch.int16)
    return bits.view(HF).reshape(256, 256)


def all_finite(dtype):
    return E.all_finite_bf16() if dtype == BF else all_finite_f16()


def gelu_bound_t(ref, c, dtype):
    """``mfma_edges.gelu_bound`` with the store's unit roundoff (2^-24 is fp16's smallest subnormal, twice SUB)."""
    return c * (UT[dtype] * ref.abs() + 2.0 ** -24)


def gelu_fwd_geometry(nvec):
    """(workgroups, unrolled iterations of lane 0, tail iterations of lane 0) of gelu_fwd's grid-stride loop."""
    blocks = min(4096, ceil_div(nvec, 1024))
    stride = blocks * 256
    v, unrolled = 0, 0
    while v + 3 * stride < nvec:
        v += 4 * stride
        unrolled += 1
    return blocks, unrolled, ceil_div(max(0, nvec - v), stride)


def gelu_bwd_h(rows, N, dtype):
    """h [rows, N] cycling through every finite pattern of the type, the cycle starting where the shape's hash
    falls (N = 8192 covers all 65536 within 8 rows)."""
    pat = all_finite(dtype).reshape(-1)
    i = (torch.arange(rows * N) * 1 + 8192 * (rows % 8)) % 65536
    return pat[i].reshape(rows, N)


def gelu_bwd_dy(family, rows, N, dtype, seed=0):
    g = _gen("gelu_dy", family, rows, N, seed)
    if family == "uniform":
        return (torch.rand(rows, N, generator=g) * 2 - 1).to(dtype)
    if family == "pow2":
        return ((torch.randint(0, 2, (rows, N), generator=g) * 2 - 1) * 2.0 ** torch.randint(-8, 5, (rows, N), generator=g)).to(dtype)
    if family == "exact":
        return (torch.randint(0, 9, (rows, N), generator=g) - 4).float().to(dtype)
    raise ValueError(family)


def gelu_exact_h(rows, N, dtype):
    return (64.0 * ((torch.arange(rows * N) * 7 // 3) % 2 * 2 - 1)).to(dtype).reshape(rows, N)


def gelu_dh_bound(dy, d, form, dtype):
    dyd = dy.double()
    return dyd.abs() * GELU_C[form, "d32"] * E23 * (d.abs() + 1) + UT[dtype] * (dyd * d).abs() + SUB[dtype] + TINY


def emu_gelu_bwd(dy, h, form, blocks, defect=None):
    """(dh, partials) of gelu_bwd_bias_kernel in fp32: gelu' unrounded, one rounding of the product, the rounded dh
    summed per column over the workgroup's rows in order."""
    dt = h.dtype
    use = {"tanh": "erf", "erf": "tanh"}[form] if defect == "form_swapped" else form
    d = E.gelu_emulated(h, use, dtype=None)[1]
    if defect == "derivative_rounded":
        d = d.to(dt).float()
    prod = dy.float() * d
    dh = prod.to(dt)
    summed = prod if defect == "db_from_unrounded" else dh.float()
    _, ranges = block_ranges(h.shape[0], blocks)
    part = torch.zeros(blocks, h.shape[1])
    for b, (lo, hi) in enumerate(ranges):
        if hi > lo:
            part[b] = _seq_sum(torch.cat([torch.zeros(1, h.shape[1]), summed[lo:hi]]))
    return dh, part


# =============================================================================== transposes

XPOSE_SHAPES = [(8, 8), (8, 72), (72, 8), (64, 64), (72, 136), (200, 40)]
FILTER_SHAPES = [(64, 64), (8, 8), (24, 40), (3, 5), (65, 7), (136, 200)]
FILTER_TAPS = (1, 3, 9)


def filters_ref(w, defect=None):
    """out[ci][t][co] = in[co][T - 1 - t][ci]."""
    if defect == "no_tap_flip":
        return w.permute(2, 1, 0).contiguous()
    if defect == "tiles_swapped":  # the 64 x 64 tile (bco, bci) written where (bci, bco) belongs
        out = w.flip(1).permute(2, 1, 0).contiguous()
        co, ci = w.shape[0], w.shape[2]
        k = min(co, ci, 128) // 2
        if k:
            a, b = out[:k, :, k:2 * k].clone(), out[k:2 * k, :, :k].clone()
            out[:k, :, k:2 * k], out[k:2 * k, :, :k] = b, a
        return out
    return w.flip(1).permute(2, 1, 0).contiguous()


def filter_runs(co, ci):
    """Of xpose_taps_kernel's 16-element runs, per tap: (vector reads, scalar reads, vector writes, scalar writes)
    over the lanes with something in range."""
    def count(rows, width):  # rows x ceil(width / 64) tiles x 4 runs
        vec = sca = 0
        for t in range(ceil_div(width, 64)):
            for c0 in range(0, 64, 16):
                lo = t * 64 + c0
                if lo >= width:
                    continue
                if lo + 16 <= width and width % 8 == 0:
                    vec += rows
                else:
                    sca += rows
        return vec, sca
    return count(co, ci) + count(ci, co)


def filter_tiles(shapes):
    """Launches of transpose_filters: 40 filters each, (filters, tiles)."""
    out = []
    for i in range(0, len(shapes), 40):
        part = shapes[i:i + 40]
        out.append((len(part), sum(t * ceil_div(co, 64) * ceil_div(ci, 64) for co, ci, t in part)))
    return out


def many_filters(count):
    """``count`` filters, each of its own shape (the middle one empty: co = 0) and its own patterns."""
    shapes = [(8 * (1 + i % 3) + (i % 2), 8 * (1 + i % 4) - (i % 3 == 0), (1, 3, 9)[i % 3]) for i in range(count)]
    shapes[count // 2] = (0, 16, 3)
    ws = []
    for i, (co, ci, t) in enumerate(shapes):
        n = co * t * ci
        ws.append(E.patterns(n + 977 * i)[977 * i:].reshape(co, t, ci) if n else torch.zeros(0, t, ci, dtype=BF))
    return shapes, ws
