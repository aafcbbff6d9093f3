"""The fused optimiser kernels (``optim.hip``, ``optim_rules.hip``, ``optim_layerwise.hip``) against
float64 references with derived per-element bounds, exact cases and path-independence checks, for all
15 rules and all 11 dtype combinations. ``optim_edges`` holds the inputs, references, bounds, emulations
and planted defects (its docstring derives every bound); this file drives them.

GPU tests (marked ``gpu``):
  bounds   every rule x combination x input family (uniform, first_step, t1000, tiny, big_x, clipped) over
           the 30 leaves of ``SIZES``, two steps, the second from what the device stored after the first.
           Every case prints its worst observed error as a fraction of its bound.
  exact    dyadic cases, bitwise against the float64 closed form: one per rule, zeros, Lion's tie, a NaN
           and a +inf gradient.
  paths    each operand alone misaligned; 30 leaves in one call == 30 calls == reversed order; the device
           blocks against the host arguments.
CPU tests (``*_cpu``) keep the GPU tests honest: the project's CPU optimiser paths meet every bound and
every exact case, each planted defect breaks one, and Lion's undecided share and the clamp share stay
inside their caps for the reference alone.
"""
import pytest
import torch

from . import optim_edges as O
from .optim_edges import COMBOS, F32, F64, LAYERWISE, PATH_COMBOS, RULES, combo_id
from .test_clip_gpu import SIZES, UNALIGNED
from .test_rules_gpu import CANARY, Guarded

gpu = pytest.mark.gpu
RC = [pytest.param(r, c, id=f"{r}-{combo_id(c)}") for r in RULES for c in COMBOS]
RP = [pytest.param(r, c, id=f"{r}-{combo_id(c)}") for r in RULES for c in PATH_COMBOS]
BLOCK_BITWISE = ("lion", "rmsprop", "adagrad", "amsgrad", "adadelta", "descent", "momentum", "nesterov")


# ------------------------------------------------------------------------------------ runners

def run_gpu(case, combo, inp, offset=None):
    """One step of the kernels on guarded device copies of ``inp``; ``offset``: the one operand ("p", "g",
    "st0".., "w") whose every leaf starts one element into its buffer. Returns the stored outputs."""
    pd, gd, sd, master = combo
    n = len(inp["p"])
    off = lambda name: tuple(range(n)) if offset == name else ()
    P, G = Guarded(inp["p"], pd, off("p")), Guarded(inp["g"], gd, off("g"))
    S = [Guarded(s, sd, off(f"st{k}")) for k, s in enumerate(inp["st"])]
    W = Guarded(inp["w"], F32, off("w")) if master else None
    table = work = None
    need = 0
    if case["rule"] in LAYERWISE:
        ct = O.ct_of(pd)
        need = 2 * sum((t.numel() + 4095) // 4096 for t in inp["p"])
        work = torch.full((need + 8,), CANARY, dtype=ct, device="cuda")
        table = torch.full((n + 8,), CANARY, dtype=ct, device="cuda")
    O.call(case, P.views, G.views, [s.views for s in S], W.views if master else None,
           ratios=table[:n] if table is not None else None, workspace=work[:need] if work is not None else None)
    torch.cuda.synchronize()
    for guard in [P, G, *S] + ([W] if master else []):
        guard.check()
    if table is not None:
        assert bool((work[need:] == CANARY).all()) and bool((table[n:] == CANARY).all()), "write past a table"
    cpu = lambda guard: [v.cpu().clone() for v in guard.views]
    return {"p": cpu(P), "g": cpu(G), "st": [cpu(s) for s in S], "w": cpu(W) if master else None,
            "q": table[:n].cpu().clone() if table is not None else None}


def _all_tensors(out):
    ts = [*out["p"], *(t for s in out["st"] for t in s), *(out["w"] or [])]
    return ts + ([out["q"]] if out["q"] is not None else [])


def _same_bits(a, b):
    return all(torch.equal(x, y) or bool(((x == y) | (x.isnan() & y.isnan())).all()) for x, y in
               zip(_all_tensors(a), _all_tensors(b)))


def _bounds(run, rule, combo, families=O.FAMILIES):
    """Two steps of every family through ``run``; prints the fractions, returns (violations, worst)."""
    msgs, worst = [], 0.0
    for fam in families:
        case, inp = O.family_case(rule, fam, combo, SIZES)
        for step in (1, 2):
            out = run(case, combo, inp)
            fr, m, info = O.check(case, combo, inp, out)
            shown = " ".join(f"{k}={v:.3f}" for k, v in fr.items())
            print(f"{rule} {combo_id(combo)} {fam} step {step}: {shown}"
                  + (f" undecided={info['undecided']:.2e}" if rule == "lion" else ""))
            msgs += [f"{fam} step {step}: {x}" for x in m]
            worst = max([worst, *fr.values()])
            case, inp = O.next_step(case, out)
    print(f"WORST {rule} {combo_id(combo)} {worst:.3f}")
    return msgs, worst


def _exact_kinds(rule):
    return ["main", "zeros"] + (["tie"] if rule == "lion" else []) + ([] if rule in LAYERWISE else ["nonfinite"])


def _exact(run, rule, combo):
    msgs = []
    outs = {}
    for kind in _exact_kinds(rule):
        case, inp = O.exact_case(rule, kind, combo)
        out = outs[kind] = run(case, combo, inp)
        msgs += [f"exact {kind}: {x}" for x in O.check_exact(case, combo, inp, out)]
        x_in, x_out = (inp["w"], out["w"]) if combo[3] else (inp["p"], out["p"])
        if kind == "tie":  # sign(0) = 0: x keeps its bits while m moves
            if not all(torch.equal(a, b) for a, b in zip(x_in, x_out)) or not all(torch.equal(a, b) for a, b in
                                                                              zip(inp["p"], out["p"])):
                msgs.append("exact tie: x changed")
            if any(torch.equal(a, b) for a, b in zip(inp["st"][0], out["st"][0])):
                msgs.append("exact tie: m did not move")
        if kind == "zeros" and not all(bool(torch.isfinite(t).all()) for t in _all_tensors(out)):
            msgs.append("exact zeros: a non-finite value")
        if kind == "nonfinite":  # the two poisoned elements, and nothing else, differ from the clean run
            i = O.EXACT_SIZES.index(24)
            for name, a, b in [("x", x_out, outs["main"]["w" if combo[3] else "p"])] + \
                    [(f"state{k}", s, outs["main"]["st"][k]) for k, s in enumerate(out["st"])]:
                hit = torch.zeros(24, dtype=torch.bool)
                hit[3] = hit[12] = True
                if not torch.equal(a[i][~hit], b[i][~hit]) or not all(torch.equal(a[j], b[j]) for j in range(len(a))
                                                                     if j != i):
                    msgs.append(f"exact nonfinite: {name}: a neighbour of a poisoned element changed")
                # (Lion's +inf gradient has a sign: its x stays finite while m becomes inf)
                if name == "x" and not (bool(a[i][3].isnan()) and (rule == "lion" or not bool(a[i][12].isfinite()))):
                    msgs.append("exact nonfinite: x stayed finite under a NaN / inf gradient")
    return msgs


# ------------------------------------------------------------------------------------ GPU: bounds and exact cases

@gpu
@pytest.mark.parametrize("rule,combo", RC)
def test_bounds_gpu(gpu_ext, rule, combo):
    msgs, worst = _bounds(run_gpu, rule, combo)
    assert not msgs, "\n".join(msgs)
    assert worst <= 1


@gpu
@pytest.mark.parametrize("rule,combo", RC)
def test_exact_gpu(gpu_ext, rule, combo):
    msgs = _exact(run_gpu, rule, combo)
    assert not msgs, "\n".join(msgs)


# ------------------------------------------------------------------------------------ GPU: path independence

@gpu
@pytest.mark.parametrize("rule,combo", RP)
def test_alignment_gpu(gpu_ext, rule, combo):
    """Each operand alone one element into its buffer (any one forces the scalar path): the bits of the
    aligned run, canaries intact (``run_gpu`` checks them)."""
    case, inp = O.family_case(rule, "clipped", combo, SIZES)
    base = run_gpu(case, combo, inp)
    names = ["p", "g"] + [f"st{k}" for k in range(len(inp["st"]))] + (["w"] if combo[3] else [])
    for name in names:
        assert _same_bits(base, run_gpu(case, combo, inp, offset=name)), f"{name} misaligned: other bits"


@gpu
@pytest.mark.parametrize("rule,combo", RP)
def test_grouping_gpu(gpu_ext, rule, combo):
    """The 30-leaf call (two launches) == 30 calls of one leaf == the leaves in reverse order, the ratio
    table of LARS / LAMB included."""
    case, inp = O.family_case(rule, "clipped", combo, SIZES)
    base = run_gpu(case, combo, inp)
    n = len(SIZES)
    sub = lambda ii: ({**case, "ts": None if case["ts"] is None else case["ts"][ii]},
                      {"p": [inp["p"][i] for i in ii], "g": [inp["g"][i] for i in ii],
                       "st": [[s[i] for i in ii] for s in inp["st"]],
                       "w": [inp["w"][i] for i in ii] if inp["w"] is not None else None})
    rev = list(range(n))[::-1]
    c, flipped = sub(rev)
    out = run_gpu(c, combo, flipped)
    back = {"p": out["p"][::-1], "st": [s[::-1] for s in out["st"]], "w": out["w"][::-1] if out["w"] else None,
            "q": out["q"].flip(0) if out["q"] is not None else None}
    assert _same_bits(base, back), "reverse order: other bits"
    for i in range(n):
        c, one = sub([i])
        out = run_gpu(c, combo, one)
        got = _all_tensors(out)
        want = [base["p"][i], *(s[i] for s in base["st"]), *([base["w"][i]] if base["w"] else []),
                *([base["q"][i:i + 1]] if base["q"] is not None else [])]
        assert all(torch.equal(a, b) for a, b in zip(got, want)), f"leaf {i} alone: other bits"


@gpu
@pytest.mark.parametrize("rule,combo", RP)
def test_device_blocks_gpu(gpu_ext, rule, combo):
    """A ``dev_hyper`` / ``dev_lr`` run meets the bound of the reference evaluated at the block's fp32
    contents, and is the host run bit for bit where the host values are fp32 numbers and the rule reads
    no ``1 - beta^t``."""
    case, inp = O.family_case(rule, "uniform", combo, SIZES)
    case["dev"] = True
    out = run_gpu(case, combo, inp)
    fr, msgs, _ = O.check(case, combo, inp, out)
    print(f"{rule} {combo_id(combo)} dev block: " + " ".join(f"{k}={v:.3f}" for k, v in fr.items()))
    assert not msgs, "\n".join(msgs)
    if rule in BLOCK_BITWISE:
        case["lr"] = 2.0 ** -10
        dev = run_gpu(case, combo, inp)
        host = run_gpu({**case, "dev": False}, combo, inp)
        assert _same_bits(dev, host), "device block: other bits than the host arguments"


# ------------------------------------------------------------------------------------ CPU

def test_combos_are_the_supported_set_cpu():
    from fluxmpi_amd.ops import optim
    assert set(COMBOS) == optim._SUPPORTED and len(COMBOS) == 11 and len(RULES) == 15
    assert len(SIZES) == 30 and SIZES[UNALIGNED] == 5000 and 4097 in SIZES and 0 in SIZES


@pytest.mark.parametrize("rule,combo", RC)
def test_emulation_meets_bounds_cpu(rule, combo):
    """The project's CPU optimiser paths, fed the same stored inputs, meet every bound and exact case."""
    msgs, worst = _bounds(O.run_cpu, rule, combo)
    msgs += _exact(O.run_cpu, rule, combo)
    assert not msgs, "\n".join(msgs)
    assert worst <= 1


@pytest.mark.parametrize("rule,combo", RC)
def test_own_emulation_meets_bounds_cpu(rule, combo):
    """The helper's fp32 evaluation of the program (what the defects are planted in) is clean itself."""
    run = lambda case, c, inp: O.emulate(case, c, inp)
    msgs, _ = _bounds(run, rule, combo, families=("uniform", "tiny"))
    msgs += _exact(run, rule, combo)
    assert not msgs, "\n".join(msgs)


@pytest.mark.parametrize("defect", sorted(O.DEFECTS))
def test_planted_defect_fails_cpu(defect):
    """Each defect, planted in the emulation, breaks a bound or an exact case in the family named in
    ``optim_edges.DEFECTS``; the emulation without it passes the same case."""
    rule, combo, fam = O.DEFECTS[defect]
    if fam.startswith("exact:"):
        case, inp = O.exact_case(rule, fam[6:], combo)
        judge = lambda out: O.check_exact(case, combo, inp, out)
    else:
        case, inp = O.family_case(rule, fam, combo, SIZES)
        judge = lambda out: O.check(case, combo, inp, out)[1]
    assert not judge(O.emulate(case, combo, inp)), "the clean emulation fails"
    msgs = judge(O.emulate(case, combo, inp, defect))
    print(defect, "->", msgs)
    assert msgs, f"{defect} goes unnoticed in {rule} {combo_id(combo)} {fam}"


@pytest.mark.parametrize("combo", COMBOS, ids=combo_id)
def test_lion_undecided_within_cap_cpu(combo):
    for fam in O.FAMILIES:
        case, inp = O.family_case("lion", fam, combo, SIZES)
        A = O.Tracked(2.0 ** -53 if combo[0] == F64 else 2.0 ** -24)
        O._step(A, case, combo, inp)
        share = float(A.undecided.double().mean())
        print(f"lion {combo_id(combo)} {fam}: undecided {share:.2e}")
        assert share <= O.UNDECIDED_CAP


@pytest.mark.parametrize("combo", COMBOS, ids=combo_id)
def test_clamp_share_cpu(combo):
    for rule in ("adam", "momentum", "lion"):
        case, inp = O.family_case(rule, "clipped", combo, SIZES)
        shares = O.clamp_share(case, inp, SIZES)
        print(f"{rule} {combo_id(combo)}: clamp share per leaf scale {[round(s, 3) for s in shares]}")
        assert all(O.CLAMP_SHARE[0] <= s <= O.CLAMP_SHARE[1] for s in shares)


@pytest.mark.parametrize("rule", RULES)
def test_exact_cases_are_exact_cpu(rule):
    """Every value of the float64 closed form of an exact case is an fp32 number: contraction and the
    order of evaluation cannot matter."""
    for kind in _exact_kinds(rule):
        case, inp = O.exact_case(rule, kind, COMBOS[0])
        r = O.closed_form(case, COMBOS[0], inp)
        for t in [r["x"], *r["st"]] + ([r["q"]] if "q" in r else []):
            ok = (t.float().double() == t) | t.isnan()
            assert bool(ok.all()), f"{rule} {kind}"
