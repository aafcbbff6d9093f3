"""The Python-visible surface of ``fluxmpi_amd._C`` against a recorded golden.

For every attribute of the module and every method of ``RcclComm``: name, number of parameters,
parameter names (``None`` where the binding names none), default values, and whether it returns
``None``, all parsed from the signature line pybind11 writes into the docstring (types are not
compared, so a change of pybind's wording does not matter).
``python -m tests.test_bindings_surface`` prints the surface of the built library in that format.

The rule: add entries, or trailing parameters with defaults, freely and re-record
``tests/golden/c_api_surface.json``. Never edit ``c_api_surface_base.json``: anything
``test_golden_extends_base`` rejects (a name gone, a parameter renamed, reordered or without its
default, a new parameter a caller has to pass) breaks callers and needs its own justification.
"""
import json
import os
import re

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "c_api_surface.json")
BASE = os.path.join(os.path.dirname(GOLDEN), "c_api_surface_base.json")
# entries that began in modules of their own beside ``_C``
MOVED_IN = ("mt_check_finite", "loss_scale_update", "mt_ema", "ema_advance", "mt_stochastic_round", "sr_advance",
            "conv3ds_bwd", "bn_relu_conv1x1_fwd_supported", "bn_relu_conv1x1_fwd", "augment_batch", "aug_block_set")
# base functions that have grown trailing defaulted parameters (loss scaling, stochastic rounding)
EXTENDED = ("adam_advance", "clip_total", "mt_adam", "mt_leaf_sumsq", "mt_rule", "mt_sgd")


def _split_top(s: str) -> list[str]:
    """Split on commas outside brackets."""
    out, depth, cur = [], 0, ""
    for ch in s:
        depth += ch in "[(" and 1 or ch in "])" and -1 or 0
        if ch == "," and depth == 0:
            out.append(cur.strip())
            cur = ""
        else:
            cur += ch
    if cur.strip():
        out.append(cur.strip())
    return out


def _signature(name: str, doc: str | None):
    m = re.match(r"\s*(\w+)\((.*)\) -> (.+)", (doc or "").splitlines()[0] if doc else "")
    if not m:
        return {"kind": "other"}
    params = []
    for p in _split_top(m.group(2)):
        if p in ("/", "*"):
            continue
        pname, _, rest = p.partition(":")
        default = rest.partition(" = ")[2] if " = " in rest else None
        pname = pname.strip()
        params.append({"name": None if re.fullmatch(r"arg\d+", pname) else pname, "default": default})
    return {"kind": "function", "nparams": len(params), "params": params, "returns_none": m.group(3).strip() == "None"}


def surface(C) -> dict:
    out = {}
    for name in sorted(n for n in dir(C) if not n.startswith("__")):
        obj = getattr(C, name)
        if isinstance(obj, type):
            members = {}
            for mn in sorted(n for n in vars(obj) if not n.startswith("__") or n == "__init__"):
                mem = vars(obj)[mn]
                if isinstance(mem, property):
                    members[mn] = {"kind": "property", "settable": mem.fset is not None}
                else:
                    members[mn] = _signature(mn, getattr(getattr(obj, mn), "__doc__", None))
                    members[mn]["static"] = isinstance(mem, staticmethod)
            out[name] = {"kind": "class", "members": members}
        else:
            out[name] = _signature(name, getattr(obj, "__doc__", None))
    return out


def _load():
    try:
        import fluxmpi_amd._C as C
    except ImportError:
        return None
    return C


def test_bindings_surface_matches_golden():
    C = _load()
    if C is None:
        pytest.skip("fluxmpi_amd._C is not built")
    with open(GOLDEN) as f:
        golden = json.load(f)
    got = surface(C)
    assert sorted(got) == sorted(golden), (sorted(set(got) ^ set(golden)))
    for name in golden:
        assert got[name] == golden[name], name


def test_golden_extends_base():
    """The recorded surface is a compatible superset of the base: every call the base allowed still binds."""
    with open(GOLDEN) as f:
        new = json.load(f)
    with open(BASE) as f:
        base = json.load(f)
    assert len(base) == 90 and len(new) == 101
    assert not set(MOVED_IN) - set(new), sorted(set(MOVED_IN) - set(new))
    differ = []
    for name, old in base.items():
        assert name in new, name
        got = new[name]
        if old["kind"] != "function":  # a class, or "other"
            assert got == old, name
            continue
        assert got["kind"] == "function" and got["returns_none"] == old["returns_none"], name
        assert got["nparams"] >= old["nparams"] == len(old["params"]) and got["nparams"] == len(got["params"]), name
        for i, (po, pn) in enumerate(zip(old["params"], got["params"])):
            assert pn["default"] == po["default"], (name, i)
            assert po["name"] is None or pn["name"] == po["name"], (name, i)
        for i, pn in enumerate(got["params"][old["nparams"]:], old["nparams"]):
            assert pn["default"] is not None, (name, i)
        if got != old:
            differ.append(name)
    assert sorted(differ) == sorted(EXTENDED)


if __name__ == "__main__":
    print(json.dumps(surface(_load()), indent=1, sort_keys=True))
