"""The native launches of the ResNet path's host layer (``scripts/launch_trace.py``) against the recorded golden:
which entries run, in what order, with which scalars, null pointers and dataflow links. The golden was recorded at
the commit before the launch helpers of ``ops/batchnorm.py`` / ``ops/_launch.py`` existed; a change of host code
that changes a launch on purpose re-records it (``python scripts/launch_trace.py --out
tests/golden/resnet_launch_trace.json``) and says so."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _script():
    spec = importlib.util.spec_from_file_location("launch_trace", os.path.join(ROOT, "scripts", "launch_trace.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_launch_trace_matches_golden(gpu_ext):
    lt = _script()
    path = os.path.join(ROOT, "tests", "golden", "resnet_launch_trace.json")
    with open(path) as f:
        text = f.read()
    golden = json.loads(text)
    got = lt.trace_all()
    assert list(got) == list(golden)  # every case, in order
    for case in golden:
        assert got[case] == golden[case], case
    assert lt.dumps(got) == text  # byte for byte
    # slabs = ceil(392 / 32) = 13 workgroups: below any CU count, so nothing recorded depends on it
    assert any("True,False,4,13," in r for r in golden["a/hybrid"])
