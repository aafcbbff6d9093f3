"""The recorder of ``scripts/launch_trace.py`` on a fake extension module: address numbering, lists, restore."""
import importlib.util
import os
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lt():
    spec = importlib.util.spec_from_file_location("launch_trace", os.path.join(ROOT, "scripts", "launch_trace.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _fake():
    calls = []
    mod = types.SimpleNamespace(launch=lambda *a, **k: calls.append(("launch", a, k)) or 7, version="1.0")
    mod.conv3ds_bwd = lambda *a: calls.append(("c3ds", a, {}))
    ext = types.SimpleNamespace(get=lambda required=True: mod)
    return ext, mod, calls


def test_addresses_are_numbered_by_first_appearance(lt):
    ext, _, calls = _fake()
    a, b, c = (1 << 40) + 512, (1 << 41), (1 << 40)
    rec = lt.Recorder()
    with lt.recording(rec, ext, vendor=False):
        C = ext.get(required=True)
        assert C.launch(b, a, 0, 392, 1e-5, True, None, (1 << 40) - 1) == 7  # forwarded, result handed back
        C.launch(a, c, b, flag=a)
        ext.get().conv3ds_bwd(c, 13)
        assert C.version == "1.0" and not hasattr(C, "missing")  # non-callables and hasattr pass through
    assert rec.records == ["launch(a0,a1,0,392,1e-05,True,None,%d)" % ((1 << 40) - 1),
                           "launch(a1,a2,a0,flag=a1)",
                           "conv3ds_bwd(a2,13)"]
    assert [c[0] for c in calls] == ["launch", "launch", "c3ds"] and calls[0][1][0] == b
    assert all(c.startswith("test_launch_trace.py:") for c in rec.callers)


def test_lists_go_element_by_element(lt):
    ext, _, _ = _fake()
    a, b = (1 << 44), (1 << 44) + 64
    rec = lt.Recorder()
    with lt.recording(rec, ext, vendor=False):
        ext.get().launch([a, 0, b], [64, 256], [[b], a], "x")
    assert rec.records == ["launch([a0,0,a1],[64,256],[[a1],a0],'x')"]


def test_originals_are_restored(lt):
    ext, mod, _ = _fake()
    get = ext.get
    with pytest.raises(ZeroDivisionError):
        with lt.recording(lt.Recorder(), ext, vendor=False):
            assert ext.get is not get and ext.get() is not mod
            1 / 0
    assert ext.get is get and ext.get() is mod


def test_vendor_calls_are_restored(lt):
    import torch
    ext, _, _ = _fake()
    conv2d, bwd = torch.nn.functional.conv2d, torch.ops.aten.convolution_backward
    rec = lt.Recorder()
    with lt.recording(rec, ext):
        y = torch.nn.functional.conv2d(torch.ones(1, 2, 4, 4), torch.ones(3, 2, 1, 1))
    assert torch.nn.functional.conv2d is conv2d and torch.ops.aten.convolution_backward is bwd
    assert y.shape == (1, 3, 4, 4) and len(rec.records) == 1 and rec.records[0].startswith("F.conv2d(1x2x4x4@")


def test_compare_aten_ignores_allocations_and_views_only(lt):
    a = {"case": {'aten::empty [[]]': 3, 'aten::add [[2],[2]]': 1, 'aten::to [[2]]': 2}}
    b = {"case": {'aten::empty [[]]': 5, 'aten::add [[2],[2]]': 1}}
    assert lt.compare_aten(a, b) == []
    b["case"]['aten::_to_copy [[2]]'] = 1
    assert lt.compare_aten(a, b) == [("case", 'aten::_to_copy [[2]]', 0, 1)]
