"""Host-side checks of the max-conv backward (csrc/max_conv.hip): the header's declarations and the workspace size."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_entry_points():
    from geot_amd import _header, _lib
    entries, constants = _header.parse()
    by_name = {e.name: e for e in entries}
    assert constants["GEOT_ABI_VERSION"] == _lib.ABI_VERSION >= 35
    hdr = open(os.path.join(ROOT, "include", "geot_hip.h")).read()
    assert int(re.search(r"GEOT_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION
    dgrad, wgrad, ws = (by_name[k] for k in ("geot_maxconv_dgrad", "geot_maxconv_wgrad", "geot_maxconv_ws_floats"))
    assert dgrad.streamed and [k for k, _ in dgrad.params] == ["int"] * 4 + ["ptr"] * 5
    assert wgrad.streamed and [k for k, _ in wgrad.params] == ["int"] * 4 + ["ptr"] * 6
    assert not ws.streamed and ws.ret == "long long" and [k for k, _ in ws.params] == ["int"] * 4
    lib = _lib.load()
    assert lib.geot_abi_version() == _lib.ABI_VERSION
    assert all(hasattr(lib, k) for k in by_name if k.startswith("geot_maxconv_"))


def test_workspace_size(monkeypatch):
    from geot_amd import _lib
    monkeypatch.delenv("GEOT_MAXCONV_CHUNK", raising=False)
    ws = _lib.load().geot_maxconv_ws_floats
    sizes = [ws(256, 512, g, 32) for g in (1, 2, 31, 32, 33, 64, 70, 100, 1000, 4096, 4097, 100000)]
    assert all(s > 0 and s % (256 * 512) == 0 for s in sizes)
    assert sizes == sorted(sizes)                                      # monotone in g
    assert ws(33, 68, 70, 32) == 3 * 33 * 68                           # a few dozen groups reach several chunks
    assert ws(256, 512, 4096, 32) == 64 * 256 * 512                    # the workload: 64 chunks, 33.5 MB
    assert sizes == [ws(256, 512, g, 32) for g in (1, 2, 31, 32, 33, 64, 70, 100, 1000, 4096, 4097, 100000)]   # of the arguments alone
    assert ws(256, 512, 70, 4) == ws(256, 512, 70, 256)                # n plays no part
    for bad in ((0, 8, 1, 4), (1025, 8, 1, 4), (8, 6, 1, 4), (8, 8, 0, 4), (8, 8, 1, 2), (8, 8, 1, 260), (8, 8, 1, 6)):
        assert ws(*bad) == -1, bad
    monkeypatch.setenv("GEOT_MAXCONV_CHUNK", "7")                      # the test knob, read per call
    assert ws(33, 68, 70, 32) == 10 * 33 * 68
