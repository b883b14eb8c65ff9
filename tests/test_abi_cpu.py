"""CPU suite, part 2: the drop-in boundary.  The C-ABI library must load and
export every symbol include/geot_hip.h declares (no compute without a GPU), and the
product must refuse to run without it rather than fall back."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    text = open(os.path.join(ROOT, "include", "geot_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(geot_[a-z0-9_]+)\s*\(", text)))


@pytest.fixture(scope="module")
def built():
    from geot_amd import build
    return build.build()


def test_library_exports_every_declared_symbol(built):
    out = subprocess.run(["nm", "-D", "--defined-only", built], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (geot_[a-z0-9_]+)", out))
    declared = _declared()
    assert len(declared) >= 23
    missing = [s for s in declared if s not in exported]
    assert not missing, "declared in geot_hip.h but not exported: %s" % missing
    extra = [s for s in exported if s not in declared]
    assert not extra, "exported but undeclared: %s" % extra


def test_ctypes_binding_covers_the_header(built):
    from geot_amd import _lib
    lib = _lib.load()
    assert lib.geot_abi_version() == _lib.ABI_VERSION == int(re.search(r"GEOT_ABI_VERSION (\d+)", open(os.path.join(ROOT, "include", "geot_hip.h")).read()).group(1))
    assert sorted(_lib.exported_symbols()) == _declared()
    assert b"invalid" in lib.geot_error_string(1).lower()


def test_code_object_is_gfx950_only(built):
    blob = open(built, "rb").read()
    targets = set(re.findall(rb"amdgcn-amd-amdhsa--(gfx[0-9a-f]+)", blob))
    assert targets == {b"gfx950"}, targets


def test_cpu_tensors_are_rejected_not_emulated(built):
    import torch
    from geot_amd.ext import pointnet2_ext, pointnet2_batch_cuda
    with pytest.raises(RuntimeError, match="CPU not supported"):
        pointnet2_ext.furthest_point_sampling(torch.zeros(1, 8, 3), 4)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        pointnet2_batch_cuda.three_nn_wrapper(1, 4, 4, torch.zeros(1, 4, 3), torch.zeros(1, 4, 3),
                                              torch.zeros(1, 4, 3), torch.zeros(1, 4, 3, dtype=torch.int32))
    # dataloader-side ops: CPU tensors are refused as well (the reference's CPU code is not re-implemented here)
    from geot_amd.openpoints.dataset import grid_subsampling, pc_norm, prepare_sample
    with pytest.raises(RuntimeError, match="CPU not supported"):
        grid_subsampling(torch.zeros(8, 3), sampleDl=0.1, device=torch.device("cpu"))
    with pytest.raises(RuntimeError, match="CPU not supported"):
        pc_norm(torch.zeros(8, 3))
    with pytest.raises(RuntimeError, match="CPU not supported"):
        prepare_sample(torch.zeros(8, 3), torch.zeros(8, dtype=torch.int32), torch.zeros(4, dtype=torch.int64))


def test_missing_library_fails_loudly(tmp_path):
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from geot_amd import _lib\n"
            "_lib.LIB_PATH = %r\n"
            "try:\n    _lib.load()\nexcept _lib.GeotLibraryError as e:\n    print('LOUD', e)\n"
            % (ROOT, str(tmp_path / "nope.so")))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert "LOUD" in out.stdout and "no CPU/PyTorch fallback" in out.stdout


def test_product_never_imports_the_oracle():
    bad = []
    for dp, _, fs in os.walk(os.path.join(ROOT, "geot_amd")):
        for f in fs:
            if f.endswith((".py", ".hip", ".h")):
                t = open(os.path.join(dp, f)).read()
                if re.search(r"^\s*(from|import)\s+oracle\b", t, flags=re.M) or "libgeot_oracle" in t:
                    bad.append(os.path.join(dp, f))
    assert not bad, bad


def test_host_only_planning_entry_points(monkeypatch):
    """Entry points that only plan (sizes, path selection) run without a GPU: sanity of their contracts."""
    from geot_amd import _lib
    lib = _lib.load()
    monkeypatch.delenv("GEOT_NN_IMPL", raising=False)
    # grid kNN: big or long-list problems qualify, small ones and k > 64 do not; env overrides both ways
    assert lib.geot_knn_grid_eligible(1, 24000, 24000, 33) == 1
    assert lib.geot_knn_grid_eligible(8, 8192, 8192, 4) == 1
    assert lib.geot_knn_grid_eligible(1, 512, 24000, 32) == 1
    assert lib.geot_knn_grid_eligible(1, 1000, 1000, 8) == 0
    assert lib.geot_knn_grid_eligible(1, 24000, 24000, 65) == 0
    monkeypatch.setenv("GEOT_NN_IMPL", "wave")
    assert lib.geot_knn_grid_eligible(1, 24000, 24000, 33) == 0
    monkeypatch.setenv("GEOT_NN_IMPL", "grid")
    assert lib.geot_knn_grid_eligible(1, 3000, 3000, 8) == 1
    monkeypatch.delenv("GEOT_NN_IMPL")
    assert lib.geot_ball_grid_eligible(1, 24000, 6000, 0.1, 32) == 1
    assert lib.geot_ball_grid_eligible(1, 24000, 6000, 0.1, 65) == 0
    assert lib.geot_ball_grid_eligible(1, 24000, 6000, -1.0, 32) == 0
    # workspace sizes: monotone, 16-byte multiples, linear in the batch
    w1, w8 = lib.geot_knn_grid_ws_bytes(1, 24000), lib.geot_knn_grid_ws_bytes(8, 24000)
    assert w1 > 24000 * 24 and w1 % 16 == 0 and w8 == 8 * w1
    assert lib.geot_knn_grid_ws_bytes(-1, 5) == -1
    assert lib.geot_ntm_threed_graph_bytes(2, 1000, 32) > 4 * (2 * 1000 * (2 * 64 + 4 * 32))
    assert lib.geot_ntm_threed_loss_ws_bytes(2, 1000, 32) > 0 and lib.geot_ntm_sig_t_mean_ws_floats(8, 24000) > 0
    assert lib.geot_ntm_correct_ws_floats(8, 24000) % 289 == 0
    # gradients: the sorted-pair-stream form (csrc/tile_scatter.hip) wherever a CU's LDS holds the targets' sums
    assert lib.geot_grad_ws_needs_zero(8, 384, 8192, 24000, 3) == 0
    assert lib.geot_grad_ws_needs_zero(8, 64, 24000, 6000 * 32, 1) == 0
    assert lib.geot_grad_ws_needs_zero(1, 3, 8, 3000, 3) == 0
    assert lib.geot_grad_ws_needs_zero(1, 16, 100000, 200000, 3) == 1        # 100 k targets, long rows: channels-last atomic accumulation
    ws = lib.geot_scatter_grad_ws_floats(8, 384, 8192, 24000, 3, 1)
    assert ws >= 8 * 384 * 8192 and lib.geot_scatter_grad_ws_floats(8, 4, 8192, 24000, 3, 1) >= 2 * 8 * 24000 * 3
    assert lib.geot_scatter_grad_ws_floats(1, 16, 100000, 200000, 3, 1) == 16 * 100000
    monkeypatch.setenv("GEOT_GATHER_IMPL", "csr")
    assert lib.geot_grad_ws_needs_zero(8, 64, 24000, 6000 * 32, 1) == 1      # the older forms: 768 KB rows do not fit LDS
    assert lib.geot_grad_ws_needs_zero(1, 16, 8192, 24000, 3) == 1           # workspace too small for their index
    monkeypatch.delenv("GEOT_GATHER_IMPL")
    assert lib.geot_sa_param_floats(3, 3, (__import__("ctypes").c_int * 3)(64, 64, 128)) == 6 * 64 + 64 + 64 * 64 + 64 + 64 * 128 + 128
    # fused EdgeConv tail (ABI 9): the plan of an eligible shape, nothing for one that is not; workspace = its query
    import ctypes
    out = (ctypes.c_longlong * 14)(*([-7] * 14))
    assert lib.geot_edgeconv_plan(8, 384, 8192, 8192, 4, 4, out, 14) == 1
    assert list(out)[:10] == [2, 1, 65536, 1, 1, 2, 1, 147456, 0, 4]
    assert out[13] == lib.geot_edgeconv_ws_bytes(8, 384, 8192, 8192, 4) and lib.geot_edgeconv_eligible(8, 384, 8192, 8192, 4, 4) == 1
    short = (ctypes.c_longlong * 14)(*([-7] * 14))
    assert lib.geot_edgeconv_plan(8, 384, 8192, 8192, 4, 4, short, 2) == 1 and list(short) == [2, 1] + [-7] * 12
    for args in ((8, 384, 8192, 8192, 4, 5), (1, 8, 100, 100, 256, 1), (1, 8, 100, 38401, 4, 1), (1, 8, 17067, 100, 4, 1)):
        untouched = (ctypes.c_longlong * 14)(*([-7] * 14))
        assert lib.geot_edgeconv_plan(*args, untouched, 14) == 0 and list(untouched) == [-7] * 14
        assert lib.geot_edgeconv_eligible(*args) == 0
    # fused SetAbstraction (ABI 10): configs[1]'s plan on 256 CUs, a prefix on request, nothing for a refused shape
    w3 = (ctypes.c_int * 3)(64, 64, 128)
    sa = (ctypes.c_longlong * 27)(*([-7] * 27))
    assert lib.geot_sa_plan(1, 6000, 32, 3, 3, w3, 256, 1, sa, 27) == 1
    assert list(sa)[:11] == [0, 12, 157696, 256, 1, 1, 2, 1, 6000, 6 * 64 + 64 + 64 * 64 + 64 + 64 * 128 + 128, 65]
    assert list(sa)[11:] == [6, 64, 64, 0, 64, 64, 128, 0, 0, 448, 4608, 0, 384, 4544, 12800, 0]
    assert sa[9] == lib.geot_sa_param_floats(3, 3, w3)
    short = (ctypes.c_longlong * 27)(*([-7] * 27))
    assert lib.geot_sa_plan(1, 6000, 32, 3, 3, w3, 256, 1, short, 2) == 1 and list(short) == [0, 12] + [-7] * 25
    for args in ((1, 6000, 24, 3, 3, w3), (1, 6000, 32, 3, 3, (ctypes.c_int * 3)(128, 128, 128)),
                 (1, 6000, 32, 3, 3, (ctypes.c_int * 3)(64, 257, 128)), (-1, 6000, 32, 3, 3, w3)):
        untouched = (ctypes.c_longlong * 27)(*([-7] * 27))
        assert lib.geot_sa_plan(*args, 256, 1, untouched, 27) == 0 and list(untouched) == [-7] * 27
    # forward gathers (ABI 28): 2 and the table-in-LDS geometry, a prefix on request, 1 / 0 and nothing written otherwise
    gp = (ctypes.c_longlong * 5)(*([-7] * 5))
    assert lib.geot_gather_plan(8, 384, 8192, 24000, gp, 5) == 2 and list(gp) == [4, 96, 1, 24000, 131072]
    short = (ctypes.c_longlong * 5)(*([-7] * 5))
    assert lib.geot_gather_plan(16, 8, 18432, 36864, short, 3) == 2 and list(short) == [2, 4, 8, -7, -7]
    for args, form in (((1, 16, 64, 4095), 1), ((1, 2, 36865, 32768), 1), ((0, 16, 64, 4096), 0), ((1, 16, 64, 0), 0)):
        untouched = (ctypes.c_longlong * 5)(*([-7] * 5))
        assert lib.geot_gather_plan(*args, untouched, 5) == form and list(untouched) == [-7] * 5
    monkeypatch.setenv("GEOT_GATHER_IMPL", "plain")             # the environment switch moves the plan with the dispatch
    assert lib.geot_gather_plan(8, 384, 8192, 24000, gp, 5) == 1
    monkeypatch.delenv("GEOT_GATHER_IMPL")
    # run-time-C NTM kernels (ABI 29): form, CP | CPAD, tails, ksplit, blocks, LDS bytes, gen_correct blocks on 256 CUs
    monkeypatch.delenv("GEOT_NTM_GENERIC", raising=False)
    npl = (ctypes.c_longlong * 7)(*([-7] * 7))
    assert lib.geot_ntm_generic_plan(2, 70001, 13, 0, 256, npl, 7) == 3 and list(npl) == [3, 16, 1, 4, 256, 4 * (2 * 2 * 256 + 2 * 32 + 16 * 32 * 36), 2048]
    assert lib.geot_ntm_generic_plan(2, 700, 5, 1, 256, npl, 7) == 2 and list(npl) == [2, 8, 0, 1, 6, 4 * (28 + 256 * 9), 350]
    short = (ctypes.c_longlong * 7)(*([-7] * 7))
    assert lib.geot_ntm_generic_plan(2, 700, 17, 0, 256, short, 2) == 4 and list(short) == [4, 0] + [-7] * 5
    assert lib.geot_ntm_generic_plan(2, 700, 13, 0, 256, None, 0) == 3
    for args in ((0, 700, 13), (2, 0, 13), (2, 700, 0), (2, 700, 33), (-1, 700, 13)):
        untouched = (ctypes.c_longlong * 7)(*([-7] * 7))
        assert lib.geot_ntm_generic_plan(*args, 0, 256, untouched, 7) == 0 and list(untouched) == [-7] * 7
    monkeypatch.setenv("GEOT_NTM_GENERIC", "wave")               # the environment switch moves the plan with the dispatch
    assert lib.geot_ntm_generic_plan(2, 700, 13, 0, 256, npl, 7) == 1 and list(npl) == [1, 0, 0, 1, 350, 4 * 14 * 169, 350]
    monkeypatch.setenv("GEOT_NTM_GENERIC", "mfma")               # fewer than four output elements never reach the MFMA form
    assert lib.geot_ntm_generic_plan(1, 3, 1, 1, 256, None, 0) == 2 and lib.geot_ntm_generic_plan(1, 4, 1, 1, 256, None, 0) == 3
    monkeypatch.delenv("GEOT_NTM_GENERIC")


def test_grid_search_plan_entry_points(monkeypatch):
    """geot_knn_grid_plan / geot_ball_grid_plan (ABI 18): host-only, filled exactly where the matching *_eligible call is
    1, a prefix on request, nothing written otherwise."""
    import ctypes
    from geot_amd import _lib
    lib = _lib.load()
    monkeypatch.delenv("GEOT_NN_IMPL", raising=False)
    out = (ctypes.c_longlong * 7)(*([-7] * 7))
    assert lib.geot_knn_grid_plan(1, 24000, 24000, 33, out, 7) == 1
    assert list(out) == [int((3 * 24000 / (5 * 33)) ** 0.5), 32, 12, 8, 48, 4, 1 << 22]
    assert lib.geot_knn_grid_plan(8, 8192, 8192, 4, out, 1) == 1 and out[0] == 32 and out[1] == 32   # G clamped to the most
    short = (ctypes.c_longlong * 7)(*([-7] * 7))
    assert lib.geot_knn_grid_plan(1, 24000, 24000, 33, short, 2) == 1 and list(short) == [20, 32] + [-7] * 5
    assert lib.geot_knn_grid_plan(1, 24000, 24000, 33, None, 0) == 1
    ball = (ctypes.c_longlong * 3)(*([-7] * 3))
    assert lib.geot_ball_grid_plan(1, 24000, 6000, 0.1, 32, ball, 3) == 1 and list(ball) == [32, 12, 4]
    for args in ((1, 1000, 1000, 8), (1, 24000, 24000, 65), (1, 24000, 24000, 0), (0, 24000, 24000, 8)):
        untouched = (ctypes.c_longlong * 7)(*([-7] * 7))
        assert lib.geot_knn_grid_eligible(*args) == 0
        assert lib.geot_knn_grid_plan(*args, untouched, 7) == 0 and list(untouched) == [-7] * 7
    for args in ((1, 24000, 6000, 0.1, 65), (1, 24000, 6000, -1.0, 32), (1, 2047, 6000, 0.1, 32)):
        untouched = (ctypes.c_longlong * 3)(*([-7] * 3))
        assert lib.geot_ball_grid_eligible(*args) == 0
        assert lib.geot_ball_grid_plan(*args, untouched, 3) == 0 and list(untouched) == [-7] * 3
    monkeypatch.setenv("GEOT_NN_IMPL", "grid")                # the environment switch moves the plan with the dispatch
    assert lib.geot_knn_grid_plan(1, 241, 2048, 8, out, 7) == 1 and out[0] == 12
    assert lib.geot_ball_grid_plan(1, 2048, 241, 0.1, 32, ball, 3) == 1
    monkeypatch.setenv("GEOT_NN_IMPL", "wave")
    assert lib.geot_knn_grid_plan(1, 24000, 24000, 33, out, 7) == 0
    assert lib.geot_ball_grid_plan(1, 24000, 6000, 0.1, 32, ball, 3) == 0


def test_header_is_plain_c_and_links(tmp_path):
    """include/geot_hip.h must be consumable from C (no C++ / torch types) and every declared entry point must
    resolve at link time against the shared library -- what a maintainer's cgo / JNI / C++ forwarder would do."""
    import re
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "geot_hip.h")).read()
    names = sorted(set(re.findall(r"\b(geot_[a-z0-9_]+)\s*\(", hdr)))
    src = tmp_path / "link_all.c"
    body = "\n".join("    p[%d] = (fn)%s;" % (i, n) for i, n in enumerate(names))
    src.write_text('#include "geot_hip.h"\n#include <stdio.h>\ntypedef void (*fn)(void);\nint main(void) {\n    fn p[%d];\n%s\n'
                   '    printf("%%d %%d\\n", geot_abi_version(), p[0] != 0);\n    return 0;\n}\n' % (len(names), body))
    lib_dir = os.path.join(root, "geot_amd")
    exe = tmp_path / "link_all"
    cmd = ["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(root, "include"), str(src), "-o", str(exe),
           "-L", lib_dir, "-lgeot_hip", "-Wl,-rpath," + lib_dir, "-Wl,--unresolved-symbols=ignore-in-shared-libs"]
    subprocess.check_call(cmd)
    assert len(names) >= 50


def test_no_undefined_global_names():
    """Static check (pyflakes is not installed): every LOAD_GLOBAL in the product, bench and tool sources
    resolves to a module-level name or a builtin.  A typo'd or never-imported global in a rarely taken branch --
    e.g. the N > 1 tail of bench.py, which no CPU test can execute -- otherwise surfaces only on the GPU box."""
    import ast
    import builtins
    import dis
    import glob
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    files = [os.path.join(root, "bench.py"), os.path.join(root, "__graft_entry__.py")]
    for sub in ("geot_amd", "tools", "oracle"):
        files += glob.glob(os.path.join(root, sub, "**", "*.py"), recursive=True)
    bad = []
    for path in files:
        src = open(path).read()
        tree = ast.parse(src)
        defined = set(dir(builtins)) | {"__file__", "__name__", "__doc__", "__builtins__", "__spec__", "__package__"}
        for node in ast.walk(tree):     # any binding anywhere that can create a module-level name
            if isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef, ast.ClassDef)):
                defined.add(node.name)
            elif isinstance(node, ast.Import):
                defined.update((a.asname or a.name).split(".")[0] for a in node.names)
            elif isinstance(node, ast.ImportFrom):
                defined.update(a.asname or a.name for a in node.names)
            elif isinstance(node, ast.Name) and isinstance(node.ctx, (ast.Store, ast.Del)):
                defined.add(node.id)
            elif isinstance(node, ast.Global):
                defined.update(node.names)

        def walk(code):
            for ins in dis.get_instructions(code):
                if ins.opname in ("LOAD_GLOBAL", "LOAD_NAME") and ins.argval not in defined:
                    bad.append("%s: %s (line %s)" % (os.path.relpath(path, root), ins.argval, ins.starts_line))
            for c in code.co_consts:
                if hasattr(c, "co_code"):
                    walk(c)
        walk(compile(src, path, "exec"))
    assert not bad, "undefined global names:\n" + "\n".join(sorted(set(bad)))
