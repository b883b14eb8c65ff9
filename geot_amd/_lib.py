"""ctypes binding of libgeot_hip.so (the C ABI declared in include/geot_hip.h).

Plain pointers and sizes, no torch types cross the boundary.  Nothing about a
signature is written down here: the argtypes and restype of every entry point
and every mirrored constant are derived at import from the header itself
(_header.parse(), the parser the compiled dispatcher is generated with), so a
signature or a limit changes in include/geot_hip.h and nowhere else.  A
maintainer's own stub may still spell its argtypes by hand.
The library is the ONLY compute path of this package: if it is
missing or fails to load, every op raises -- there is no CPU or PyTorch
fallback.
"""
import ctypes
import os

from . import _header

_HERE = os.path.dirname(os.path.abspath(__file__))
# GEOT_DISTANCE selects the squared-distance arithmetic of every index-producing op (include/geot_hip.h
# geot_distance_mode): "exact" (default) | "fma" | "fma_xy"; one library per mode, chosen once at load time.
DISTANCE_MODES = {"exact": (0, "libgeot_hip.so"), "fma": (1, "libgeot_hip_fma.so"), "fma_xy": (2, "libgeot_hip_fma_xy.so")}
DISTANCE = os.environ.get("GEOT_DISTANCE", "exact")
if DISTANCE not in DISTANCE_MODES:
    raise ImportError("GEOT_DISTANCE must be one of %s, got %r" % (sorted(DISTANCE_MODES), DISTANCE))
LIB_PATH = os.path.join(_HERE, DISTANCE_MODES[DISTANCE][1])

_ENTRIES, CONSTANTS = _header.parse()       # once per process, here: nothing is parsed after import
_CTYPES = {"ptr": ctypes.c_void_p,          # device and host pointers alike are passed as raw addresses
           "int": ctypes.c_int, "unsigned": ctypes.c_uint, "long long": ctypes.c_longlong,
           "unsigned long long": ctypes.c_ulonglong, "float": ctypes.c_float, "double": ctypes.c_double,
           "const char *": ctypes.c_char_p}
# name -> (argtypes, restype) of every declaration, in include/geot_hip.h order
SIGNATURES = {e.name: ([_CTYPES[kind] for kind, _ in e.params], _CTYPES[e.ret]) for e in _ENTRIES}
_SPECIAL = ("geot_abi_version", "geot_distance_mode", "geot_error_string")      # in neither table below
# name -> argtypes of the entry points that launch: "(..., void *stream) -> hipError_t"
PROTOTYPES = {e.name: SIGNATURES[e.name][0] for e in _ENTRIES if e.streamed}
# name -> (argtypes, restype) of the host-only ones: sizes, plans, path selection
PLAIN = {e.name: SIGNATURES[e.name] for e in _ENTRIES if not e.streamed and e.name not in _SPECIAL}

# the header's constants under the names the package uses
ABI_VERSION = CONSTANTS["GEOT_ABI_VERSION"]           # a library of another version is refused by load()
KNN_KMAX_HEAP = CONSTANTS["GEOT_KNN_KMAX_HEAP"]       # largest nsample of the heap-ordered kNN (knnquery_cuda, pointops.knn)
KNN_KMAX_SORTED = CONSTANTS["GEOT_KNN_KMAX_SORTED"]   # largest k of the sorted kNN (knn_cuda.KNN, knn_point in 3-D)
NTM_MAX_C = CONSTANTS["GEOT_NTM_MAX_C"]               # largest class count of the per-point kernels (NTM, criteria, meters)
MESH_NEIGHBOURS_LANE_ROW = CONSTANTS["GEOT_MESH_NEIGHBOURS_LANE_ROW"]     # geot_mesh_neighbours: the longest raw row one lane tidies
CURVATURE_MAX_SCAN = CONSTANTS["GEOT_CURVATURE_MAX_SCAN"]     # geot_mesh_angle_defects / geot_scan_ball_sum: vertices of one scan
VIEW_JOB_WORDS = CONSTANTS["GEOT_VIEW_JOB_WORDS"]   # 32-bit words of one geot_fixmatch_views job record
VIEW_REG_POINTS = CONSTANTS["GEOT_VIEW_REG_POINTS"]   # largest cloud geot_fixmatch_views holds in registers
VIEW_MAX_OPS = CONSTANTS["GEOT_VIEW_MAX_OPS"]         # ops of one geot_view_program job
VIEW_PROGRAM_JOB_WORDS = CONSTANTS["GEOT_VIEW_PROGRAM_JOB_WORDS"]
VIEW_DRAW_MAX_STEPS = CONSTANTS["GEOT_VIEW_DRAW_MAX_STEPS"]     # drawn quantities of one geot_view_draw job
VIEW_DRAW_PLAN_WORDS = CONSTANTS["GEOT_VIEW_DRAW_PLAN_WORDS"]
VOTE_SET, VOTE_FINISH = CONSTANTS["GEOT_VOTE_SET"], CONSTANTS["GEOT_VOTE_FINISH"]     # geot_scan_vote's mode bits
PSEUDO_MODES = {"max": CONSTANTS["GEOT_PSEUDO_MAX"], "margin": CONSTANTS["GEOT_PSEUDO_MARGIN"],
                "margin_v1": CONSTANTS["GEOT_PSEUDO_MARGIN_V1"]}
PSEUDO_REFINE_MAX_N = CONSTANTS["GEOT_PSEUDO_REFINE_MAX_N"]
CONTRAST_MAX_B = CONSTANTS["GEOT_CONTRAST_MAX_B"]     # the geot_contrast_* entry points: clouds, channels, sample_nums
CONTRAST_MAX_D = CONSTANTS["GEOT_CONTRAST_MAX_D"]
CONTRAST_MAX_S = CONSTANTS["GEOT_CONTRAST_MAX_S"]
OPTIM_TAIL_CAP = CONSTANTS["GEOT_OPTIM_TAIL_CAP"]     # the geot_optim_tail_* entry points: records per launch,
OPTIM_TAIL_BLOCK_ELEMS = CONSTANTS["GEOT_OPTIM_TAIL_BLOCK_ELEMS"]     # elements per workgroup,
OPTIM_TAIL_STEP_CAP = CONSTANTS["GEOT_OPTIM_TAIL_STEP_CAP"]           # step counters per finish launch,
OPTIM_TAIL_REC_WORDS = CONSTANTS["GEOT_OPTIM_TAIL_REC_WORDS"]         # 32-bit words of a record / of a group,
OPTIM_TAIL_GROUP_WORDS = CONSTANTS["GEOT_OPTIM_TAIL_GROUP_WORDS"]
OPTIM_TAIL_MAX_GROUPS = CONSTANTS["GEOT_OPTIM_TAIL_MAX_GROUPS"]
OPTIM_TAIL_CLIPPED, OPTIM_TAIL_VECTOR = CONSTANTS["GEOT_OPTIM_TAIL_CLIPPED"], CONSTANTS["GEOT_OPTIM_TAIL_VECTOR"]     # record flags
OPTIM_TAIL_EMA_ONLY, OPTIM_TAIL_INT64 = CONSTANTS["GEOT_OPTIM_TAIL_EMA_ONLY"], CONSTANTS["GEOT_OPTIM_TAIL_INT64"]

_lib = None


class GeotLibraryError(RuntimeError):
    pass


def load():
    """Load libgeot_hip.so once.  Raises GeotLibraryError if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise GeotLibraryError(
            "geot_amd: %s is missing -- build it with `python -m geot_amd.build %s` "
            "(there is no CPU/PyTorch fallback)" % (LIB_PATH, DISTANCE))
    # Make sure the HIP runtime torch already uses is the one the library binds
    # to (same SONAME libamdhip64.so.7 => the loader reuses the loaded copy), so
    # torch's stream handles are valid in our launches.
    try:
        import torch  # noqa: F401
        tl = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
        if os.path.exists(tl):
            ctypes.CDLL(tl, mode=ctypes.RTLD_GLOBAL)
    except ImportError:
        pass
    try:
        lib = ctypes.CDLL(LIB_PATH)
    except OSError as e:
        raise GeotLibraryError("geot_amd: cannot load %s: %s" % (LIB_PATH, e))
    def bind(name):     # AttributeError here = header/library mismatch
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = SIGNATURES[name]
        return fn

    if bind("geot_abi_version")() != ABI_VERSION:
        raise GeotLibraryError("geot_amd: %s is ABI version %d, this package binds version %d -- rebuild it with "
                               "`python -m geot_amd.build`" % (LIB_PATH, lib.geot_abi_version(), ABI_VERSION))
    if bind("geot_distance_mode")() != DISTANCE_MODES[DISTANCE][0]:
        raise GeotLibraryError("geot_amd: %s was built with distance mode %d, GEOT_DISTANCE=%s needs %d" %
                               (LIB_PATH, lib.geot_distance_mode(), DISTANCE, DISTANCE_MODES[DISTANCE][0]))
    for name in SIGNATURES:
        bind(name)
    _lib = lib
    return lib


def check(err, what):
    if err != 0:
        msg = load().geot_error_string(err)
        raise RuntimeError("geot_amd: %s failed: %s (hipError %d)" %
                           (what, msg.decode() if msg else "?", err))


def exported_symbols():
    """All C-ABI symbol names the Python side binds."""
    return list(_SPECIAL) + list(PROTOTYPES) + list(PLAIN)
