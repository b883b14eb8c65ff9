"""The header parser (geot_amd/_header.py) and what geot_amd/_lib.py derives from it: the ctypes signatures of every entry
point of include/geot_hip.h and the mirrored constants.  The expected signatures of the pinned entries are written out by
hand from the header, one per scalar kind and return type; the synthetic headers are the smallest inputs at which the
parser can go wrong."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I, F, D, L, U, P = ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_longlong, ctypes.c_ulonglong, ctypes.c_void_p

# name -> (argtypes, restype), read off include/geot_hip.h by hand
PINNED = {
    # (int b, int n, int m, float radius, int nsample, const float *new_xyz, const float *xyz, int *idx, void *stream)
    "geot_ball_query": ([I, I, I, F, I, P, P, P, P], I),
    # (int c, double geo_lambda, double ema_decay, 4 x const float *, 4 x float *, void *stream)
    "geot_ntm_class_transition": ([I, D, D, P, P, P, P, P, P, P, P, P], I),
    # (int b, int c, int m, int n, points, idx, weight, out, long long out_bstride, void *stream)
    "geot_three_interpolate_into": ([I, I, I, I, P, P, P, P, L, P], I),
    # (int j, int m, int n_noise, int n_mask, 4 x const void *, unsigned long long seed, unsigned long long draw_base,
    #  void *jobs, float *noise, float *mask, void *stream)
    "geot_view_draw": ([I, I, I, I, P, P, P, P, U, U, P, P, P, P], I),
    # (int b, int npoint, int nsample, int c_feat, int nlayers, const int *widths, int cus, int out_aligned16,
    #  long long *out, int n_out): both host arrays are plain addresses
    "geot_sa_plan": ([I, I, I, I, I, P, I, I, P, I], I),
    # (int b, int c, int m_targets, long long n_sources, int slots_per_source, int weighted, long long *out, int n_out)
    "geot_scatter_grad_plan": ([I, I, I, L, I, I, P, I], I),
    # (int b, int c, int m_table, long long n_out_elems, long long *out, int n_out): host array, no stream
    "geot_gather_plan": ([I, I, I, L, P, I], I),
    # (int b, int n, int c, int backward, int cus, long long *out, int n_out): host array, no stream
    "geot_ntm_generic_plan": ([I, I, I, I, I, P, I], I),
    "geot_knn_grid_ws_bytes": ([I, I], L),                      # long long (int b, int nr)
    "geot_error_string": ([I], ctypes.c_char_p),                # const char * (int hip_error)
}
STREAMED = {"geot_ball_query", "geot_ntm_class_transition", "geot_three_interpolate_into", "geot_view_draw"}


def test_pinned_entries_of_the_real_header():
    from geot_amd import _lib
    for name, want in PINNED.items():
        assert _lib.SIGNATURES[name] == want, name
        if name in STREAMED:
            assert _lib.PROTOTYPES[name] == want[0] and name not in _lib.PLAIN, name
        elif name != "geot_error_string":
            assert _lib.PLAIN[name] == want and name not in _lib.PROTOTYPES, name
    assert "geot_error_string" not in _lib.PROTOTYPES and "geot_error_string" not in _lib.PLAIN


def test_every_entry_is_bound_as_derived_after_load():
    from geot_amd import _header, _lib, build
    build.build()
    lib = _lib.load()
    entries, _ = _header.parse()
    assert len(entries) == len(_lib.SIGNATURES) >= 158
    assert len(_lib.PROTOTYPES) + len(_lib.PLAIN) + 3 == len(entries)
    assert sorted(_lib.exported_symbols()) == sorted(e.name for e in entries)
    for e in entries:
        argtypes, restype = _lib.SIGNATURES[e.name]
        fn = getattr(lib, e.name)
        assert fn.argtypes == argtypes and len(argtypes) == len(e.params), e.name
        assert fn.restype is restype, e.name
        assert (e.name in _lib.PROTOTYPES) == e.streamed, e.name
        if e.streamed:
            assert restype is ctypes.c_int and argtypes[-1] is ctypes.c_void_p and _lib.PROTOTYPES[e.name] is argtypes, e.name
    for name, want in PINNED.items():
        assert (getattr(lib, name).argtypes, getattr(lib, name).restype) == want, name


SYNTHETIC = """
#ifndef GEOT_HIP_H
#define GEOT_HIP_H
#define GEOT_A 3
#define GEOT_B (8 + 14 * GEOT_A)   /* over an earlier name */
#  define GEOT_C (GEOT_B - 2 * GEOT_A)
int geot_spread(int b,
                const float *xyz, /* (b, n, 3) , not; a parameter */
                long long n, void *stream);
long long geot_nothing(void);
// int geot_fake(int a, void *stream);
/* int geot_fake_too(int a); */
int geot_unsigned(unsigned int a, unsigned b, unsigned long long c, double d, float *out);
const char *geot_text( int  code );
#endif
"""


def test_synthetic_header():
    from geot_amd import _header
    entries, constants = _header.parse(SYNTHETIC)
    assert entries == [
        ("int", "geot_spread", [("int", "int b"), ("ptr", "const float *xyz"), ("long long", "long long n"), ("ptr", "void *stream")], True),
        ("long long", "geot_nothing", [], False),
        ("int", "geot_unsigned", [("unsigned", "unsigned int a"), ("unsigned", "unsigned b"),
                                  ("unsigned long long", "unsigned long long c"), ("double", "double d"), ("ptr", "float *out")], False),
        ("const char *", "geot_text", [("int", "int code")], False)]
    assert entries[0].name == "geot_spread" and entries[0].streamed and entries[2].params[1] == ("unsigned", "unsigned b")
    assert constants == {"GEOT_A": 3, "GEOT_B": 8 + 14 * 3, "GEOT_C": 50 - 6}          # the include guard is skipped


@pytest.mark.parametrize("decl, named", [
    ("int geot_bad(int a, size_t n, void *stream);", "geot_bad"),                    # a scalar type the parser does not know
    ("int geot_ok(int a);\nint geot_cb(void (*cb)(int), void *stream);", "geot_cb"),   # the prototype pattern cannot take it
    ("size_t geot_ret(int a);", "geot_ret"),                                         # nor an unknown return type
    ("int geot_ok(int a);\nint geot_body(int a) { return a; }", "geot_body"),
])
def test_a_declaration_the_parser_cannot_type_raises(decl, named):
    from geot_amd import _header
    with pytest.raises(ValueError, match=r"\b%s\b" % named):
        _header.parse(decl)


@pytest.mark.parametrize("define", [
    "#define GEOT_X 1.5", '#define GEOT_X "text"', "#define GEOT_X __import__('os').getpid()", "#define GEOT_X abs(3)",
    "#define GEOT_X GEOT_LATER + 1\n#define GEOT_LATER 2", "#define GEOT_X (int)3", "#define GEOT_X 7 / 2", "#define GEOT_X 2 ** 3",
    "#define GEOT_X 1 << 4", "#define GEOT_X -1", "#define GEOT_X True", "#define GEOT_X(a) 3",
])
def test_a_define_that_is_no_integer_expression_raises_and_runs_nothing(define):
    from geot_amd import _header
    with pytest.raises(ValueError, match="GEOT_X"):
        _header.parse(define + "\nint geot_ok(int a);\n")


def test_constants_of_the_real_header_and_their_mirrors():
    from geot_amd import _header, _lib
    hdr = open(os.path.join(ROOT, "include", "geot_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    _, constants = _header.parse()
    defined = re.findall(r"^#define (GEOT_\w+)[ \t]+\S", hdr, flags=re.M)
    assert sorted(defined) == sorted(constants) and len(defined) == len(set(defined)) >= 16 and "GEOT_HIP_H" not in constants
    for name, text in re.findall(r"^#define (GEOT_\w+)[ \t]+(\d+)[ \t]*$", hdr, flags=re.M):     # the plain literals, read independently
        assert constants[name] == int(text), name
    assert constants["GEOT_VIEW_PROGRAM_JOB_WORDS"] == 8 + 14 * 16 == 232        # (8 + 14 * GEOT_VIEW_MAX_OPS)
    assert constants["GEOT_VIEW_DRAW_PLAN_WORDS"] == 8 + 12 * 24 == 296          # (8 + 12 * GEOT_VIEW_DRAW_MAX_STEPS)
    modes = {"GEOT_PSEUDO_MAX": "max", "GEOT_PSEUDO_MARGIN": "margin", "GEOT_PSEUDO_MARGIN_V1": "margin_v1"}
    assert len(_lib.PSEUDO_MODES) == len(modes)
    for name, value in constants.items():        # every constant has its mirror in _lib, under its name without the prefix
        mirror = _lib.PSEUDO_MODES[modes[name]] if name in modes else getattr(_lib, name[len("GEOT_"):])
        assert mirror == value and type(mirror) is int, name


def test_no_second_copy_of_a_header_constant(monkeypatch):
    from geot_amd import _lib, meters, ntm, train_step, validation
    from geot_amd.openpoints.loss import build as loss_build
    assert train_step.PSEUDO_REFINE_MAX_SIZE == _lib.PSEUDO_REFINE_MAX_N == 32
    assert loss_build.MAX_FUSED_CLASSES == ntm.NTM_MAX_CLASSES == _lib.NTM_MAX_C == 32
    assert validation._need_classes(32, "t") == 32
    with pytest.raises(RuntimeError, match=r"1\.\.32 classes"):
        validation._need_classes(33, "t")
    with pytest.raises(RuntimeError, match=r"1\.\.32 classes"):
        meters.FixMatchMeters(33, "cpu")
    monkeypatch.setattr(_lib, "NTM_MAX_C", 4)        # the two checks read _lib's value, not a literal of their own
    with pytest.raises(RuntimeError, match=r"1\.\.4 classes"):
        validation._need_classes(5, "t")
    with pytest.raises(RuntimeError, match=r"1\.\.4 classes"):
        meters.FixMatchMeters(5, "cpu")
