"""CPU: the C-ABI library builds/loads and exports every symbol include/gomatching_hip.h declares, and the ctypes binding
(signatures, structs, constants) is what that header states (no compute)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    text = open(os.path.join(ROOT, "include", "gomatching_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(gom_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_exported_and_bound():
    import __graft_entry__ as entry
    entry.build()
    from gomatching_amd import lib
    handle = lib.load()
    names = _declared()
    assert len(names) >= 28
    for n in names:
        assert hasattr(handle, n), "symbol %s declared in the header but not exported" % n
        assert n in lib.SIGNATURES, "symbol %s has no ctypes signature" % n
    for n in lib.SIGNATURES:
        assert n in names, "bound symbol %s is not declared in include/gomatching_hip.h" % n
    assert handle.gom_abi_version() == 1


_INLINE = """
/* a comment that names gom_foo( int x ); must yield no entry */
#ifndef T_H_
#define T_H_
#ifdef __cplusplus
extern "C" {
#endif
#define GOM_X 12
#define GOM_Y 0x10
#define GOM_RATE 0.5
typedef struct gom_pair {
    const float* data;
    long n;
    double w;
} gom_pair;
int gom_scalars(int a, long b, float c, double d, unsigned e, unsigned int f, unsigned long long g);
int gom_pointers(const float* a, float* b, const gom_pair* c, void** d, const char* e);   /* [host] */
int gom_nothing(void);
void gom_quiet(void* handle);
const char* gom_name(void);
void* gom_make(int n);
long gom_wrapped(const float* x,
                 int ldx,
                 void* stream);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_parser_on_inline_headers():
    import ctypes as C
    from gomatching_amd import lib
    sigs, structs, consts = lib.parse_header(_INLINE)
    assert sigs == {
        "gom_scalars": (C.c_int, [C.c_int, C.c_long, C.c_float, C.c_double, C.c_uint, C.c_uint, C.c_ulonglong]),
        "gom_pointers": (C.c_int, [C.c_void_p] * 5),          # const T*, T*, a struct pointer, T**, const char* as an argument
        "gom_nothing": (C.c_int, []),
        "gom_quiet": (None, [C.c_void_p]),
        "gom_name": (C.c_char_p, []),
        "gom_make": (C.c_void_p, [C.c_int]),
        "gom_wrapped": (C.c_long, [C.c_void_p, C.c_int, C.c_void_p]),
    }
    assert "gom_foo" not in sigs
    assert consts == {"GOM_X": 12, "GOM_Y": 16}               # integers only; the include guard has no value
    assert list(structs) == ["gom_pair"] and issubclass(structs["gom_pair"], C.Structure)
    assert structs["gom_pair"]._fields_ == [("data", C.c_void_p), ("n", C.c_long), ("w", C.c_double)]


@pytest.mark.parametrize("decl, named", [
    ("int gom_bad(const float* x, int64_t n);", ["gom_bad", "int64_t n"]),          # by-value int64_t
    ("int gom_bad(short s);", ["gom_bad", "short s"]),
    ("short gom_bad(int n);", ["gom_bad", "short"]),
    ("int gom_bad(gom_pair p);", ["gom_bad", "gom_pair p"]),                        # a struct by value
    ("int gom_bad(int);", ["gom_bad", "int"]),                                      # an argument without a name
    ("int gom_bad(int a[3]);", ["gom_bad", "a[3]"]),
    ("typedef struct gom_s { short v; } gom_s;", ["gom_s", "short v"]),
    ("int other_name(int n);", ["other_name"]),                                     # not a gom_ entry: not skipped
    ("#if defined(X)\nint gom_bad(int n);\n#endif", ["#if defined(X)"]),            # a conditional it cannot follow
    ("#\nint gom_ok(int n);", ["directive"]),
])
def test_parser_refuses_what_it_cannot_map(decl, named):
    from gomatching_amd import lib
    with pytest.raises(lib.GomError) as e:
        lib.parse_header(decl)
    for text in named:
        assert text in str(e.value)


def test_missing_header_fails_loudly(tmp_path):
    from gomatching_amd import lib
    path = str(tmp_path / "nowhere" / "gomatching_hip.h")
    with pytest.raises(lib.GomError) as e:
        lib._parse_file(path)
    assert path in str(e.value)


def _header_text():
    text = open(os.path.join(ROOT, "include", "gomatching_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_signatures_against_the_real_header():
    import ctypes as C
    from gomatching_amd import lib
    text = _header_text()
    decls = re.findall(r"\b(gom_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text)
    assert sorted(n for n, _ in decls) == sorted(lib.SIGNATURES) == _declared() and len(decls) == len(lib.SIGNATURES)
    for name, args in decls:
        want = 0 if args.strip() == "void" else args.count(",") + 1
        assert len(lib.SIGNATURES[name][1]) == want, name
    for name in ("gom_tracker_destroy", "gom_gemm_k256_set_lines", "gom_gemm_k256_set_interleave"):
        assert lib.SIGNATURES[name][0] is None, name
    assert lib.SIGNATURES["gom_built_for_arch"] == (C.c_char_p, [])
    assert lib.SIGNATURES["gom_tracker_create"][0] is C.c_void_p
    # int gom_dropout_f32(const float* x, long ldx, const float* r, long ldr, float* y, long ldy, long rows, long cols,
    #                     unsigned long long seed, unsigned site, unsigned iteration, unsigned rank, long threshold, float scale, void* stream)
    P, L, U = C.c_void_p, C.c_long, C.c_uint
    assert lib.SIGNATURES["gom_dropout_f32"] == (C.c_int, [P, L, P, L, P, L, L, L, C.c_ulonglong, U, U, U, L, C.c_float, P])


def test_structs_mirror_the_header():
    import ctypes as C
    from gomatching_amd import lib, ops
    text = _header_text()
    for cls, name in ((lib.OptimTensor, "gom_optim_tensor"), (lib.MatcherLayer, "gom_matcher_layer")):
        body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), text, flags=re.S).group(1)
        fields = [re.search(r"(\w+)\s*$", f).group(1) for f in body.split(";") if f.strip()]
        assert [n for n, _ in cls._fields_] == fields and len(fields) == 8
        assert C.sizeof(cls) == 64 and lib.STRUCTS[name] is cls
    types = dict(lib.OptimTensor._fields_)
    assert types["lr"] is C.c_double and types["weight_decay"] is C.c_double
    assert types["n"] is C.c_long and types["step"] is C.c_long
    assert all(t is C.c_void_p for t in (types["param"], types["grad"], types["exp_avg"], types["exp_avg_sq"]))
    assert all(t is C.c_void_p for _, t in lib.MatcherLayer._fields_)
    assert not hasattr(ops, "MatcherLayer")                    # one mirror per struct


def test_constants_come_from_the_header():
    from gomatching_amd import jpeg, lexicon, lib, ops
    defines = re.findall(r"^[ \t]*#[ \t]*define[ \t]+(GOM_\w+)[ \t]+(\S+)[ \t]*$", _header_text(), flags=re.M)
    ints = {n: int(v, 0) for n, v in defines if re.fullmatch(r"-?(0|[1-9]\d*|0[xX][0-9a-fA-F]+)", v)}
    assert lib.CONSTANTS == ints and len(ints) >= 20
    assert ops.RESULT_ROWS_WORDS == 234 and ops.RESULT_ROWS_DESC_WORDS == 6
    assert ops.INGEST_MOTION_MAX_FRAMES == 16
    assert lexicon.MAX_LEN == ops.LEXICON_MAX_LEN == 64 and lexicon.NO_MATCH_DIST == 100
    assert jpeg.MAX_WIDTH == ops.JPEG_MAX_WIDTH == 4096 and ops.JPEG_MAX_HEIGHT == 65535
    assert lib.GOM_OK == 0 and lib._ERR_HIP_BASE == 1000 and sorted(lib._ERR) == [1, 2]


def test_library_defines_no_undeclared_entry():
    """The other direction of the export check: every gom_* symbol the built library defines is declared in the header."""
    import shutil
    import subprocess
    nm = shutil.which("nm")
    if nm is None:
        pytest.skip("no nm on the path")
    from gomatching_amd import build
    out = subprocess.run([nm, "-D", "--defined-only", build.build()], capture_output=True, text=True, check=True).stdout
    defined = {line.split()[-1] for line in out.splitlines() if line.split() and line.split()[-1].startswith("gom_")}
    assert len(defined) >= 183
    assert sorted(defined - set(_declared())) == []


def test_call_names_the_entry_that_ran(monkeypatch):
    from gomatching_amd import lib, ops

    class Stub:
        def __init__(self):
            self.seen = []

        def gom_first(self, *args):
            self.seen.append(("gom_first", args))
            return 0

        def gom_second(self, rc):
            self.seen.append(("gom_second", (rc,)))
            return rc

    stub = Stub()
    monkeypatch.setattr(lib, "_lib", stub)
    assert ops._call("gom_first", 1, None, 2.5) is None
    assert ops._call("gom_second", 0) is None
    assert stub.seen == [("gom_first", (1, None, 2.5)), ("gom_second", (0,))]
    with pytest.raises(lib.GomError) as e:
        ops._call("gom_second", 1)
    assert str(e.value).startswith("gom_second failed: GOM_ERR_INVALID_ARG")
    with pytest.raises(lib.GomError) as e:
        ops._call("gom_second", 2)
    assert str(e.value) == "gom_second failed: GOM_ERR_UNSUPPORTED"
    with pytest.raises(lib.GomError) as e:
        ops._call("gom_second", 1000 + 719)
    assert str(e.value) == "gom_second failed: HIP error 719"
    with pytest.raises(lib.GomError) as e:
        ops._call("gom_second", 7)
    assert str(e.value) == "gom_second failed: error 7"
    with pytest.raises(AttributeError):
        ops._call("gom_third")


def test_product_has_no_oracle_dependency():
    """The shipped package must never import the oracle (or /root/reference)."""
    pkg = os.path.join(ROOT, "gomatching_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py") and f != "smoke.py":
                src = open(os.path.join(dirpath, f)).read()
                assert "oracle" not in re.sub(r'""".*?"""', "", src, flags=re.S).replace("# oracle", ""), f
                assert "/root/reference" not in re.sub(r'""".*?"""', "", src, flags=re.S), f


def test_missing_library_fails_loudly(monkeypatch):
    from gomatching_amd import lib
    monkeypatch.setattr(lib, "_lib", None)
    monkeypatch.setattr(lib, "LIB_PATH", "/nonexistent/libgomatching_hip.so")
    with pytest.raises(lib.GomError):
        lib.load()


def test_entry_points_reject_bad_arguments_without_a_gpu():
    """Argument checks run before any HIP call: the newer entry points turn nonsense into GOM_ERR_INVALID_ARG /
    GOM_ERR_UNSUPPORTED instead of launching (error behaviour of the boundary; no compute, no device needed)."""
    import ctypes
    from gomatching_amd import lib
    L = lib.load()
    INVALID = 1                                                   # GOM_ERR_INVALID_ARG (include/gomatching_hip.h)
    p = ctypes.c_void_p(0x1000)                                   # a non-null, 16-byte aligned address that is never dereferenced
    assert L.gom_flash_attention_f32(p, p, p, p, 1, 64, 2, 32, 192, 64, None, None) == INVALID         # head_dim 32: not served
    assert L.gom_flash_attention_f32(None, p, p, p, 1, 64, 2, 64, 384, 128, None, None) == INVALID
    assert L.gom_flash_attention_f32(p, p, p, p, 1, 64, 2, 64, 100, 128, None, None) == INVALID         # row stride < 3C
    assert L.gom_im2col_nhwc_f32(p, p, 1, 8, 8, 3, 3, 3, 1, 1, 1, 32, None) == INVALID                  # C % 4 != 0
    assert L.gom_im2col_nhwc_f32(p, p, 1, 8, 8, 4, 3, 3, 1, 1, 1, 20, None) == INVALID                  # ldo < KH*KW*C
    assert L.gom_grouped_conv3x3_nhwc_f32(p, p, None, p, None, 0, p, 1, 8, 8, 64, 64, 8, 1, None) == INVALID   # 8 channels per group: only 4 and 16 are built
    assert L.gom_grouped_conv3x3_nhwc_f32(p, p, None, p, None, 7, p, 1, 8, 8, 64, 64, 16, 1, None) == INVALID  # unknown activation
    assert L.gom_vitae_window_attention_f32(p, p, 4, 3, 96, None) == INVALID                             # head_dim 32
    assert L.gom_softmax_rows_scaled_f32(p, 4, 9000, 9000, 1.0, None) == INVALID                         # > 8192 columns
    assert L.gom_transpose_f32(p, p, 8, 8, 4, 8, None) == INVALID                                        # ld < cols
    assert L.gom_copy_words(None, p, 4, None) == INVALID
    assert L.gom_tracker_create(0, 0.2, 1, 1, 1, 1.0, None, 0, None, 0, 1024, 8, 1024) is None           # test_len < 1
    assert L.gom_tracker_create(6, 0.2, 1, 1, 1, 1.0, None, 1, None, 0, 1024, 8, 1024) is None           # layers without weights
    # round 6: the CU-cooperative decoder tail
    assert L.gom_dec_tail2_wave_bytes(256, 1024, 1, 1, 4) == (64 + 12 * 64) * 1024 and L.gom_dec_tail2_wave_bytes(256, 1000, 1, 1, 4) == -1
    assert L.gom_dec_tail2_wave_bytes(256, 1024, 1, 1, 8) == (32 + 12 * 32) * 1024 and L.gom_dec_tail2_wave_bytes(256, 1024, 1, 1, 6) == -1   # 4 or 8 waves
    assert L.gom_dec_tail2_image_lin(p, 1, 128, p, 1 << 20, 0, 8, None) == INVALID                       # ld < 256
    assert L.gom_dec_tail2_image_lin(p, 1, 256, p, 1 << 20, 0, 5, None) == INVALID                       # waves
    assert L.gom_dec_tail2_image_mlp(p, 1, 256, p, 1, 256, 192, p, 1 << 20, 0, 8, None) == INVALID        # hidden % 128 != 0
    # round 6: the self-attention blocks on 16-token waves (same contract as gom_dec_attn_*)
    assert L.gom_dec_attn2_image_bytes(256, 8) == (4 + 32 * 33) * 1024 and L.gom_dec_attn2_image_bytes(128, 8) == -1
    assert L.gom_dec_attn2_raw_image_bytes() == (4 + 44 * 33) * 1024
    assert L.gom_dec_attn2_image(p, 1, 128, p, p, p, 1, 256, p, p, p, p, 0, p, 1 << 22, None) == INVALID    # ld_in < 256
    assert L.gom_dec_attn2_image(p, 1, 256, p, p, p, 1, 256, p, p, p, p, 0, p, 1024, None) == INVALID       # image too small
    assert L.gom_dec_attn2_f32(p, 256, None, 0, p, 1e-5, p, 256, 4, 25, 1, 0, None, None) == INVALID        # intra without query_pos
    assert L.gom_dec_attn2_f32(p, 256, p, 256, p, 1e-5, p, 256, 4, 33, 1, 0, None, None) == INVALID         # > 32 points
    assert L.gom_dec_attn2_f32(p, 256, None, 0, p, 1e-5, p, 256, 4, 129, 25, 1, None, None) == INVALID      # > 128 queries
    assert L.gom_dec_attn2_raw_f32(p, 256, p, 1e-5, p, 256, p, 256, p, 380, 4, 100, 25, None, None) == INVALID   # ldraw < 384


def test_library_has_no_packed_fp32_instructions():
    """DESIGN.md "Tracker determinism": `v_pk_fma_f32` gave wrong low halves beside the bf16x6 GEMM kernel on MI355X, so
    the device code is built with the packed-fp32 target feature off.  Checked on the disassembly of the shipped library."""
    import shutil
    import subprocess
    from gomatching_amd import build
    lib = build.build()
    objdump = shutil.which("llvm-objdump") or "/opt/rocm/lib/llvm/bin/llvm-objdump"
    bundler = "/opt/rocm/lib/llvm/bin/clang-offload-bundler"
    objcopy = "/opt/rocm/lib/llvm/bin/llvm-objcopy"
    if not (os.path.exists(objdump) and os.path.exists(bundler) and os.path.exists(objcopy)):
        pytest.skip("ROCm llvm tools not found")
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        total = 0
        for src in build.SOURCES:
            if not src.endswith(".hip") or src == "abi.hip":       # abi.hip holds no kernel
                continue
            obj = os.path.join(build.OBJ, src + ".o")
            fat, co = os.path.join(tmp, src + ".fatbin"), os.path.join(tmp, src + ".co")
            r = subprocess.run([objcopy, "--dump-section", ".hip_fatbin=" + fat, obj], capture_output=True, text=True)
            if r.returncode != 0 and "not found" in r.stderr:      # host-only translation unit (no kernel)
                continue
            assert r.returncode == 0 and os.path.getsize(fat) > 0, (src, r.stderr)
            r = subprocess.run([bundler, "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                                "--input=" + fat, "--output=" + co], capture_output=True, text=True)
            assert r.returncode == 0 and os.path.getsize(co) > 0, (src, r.stderr)
            dis = subprocess.run([objdump, "-d", "--mcpu=gfx950", co], capture_output=True, text=True).stdout
            assert "s_endpgm" in dis, src
            bad = [l for l in dis.splitlines() if "v_pk_fma_f32" in l or "v_pk_add_f32" in l or "v_pk_mul_f32" in l]
            assert not bad, (src, bad[:3])
            total += dis.count("s_endpgm")
        assert total > 50
    assert os.path.exists(lib)
