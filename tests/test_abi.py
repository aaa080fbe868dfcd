"""CPU tests of the C ABI.  makani_amd/_lib.py derives its binding from include/makani_amd.h, so "binding == header" would be a
tautology: these tests pin the header parser against things written independently of it — signatures typed out by hand, the
struct layout a C compiler gives the header, the symbols of the built library, and the constants' values as numbers."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

from makani_amd import _lib, build
from makani_amd._lib import HEADER

HEADER_TEXT = open(HEADER).read()


def test_header_path_is_the_one_of_the_build():
    assert build.HEADER is HEADER and os.path.samefile(HEADER, os.path.join(ROOT, "include", "makani_amd.h"))


# ---- frozen signatures: between them every type of the header's vocabulary ------------------------------------------------------
_T = {"v": C.c_void_p, "i": C.c_int, "l": C.c_longlong, "f": C.c_float, "d": C.c_double, "s": C.c_char_p, "-": None}
FROZEN = {          # typed from the header by hand; G / S / A: pointer to MkGemm / MkFftSeg / MkAdamTensor
    "mk_si_assemble": ("v v i v v v i v i v i v d i i i i i i l v", "i"),                              # the double
    "mk_si_step": ("v l i v i v i v v i v i v i f f f f f i i i i i i l v", "i"),                      # the longest; a float run
    "mk_sgemm_presplit_batched": ("G v l l l i v v i v", "i"),                                         # struct pointer, long long run, const int*
    "mk_rfft_rows_seg": ("v i v v i i i i f f f S v", "i"),
    "mk_adamw_multi": ("A i v f f f f f i v v", "i"),
    "mk_conv1x1_wgrad_workspace": ("i i i l", "l"),                                                    # long long return
    "mk_noise_advance": ("v l v", "i"),                                                                # long long*
    "mk_rfft_rows": ("v i v v v i i i i i i i f f f v", "i"),                                          # the host radix array: a plain pointer
    "mk_last_error": ("", "s"),
    "mk_version": ("", "i"),
}


@pytest.mark.parametrize("name", sorted(FROZEN))
def test_frozen_signature(name):
    t = dict(_T, G=C.POINTER(_lib.MkGemm), S=C.POINTER(_lib.MkFftSeg), A=C.POINTER(_lib.MkAdamTensor))
    args, res = FROZEN[name]
    assert _lib._SIGS[name] == ([t[a] for a in args.split()], t[res])


def test_the_loaded_library_is_bound_as_parsed():
    _built_library()
    L = _lib.lib()
    assert len(_lib._SIGS) >= 108 and _lib.EXPORTS == sorted(_lib._SIGS)
    for name, (args, res) in _lib._SIGS.items():
        fn = getattr(L, name)
        assert list(fn.argtypes) == args and fn.restype is res, name
    assert isinstance(L.mk_last_error(), bytes)


# ---- struct layout against a C compiler -----------------------------------------------------------------------------------------
def _host_cc():
    rocm_clang = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang")
    return shutil.which("cc") or (rocm_clang if os.path.exists(rocm_clang) else None)


def test_struct_layout_matches_the_c_compiler(tmp_path):
    cc = _host_cc()
    if cc is None:
        pytest.skip("no host C compiler: neither cc nor the clang of the ROCm tree")
    structs = {"MkGemm": _lib.MkGemm, "MkFftSeg": _lib.MkFftSeg, "MkAdamTensor": _lib.MkAdamTensor}
    assert set(_lib.STRUCTS) == set(structs)
    assert {n: len(s._fields_) for n, s in structs.items()} == {"MkGemm": 28, "MkFftSeg": 8, "MkAdamTensor": 10}
    lines = [f'    printf("{n} %zu\\n", sizeof({n}));' for n in structs]
    lines += [f'    printf("{n}.{f} %zu\\n", offsetof({n}, {f}));' for n, s in structs.items() for f, _ in s._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "makani_amd.h"\nint main(void) {\n' + "\n".join(lines)
                   + "\n    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([cc, "-std=c99", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    want = {n: C.sizeof(s) for n, s in structs.items()}
    want.update({f"{n}.{f}": getattr(s, f).offset for n, s in structs.items() for f, _ in s._fields_})
    assert {k: int(v) for k, v in got.items()} == want
    # the figures the layout had when the hand-written mirrors were retired
    assert (want["MkGemm"], want["MkFftSeg"], want["MkAdamTensor"]) == (184, 616, 72)
    assert (want["MkFftSeg.base"], want["MkFftSeg.x_nlat"], want["MkAdamTensor.cols"]) == (80, 608, 56)
    assert [f for f, _ in _lib.MkGemm._fields_][:4] == ["A", "B", "C", "a_batch"] and _lib.MkGemm._fields_[-1][0] == "beta"


def test_struct_construction_by_position_and_keyword():
    t = _lib.MkAdamTensor(None, 64, None, None, 5, None, None, 3, 2, 1)
    assert (t.p, t.g, t.n, t.cols, t.ld, t.ld_t) == (None, 64, 5, 3, 2, 1)
    g = _lib.MkGemm(A=16, M=3, a_k=1, beta=1)
    assert (g.A, g.M, g.a_k, g.beta, g.N) == (16, 3, 1, 1, 0)
    s = _lib.MkFftSeg()
    assert len(s.m_off) == len(s.r_off) == 9 and len(s.base) == 8 and len(s.base[0]) == 8


# ---- library against header -----------------------------------------------------------------------------------------------------
def _built_library():
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return C.CDLL(_lib.LIB_PATH)


def test_library_exports_every_declared_symbol():
    L = _built_library()
    declared = set(re.findall(r"\b(mk_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", HEADER_TEXT, flags=re.S)))
    assert len(declared) >= 108
    assert set(_lib.EXPORTS) == declared, set(_lib.EXPORTS) ^ declared
    for sym in declared:
        assert hasattr(L, sym), f"{sym} declared in include/makani_amd.h but not exported"
    assert _lib.lib().mk_version() >= 100


def test_library_exports_nothing_the_header_does_not_declare():
    _built_library()
    nm = shutil.which("nm")
    if nm is None:
        pytest.skip("no nm to list the symbols of the library")
    out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {ln.split()[2] for ln in out.splitlines() if len(ln.split()) == 3 and ln.split()[1] == "T" and ln.split()[2].startswith("mk_")}
    assert exported == set(_lib.EXPORTS), exported ^ set(_lib.EXPORTS)


# ---- constants: the numbers the kernels were written against --------------------------------------------------------------------
def test_constants_have_the_values_the_kernels_use():
    from makani_amd import metrics as mm, noise, ops
    assert (_lib.MK_F32, _lib.MK_BF16, _lib.MK_FFT_SEG_MAX) == (0, 1, 8)
    assert (_lib.CONSTS["MK_EINVAL"], _lib.CONSTS["MK_EUNSUP"]) == (-1, -2)
    assert (_lib.TRI_NONE, _lib.TRI_ROW_GE, _lib.TRI_K_GE, _lib.TRI_ROW_LE, _lib.TRI_K_LE) == (0, 1, 2, 3, 4)
    assert (mm.SUM_L1, mm.SUM_L2, mm.SUM_XY, mm.SUM_XX, mm.SUM_YY) == (1, 2, 4, 8, 16)          # bit k selects slot k of out (B, C, 5)
    assert (mm.SUM_ALL, mm.SUM_ACC) == (31, 28)
    assert (mm.ENS_SKILL, mm.ENS_SPREAD, mm.ENS_HIST) == (1, 2, 4)
    assert (noise.MODE_WHITE, noise.MODE_AR, noise.MODE_REPLACE) == (0, 1, 2)
    assert (ops.CMIX_ROWS, ops.CMIX_LEVELS, ops.CMIX_RESID, ops.CMIX_Q_ROUNDTRIP) == (32, 16, 1, 2)
    # the static_assert of csrc/constraints.hip with ROWS = 32, LEV = 16: IT_COPY = 2 ROWS + 2 LEV, FT_CL + ROWS = 7 ROWS + 2 LEV + 4 ROWS^2
    assert (_lib.CONSTS["MK_CMIX_ITAB"], _lib.CONSTS["MK_CMIX_FTAB"]) == (96, 4352)
    assert len(_lib.CONSTS) == len(re.findall(r"^#define MK_\w+ +\S", HEADER_TEXT, re.M)) >= 27          # no #define skipped


# ---- the parser on doctored header text -----------------------------------------------------------------------------------------
def _doctor(old, new):
    assert HEADER_TEXT.count(old) == 1, old
    text = HEADER_TEXT.replace(old, new)
    return text, text[:text.index(new)].count("\n") + 1


def test_parser_names_an_unknown_parameter_type():
    text, line = _doctor("int mk_fft_seg_supported(int nlon);", "int mk_fft_seg_supported(unsigned nlon);")
    with pytest.raises(ValueError, match=rf"doctored\.h:{line}: mk_fft_seg_supported: type 'unsigned' is outside the vocabulary"):
        _lib.parse_header(text, "doctored.h")
    text, line = _doctor("int mk_version(void);", "short mk_version(void);")
    with pytest.raises(ValueError, match=rf"doctored\.h:{line}: mk_version: type 'short'"):
        _lib.parse_header(text, "doctored.h")
    text, line = _doctor("int mk_fft_seg_supported(int nlon);", "int mk_fft_seg_supported(const char* nlon);")          # a return type only
    with pytest.raises(ValueError, match=rf"doctored\.h:{line}: mk_fft_seg_supported: type 'const char\*'"):
        _lib.parse_header(text, "doctored.h")


def test_parser_reads_a_prototype_split_across_lines():
    text, _ = _doctor("int mk_noise_advance(long long* rng, long long n, void* stream);",
                      "int\nmk_noise_advance\n  (long\n long *rng,long   long\nn , void\n*\nstream)\n;")
    consts, structs, sigs = _lib.parse_header(text, "doctored.h")
    assert sigs["mk_noise_advance"] == ([C.c_void_p, C.c_longlong, C.c_void_p], C.c_int)
    assert list(sigs) == list(_lib._SIGS) and consts == _lib.CONSTS and list(structs) == list(_lib.STRUCTS)
    for name, (args, res) in sigs.items():          # (struct classes are made per parse: compare by name)
        assert [getattr(a, "__name__", a) for a in args] == [getattr(a, "__name__", a) for a in _lib._SIGS[name][0]], name


def test_parser_names_an_unknown_array_extent():
    text, line = _doctor("int m_off[MK_FFT_SEG_MAX + 1];", "int m_off[MK_FFT_SEGS + 1];")
    with pytest.raises(ValueError, match=rf"doctored\.h:{line}: struct MkFftSeg: 'MK_FFT_SEGS \+ 1' is not an integer constant "
                                         r"expression \(unknown name MK_FFT_SEGS\)"):
        _lib.parse_header(text, "doctored.h")
    text, line = _doctor("    long long x_stride;", "    unsigned x_stride;")
    with pytest.raises(ValueError, match=rf"doctored\.h:{line}: struct MkFftSeg: type 'unsigned'"):
        _lib.parse_header(text, "doctored.h")


def test_parser_skips_nothing():
    text, line = _doctor("int mk_version(void);", "int mk_version(void) { return 1; }")          # not a prototype: named, not skipped
    with pytest.raises(ValueError, match=rf"doctored\.h:{line}: "):
        _lib.parse_header(text, "doctored.h")
    text, line = _doctor("int mk_version(void);", "int mk_version(void);\nenum mk_mode { A };")
    with pytest.raises(ValueError, match=rf"doctored\.h:{line + 1}: not a prototype"):
        _lib.parse_header(text, "doctored.h")


def test_constant_expressions_admit_integers_names_and_three_operators_only():
    names = {"MK_A": 3}
    assert _lib._const_expr("(2 * MK_A + 1) * MK_A - 4", names) == 17 and _lib._const_expr("-1", names) == -1
    for bad in ("MK_B", "2 ** 3", "4 / 2", "1.5", "__import__('os')", "MK_A if 1 else 2", "(1, 2)", "1 +", "'a'"):
        with pytest.raises(ValueError, match="not an integer constant expression"):
            _lib._const_expr(bad, names)
    text, line = _doctor("#define MK_CMIX_LEVELS 16", "#define MK_CMIX_LEVELS sizeof(int)")
    with pytest.raises(ValueError, match=rf"doctored\.h:{line}: MK_CMIX_LEVELS: "):
        _lib.parse_header(text, "doctored.h")
