"""CPU: the normalisation test primitives of the C ABI — tvr_lnpre_rows and tvr_center_rows — are declared,
exported, bound, documented as ABI-11 additions, the header's argument struct and the ctypes one agree field
for field, and null arguments are refused without a device."""
import ctypes
import re
from pathlib import Path

from tvr_amd import _lib

ROOT = Path(__file__).resolve().parents[1]
CTYPE = {"int32_t": ctypes.c_int32, "float": ctypes.c_float}


def header():
    text = (ROOT / "include" / "tvr.h").read_text()
    return text, re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def header_fields(code, name):
    """[(field, ctype)] of ``typedef struct name { .. } name;`` in declaration order (pointers: c_void_p)."""
    body = re.search(r"typedef\s+struct\s+" + name + r"\s*\{(.*?)\}\s*" + name + r"\s*;", code, flags=re.S).group(1)
    out = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        m = re.fullmatch(r"(?:const\s+)?(\w+)\s*(\*?)\s*(.+)", decl, flags=re.S)
        base, star, names = m.group(1), m.group(2), m.group(3)
        for n in (n.strip() for n in names.split(",")):
            ptr = bool(star) or n.startswith("*")
            out.append((n.lstrip("* "), ctypes.c_void_p if ptr else CTYPE[base]))
    return out


def test_header_declares_and_library_exports_the_primitives():
    text, code = header()
    sep = r"\s*,\s*"
    assert re.search(r"\bint\s+tvr_lnpre_rows\s*\(\s*" + sep.join([
        r"tvr_model\s*\*\s*model", r"const\s+tvr_lnpre_args\s*\*\s*args", r"void\s*\*\s*stream"]) + r"\s*\)", code)
    assert re.search(r"\bint\s+tvr_center_rows\s*\(\s*" + sep.join([
        r"const\s+float\s*\*\s*src", r"float\s*\*\s*dst", r"int32_t\s+rows", r"int32_t\s+d", r"void\s*\*\s*stream"]) +
                     r"\s*\)", code)
    assert "#define TVR_ABI_VERSION 11" in text  # backward-compatible additions
    for decl in ("typedef struct tvr_lnpre_args", "int tvr_center_rows("):
        doc = text[:text.index(decl)].rstrip()
        assert doc.endswith("(Backward-compatible addition: ABI 11.) */"), decl
        assert "A test primitive" in doc[doc.rindex("/*"):]
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    assert hasattr(lib, "tvr_lnpre_rows") and hasattr(lib, "tvr_center_rows")
    assert _lib.load().tvr_abi_version() == _lib.ABI_VERSION == 11


def test_args_struct_matches_the_header_field_for_field():
    _, code = header()
    want = header_fields(code, "tvr_lnpre_args")
    got = list(_lib.CLnpreArgs._fields_)
    assert [n for n, _ in got] == [n for n, _ in want] == [
        "fmt", "rows", "d", "ldx", "ldy", "x_rows", "copy_rows", "eps", "x", "row_idx", "y", "stats", "copy", "g1", "g2",
        "y2"]
    assert got == want
    # seven int32 and a float, then eight pointers: no padding anywhere
    assert ctypes.sizeof(_lib.CLnpreArgs) == 8 * 4 + 8 * ctypes.sizeof(ctypes.c_void_p)
    assert _lib.CLnpreArgs.x.offset == 32 and _lib.CLnpreArgs.eps.offset == 28


def test_bound_signatures():
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    res, args = _lib.SIGNATURES["tvr_lnpre_rows"]
    assert res is ctypes.c_int and args == [vp, ctypes.POINTER(_lib.CLnpreArgs), vp]
    res, args = _lib.SIGNATURES["tvr_center_rows"]
    assert res is ctypes.c_int and args == [vp, vp, i32, i32, vp]


def test_null_arguments_are_invalid_without_a_device():
    lib = _lib.load()
    buf = ctypes.cast((ctypes.c_float * 8)(), ctypes.c_void_p)
    assert lib.tvr_lnpre_rows(None, None, None) == _lib.TVR_ERR_INVALID
    assert lib.tvr_last_error().startswith(b"tvr_lnpre_rows: null args")
    a = _lib.CLnpreArgs(fmt=0, rows=1, d=4, ldx=4, ldy=4, x_rows=1, eps=1e-5)
    assert lib.tvr_lnpre_rows(None, ctypes.byref(a), None) == _lib.TVR_ERR_INVALID
    assert lib.tvr_last_error().startswith(b"tvr_lnpre_rows: null x")
    a.x = buf
    assert lib.tvr_lnpre_rows(None, ctypes.byref(a), None) == _lib.TVR_ERR_INVALID
    assert lib.tvr_last_error().startswith(b"tvr_lnpre_rows: null y")
    assert lib.tvr_center_rows(None, buf, 1, 4, None) == _lib.TVR_ERR_INVALID
    assert lib.tvr_last_error().startswith(b"tvr_center_rows: null")
    assert lib.tvr_center_rows(buf, None, 1, 4, None) == _lib.TVR_ERR_INVALID
    assert lib.tvr_center_rows(buf, buf, 0, 4, None) == _lib.TVR_ERR_INVALID
    assert lib.tvr_last_error().startswith(b"tvr_center_rows: rows and d")
    # (the other refusals are checked next to the launches: tests/test_gpu_norm.py)
