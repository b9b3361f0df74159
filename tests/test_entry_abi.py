"""CPU: the site-entry and head-set test primitives of the C ABI — tvr_site_entry and tvr_headset_apply — are
declared, exported, bound, documented as ABI-11 additions and refuse null arguments without a device."""
import ctypes
import re
from pathlib import Path

from tvr_amd import _lib

ROOT = Path(__file__).resolve().parents[1]
I32P, CF32P, F32P, VP = r"const\s+int32_t\s*\*\s*", r"const\s+float\s*\*\s*", r"float\s*\*\s*", r"void\s*\*\s*"
I32 = r"int32_t\s+"


def test_header_declares_and_library_exports_the_primitives():
    text = (ROOT / "include" / "tvr.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    sep = r"\s*,\s*"
    assert re.search(r"\bint\s+tvr_site_entry\s*\(\s*" + sep.join([
        r"tvr_model\s*\*\s*model", I32P + "seq_lens", I32 + "n_seq", I32P + "token_ids", I32 + "tokens", CF32P + "resid",
        CF32P + "z", r"const\s+tvr_site\s*\*\s*sites", I32 + "n_sites", I32P + "set_off",
        r"const\s+tvr_head_patch\s*\*\s*patches", CF32P + "vectors", I32 + "n_vectors", I32 + "flags", F32P + "out",
        I32 + "out_rows", r"int32_t\s*\*\s*site_row0", r"int32_t\s*\*\s*site_rows", r"int32_t\s*\*\s*site_p0",
        VP + "stream"]) + r"\s*\)", code)
    assert re.search(r"\bint\s+tvr_headset_apply\s*\(\s*" + sep.join([
        r"tvr_model\s*\*\s*model", I32 + "fmt", r"const\s+tvr_headset_item\s*\*\s*items", I32 + "n_items",
        r"const\s+tvr_headset_patch\s*\*\s*patches", I32 + "n_patches", CF32P + "vectors", I32 + "n_vectors",
        VP + "a2", F32P + "resid", I32 + "rows", VP + "stream"]) + r"\s*\)", code)
    assert re.search(r"typedef\s+struct\s+tvr_headset_item\s*\{\s*int32_t\s+row0\s*,\s*n_rows\s*,\s*first_patch\s*,"
                     r"\s*n_patches\s*;\s*\}", code)
    assert re.search(r"typedef\s+struct\s+tvr_headset_patch\s*\{\s*int32_t\s+head\s*,\s*vec\s*;\s*\}", code)
    assert re.search(r"TVR_ENTRY_FORCE_VALU\s*=\s*1\b", code) and _lib.ENTRY_FORCE_VALU == 1
    assert "#define TVR_ABI_VERSION 11" in text  # backward-compatible additions
    # each is documented as one: the comment that ends right before the declaration says so
    for decl in ("enum { TVR_ENTRY_FORCE_VALU", "typedef struct tvr_headset_item"):
        doc = text[:text.index(decl)].rstrip()
        assert doc.endswith("(Backward-compatible addition: ABI 11.) */"), decl
        assert "A test primitive" in doc[doc.rindex("/*"):]
    assert "tvr_site_entry does check" in text  # the plain sweep's vectors note points to the stricter check
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    assert hasattr(lib, "tvr_site_entry") and hasattr(lib, "tvr_headset_apply")
    assert _lib.load().tvr_abi_version() == _lib.ABI_VERSION == 11


def test_bound_signatures():
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    res, args = _lib.SIGNATURES["tvr_site_entry"]
    assert res is ctypes.c_int
    assert args == [vp, vp, i32, vp, i32, vp, vp, vp, i32, vp, vp, vp, i32, i32, vp, i32, vp, vp, vp, vp]
    res, args = _lib.SIGNATURES["tvr_headset_apply"]
    assert res is ctypes.c_int
    assert args == [vp, i32, vp, i32, vp, i32, vp, i32, vp, vp, i32, vp]
    assert ctypes.sizeof(_lib.CHeadsetItem) == 16 and [f for f, _ in _lib.CHeadsetItem._fields_] == [
        "row0", "n_rows", "first_patch", "n_patches"]
    assert ctypes.sizeof(_lib.CHeadsetPatch) == 8 and [f for f, _ in _lib.CHeadsetPatch._fields_] == ["head", "vec"]


def test_null_arguments_are_invalid_without_a_device():
    lib = _lib.load()
    buf = ctypes.cast((ctypes.c_int32 * 4)(), ctypes.c_void_p)
    rc = lib.tvr_site_entry(None, buf, 1, None, 4, buf, buf, buf, 1, None, None, None, 0, 0, buf, 4, buf, buf, buf, None)
    assert rc == _lib.TVR_ERR_INVALID and lib.tvr_last_error().startswith(b"tvr_site_entry: null model")
    rc = lib.tvr_site_entry(None, None, 0, None, 0, None, None, None, 0, None, None, None, 0, 0, None, 0, None, None,
                            None, None)
    assert rc == _lib.TVR_ERR_INVALID and lib.tvr_last_error().startswith(b"tvr_site_entry: null model")
    rc = lib.tvr_headset_apply(None, 0, buf, 1, buf, 1, buf, 1, buf, buf, 1, None)
    assert rc == _lib.TVR_ERR_INVALID and lib.tvr_last_error().startswith(b"tvr_headset_apply: null model")
    rc = lib.tvr_headset_apply(None, 0, None, 0, None, 0, None, 0, None, None, 0, None)
    assert rc == _lib.TVR_ERR_INVALID and lib.tvr_last_error().startswith(b"tvr_headset_apply: null model")
    # (the other refusals need a model, hence a device: tests/test_gpu_entry.py)
