"""CPU: the validation entry points added after ABI 6 without a version bump (cmlpl_eval_workspace_bytes,
cmlpl_infer_pixels, cmlpl_confusion): header and binding agree on the prototypes, the library exports them, the version
is still 6, and every malformed call comes back with the documented code from the argument checks, which run in front
of any launch (so these calls need no GPU: the pointers are never followed)."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_SHAPE, E_WORKSPACE = -1, -2, -3
FAKE = 0x10000          # a non-null "device pointer" (never dereferenced)
NEW = ("cmlpl_eval_workspace_bytes", "cmlpl_infer_pixels", "cmlpl_confusion")


def _prototype(name):
    """parameter types of `name` in include/cmlpl.h, comments stripped: ('const cmlpl_shape*', 'int', ...)"""
    text = open(os.path.join(ROOT, "include", "cmlpl.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    m = re.search(r"\b(size_t|int)\s+%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, f"{name} is not declared in cmlpl.h"
    params = []
    for prm in m.group(2).split(","):
        toks = prm.split()
        ty = " ".join(toks[:-1])
        stars = toks[-1].count("*")
        params.append(ty + "*" * stars if stars else ty)
    return m.group(1), tuple(p.replace(" *", "*") for p in params)


def _ctype_of(c_type):
    from cmlpl_amd import _lib
    if c_type == "const cmlpl_shape*":
        return C.POINTER(_lib.Shape)
    if c_type.endswith("*"):
        return C.c_void_p
    return {"int": C.c_int, "int64_t": C.c_int64, "size_t": C.c_size_t}[c_type]


def test_header_binding_and_library_agree():
    from cmlpl_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION == 6 and lib.cmlpl_abi_version() == 6
    for name in NEW:
        assert name in _lib.EXPORTS, name
        ret, params = _prototype(name)
        fn = getattr(lib, name)                         # exported
        assert [_ctype_of(p) for p in params] == list(fn.argtypes), (name, params, fn.argtypes)
        assert fn.restype is (C.c_size_t if ret == "size_t" else C.c_int), name
    assert len(_prototype("cmlpl_infer_pixels")[1]) == 18 and len(_prototype("cmlpl_confusion")[1]) == 8
    header = open(os.path.join(ROOT, "include", "cmlpl.h")).read()
    assert "ADDED AFTER ABI 6 WITHOUT A VERSION BUMP" in header


def test_a_library_without_the_new_symbols_is_refused(tmp_path, monkeypatch):
    """the binding's existing error: a stale library is reported, not half-used"""
    import pytest
    from cmlpl_amd import _lib
    stale = tmp_path / "libstale.so"
    import shutil
    import subprocess
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    (tmp_path / "s.c").write_text("int cmlpl_abi_version(void) { return 6; }\n")
    subprocess.run([cc, "-shared", "-fPIC", str(tmp_path / "s.c"), "-o", str(stale)], check=True)
    monkeypatch.setattr(_lib, "_lib", None)
    with pytest.raises(_lib.CmlplLibraryError) as e:
        _lib.load(str(stale))
    assert "cmlpl_infer_pixels" in str(e.value) and "cmlpl_confusion" in str(e.value)


def _infer(lib, shape, nets=2, params=FAKE, pstride=1 << 24, packed=FAKE, kstride=1 << 24, cube=FAKE, rows=64, cols=64,
           spectra=FAKE, spec_row=None, pix=FAKE, n=16, labels=FAKE, logits=None, ws=FAKE, ws_bytes=1 << 30):
    from cmlpl_amd import _lib
    cs = _lib.Shape(*shape)
    return lib.cmlpl_infer_pixels(C.byref(cs), nets, params, pstride, packed, kstride, cube, rows, cols, spectra, spec_row,
                                  pix, n, labels, logits, ws, ws_bytes, None)


B2, P = (103, 11, 11, 103, 9), (60, 20, 20, 103, 9)


def test_infer_pixels_argument_checks():
    from cmlpl_amd import _lib
    lib = _lib.load()
    for null in ("params", "packed", "cube", "spectra", "pix", "labels", "ws"):
        assert _infer(lib, B2, **{null: None}) == E_ARG, null
    assert _infer(lib, B2, n=0) == E_ARG
    assert _infer(lib, B2, nets=0) == E_ARG and _infer(lib, B2, nets=3) == E_ARG
    assert _infer(lib, B2, rows=4) == E_ARG and _infer(lib, B2, cols=4) == E_ARG       # smaller than half an 11-window
    assert _infer(lib, B2, pstride=8) == E_ARG                                        # two networks closer than one network
    assert _infer(lib, P) == E_SHAPE                                                  # 400 window pixels: by patches
    assert _infer(lib, (103, 11, 11, 103, 65)) == E_SHAPE                             # K > 64
    assert _infer(lib, (103, 11, 9, 103, 9)) == E_SHAPE                               # not square
    assert _infer(lib, B2, ws_bytes=16 * 2 * 4096 - 1) == E_WORKSPACE
    cs = _lib.Shape(*B2)
    assert lib.cmlpl_eval_workspace_bytes(C.byref(cs), 2, 16) == 16 * 2 * 4096
    assert lib.cmlpl_eval_workspace_bytes(C.byref(cs), 1, 16) == lib.cmlpl_infer_workspace_bytes(C.byref(cs), 16)
    assert lib.cmlpl_eval_workspace_bytes(C.byref(cs), 3, 16) == 0 and lib.cmlpl_eval_workspace_bytes(C.byref(cs), 2, 0) == 0
    assert lib.cmlpl_eval_workspace_bytes(C.byref(_lib.Shape(*P)), 2, 16) == 0


def test_confusion_argument_checks():
    from cmlpl_amd import _lib
    lib = _lib.load()
    ok = dict(pred=FAKE, nets=2, truth=FAKE, n=10, K=9, cm=FAKE, ign=None)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.cmlpl_confusion(a["pred"], a["nets"], a["truth"], a["n"], a["K"], a["cm"], a["ign"], None)
    for null in ("pred", "truth", "cm"):
        assert call(**{null: None}) == E_ARG, null
    assert call(n=0) == E_ARG and call(nets=0) == E_ARG and call(nets=3) == E_ARG
    assert call(K=0) == E_ARG and call(K=65) == E_ARG
