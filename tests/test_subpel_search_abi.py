"""hmx_batch_subpel_search exists in every layer: declared in include/hmx.h, exported by libhmx.so, bound by thevc_amd/capi.py
with the arity of the declaration; hmx_subpel_result has the layout of the header.  No GPU needed."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    return open(os.path.join(ROOT, "include", "hmx.h")).read()


def test_header_declares_fifteen_arguments():
    m = re.search(r"\bint\s+hmx_batch_subpel_search\s*\(([^;]*?)\)\s*;", header(), re.S)
    assert m, "include/hmx.h does not declare hmx_batch_subpel_search"
    assert len([a for a in m.group(1).split(",") if a.strip()]) == 15


def test_library_exports_and_capi_binds():
    from thevc_amd import capi
    fn = capi.lib().hmx_batch_subpel_search  # AttributeError: the symbol is not exported
    assert C.cast(fn, C.c_void_p).value
    assert fn.argtypes is not None and len(fn.argtypes) == 15 and fn.restype is C.c_int


def test_result_structure():
    from thevc_amd import capi
    assert C.sizeof(capi.SubpelResult) == capi.SUBPEL_RESULT_DTYPE.itemsize == 12
    names = ("mvx", "mvy", "dist", "cost")
    assert [capi.SUBPEL_RESULT_DTYPE.fields[n][1] for n in names] == [getattr(capi.SubpelResult, n).offset for n in names] == [0, 2, 4, 8]
    m = re.search(r"typedef struct \{([^}]*)\}\s*hmx_subpel_result\s*;", header())
    assert m and re.findall(r"(\w+)\s*[,;]", m.group(1)) == list(capi.SUBPEL_RESULT_DTYPE.names)
    assert re.findall(r"(\w+)\s+\w+\s*[,;]", m.group(1))[0] == "int16_t"


def test_context_methods():
    from thevc_amd import capi
    for m in ("batch_subpel_search", "batch_fullpel_search_device", "batch_fullpel_search"):
        assert callable(getattr(capi.Context, m))


def test_neighbouring_entries_stay():
    from thevc_amd import capi
    L = capi.lib()
    assert len(L.hmx_batch_subpel_cost.argtypes) == 10 and len(L.hmx_batch_fullpel_search.argtypes) == 13
