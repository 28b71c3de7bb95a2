"""The batched loop-filter entries (hmx_deblock_strengths_multi, hmx_deblock_picture_multi, hmx_sao_picture_multi) exist
in every layer: declared in include/hmx.h, exported by libhmx.so, bound by thevc_amd/capi.py with the arity of the
declaration.  No GPU needed."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"hmx_deblock_strengths_multi": 10, "hmx_deblock_picture_multi": 11, "hmx_sao_picture_multi": 8}


def declared_arity(name):
    text = open(os.path.join(ROOT, "include", "hmx.h")).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, re.S)
    assert m, f"include/hmx.h does not declare {name}"
    return len([a for a in m.group(1).split(",") if a.strip()])


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_header_declares(name):
    assert declared_arity(name) == ENTRIES[name]


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_library_exports_and_capi_binds(name):
    from thevc_amd import capi
    L = capi.lib()
    fn = getattr(L, name)  # AttributeError: the symbol is not exported
    assert C.cast(fn, C.c_void_p).value
    assert fn.argtypes is not None and len(fn.argtypes) == declared_arity(name)


def test_context_methods():
    from thevc_amd import capi
    for m in ("deblock_strengths", "deblock_pictures", "sao_pictures"):
        assert callable(getattr(capi.Context, m))


def test_single_picture_entries_stay():
    from thevc_amd import capi
    L = capi.lib()
    for name, n in (("hmx_deblock_strengths", 9), ("hmx_deblock_picture", 10), ("hmx_sao_picture", 7)):
        assert len(getattr(L, name).argtypes) == n == declared_arity(name)
