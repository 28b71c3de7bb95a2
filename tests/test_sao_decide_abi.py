"""The SAO decision entries exist in every layer: declared in include/hmx.h, exported by libhmx.so, bound by thevc_amd/capi.py with
the arity of the declaration; the structures have the layout of the header; the new translation unit is part of both builds.
No GPU needed."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"hmx_sao_decide_multi": 10, "hmx_sao_decide": 9, "hmx_sao_encode_multi": 14, "hmx_sao_ctx_init": 3, "hmx_sao_rate_flags": 3,
           "hmx_sao_rate_update": 4, "hmx_sao_merge_allow": 6}


def header():
    return open(os.path.join(ROOT, "include", "hmx.h")).read()


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_header_declares(name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", header(), re.S)
    assert m, f"include/hmx.h does not declare int {name}"
    assert len([a for a in m.group(1).split(",") if a.strip()]) == ENTRIES[name]


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_library_exports_and_capi_binds(name):
    from thevc_amd import capi
    fn = getattr(capi.lib(), name)  # AttributeError: the symbol is not exported
    assert C.cast(fn, C.c_void_p).value
    assert fn.argtypes is not None and len(fn.argtypes) == ENTRIES[name] and fn.restype is C.c_int


def struct_fields(name):
    m = re.search(r"typedef struct " + name + r"\s*\{(.*?)\}\s*" + name + r"\s*;", header(), re.S)
    assert m, name
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    return [f for decl in body.split(";") for f in re.findall(r"(\w+)(?:\[[^\]]*\])*\s*(?:,|$)", decl.strip())]


def test_structures():
    from thevc_amd import capi
    assert struct_fields("hmx_sao_decide_param") == list(capi.SAO_DECIDE_PARAM_DTYPE.names) and capi.SAO_DECIDE_PARAM_DTYPE.itemsize == 24
    assert [capi.SAO_DECIDE_PARAM_DTYPE.fields[n][1] for n in capi.SAO_DECIDE_PARAM_DTYPE.names] == [0, 8, 16, 18, 20]
    assert struct_fields("hmx_sao_unit") == list(capi.SAO_UNIT_DTYPE.names) and capi.SAO_UNIT_DTYPE.itemsize == 8
    assert struct_fields("hmx_sao_result") == list(capi.SAO_RESULT_DTYPE.names) and capi.SAO_RESULT_DTYPE.itemsize == 16
    assert [capi.SAO_RESULT_DTYPE.fields[n][1] for n in capi.SAO_RESULT_DTYPE.names] == [0, 8, 10, 12]
    assert struct_fields("hmx_sao_lcu") == list(capi.SAO_LCU_DTYPE.names) and capi.SAO_LCU_DTYPE.itemsize == 6
    assert re.search(r"#define\s+HMX_SAO_RATE_DEPTHS\s+4\b", header()) and capi.SAO_RATE_DEPTHS == 4


def test_translation_unit_is_built_both_ways():
    import __graft_entry__ as g
    assert "hmx_saodec" in g.PARTS
    assert '#include "hmx_saodec.hip"' in open(os.path.join(ROOT, "thevc_amd", "csrc", "hmx_lib.hip")).read()
    text = open(os.path.join(ROOT, "thevc_amd", "csrc", "hmx_saodec.hip")).read()
    assert "#pragma clang fp contract(off)" in text


def test_header_points_from_the_statistics_to_the_decision():
    text = header()
    assert "everything after the statistics" not in text and "hmx_sao_decide_multi further down" in text
    for out_of_scope in ("rdoSaoOnePart", "runQuadTreeDecision", "SaoLcuBoundary", "writing the bitstream"):
        assert out_of_scope in text
