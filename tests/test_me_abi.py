"""The integer motion search entries (hmx_mvBits, hmx_mvCost, hmx_setSearchRange, hmx_getSAD, hmx_batch_fullpel_search) exist in
every layer: declared in include/hmx.h, exported by libhmx.so, bound by thevc_amd/capi.py with the arity of the declaration;
the two structures have the layout of the header; the three host helpers equal tests/me_oracle.py.  No GPU needed."""
import ctypes as C
import os
import re

import pytest

import me_oracle as mo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"hmx_mvBits": ("uint32_t", 5), "hmx_mvCost": ("uint32_t", 6), "hmx_setSearchRange": ("void", 12), "hmx_getSAD": ("int", 9),
           "hmx_batch_fullpel_search": ("int", 13)}


def declared_arity(name, ret="int"):
    text = open(os.path.join(ROOT, "include", "hmx.h")).read()
    m = re.search(r"\b" + ret + r"\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, re.S)
    assert m, f"include/hmx.h does not declare {ret} {name}"
    return len([a for a in m.group(1).split(",") if a.strip()])


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_header_declares(name):
    assert declared_arity(name, ENTRIES[name][0]) == ENTRIES[name][1]


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_library_exports_and_capi_binds(name):
    from thevc_amd import capi
    L = capi.lib()
    fn = getattr(L, name)  # AttributeError: the symbol is not exported
    assert C.cast(fn, C.c_void_p).value
    assert fn.argtypes is not None and len(fn.argtypes) == ENTRIES[name][1]
    assert fn.restype is {"uint32_t": C.c_uint32, "void": None, "int": C.c_int}[ENTRIES[name][0]]


def test_structures():
    from thevc_amd import capi
    assert C.sizeof(capi.MeUnit) == capi.ME_UNIT_DTYPE.itemsize == 20
    assert C.sizeof(capi.MeResult) == capi.ME_RESULT_DTYPE.itemsize == 12
    names = ("x", "y", "w", "h", "ref", "sub_shift", "pred_x", "pred_y", "left", "top", "right", "bottom")
    assert [capi.ME_UNIT_DTYPE.fields[n][1] for n in names] == [getattr(capi.MeUnit, n).offset for n in names] == \
        [0, 2, 4, 5, 6, 7, 8, 10, 12, 14, 16, 18]
    names = ("mvx", "mvy", "sad", "cost")
    assert [capi.ME_RESULT_DTYPE.fields[n][1] for n in names] == [getattr(capi.MeResult, n).offset for n in names] == [0, 2, 4, 8]
    text = open(os.path.join(ROOT, "include", "hmx.h")).read()
    m = re.search(r"typedef struct \{((?:(?!typedef).)*?)\}\s*hmx_me_unit\s*;", text, re.S)  # a comment of the body holds braces
    assert m and re.findall(r"(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)) == list(capi.ME_UNIT_DTYPE.names)
    m = re.search(r"typedef struct \{([^}]*)\}\s*hmx_me_result\s*;", text)
    assert m and re.findall(r"(\w+)\s*[,;]", m.group(1)) == list(capi.ME_RESULT_DTYPE.names)


def test_context_methods_and_module_functions():
    from thevc_amd import capi, workload
    for m in ("getSAD", "batch_fullpel_search"):
        assert callable(getattr(capi.Context, m))
    for f in ("mv_bits", "mv_cost", "set_search_range"):
        assert callable(getattr(capi, f))
    u = workload.make_me_units(5, 192, 128, 2, 9)
    assert u.dtype == capi.ME_UNIT_DTYPE and len(u) > 10 and set(u["w"]) <= set(mo.SIZES) and set(u["h"]) <= set(mo.SIZES)
    for r in u:
        assert (int(r["left"]), int(r["top"]), int(r["right"]), int(r["bottom"])) == \
            mo.set_search_range(int(r["pred_x"]), int(r["pred_y"]), 9, int(r["x"]), int(r["y"]), 192, 128)
        assert r["sub_shift"] == 0 or r["h"] > 8


PREDS = [(0, 0), (1, -1), (-3, 7), (255, -256), (-511, 333), (6, 2)]  # quarter samples: zero, odd, negative, large


def test_mv_bits_and_cost_vs_oracle():
    from thevc_amd import capi
    lambdas = [0, 1, 65535, 65536, 1234567, 0x7FFFFFFF, 0xFFFFFFFF]  # the last two: lambda * bits wraps 2^32
    n = 0
    for px, py in PREDS:
        for x in (-64, -17, -1, 0, 1, 2, 33, 64):
            for y in (-64, -2, 0, 1, 63):
                for sc in (0, 1, 2):
                    assert capi.mv_bits(x, y, px, py, sc) == mo.mv_bits(x, y, px, py, sc), (x, y, px, py, sc)
                for lam in lambdas:
                    assert capi.mv_cost(lam, x, y, px, py, 2) == mo.mv_cost(lam, x, y, px, py, 2), (lam, x, y, px, py)
                    n += 1
    assert mo.mv_cost(0xFFFFFFFF, 64, 64, 0, 0, 2) != (0xFFFFFFFF * mo.mv_bits(64, 64, 0, 0, 2)) >> 16  # the wrap is exercised
    assert n > 1000


def test_set_search_range_vs_oracle():
    from thevc_amd import capi
    W, H = 192, 128
    corners = [(0, 0), (W - 64, 0), (0, H - 64), (W - 64, H - 64), (W - 8, H - 8), (64, 64)]
    for cu_x, cu_y in corners:
        for px, py in PREDS + [(-400, -400), (400, 400), (-400, 400)]:
            for rng_ in (1, 4, 9, 64):
                got = capi.set_search_range(px, py, rng_, cu_x, cu_y, W, H, 64)
                assert got == mo.set_search_range(px, py, rng_, cu_x, cu_y, W, H, 64), (cu_x, cu_y, px, py, rng_)
                assert got[0] <= got[2] and got[1] <= got[3]


def test_existing_inter_entries_stay():
    from thevc_amd import capi
    L = capi.lib()
    for name, n in (("hmx_batch_subpel_cost", 10), ("hmx_motionCompensation", 10), ("hmx_batch_motionCompensation", 6),
                    ("hmx_batch_motionCompensation_multi", 3), ("hmx_getSSE", 8), ("hmx_calcHAD", 8)):
        assert len(getattr(L, name).argtypes) == n == declared_arity(name)
