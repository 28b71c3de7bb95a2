"""The weighted-prediction entries (hmx_addWeightUni, hmx_addWeightBi, hmx_motionCompensation_wp,
hmx_batch_motionCompensation_wp_multi) exist in every layer: declared in include/hmx.h, exported by libhmx.so, bound by
thevc_amd/capi.py with the arity of the declaration; the two structures have the layout of the header.  No GPU needed."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"hmx_addWeightUni": 10, "hmx_addWeightBi": 14, "hmx_motionCompensation_wp": 12, "hmx_batch_motionCompensation_wp_multi": 4}


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


def test_structures():
    from thevc_amd import capi
    assert C.sizeof(capi.Wp) == 16
    assert C.sizeof(capi.McWp) == 2 * C.sizeof(C.c_void_p)
    assert capi.WP_DTYPE.itemsize == 16
    assert [capi.WP_DTYPE.fields[n][1] for n in ("weight", "offset", "log2_denom", "reserved")] == \
        [getattr(capi.Wp, n).offset for n in ("weight", "offset", "log2_denom", "reserved")] == [0, 6, 12, 15]
    text = open(os.path.join(ROOT, "include", "hmx.h")).read()
    assert re.search(r"\}\s*hmx_wp\s*;", text) and re.search(r"\}\s*hmx_mc_wp\s*;", text)


def test_context_methods_and_table_helper():
    import numpy as np
    from thevc_amd import capi
    for m in ("addWeightUni", "addWeightBi", "motion_compensation_wp", "batch_motion_compensation_wp"):
        assert callable(getattr(capi.Context, m))
    l0 = np.zeros(2, capi.WP_DTYPE)
    l0["weight"], l0["offset"], l0["log2_denom"] = [[1, 2, 3], [-4, 5, 255]], [[0, -128, 127], [1, 2, 3]], [[7, 0, 1], [2, 2, 2]]
    arr, keep = capi.mc_wp_array([(l0, None), None])
    assert len(arr) == 2 and not arr[0].l1 and not arr[1].l0 and not arr[1].l1
    assert list(arr[0].l0[1].weight) == [-4, 5, 255] and list(arr[0].l0[0].offset) == [0, -128, 127] and list(arr[0].l0[0].log2_denom) == [7, 0, 1]
    e = capi.wp_entry([1, 2, 3], [4, 5, 6], [7, 6, 5])
    assert (list(e.weight), list(e.offset), list(e.log2_denom)) == ([1, 2, 3], [4, 5, 6], [7, 6, 5])


def test_unweighted_entries_stay():
    from thevc_amd import capi
    L = capi.lib()
    for name, n in (("hmx_motionCompensation", 10), ("hmx_batch_motionCompensation", 6), ("hmx_batch_motionCompensation_multi", 3), ("hmx_addAvg", 9)):
        assert len(getattr(L, name).argtypes) == n == declared_arity(name)
