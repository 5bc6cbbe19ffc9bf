"""The eight *Info classes of speck_amd.api without a GPU: each wraps its C struct of include/speck_c_api.h -- the class
name, every attribute as int (a tuple of ints for an array field) and the repr, character for character."""
import pytest

import speck_amd
from speck_amd import _lib

# (class name, the C struct, its fields filled with distinct small integers, the repr of the wrapped struct)
CASES = [
    ("SortInfo", _lib.CSortInfo, dict(rows_in_order=1, rows_sorted=(2, 3, 4), duplicates=5, nnz_out=6),
     "SortInfo(rows_in_order=1, rows_sorted=(2, 3, 4), duplicates=5, nnz_out=6)"),
    ("MaskedInfo", _lib.CMaskedInfo, dict(rows_idle=1, rows_class=(2, 3, 4), products=5, hits=6, nnz_out=7),
     "MaskedInfo(rows_idle=1, rows_class=(2, 3, 4), products=5, hits=6, nnz_out=7)"),
    ("SelectInfo", _lib.CSelectInfo, dict(kept=1, dropped=2, rows_unchanged=3, nnz_out=4),
     "SelectInfo(kept=1, dropped=2, rows_unchanged=3, nnz_out=4)"),
    ("AddInfo", _lib.CAddInfo, dict(only_a=1, only_b=2, both=3, nnz_out=4),
     "AddInfo(only_a=1, only_b=2, both=3, nnz_out=4)"),
    ("ReduceInfo", _lib.CReduceInfo, dict(rows_empty=1, rows_split=2, tiles=3, entries=4),
     "ReduceInfo(rows_empty=1, rows_split=2, tiles=3, entries=4)"),
    ("ScaleInfo", _lib.CScaleInfo, dict(entries=1, nonfinite=2, tiles=3),
     "ScaleInfo(entries=1, nonfinite=2, tiles=3)"),
    ("SpmvInfo", _lib.CSpmvInfo, dict(rows_empty=1, rows_split=2, tiles=3, entries=4),
     "SpmvInfo(rows_empty=1, rows_split=2, tiles=3, entries=4)"),
    ("SpmmInfo", _lib.CSpmmInfo, dict(rows_empty=1, rows_split=2, tiles=3, entries=4, terms=5),
     "SpmmInfo(rows_empty=1, rows_split=2, tiles=3, entries=4, terms=5)"),
]


@pytest.mark.parametrize("name, cstruct, values, text", CASES, ids=[c[0] for c in CASES])
def test_info_class_wraps_its_c_struct(name, cstruct, values, text):
    assert [f for f, _ in cstruct._fields_] == list(values)  # (the case names every field of the struct, in its order)
    c = cstruct()
    for field, v in values.items():
        if isinstance(v, tuple):
            for i, x in enumerate(v):
                getattr(c, field)[i] = x
        else:
            setattr(c, field, v)
    cls = getattr(speck_amd, name)
    assert cls is getattr(speck_amd.api, name) and cls.__name__ == name
    info = cls(c)
    assert type(info).__name__ == name
    assert vars(info) == values
    for field, v in values.items():
        got = getattr(info, field)
        assert got == v
        assert all(type(x) is int for x in got) and type(got) is tuple if isinstance(v, tuple) else type(got) is int
    assert repr(info) == text
