"""The kg_cycle_one boundary (ABI 13) without a GPU: the library exports the entry point, the header, the C struct
and the Python mirrors agree."""
import ctypes
import os
import re

from koordinator_amd import _native as nat

HEADER = os.path.join(os.path.dirname(__file__), "..", "include", "koord_gpu.h")


def test_library_exports_kg_cycle_one():
    L = nat.lib()
    assert hasattr(L, "kg_cycle_one")
    assert "kg_cycle_one" in nat.EXPORTED
    assert L.kg_cycle_one.restype is ctypes.c_int32 and len(L.kg_cycle_one.argtypes) == 6


def test_cycle_out_size_matches_the_mirrors():
    L = nat.lib()
    text = open(HEADER).read()
    ids = re.search(r"enum kg_struct_id \{(.*?)\}", text, flags=re.S).group(1)
    names = [n.split("=")[0].strip() for n in ids.replace("\n", " ").split(",") if n.strip()]
    assert names.index("KG_SID_CYCLE_OUT") == nat.SID_CYCLE_OUT == names.index("KG_SID_COUNT") - 1
    assert L.kg_struct_size(nat.SID_CYCLE_OUT) == ctypes.sizeof(nat.CycleOut) == nat.CYCLE_OUT.itemsize == 24
    assert nat.STRUCT_IDS[nat.SID_CYCLE_OUT] is nat.CYCLE_OUT   # check_abi's loop covers it
    for (name, ct), field in zip(nat.CycleOut._fields_, nat.CYCLE_OUT.names):
        assert name == field
        assert getattr(nat.CycleOut, name).offset == nat.CYCLE_OUT.fields[field][1]
        assert ctypes.sizeof(ct) == nat.CYCLE_OUT.fields[field][0].itemsize
    assert L.kg_struct_size(nat.SID_CYCLE_OUT + 1) <= 0   # KG_SID_COUNT is no struct


def test_header_cycle_commit_matches_python():
    text = open(HEADER).read()
    m = re.search(r"#define KG_CYCLE_COMMIT (0x[0-9a-fA-F]+)u", text)
    assert m and int(m.group(1), 16) == nat.CYCLE_COMMIT
    assert int(re.search(r"#define KG_ABI_VERSION (\d+)", text).group(1)) == nat.ABI_VERSION == 13
    assert nat.lib().kg_abi_version() == 13
