"""CPU checks of the multi-view training ABI (include/egr_raytracer.h: egr_train_batch, egr_train_views): the ctypes mirror against the header text,
the exported symbol, and a NULL context."""
import importlib
import os
import re

import pytest

pytest.importorskip("torch")
PKG = "editable-gaussian-reflections_amd"
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "egr_raytracer.h")


def header_fields(struct):
    hdr = open(HEADER).read()
    body = re.search(r"typedef struct " + struct + r" \{(.*?)\} " + struct + ";", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [re.sub(r"\[.*?\]", "", part.strip().split()[-1].lstrip("*")) for decl in body.split(";") if decl.strip() for part in decl.split(",")]


def test_train_batch_mirror_matches_the_header():
    cabi = importlib.import_module(PKG + ".c_abi")
    assert [f[0] for f in cabi.egr_train_batch._fields_] == header_fields("egr_train_batch")
    assert header_fields("egr_train_batch")[:1] == ["num_views"]
    assert set(cabi.TRAIN_BATCH_TARGETS) <= set(header_fields("egr_train_batch"))
    # the field types: one uint32, three device pointers, two floats, six device pointers
    C = importlib.import_module("ctypes")
    types = [f[1] for f in cabi.egr_train_batch._fields_]
    assert types == [C.c_uint32] + [C.c_void_p] * 3 + [C.c_float] * 2 + [C.c_void_p] * 6


def test_train_views_is_exported_and_declared():
    cabi = importlib.import_module(PKG + ".c_abi")
    L = cabi.lib()
    assert hasattr(L, "egr_train_views")
    assert re.search(r"\bint egr_train_views\(egr_context \*ctx, const egr_train_batch \*batch, void \*hip_stream\);", open(HEADER).read())
    assert L.egr_train_views.argtypes is not None


def test_null_context_is_refused():
    cabi = importlib.import_module(PKG + ".c_abi")
    L = cabi.lib()
    b = cabi.egr_train_batch(num_views=1)
    assert L.egr_train_views(None, b, None) != 0  # refused, not dereferenced
    assert L.egr_train_views(None, None, None) != 0
