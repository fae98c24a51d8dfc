"""CPU tests (no GPU) of bv_engine_tiles_add_sparse_many, the batched form of bv_engine_tiles_add_sparse: the public header
declares it, the built library exports it, the ctypes layer binds it with its prototype, and a call without an engine is
refused before anything touches a device."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "bv_engine_tiles_add_sparse_many"


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from basevar_amd import _capi
    return _capi.load()


def test_header_declares_the_batched_packed_tile_call():
    hdr = open(os.path.join(ROOT, "include", "basevar_amd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"int\s+%s\s*\(([^)]*)\)\s*;" % NAME, hdr)
    assert m, "include/basevar_amd.h does not declare %s" % NAME
    params = [p.strip() for p in m.group(1).split(",")]
    assert params == ["bv_engine *e", "uint32_t n_tiles", "const bv_sparse_tile *tiles", "void *stream"], params
    assert re.search(r"#define BV_ABI_VERSION 2\b", open(os.path.join(ROOT, "include", "basevar_amd.h")).read())


def test_library_exports_it_and_capi_binds_it(lib):
    from basevar_amd import _capi
    assert NAME in _capi.EXPORTS
    fn = getattr(lib, NAME)
    assert fn.restype is C.c_int
    assert list(fn.argtypes) == [C.c_void_p, C.c_uint32, C.POINTER(_capi.SparseTile), C.c_void_p]
    from basevar_amd.engine import BaseTypeEngine
    assert callable(getattr(BaseTypeEngine, "tiles_add_sparse_many", None))


def test_without_an_engine_the_call_is_refused(lib):
    from basevar_amd import _capi
    tiles = (_capi.SparseTile * 2)()
    assert getattr(lib, NAME)(None, 2, tiles, None) == _capi.BV_ERR_INVALID_ARG
    assert NAME.encode() in lib.bv_last_error(None)
    assert getattr(lib, NAME)(None, 0, None, None) == _capi.BV_ERR_INVALID_ARG
