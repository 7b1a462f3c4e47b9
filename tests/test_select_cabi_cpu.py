"""The C boundary of the batch-aware selection: include/gpfit_mi355x.h declares gpfit_pool_covariance and
gpfit_select_batch with the argument lists the ctypes table binds, the built library exports them, and the host module
offers pool_covariance, select_batch and select_round.  No compute call touches a GPU here."""
import os
import re

import pytest

from conftest import ROOT
from gaussian_processes_amd import _lib

NAMES = ("gpfit_pool_covariance", "gpfit_select_batch")


def _declaration(name):
    hdr = open(os.path.join(ROOT, "include", "gpfit_mi355x.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    found = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
    assert found, f"{name} is not declared in the header"
    return [a.strip() for a in found.group(1).split(",")]


@pytest.mark.parametrize("name", NAMES)
def test_header_declares_what_the_ctypes_table_binds(name):
    args = _declaration(name)
    assert name in _lib.exported_symbols()
    res, bound = _lib._SIGS[name]
    assert res is _lib.i32 and len(bound) == len(args), (len(bound), args)
    for decl, ctype in zip(args, bound):
        if "*" in decl:
            assert ctype in (_lib.vp, _lib.pd), decl
        elif decl.startswith("int64_t"):
            assert ctype is _lib.i64, decl
        elif decl.startswith("double"):
            assert ctype is _lib.f64, decl
        else:
            assert decl.startswith("int ") and ctype is _lib.i32, decl


def test_select_max_is_the_append_block():
    hdr = open(os.path.join(ROOT, "include", "gpfit_mi355x.h")).read()
    assert re.search(r"#define\s+GPFIT_SELECT_MAX\s+128\b", hdr)
    from gaussian_processes_amd import utils as gp
    assert gp.SELECT_MAX == 128 and gp.SHORTLIST == 1024 and gp.SHORTLIST <= gp.POOL_ROWS


def test_library_exports_both_symbols():
    from gaussian_processes_amd.build import build_library
    build_library(verbose=False)
    lib = _lib.load()
    for name in NAMES:
        assert hasattr(lib, name)


def test_host_module_argument_checks_need_no_gpu():
    from gaussian_processes_amd import utils as gp
    for name in ("pool_covariance", "select_batch", "select_round"):
        assert callable(getattr(gp, name)), name
    with pytest.raises(ValueError, match="n_select"):
        gp.select_batch([None], [None], [None], None, 0)
    with pytest.raises(ValueError, match="n_select"):
        gp.select_batch([None], [None], [None], None, 129)
    with pytest.raises(ValueError, match="units"):
        gp.select_batch([None] * 17, [None] * 17, [None] * 17, None, 8)
    with pytest.raises(ValueError, match="shortlist"):
        gp.select_round(None, [{}], 8, None, shortlist=gp.POOL_ROWS + 1)
    with pytest.raises(ValueError, match="cells"):
        gp.select_round(None, [], 8, None)
