"""CPU-side checks of the block append (gpfit_potrf_append_block, utils.cholesky_append_block): the library builds
with it, header, ctypes table and library agree on the symbol, and every argument check answers before the context or
the device is touched.  No call reaches a GPU here."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT
from gaussian_processes_amd import _lib
from gaussian_processes_amd.build import build_library

NAME = "gpfit_potrf_append_block"


@pytest.fixture(scope="module")
def lib():
    build_library(verbose=False)
    return _lib.load()


def test_symbol_is_declared_listed_and_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "gpfit_mi355x.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+" + NAME + r"\s*\(", hdr), "not declared in the header"
    assert NAME in _lib.exported_symbols()
    assert hasattr(lib, NAME)


def _call(lib, ctx, n, k, ldl=None, ldi=None, ldk=None, L=True, Li=True, Kc=True):
    """The call with dummy (host) pointers: legal only for arguments the checks refuse before anything is dereferenced."""
    buf = (ctypes.c_double * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    logdet, info = ctypes.c_double(1.5), ctypes.c_int(-7)
    rc = lib.gpfit_potrf_append_block(ctx, None, p if L else None, n + k if ldl is None else ldl, p if Li else None,
                                      n + k if ldi is None else ldi, n, k, p if Kc else None, max(k, 1) if ldk is None else ldk,
                                      ctypes.byref(logdet), ctypes.byref(info))
    return rc, lib.gpfit_last_error().decode(), logdet.value


def test_null_context_is_refused(lib):
    rc, msg, logdet = _call(lib, None, 100, 4)
    assert rc == -3 and NAME in msg and logdet == 1.5


@pytest.mark.parametrize("k", [0, 129, -1])
def test_k_outside_1_to_128_is_refused_before_the_context_is_read(lib, k):
    # a context pointer that is not a context: the answer must come from the arguments alone
    fake = (ctypes.c_double * 8)()
    rc, msg, logdet = _call(lib, ctypes.cast(fake, ctypes.c_void_p), 100, k)
    assert rc == -3 and NAME in msg and "128" in msg and logdet == 1.5


def test_other_argument_checks_come_before_the_context_is_read(lib):
    fake = ctypes.cast((ctypes.c_double * 8)(), ctypes.c_void_p)
    for kw in (dict(n=0, k=4), dict(n=100, k=4, ldl=103), dict(n=100, k=4, ldi=103), dict(n=100, k=4, ldk=3),
               dict(n=100, k=4, L=False), dict(n=100, k=4, Li=False), dict(n=100, k=4, Kc=False)):
        rc, msg, _ = _call(lib, fake, **kw)
        assert rc == -3 and NAME in msg, kw


def test_host_wrapper_refuses_cpu_tensors_and_wrong_shapes():
    from gaussian_processes_amd import utils as gp
    assert callable(gp.cholesky_append_block)
    L, Li = torch.zeros(12, 12, dtype=torch.float64), torch.zeros(12, 12, dtype=torch.float64)
    with pytest.raises(ValueError, match="cholesky_append_block"):
        gp.cholesky_append_block(L, Li, torch.zeros(12, 3, dtype=torch.float64))          # host tensors
    with pytest.raises(ValueError, match="cholesky_append_block"):
        gp.cholesky_append_block(L, Li, torch.zeros(11, 3, dtype=torch.float64))          # rows of Kcols != n + k
    with pytest.raises(ValueError, match="cholesky_append_block"):
        gp.cholesky_append_block(L, Li, torch.zeros(12, dtype=torch.float64))             # not a matrix
    with pytest.raises(ValueError, match="cholesky_append_block"):
        gp.cholesky_append_block(L, Li, torch.zeros(12, 12, dtype=torch.float64))         # nothing to start from (n = 0)
