"""gpfit_estep_chain_full without a GPU: the symbol is exported and bound, and the argument checks that need no device
answer -3 with a message before anything touches one."""
import ctypes

from gaussian_processes_amd import _lib

CAP = 1024   # GPFIT_ESTEP_CHAIN_MAX_STEPS of include/gpfit_mi355x.h


def call(ctx, n_steps):
    """The entry point with null device pointers: every case here has to be refused before any of them is read."""
    lib = _lib.load()
    rec = (ctypes.c_double * 12)()
    return lib.gpfit_estep_chain_full(ctx, None, None, 8, 8, None, None, None, None, None, 8, None, None, 0.0, 0, 0.0,
                                      n_steps, 4, 4, 0.1, 1e-7, 1e-9, rec)


def test_symbol_is_exported_and_bound():
    assert "gpfit_estep_chain_full" in _lib.exported_symbols()
    fn = _lib.load().gpfit_estep_chain_full
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 23


def test_null_context_is_refused():
    assert call(None, 1) == -3
    assert "gpfit_estep_chain_full" in _lib.last_error() and "bad argument" in _lib.last_error()


def test_zero_steps_are_refused():
    assert call(None, 0) == -3
    assert "gpfit_estep_chain_full" in _lib.last_error() and "n_steps 0" in _lib.last_error()


def test_steps_above_the_cap_are_refused():
    assert call(None, CAP + 1) == -3
    assert "gpfit_estep_chain_full" in _lib.last_error() and f"n_steps {CAP + 1}" in _lib.last_error()
    assert call(None, CAP) == -3 and "bad argument" in _lib.last_error()   # the cap itself passes the n_steps check
