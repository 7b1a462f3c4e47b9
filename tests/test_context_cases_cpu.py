"""The registry of tests/context_cases.py against the C ABI, and the table of work buffers of csrc/api_dev.hip
(``gpfit_dev_ctx_buffer_name``) against the members of ``struct gpfit_ctx``: an entry point or a work buffer added later
fails here until it has a probe, a table entry, or a stated reason to have none.  No GPU."""
import ctypes
import os
import re
import struct

import numpy as np
import pytest

import context_cases as cc
from conftest import ROOT
from gaussian_processes_amd import _lib
from gaussian_processes_amd.build import build_library

# Members of gpfit_ctx of type double* or void* that gpfit_dev_ctx_fill must not know, each with its reason.
NOT_WORK_BUFFERS = {
    "scal_host": "pinned host memory: the host writes it as well, and the device only through a mapping",
    "chain_host": "pinned host memory: the step records of a chain, copied once at the chain's end",
}


@pytest.fixture(scope="module")
def lib():
    build_library(verbose=False)
    return _lib.load()


def header_entry_points():
    """name -> True for every function of the header whose first parameter is a context or a table of contexts."""
    hdr = open(os.path.join(ROOT, "include", "gpfit_mi355x.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return set(re.findall(r"\b(gpfit_\w+)\s*\(\s*gpfit_ctx\s*\*\s*(?:const\s*\*\s*)?\w+", hdr))


def test_every_context_entry_point_has_a_probe_or_a_reason(lib):
    takes_ctx = header_entry_points()
    assert len(takes_ctx) > 40 and takes_ctx <= set(_lib.exported_symbols())
    probed = {p.entry for p in cc.PROBES}
    assert not probed & set(cc.EXEMPT), probed & set(cc.EXEMPT)
    missing = takes_ctx - probed - set(cc.EXEMPT)
    assert not missing, f"entry points that take a context without a probe in tests/context_cases.py: {sorted(missing)}"
    stale = (probed | set(cc.EXEMPT)) - takes_ctx
    assert not stale, f"probes or exemptions of names the header does not declare with a context: {sorted(stale)}"
    assert all(isinstance(why, str) and len(why) > 10 for why in cc.EXEMPT.values())
    # a batch entry point is probed with several units, a single one with one; every probe states its cache class
    for p in cc.PROBES + cc.LARGE:
        assert (p.units == cc.GROUP_UNITS) == p.entry.endswith(("_batch", "_batch_f32")), p.name
        assert p.cache in (cc.KEEPS, cc.DROPS) and callable(p.build), p.name
    assert len({p.name for p in cc.PROBES + cc.LARGE}) == len(cc.PROBES + cc.LARGE)
    assert {p.entry for p in cc.LARGE} <= probed and set(cc.BY_NAME) == {p.name for p in cc.PROBES + cc.LARGE}


def test_the_buffer_table_covers_the_context(lib):
    names = cc.buffer_names()
    assert len(names) == len(set(names)) >= 45
    buf = ctypes.create_string_buffer(64)
    assert lib.gpfit_dev_ctx_buffer_name(len(names), buf, 64) == -3 and lib.gpfit_dev_ctx_buffer_name(-1, buf, 64) == -3
    assert lib.gpfit_dev_ctx_buffer_name(0, buf, len(names[0])) == -3 and lib.gpfit_dev_ctx_buffer_name(0, buf, len(names[0]) + 1) == 0
    src = open(os.path.join(ROOT, "gaussian_processes_amd", "csrc", "context.h")).read()
    body = re.search(r"struct gpfit_ctx \{(.*?)^\};", src, flags=re.S | re.M).group(1)
    body = re.sub(r"//[^\n]*|/\*.*?\*/", "", body, flags=re.S)
    members = set()
    for decl in re.findall(r"^\s*(?:double|void)\s*\*[^;()]*;", body, flags=re.M):
        for name, dims in re.findall(r"\*\s*(\w+)\s*(\[\d+\])?\s*(?:=[^,;]*)?[,;]", decl):
            members |= {f"{name}[{i}]" for i in range(int(dims[1:-1]))} if dims else {name}
    assert {"Kbuf", "LVbuf", "tvec", "rect_part", "sk_ws[0]", "sk_ws[1]", "scal", "scal_host"} <= members, members
    assert not set(NOT_WORK_BUFFERS) & set(names)
    assert members - set(NOT_WORK_BUFFERS) == set(names), (sorted(members - set(NOT_WORK_BUFFERS) - set(names)),
                                                             sorted(set(names) - members))
    # the integer buffers and the chain block are not floating-point work buffers and are not in the table
    assert re.search(r"int\* pix\b", body) and re.search(r"int\* info\b", body) and "ChainBlock* chain" in body
    assert not {"pix", "info", "chain", "pix_host", "info_host"} & set(names)


def test_the_poison_bytes():
    """0xFF is NaN as fp64 and as fp32; 0x47 is finite in both and far from anything in the data."""
    nan, far = cc.POISON
    assert np.isnan(struct.unpack("<d", bytes([nan]) * 8)[0]) and np.isnan(struct.unpack("<f", bytes([nan]) * 4)[0])
    d, f = struct.unpack("<d", bytes([far]) * 8)[0], struct.unpack("<f", bytes([far]) * 4)[0]
    assert np.isfinite(d) and np.isfinite(f) and d > 1e30 and 4e4 < f < 6e4
    assert np.frombuffer(bytes([far]) * 8, dtype=np.float64)[0] == d


def test_the_inputs_have_padding_on_every_axis():
    h = cc.host()
    assert h["d"] == 56 and h["mask"].sum() == 56 and h["mask"].size == cc.D_FULL
    for n in (cc.N, cc.NB, cc.NT, cc.KS, cc.P, cc.N_BASE):
        assert n % 128 != 0 and -(-n // 128) * 128 < cc.CAP
    assert -(-cc.N_LARGE // 128) * 128 == 2176 < cc.CAP_LARGE and 2176 >= 2048
    for key in ("pK", "pV", "full_K", "full_V", "V"):
        assert np.array_equal(h[key], h[key].T) and np.linalg.eigvalsh(h[key])[0] > 0, key
    assert np.array_equal(h["app1_L"][cc.N - 1], np.zeros(cc.N)) and np.array_equal(np.triu(h["Linv"], 1), np.zeros((cc.NB, cc.NB)))
