"""The narrow host-trace upload without a GPU: the C ABI declares and exports nx_upload_columns_narrow,
nx_prover_tree_commit_host_narrow and nx_prove_machine_host_narrow with the five NX_COL_* kinds, refuses NULL arguments with NX_ERR_ARG,
the generated -sys crate binds them, and the host pack / check routine (csrc/host/narrow_pack.h) packs exactly and refuses the same
(column, row) under every thread count (tests/native/narrow_pack_selftest.cpp)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("nx_upload_columns_narrow", "nx_prover_tree_commit_host_narrow", "nx_prove_machine_host_narrow")
KINDS = {"NX_COL_U32": 0, "NX_COL_U16": 1, "NX_COL_U8": 2, "NX_COL_U32_AS_U16": 3, "NX_COL_U32_AS_U8": 4}


def _header():
    return open(os.path.join(ROOT, "include", "nexus_hip.h")).read()


def test_header_declares_the_kinds_and_the_entry_points():
    text = _header()
    for name, value in KINDS.items():
        assert re.search(r"^#define %s %d\b" % (name, value), text, flags=re.M), name
    import nexus_zkvm_amd as nz
    assert set(NEW) <= set(nz.declared_symbols())
    assert (nz.COL_U32, nz.COL_U16, nz.COL_U8, nz.COL_U32_AS_U16, nz.COL_U32_AS_U8) == tuple(KINDS.values())
    assert '"host.pack_threads"' in text


def test_library_exports_them_and_null_arguments_are_errors():
    import nexus_zkvm_amd as nz
    if not os.path.exists(nz.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    L = nz.load_library()
    for name in NEW:
        assert hasattr(L, name), name
    calls = {
        "nx_upload_columns_narrow": lambda: L.nx_upload_columns_narrow(None, None, None, 0, 0, None, 0),
        "nx_prover_tree_commit_host_narrow": lambda: L.nx_prover_tree_commit_host_narrow(None, None, None, 0, None, 0, None, None),
        "nx_prove_machine_host_narrow": lambda: L.nx_prove_machine_host_narrow(None, None, 0, None, None, None, None, None, 0, None, C.c_size_t(0), None, None, None),
    }
    for name, call in calls.items():
        assert call() == -2, name                       # NX_ERR_ARG
        assert L.nx_last_error(None), name


def test_sys_crate_binds_them():
    src = open(os.path.join(ROOT, "rust", "nexus-hip-sys", "src", "lib.rs")).read()
    for name, value in KINDS.items():
        assert "pub const %s: c_int = %d;" % (name, value) in src, name
    for name in NEW:
        assert re.search(r"pub fn %s\(.*\*const \*const c_void.*\*const u8" % name, src), name
    wrap = open(os.path.join(ROOT, "rust", "nexus-hip", "src", "lib.rs")).read()
    assert "pub fn upload_narrow(&mut self, host_cols: &[(*const c_void, u8)]" in wrap and "sys::nx_upload_columns_narrow(" in wrap
    assert "pub fn tree_commit_host_narrow(&mut self, host_cols: &[(*const c_void, u8)]" in wrap and "sys::nx_prover_tree_commit_host_narrow(" in wrap


def test_python_kinds_follow_the_dtype_and_as_kind():
    import numpy as np
    import nexus_zkvm_amd as nz
    cols = [np.zeros(4, np.uint8), np.zeros(4, np.uint16), np.zeros(4, np.uint32), np.zeros(4, np.uint32), np.zeros(4, np.uint32)]
    _, kinds = nz._narrow_columns(cols, [None, None, None, np.uint8, "u16"])
    assert list(kinds) == [nz.COL_U8, nz.COL_U16, nz.COL_U32, nz.COL_U32_AS_U8, nz.COL_U32_AS_U16]
    _, kinds = nz._narrow_columns(cols[2:], np.uint8)
    assert list(kinds) == [nz.COL_U32_AS_U8] * 3
    with pytest.raises(ValueError):
        nz._narrow_columns(cols[:1], np.uint16)           # as_kind narrows uint32 columns only
    with pytest.raises(ValueError):
        nz._narrow_columns(cols[2:3], np.int64)


def test_pack_routine_packs_exactly_and_refuses_the_lowest_column_then_row(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "narrow_pack_selftest")
    subprocess.run([hipcc, "-O2", "-std=c++17", "--offload-arch=gfx950", os.path.join(ROOT, "tests", "native", "narrow_pack_selftest.cpp"), "-o", exe],
                   check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 mismatches" in r.stdout
