"""GPU parity of nx_twiddles_create's four tables (-m gpu): the twiddles, their inverses and both doubled tables are written by one
kernel, four words per lane, and have to equal the CPU oracle's tree word for word.  The sizes cover a tree smaller than one lane's
group of four words (log_half 1), exactly one group (2), the smallest tree with a vectorised group (3), trees inside one workgroup
(8, 9) and trees of several workgroups (13, 16)."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (before libnexus_hip.so: see test_gpu_parity.py)

pytestmark = pytest.mark.gpu


class TwiddlesC(C.Structure):      # struct nx_twiddles (csrc/internal.h)
    _fields_ = [("ctx", C.c_void_p), ("log_half", C.c_uint32), ("d_tw", C.c_void_p), ("d_itw", C.c_void_p), ("d_tw2", C.c_void_p), ("d_itw2", C.c_void_p)]


@pytest.fixture(scope="module")
def be():
    import nexus_zkvm_amd as nz
    b = nz.HipBackend(0)
    yield b
    b.close()


def table(be, ptr, n):
    out = np.empty(n, np.uint32)
    be._chk(be.L.nx_download(be.ctx, out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), C.c_size_t(n)))
    return out


@pytest.mark.parametrize("log_half", [1, 2, 3, 8, 9, 13, 16])
def test_four_tables_match_oracle(be, oracle, log_half):
    tw = be.precompute_twiddles(log_half)
    st = TwiddlesC.from_address(tw.h.value)
    assert st.log_half == log_half
    n = 1 << log_half
    got = [table(be, p, n) for p in (st.d_tw, st.d_itw, st.d_tw2, st.d_itw2)]
    otw, oitw = oracle.Twiddles(log_half).arrays()
    assert np.array_equal(got[0], otw)
    assert np.array_equal(got[1], oitw)
    # the doubled tables: twice the plain ones as integers (2 (p - 1) fits 32 bits), not reduced
    assert np.array_equal(got[2].astype(np.uint64), 2 * otw.astype(np.uint64))
    assert np.array_equal(got[3].astype(np.uint64), 2 * oitw.astype(np.uint64))
    d_tw, d_itw = tw.to_cpu()                                       # the public download sees the same two tables
    assert np.array_equal(d_tw, otw) and np.array_equal(d_itw, oitw)
