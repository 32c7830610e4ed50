"""The columns a machine's logup fractions read are produced IN the buffers that keep their evaluations, and the commitment's inverse
transform reads them from there: no clone (-m gpu).

A proof has to come out word for word as the CPU reference prover's (machine_ref), by both routes that produce a trace — filled on the
device, and handed over in host memory and uploaded under the commit — and on both sides of the size at which the transform takes a
separate source: 2^13 rows are transformed in place (the kept evaluations are copied into the tree's slab first), 2^16 rows go through
the fused passes whose first inverse pass reads the kept buffer and writes the slab."""
import os

import numpy as np
import pytest
import torch  # noqa: F401  (HIP runtime load order, see test_gpu_parity.py)

import machine_ref as M
import oracle_lib as O

pytestmark = pytest.mark.gpu
THREADS = max(4, os.cpu_count() or 4)
SEED, AD, KW = 77, b"keep", dict(pow_bits=6)
# the bench's machine at two sizes; a component of 17 main columns and three fractions, which read columns 0, 3, 10, 11 and 16:
# the first and the last column of the tree are kept ones, and they lie in different 16-column chunks of the host feed
CASES = {"bench-2^13": [(13, 27, 347, 64)], "bench-2^16": [(16, 27, 347, 64)], "first-and-last-kept": [(14, 3, 17, 12)]}


@pytest.fixture(scope="module")
def be():
    import nexus_zkvm_amd as nz
    b = nz.HipBackend(0)
    yield b
    b.close()


_refs = {}


def reference(name):
    if name not in _refs:
        _refs[name] = M.prove_machine(CASES[name], O.default_cfg(**KW), seed=SEED, ad=AD, threads=THREADS)
    return _refs[name]


def same(ref, words):
    assert len(ref) == len(words), (len(ref), len(words))
    if not np.array_equal(ref, words):
        pytest.fail(f"first differing proof word {int(np.nonzero(ref != words)[0][0])} of {len(ref)}")


@pytest.mark.parametrize("name", list(CASES))
def test_device_filled_trace(be, oracle, name):
    import nexus_zkvm_amd as nz
    same(reference(name), be.prove_machine(CASES[name], nz.default_config(**KW), seed=SEED, ad=AD))


@pytest.mark.parametrize("name", list(CASES))
def test_host_trace(be, oracle, name):
    import nexus_zkvm_amd as nz
    comps = CASES[name]
    pre = [c for s in be.synth_fill_tree(comps, 0, SEED) for c in s.to_cpu()]
    main = [c for s in be.synth_fill_tree(comps, 1, SEED) for c in s.to_cpu()]
    same(reference(name), be.prove_machine_host(comps, nz.default_config(**KW), pre, main, ad=AD))
