"""What the compiler makes of the Blake2s column-chaining kernels (no GPU: hipcc cross-compiles merkle.hip for gfx950 and reports each
kernel's resources, -Rpass-analysis=kernel-resource-usage).

merkle_leaf_chain_kernel and merkle_layer_kernel hold two 16-word message buffers, the 16-word working state and the 8-word chaining
state in registers.  Two things about them rest on how the compiler treats the source, not on the source alone (DESIGN.md section 6
item 69): the column loads keep the `global_load_dword v, v_off, s[base]` form inside the column loop — with a 64-bit address per load
the kernels need 76 VGPRs — and nothing spills.  The bounds: no scratch, and at most 64 VGPRs, the most a kernel may allocate and still
hold 8 waves per SIMD (512 registers per lane and SIMD, allocated in steps of 8).  At 8 waves per SIMD a CU holds eight 256-lane
blocks, the GPU 2048, and every launch of 2^19 rows or more is a whole number of generations; that is why the launches have no
grid-stride loop.  A compiler that changes either figure shows here, not as a slower prove."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nexus-zkvm_amd", "csrc")
KERNELS = ("merkle_leaf_chain_kernel", "merkle_layer_kernel")


def test_chain_kernels_hold_eight_waves_without_scratch(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", "merkle.hip", "-o", str(tmp_path / "merkle.s"),
                          "-Rpass-analysis=kernel-resource-usage"], cwd=CSRC, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    found, name = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            continue
        m = re.search(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and name and any(k in name for k in KERNELS):
            found.setdefault(name, {})[m.group(1).split(" ")[0]] = int(m.group(2))
    # hash mode 0 / 1 times pointer table / base + stride, for both kernels
    assert len(found) == 8, sorted(found)
    for name, r in found.items():
        print(name, r)
        assert r["ScratchSize"] == 0, (name, r)
        assert r["VGPRs"] <= 64, (name, r)
        assert r["Occupancy"] == 8, (name, r)
