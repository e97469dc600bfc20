"""What one wavefront of the batched alignment kernel holds on a CU (no GPU needed): registers and scratch from
the kernel metadata of the gfx950 code object inside the built libsvo_hip.so (what ships), dynamic LDS from the
host's shape choice. A SIMD has 512 registers per lane and a CU 160 KiB of LDS; beside k alignment wavefronts
(one per sequence, each on a SIMD for milliseconds) the window kernels of the other sequence groups get what is
left, the smaller of what the two allow. Both bounds have to hold together: above 256
registers an alignment wavefront costs its SIMD three 128-register KLT wavefronts instead of two, above 18 KiB
the LDS runs out before the registers do."""
import os
import re
import subprocess

import pytest

from stereo_svo_slam_amd import hip_lib, synth
from stereo_svo_slam_amd.stereo_slam import pick_launch_shapes, pick_sia_lds_bytes

LLVM_BIN = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")
TOOLS = [os.path.join(LLVM_BIN, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")]
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
KERNEL = "_ZN3svo13sia_gn_kernelILi1ELi2EEEvPKNS_7SiaArgsEii"      # svo::sia_gn_kernel<1, 2>

REGISTER_GRANULE = 8          # gfx950 allocates a wavefront's unified VGPR + AGPR file in blocks of 8
MAX_REGISTERS = 256           # two such wavefronts, or one and 256 registers of window kernels, per SIMD
MAX_LDS_BYTES = 18 * 1024     # 160 bytes of sums + 7 planes of 32 keypoints' rows (18 192 B)


def _kernel_metadata(lib_path, kernel, tmp):
    """{field: int} of `kernel`'s entry in the amdhsa.kernels note of the gfx950 code object in lib_path. The
    library's .hip_fatbin section holds one offload bundle per translation unit, back to back."""
    objcopy, bundler, readelf = TOOLS
    fat = os.path.join(tmp, "fat.bin")
    subprocess.check_call([objcopy, "--dump-section", f".hip_fatbin={fat}", lib_path, os.path.join(tmp, "rest.o")])
    blob = open(fat, "rb").read()
    starts = [m.start() for m in re.finditer(BUNDLE_MAGIC, blob)]
    assert starts, "no offload bundle in .hip_fatbin"
    found = []
    for k, off in enumerate(starts):
        end = starts[k + 1] if k + 1 < len(starts) else len(blob)
        part, co = os.path.join(tmp, f"bundle{k}.bin"), os.path.join(tmp, f"gfx950_{k}.co")
        with open(part, "wb") as f:
            f.write(blob[off:end])
        subprocess.check_call([bundler, "--unbundle", "--type=o", f"--targets={TARGET}", f"--input={part}",
                               f"--output={co}"])
        notes = subprocess.run([readelf, "--notes", co], check=True, capture_output=True, text=True).stdout
        # one YAML list item per kernel, its fields sorted by name: ".agpr_count" opens the item
        for item in notes.split("  - .agpr_count:")[1:]:
            if re.search(r"\.name:\s+" + re.escape(kernel) + r"\s", item):
                fields = dict(re.findall(r"\.(\w+):\s+(\d+)\s*$", "    .agpr_count:" + item, flags=re.M))
                found.append({k_: int(v) for k_, v in fields.items()})
    assert len(found) == 1, f"{kernel}: {len(found)} entries in {lib_path}"
    return found[0]


@pytest.mark.skipif(not all(os.path.exists(t) for t in TOOLS), reason="ROCm LLVM tools (llvm-objcopy, "
                    "clang-offload-bundler, llvm-readelf) are not installed")
def test_batched_alignment_kernel_fits_256_registers_without_scratch(tmp_path):
    md = _kernel_metadata(hip_lib.LIB_PATH, KERNEL, str(tmp_path))
    print("sia_gn_kernel<1,2>:", {k: md[k] for k in ("vgpr_count", "agpr_count", "private_segment_fixed_size",
                                                     "vgpr_spill_count", "sgpr_count")})
    # gfx90a and later: .vgpr_count is the unified total, the AGPRs (.agpr_count) included
    assert md["agpr_count"] <= md["vgpr_count"]
    allocated = (md["vgpr_count"] + REGISTER_GRANULE - 1) // REGISTER_GRANULE * REGISTER_GRANULE
    assert allocated <= MAX_REGISTERS, md
    assert md["private_segment_fixed_size"] == 0 and md["vgpr_spill_count"] == 0, md
    assert md["wavefront_size"] == 64 and md["max_flat_workgroup_size"] == 64, md


def test_batched_alignment_lds_of_the_headline_shape():
    """`euroc` sequences in a batch: one wave per sequence up to 192 keypoints; the staging area of the ordered
    accumulation is all the LDS that shape asks for, whatever the cap."""
    cfg = synth.CONFIGS["euroc"]
    for n_bound, cap in ((64, 64), (125, 128), (129, 192), (192, 192)):
        assert pick_launch_shapes(cfg, 256, n_bound)[0] == ("sia_gn_kernel", 1, 2, cap)
        lds = pick_sia_lds_bytes(cfg, 256, n_bound)
        print(f"euroc, 256 sequences, {n_bound} keypoints: cap {cap}, {lds} B of LDS")
        assert 0 < lds <= MAX_LDS_BYTES, (n_bound, lds)
    # the two-wave shape and a lone sequence stage 64 keypoints at a time and keep more than that in LDS
    assert pick_launch_shapes(cfg, 256, 200)[0] == ("sia_gn_kernel", 2, 2, 256)
    assert pick_sia_lds_bytes(cfg, 256, 200) > MAX_LDS_BYTES
    assert pick_sia_lds_bytes(cfg, 1, 125) > MAX_LDS_BYTES
