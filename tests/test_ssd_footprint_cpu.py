"""What one workgroup of ssd_disparity_kernel holds on a CU (no GPU needed), from the kernel metadata of the gfx950
code object inside the built libsvo_hip.so, for both instantiations. The kernel is one wavefront per keypoint: it must
stay a single-wave workgroup, fit four to a SIMD (128 registers) without scratch, and never take more LDS than the
four-wave kernel it replaced did (14 960 bytes; it stands at 9 408 for the small shape and 10 944 for the large).
What it holds is what the other sequence groups' kernels do not get."""
import os

import pytest

from stereo_svo_slam_amd import hip_lib
from test_sia_footprint_cpu import REGISTER_GRANULE, TOOLS, _kernel_metadata

KERNELS = {"<31,13>": "_ZN3svo20ssd_disparity_kernelILi31ELi13EEEvPKNS_7SsdArgsE",
           "<35,17>": "_ZN3svo20ssd_disparity_kernelILi35ELi17EEEvPKNS_7SsdArgsE"}
MAX_REGISTERS = 128           # four wavefronts per SIMD
MAX_LDS_BYTES = 14960         # the four-wave kernel's <31,13>


@pytest.mark.skipif(not all(os.path.exists(t) for t in TOOLS), reason="ROCm LLVM tools (llvm-objcopy, "
                    "clang-offload-bundler, llvm-readelf) are not installed")
@pytest.mark.parametrize("shape", sorted(KERNELS))
def test_ssd_kernel_is_one_wave_of_128_registers_without_scratch(tmp_path, shape):
    md = _kernel_metadata(hip_lib.LIB_PATH, KERNELS[shape], str(tmp_path))
    print(f"ssd_disparity_kernel{shape}:", {k: md[k] for k in ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size",
                                                              "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count",
                                                              "max_flat_workgroup_size")})
    assert md["wavefront_size"] == 64 and md["max_flat_workgroup_size"] == 64, md
    # gfx90a and later: .vgpr_count is the unified total, the AGPRs (.agpr_count) included
    assert md["agpr_count"] <= md["vgpr_count"]
    allocated = (md["vgpr_count"] + REGISTER_GRANULE - 1) // REGISTER_GRANULE * REGISTER_GRANULE
    assert allocated <= MAX_REGISTERS, md
    assert md["private_segment_fixed_size"] == 0 and md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0, md
    assert md["group_segment_fixed_size"] <= MAX_LDS_BYTES, md
