"""The four-wave batched alignment shape (sia_gn_kernel<4,2>: a batch of sequences whose keypoint sets pass 384, the
1920x1080 configuration) shares cost() and the per-keypoint half of get_gradient with the one-wave shape, batched
loads included: it has to keep them in 256 registers and out of scratch as well (no GPU needed; the kernel metadata
of the gfx950 code object inside the built libsvo_hip.so, read as tests/test_sia_footprint_cpu.py reads it)."""
import os

import pytest

from stereo_svo_slam_amd import hip_lib
from test_sia_footprint_cpu import MAX_REGISTERS, REGISTER_GRANULE, TOOLS, _kernel_metadata

KERNEL_4_2 = "_ZN3svo13sia_gn_kernelILi4ELi2EEEvPKNS_7SiaArgsEii"      # svo::sia_gn_kernel<4, 2>


@pytest.mark.skipif(not all(os.path.exists(t) for t in TOOLS), reason="ROCm LLVM tools (llvm-objcopy, "
                    "clang-offload-bundler, llvm-readelf) are not installed")
def test_four_wave_batched_alignment_kernel_fits_256_registers_without_scratch(tmp_path):
    md = _kernel_metadata(hip_lib.LIB_PATH, KERNEL_4_2, str(tmp_path))
    print("sia_gn_kernel<4,2>:", {k: md[k] for k in ("vgpr_count", "agpr_count", "private_segment_fixed_size",
                                                     "vgpr_spill_count", "sgpr_count")})
    # gfx90a and later: .vgpr_count is the unified total, the AGPRs (.agpr_count) included
    assert md["agpr_count"] <= md["vgpr_count"]
    allocated = (md["vgpr_count"] + REGISTER_GRANULE - 1) // REGISTER_GRANULE * REGISTER_GRANULE
    assert allocated <= MAX_REGISTERS, md
    assert md["private_segment_fixed_size"] == 0 and md["vgpr_spill_count"] == 0, md
    assert md["wavefront_size"] == 64 and md["max_flat_workgroup_size"] == 256, md
