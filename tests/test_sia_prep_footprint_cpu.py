"""What one wavefront of sia_prep_kernel holds on a SIMD (no GPU needed), from the kernel metadata of the gfx950 code
object inside the built libsvo_hip.so. The kernel it replaced had 69 registers, 7 wavefronts per SIMD; the rewrite
must not fall below that (it stands at 63, 8 per SIMD), and it needs neither LDS nor scratch. Several constructs in
sia.hip exist only to keep it there (the rolled pixel loop, each patch sum pinned where it is formed, store bases in
SGPRs): a compiler that stops honouring them shows here."""
import os

import pytest

from stereo_svo_slam_amd import hip_lib
from test_sia_footprint_cpu import REGISTER_GRANULE, TOOLS, _kernel_metadata

KERNEL = "_ZN3svo15sia_prep_kernelEPKNS_7SiaArgsE"       # svo::sia_prep_kernel
MAX_REGISTERS = 72            # 512 / 72 = 7 wavefronts per SIMD


@pytest.mark.skipif(not all(os.path.exists(t) for t in TOOLS), reason="ROCm LLVM tools (llvm-objcopy, "
                    "clang-offload-bundler, llvm-readelf) are not installed")
def test_records_kernel_keeps_seven_waves_per_simd_without_lds_or_scratch(tmp_path):
    md = _kernel_metadata(hip_lib.LIB_PATH, KERNEL, str(tmp_path))
    print("sia_prep_kernel:", {k: md[k] for k in ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size",
                                                  "private_segment_fixed_size", "vgpr_spill_count")})
    allocated = (md["vgpr_count"] + REGISTER_GRANULE - 1) // REGISTER_GRANULE * REGISTER_GRANULE
    assert allocated <= MAX_REGISTERS, md
    assert md["group_segment_fixed_size"] == 0, md
    assert md["private_segment_fixed_size"] == 0 and md["vgpr_spill_count"] == 0, md
    assert md["wavefront_size"] == 64 and md["max_flat_workgroup_size"] == 64, md
