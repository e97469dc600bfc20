"""Diagnostic (not a test, not the product): loads a libsvo_hip built with -DSVO_SIA_STAMPS
(tools/build_variants.sh stamps -> build_ab/libsvo_hip_stamps.so) and prints where one
sparse-alignment launch spends its cycles (s_memtime on thread 0), for a lone sequence
(workgroup shape by keypoint count) and, with `batch`, for the one-wave shape of batched launches.
"grad: solve" is split into "solve: sweeps" (rows in, Jacobi sweeps) and "solve: tail+step" (singular
values, sort, pseudo-inverse, delta); what is left of it is exponential_map and the rotation.
Usage: sia_stamps.py [config] [exact]
       sia_stamps.py batch [bench.py arguments]
`batch` runs bench.py's workload in this process on the stamps library (SVO_GROUPS=1 --seqs 256 --loops 16: the
alignment launches alone; the default: beside the other groups' kernels) and reads the stamps of the last 4096 sequences
that finished an alignment launch (MODE 2: every operand from L2). Besides the phases above, the time a pass stands
at an s_waitcnt vmcnt(0) the diagnostic build puts where the pass needs what it asked of memory: "cost: wait operands"
(flag, point, records; with -DSVO_SIA_PRELOAD=0, build_variants.sh stamps_chain, the three waits of the chain one behind
the other), "cost: wait taps", "grad: wait operands" (chain: flag, point, projection, 16 reference patch sums), "grad:
wait taps" (with the projections in registers: the taps and the operands, asked for together), "grad: wait gradients"
(REC_G0/G1 of a 32-keypoint chunk). The waits make the kernel slower than the product's and serialise what the product
overlaps: they show what a round trip costs, the phase totals of the two builds what was saved.
SVO_HIP_LIB chooses another stamps library."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("SVO_HIP_LIB", os.path.join(ROOT, "build_ab", "libsvo_hip_stamps.so"))
sys.path[:0] = [ROOT, os.path.join(ROOT, "stereo-svo-slam_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import numpy as np, torch
NAMES = ["levels: image + records", "cost: pose_mats", "cost: keypoints", "cost: ordered sum", "n_cost",
         "grad: pose+keypoints", "grad: reduce", "grad: solve", "n_grad", "kernel_total",
         "solve: sweeps", "solve: tail+step", "cost: wait operands", "cost: wait taps", "grad: wait operands",
         "grad: wait taps", "grad: wait gradients", "cost passes", "grad passes", "keypoints"]


def batch(argv):
    import ctypes as C
    sys.argv = ["bench.py", "--no-cpu-baseline"] + argv
    import bench
    bench.main()
    from stereo_svo_slam_amd import hip_lib
    ring = np.zeros((4096, len(NAMES)), np.float32)
    rows = C.c_uint(0)
    assert hip_lib.lib().svo_sia_stamps_read(ring.ctypes.data_as(C.c_void_p), C.byref(rows)) == 0
    r = ring[:min(rows.value, len(ring))]
    print(f"{os.environ['SVO_HIP_LIB']}: {rows.value} stamped sequence launches, the last {len(r)} read; "
          f"SVO_GROUPS={os.environ.get('SVO_GROUPS', '-')}, arguments {argv}")
    if not len(r):
        return
    col = {n_: k for k, n_ in enumerate(NAMES)}
    slow = r[np.argsort(r[:, col["kernel_total"]])[-max(len(r) // 100, 1):]]       # the slowest 1 %: what a launch lasts
    for label, q in (("mean sequence", r), ("slowest 1 % of the sequences", slow)):
        m = q.mean(axis=0)
        print(f"-- {label}: {m[col['keypoints']]:.0f} keypoints, {m[col['n_cost']]:.1f} cost calls in {m[col['cost passes']]:.1f} "
              f"passes, {m[col['n_grad']]:.1f} gradient calls in {m[col['grad passes']]:.1f} passes, kernel {m[col['kernel_total']]:.0f} ticks")
        for n_ in NAMES:
            if n_ in ("n_cost", "n_grad", "kernel_total", "cost passes", "grad passes", "keypoints"):
                continue
            v = m[col[n_]]
            calls = m[col["n_cost"]] if n_.startswith("cost") else m[col["n_grad"]] if n_.startswith(("grad", "solve")) else 1
            passes = m[col["cost passes"]] if n_.startswith("cost") else m[col["grad passes"]] if n_.startswith("grad") else 0
            per_pass = f"  per pass {v / passes:8.0f}" if passes and ("wait" in n_ or "keypoints" in n_) else ""
            print(f"{n_:26s} total {v:10.0f} ({100 * v / m[col['kernel_total']]:5.1f} % of the kernel)  per call {v / max(calls, 1):8.0f}{per_pass}")


if len(sys.argv) > 1 and sys.argv[1] == "batch":
    batch(sys.argv[2:])
    sys.exit(0)
import oracle_py as O
from stereo_svo_slam_amd import hip_lib
import util
config = sys.argv[1] if len(sys.argv) > 1 and sys.argv[1] not in ("fast",) else "euroc"
exact = "fast" not in sys.argv[1:]
sc = util.scenario(config, 3, 0, 1)
cfg = sc["cfg"]; nl = cfg["max_pyramid_levels"]
prev, cur = O.build_pyramid(sc["L"][0], nl), O.build_pyramid(sc["L"][1], nl)
d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
H = hip_lib.Handle(0, 448)
H.set_exact_pinv(exact)
args = ([d(x) for x in prev], [d(x) for x in cur], d(sc["kps2d"]), d(sc["kps3d"]), d(util.flags_of(sc["info"])),
        hip_lib.CameraSettings.from_dict(cfg), d(np.zeros(6, np.float32)))
for it in range(3):
    pose, cost, trace, dbg = H.sparse_align(*args, dbg_level=0)
    torch.cuda.synchronize()
s = dbg.cpu().numpy()[:12]
tr = hip_lib.trace_to_numpy(trace)
ng = sum(int(t["n_gradient"]) for t in tr); nc = sum(int(t["n_cost"]) for t in tr)
names = NAMES[:12]
print(f"{config}: n = {len(sc['kps2d'])}, exact = {exact}, n_grad {ng}, n_cost {nc}")
for n_, v in zip(names, s):
    per = v / max(s[4], 1) if n_.startswith("cost") else (v / max(s[8], 1) if n_.startswith(("grad", "solve")) else v)
    print(f"{n_:26s} total {v:12.0f}  per call {per:10.0f} cycles (100 MHz ticks x clock ratio)")
