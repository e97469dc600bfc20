"""The lane-parallel 6x6 Jacobi SVD of the Gauss-Newton solves (jacobi_svd6_lanes) against its
sequential reference (jacobi_svd6_reg), through svo_pinv6_check: Hinv, W, Vt, U^T and the sweep
count must agree bit for bit on about a million systems, and Hinv with the CPU oracle on a sample."""
import numpy as np
import pytest
import torch

import oracle_py as O
from stereo_svo_slam_amd import hip_lib

pytestmark = pytest.mark.gpu

CHUNK = 1 << 17


@pytest.fixture(scope="module")
def H():
    h = hip_lib.Handle(0, max_keypoints=1024)
    yield h
    h.close()


def pose_jacobians(rng, n):
    """[n, 2, 6] Jacobians of pose_estimator.cpp:343-344 at points in front of the camera."""
    fx, fy = 458.654 / 2, 457.296 / 2
    x = rng.uniform(-3, 3, n)
    y = rng.uniform(-2, 2, n)
    z = rng.uniform(0.5, 12, n)
    J = np.zeros((n, 2, 6))
    J[:, 0, 0] = -fx / z
    J[:, 0, 2] = fx * x / (z * z)
    J[:, 0, 3] = fx * x * y / (z * z)
    J[:, 0, 4] = -fx * (1 + x * x / (z * z))
    J[:, 0, 5] = fx * y / z
    J[:, 1, 1] = -fy / z
    J[:, 1, 2] = fy * y / (z * z)
    J[:, 1, 3] = fy * (1 + y * y / (z * z))
    J[:, 1, 4] = -fy * x * y / (z * z)
    J[:, 1, 5] = -fy * x / z
    return J.astype(np.float32)


def alignment_hessians(rng, n, kps=(8, 40), patch=16, col_mask=False):
    """sum over keypoints and patch pixels of (grad I . J)^T (grad I . J) in float32, like the alignment."""
    out = np.empty((n, 6, 6), np.float32)
    b = 4096
    for s in range(0, n, b):
        m = min(b, n - s)
        k = int(rng.integers(kps[0], kps[1] + 1))
        J = pose_jacobians(rng, m * k).reshape(m, k, 2, 6)
        g = rng.normal(0, 20, (m, k, patch, 2)).astype(np.float32)
        rows = np.matmul(g, J)
        if col_mask:
            keep = rng.random((m, 1, 1, 6)) < 0.6
            rows = rows * keep
        rows = rows.reshape(m, k * patch, 6)
        out[s:s + m] = np.matmul(rows.transpose(0, 2, 1), rows)
    return out


def build_inputs():
    rng = np.random.default_rng(2024)
    sets = {}
    sets["alignment"] = alignment_hessians(rng, 500_000)
    sets["few_keypoints"] = alignment_hessians(rng, 60_000, kps=(1, 3), patch=4)    # rank 2..6
    sets["zero_columns"] = alignment_hessians(rng, 60_000, col_mask=True)
    sets["zero"] = np.zeros((64, 6, 6), np.float32)
    diag = np.zeros((40_000, 6, 6), np.float32)
    vals = rng.choice(np.array([0.0, 1.0, 2.0, 1e3], np.float32), (40_000, 6))
    vals[:10_000] = rng.choice(np.array([1.0, 5.0], np.float32), (10_000, 1))          # all equal
    diag[:, np.arange(6), np.arange(6)] = vals
    sets["diagonal_ties"] = diag
    base = alignment_hessians(rng, 100_000)
    base /= np.abs(base).reshape(-1, 36).max(1)[:, None, None]
    scale = (10.0 ** rng.uniform(-30, 30, 100_000)).astype(np.float32)
    sets["scales"] = (base * scale[:, None, None]).astype(np.float32)
    sets["denormal"] = (base[:20_000] * np.float32(1e-39)).astype(np.float32)
    special = alignment_hessians(rng, 20_000)
    idx = rng.integers(0, 36, (20_000, 2))
    vals = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), 20_000)
    flat = special.reshape(-1, 36)
    flat[np.arange(20_000), idx[:, 0]] = vals
    flat[np.arange(20_000), idx[:, 1]] = vals
    sets["nan_inf"] = special
    sets["general"] = rng.normal(0, 1, (100_000, 6, 6)).astype(np.float32)
    graded = rng.normal(0, 1, (100_000, 6, 6)) * (10.0 ** rng.uniform(-6, 6, (100_000, 1, 6)))
    sets["graded"] = graded.astype(np.float32)
    return sets


def run(h, A, impl):
    outs, sweeps = [], []
    for s in range(0, len(A), CHUNK):
        d = torch.from_numpy(np.ascontiguousarray(A[s:s + CHUNK].reshape(-1, 36))).cuda()
        o, w = h.pinv6_check(d, impl)
        h.synchronize()
        outs.append(o.cpu().numpy())
        sweeps.append(w.cpu().numpy())
    return np.concatenate(outs), np.concatenate(sweeps)


@pytest.fixture(scope="module")
def results(H):
    sets = build_inputs()
    return {k: (A, run(H, A, 0), run(H, A, 1)) for k, A in sets.items()}


def test_lanes_equal_reference_bits(results):
    total = 0
    max_sweeps = {}
    for name, (A, (o0, w0), (o1, w1)) in results.items():
        bad = np.nonzero((o0.view(np.uint32) != o1.view(np.uint32)).any(1) | (w0 != w1))[0]
        assert bad.size == 0, (name, bad[:8], A[bad[0]] if bad.size else None)
        total += len(A)
        max_sweeps[name] = int(w0.max())
    print("systems", total, "max sweeps per set", max_sweeps)
    assert total >= 1_000_000


def test_sweep_range_covered(results):
    sw = np.concatenate([r[1][1] for r in results.values()])
    assert sw.min() >= 1 and sw.max() <= 30
    assert (sw == 1).any() and (sw == 30).any()
    counts = np.bincount(sw, minlength=31)
    print("sweep histogram", {i: int(c) for i, c in enumerate(counts) if c})
    # NaN entries rotate in every sweep: the 30-sweep cap
    assert (results["nan_inf"][1][1] == 30).any()


@pytest.mark.parametrize("name", ["alignment", "few_keypoints", "zero_columns", "zero", "diagonal_ties",
                                  "general", "graded"])
def test_lanes_match_oracle(results, name):
    A, _, (o1, _) = results[name]
    rng = np.random.default_rng(7)
    for i in rng.choice(len(A), min(300, len(A)), replace=False):
        ref, _ = O.inv_svd(A[i])
        assert np.array_equal(o1[i, :36].view(np.uint32), ref.reshape(36).view(np.uint32)), (name, i)
