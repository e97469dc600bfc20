"""The lane-resident exact solve of the Gauss-Newton kernels (svd6_sweeps_lanes + svd6_tail_lanes)
against the round-4 solve (jacobi_svd6_lanes, then svd6_finish, svd6_pinv and delta = Hinv b on
wave-uniform values), through svo_solve6_check: Hinv, W, Vt, U^T, delta and the sweep count must
agree bit for bit on about a million systems (the system families of test_svd_lanes_gpu.py).
One exception: where W, Vt or U^T hold a NaN (the NaN/Inf family), only its position must agree. Which
of two NaN operands an instruction passes on (and so the NaN's sign) depends on the operand order the
compiler picks, which differs between the two check kernels even inside the sweeps they share. Hinv and
delta, the outputs the kernels use, must agree in every bit, NaNs included."""
import numpy as np
import pytest
import torch

from stereo_svo_slam_amd import hip_lib
from test_svd_lanes_gpu import build_inputs

pytestmark = pytest.mark.gpu

CHUNK = 1 << 17


@pytest.fixture(scope="module")
def H():
    h = hip_lib.Handle(0, max_keypoints=1024)
    yield h
    h.close()


def right_hand_sides(rng, n):
    """b vectors: gradients at alignment scale, wide exponents, zeros, and a few NaN / +-Inf entries."""
    b = rng.normal(0, 1e3, (n, 6)) * (10.0 ** rng.uniform(-12, 12, (n, 1)))
    b[rng.random(n) < 0.02] = 0
    special = rng.random(n) < 0.01
    b[special, rng.integers(0, 6, special.sum())] = rng.choice([np.nan, np.inf, -np.inf], special.sum())
    return b.astype(np.float32)


def run(h, A, B, impl):
    outs, sweeps = [], []
    for s in range(0, len(A), CHUNK):
        dA = torch.from_numpy(np.ascontiguousarray(A[s:s + CHUNK].reshape(-1, 36))).cuda()
        dB = torch.from_numpy(np.ascontiguousarray(B[s:s + CHUNK])).cuda()
        o, w = h.solve6_check(dA, dB, impl)
        h.synchronize()
        outs.append(o.cpu().numpy())
        sweeps.append(w.cpu().numpy())
    return np.concatenate(outs), np.concatenate(sweeps)


@pytest.fixture(scope="module")
def results(H):
    rng = np.random.default_rng(99)
    out = {}
    for k, A in build_inputs().items():
        B = right_hand_sides(rng, len(A))
        out[k] = (A, B, run(H, A, B, 0), run(H, A, B, 1))
    return out


def test_lane_solve_equals_round4_bits(results):
    total = 0
    for name, (A, B, (o0, w0), (o1, w1)) in results.items():
        assert o0.shape[1] == 120
        diff = o0.view(np.uint32) != o1.view(np.uint32)
        diff[:, 36:114] &= ~(np.isnan(o0[:, 36:114]) & np.isnan(o1[:, 36:114]))
        bad = np.nonzero(diff.any(1) | (w0 != w1))[0]
        assert bad.size == 0, (name, bad[:8], A[bad[0]] if bad.size else None, B[bad[0]] if bad.size else None)
        total += len(A)
    print("systems", total)
    assert total >= 1_000_000


def test_cases_are_exercised(results):
    # the sort's ties, the ok zeroing (H = 0, rank deficient), the 30-sweep cap and non-finite steps occur
    o = np.concatenate([r[3][0] for r in results.values()])
    sw = np.concatenate([r[3][1] for r in results.values()])
    W = o[:, 36:42]
    assert (W[:, :-1] == W[:, 1:]).any()
    assert (o[:, :36] == 0).all(1).any() and (o[:, :36] != 0).any(1).any()
    assert sw.min() >= 1 and sw.max() == 30
    d = o[:, 114:]
    assert (~np.isfinite(d)).any() and np.isfinite(d).all(1).any()
