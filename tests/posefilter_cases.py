"""The 12-state pose filter (StereoSlam::update_pose, src/lib/stereo_slam.cpp:296-359) restated in plain numpy, and
the crafted filter states and samples of the pose-filter tests.

The restatement is cv::KalmanFilter(12, 12) on float data as OpenCV computes it: every gemm multiplies floats and
accumulates in double in p = 0..11 order, then * alpha, + c * beta, one rounding to float; the gain comes out of
cv::solve(DECOMP_SVD), a one-sided Jacobi SVD on the rows of the transposed matrix (float data, double dot products,
at most 30 sweeps, selection sort, rows scaled to unit length) followed by the back substitution whose float product
s * B[r][j] is rounded before it is widened. It multiplies everything out: A, Hm, Q and R are full matrices here.
It imports neither the oracle nor the library."""
import math

import numpy as np

N = 12
F32, F64 = np.float32, np.float64
FLT_EPSILON = float(np.finfo(np.float32).eps)
FLT_MIN = float(np.finfo(np.float32).tiny)
DBL_EPSILON = float(np.finfo(np.float64).eps)

# svo_pose_sample (include/svo_types.h), written out here on its own: test_posefilter_cpu.py compares it with the
# library's dtype and the C header
SAMPLE_FIELDS = (("pose", 0, "<f4", 6), ("speed", 24, "<f4", 6), ("pose_var", 48, "<f4", 6), ("speed_var", 72, "<f4", 6),
                 ("dt", 96, "<f8", 1), ("flags", 104, "<u4", 1), ("_pad", 108, "<u4", 1))
SAMPLE_BYTES = 112
SAMPLE_DTYPE = np.dtype({"names": [f[0] for f in SAMPLE_FIELDS],
                         "formats": [(f[2], (f[3],)) if f[3] > 1 else f[2] for f in SAMPLE_FIELDS],
                         "offsets": [f[1] for f in SAMPLE_FIELDS], "itemsize": SAMPLE_BYTES})
CHAIN = 1
IN_FLOATS, OUT_FLOATS = N + N * N, 2 * N + 3 * N * N


def gemm(a, b, bt, alpha, c, beta):
    """d = alpha * a * op(b) + beta * c: float data, double accumulation in p order, float store"""
    a = np.asarray(a, F32)
    b = np.asarray(b, F32)
    if bt:
        b = b.T
    s = np.zeros((a.shape[0], b.shape[1]), F64)
    for p in range(a.shape[1]):
        s += a[:, p, None].astype(F64) * b[None, p, :].astype(F64)
    s *= F64(alpha)
    if c is not None:
        s += np.asarray(c, F32).astype(F64) * F64(beta)
    return s.astype(F32)


def _hypot(a, b):
    a, b = abs(a), abs(b)
    if a > b:
        b /= a
        return a * math.sqrt(1 + b * b)
    if b > 0:
        a /= b
        return b * math.sqrt(1 + a * a)
    return 0.0


def _sum_sq(row):
    s = 0.0
    for t in row.astype(F64).tolist():
        s += t * t
    return s


def jacobi_svd(At, trace=None):
    """JacobiSVDImpl_<float> on the rows of At [n, m] (changed in place): returns (W [n], Vt [n, n], sweeps)"""
    n, m = At.shape
    eps = float(F32(FLT_EPSILON * 2))
    Wd = [_sum_sq(At[i]) for i in range(n)]
    Vt = np.eye(n, dtype=F32)
    sweeps = 0
    for _ in range(max(m, 30)):
        changed = False
        sweeps += 1
        for i in range(n - 1):
            for j in range(i + 1, n):
                a, b, p = Wd[i], Wd[j], 0.0
                for t in (At[i].astype(F64) * At[j].astype(F64)).tolist():    # (a product of two floats is exact in double)
                    p += t
                if abs(p) <= eps * math.sqrt(a * b):
                    continue
                p *= 2
                beta = a - b
                gamma = _hypot(p, beta)
                if trace is not None:
                    trace.beta_neg += beta < 0
                    trace.beta_pos += beta >= 0
                if beta < 0:
                    delta = (gamma - beta) * 0.5
                    s = F32(math.sqrt(delta / gamma))
                    c = F32(p / (gamma * float(s) * 2))
                else:
                    c = F32(math.sqrt((gamma + beta) / (gamma * 2)))
                    s = F32(p / (gamma * float(c) * 2))
                t0 = c * At[i] + s * At[j]            # float32 arithmetic, one rounding per operation
                t1 = -s * At[i] + c * At[j]
                At[i], At[j] = t0, t1
                Wd[i], Wd[j] = _sum_sq(t0), _sum_sq(t1)
                changed = True
                v0 = c * Vt[i] + s * Vt[j]
                v1 = -s * Vt[i] + c * Vt[j]
                Vt[i], Vt[j] = v0, v1
        if not changed:
            break
    Wd = [math.sqrt(_sum_sq(At[i])) for i in range(n)]
    for i in range(n - 1):
        j = i
        for k in range(i + 1, n):
            if Wd[j] < Wd[k]:
                j = k
        if i != j:
            Wd[i], Wd[j] = Wd[j], Wd[i]
            At[[i, j]] = At[[j, i]]
            Vt[[i, j]] = Vt[[j, i]]
    W = np.array(Wd, F64).astype(F32)
    for i in range(n):
        s = F32(1 / Wd[i] if Wd[i] > FLT_MIN else 0.0)
        At[i] = At[i] * s
    return W, Vt, sweeps


class Trace:
    """what the tests want to know about the branches a run took"""

    def __init__(self):
        self.sweeps, self.skipped, self.beta_neg, self.beta_pos = [], 0, 0, 0


def solve_svd(A, B, trace=None):
    """cv::solve(A, B, X, DECOMP_SVD) for square float matrices"""
    At = np.ascontiguousarray(np.asarray(A, F32).T).copy()
    W, Vt, sweeps = jacobi_svd(At, trace)
    X = np.zeros((N, N), F32)
    threshold = 0.0
    for w in W.tolist():
        threshold += w
    threshold *= float(F32(DBL_EPSILON * 2))
    for i in range(N):
        wi = float(W[i])
        if abs(wi) <= threshold:
            if trace is not None:
                trace.skipped += 1
            continue
        wi = 1 / wi
        buf = np.zeros(N, F64)
        for r in range(N):
            buf = buf + (At[i, r] * B[r]).astype(F64)             # the float product is rounded, then widened
        buf = buf * wi
        for r in range(N):
            X[r] = (X[r].astype(F64) + F64(Vt[i, r]) * buf).astype(F32)
    if trace is not None:
        trace.sweeps.append(sweeps)
    return X


class Filter:
    """cv::KalmanFilter(12, 12) as the StereoSlam ctor sets it up (src/lib/stereo_slam.cpp:29-41)"""

    def __init__(self, state_post=None, cov_post=None):
        self.A, self.Hm, self.Q = np.eye(N, dtype=F32), np.eye(N, dtype=F32), np.eye(N, dtype=F32) * F32(100)
        self.R = np.eye(N, dtype=F32)
        self.statePre = np.zeros(N, F32)
        self.statePost = np.zeros(N, F32) if state_post is None else np.array(state_post, F32)
        self.errorCovPre = np.zeros((N, N), F32)
        self.errorCovPost = np.eye(N, dtype=F32) if cov_post is None else np.array(cov_post, F32).reshape(N, N)
        self.gain = np.zeros((N, N), F32)

    def update(self, pose, speed, pose_var, speed_var, dt, trace=None):
        for i in range(6):
            self.A[i, 6 + i] = F32(dt)
        # predict
        self.statePre = gemm(self.A, self.statePost[:, None], False, 1, None, 0)[:, 0]
        temp1 = gemm(self.A, self.errorCovPost, False, 1, None, 0)
        self.errorCovPre = gemm(temp1, self.A, True, 1, self.Q, 1)
        self.statePost = self.statePre.copy()
        self.errorCovPost = self.errorCovPre.copy()
        for i in range(6):
            self.R[i, i] = F32(pose_var[i])
            self.R[6 + i, 6 + i] = F32(speed_var[i])
        z = np.concatenate([np.asarray(pose, F32), np.asarray(speed, F32)])
        # correct
        temp2 = gemm(self.Hm, self.errorCovPre, False, 1, None, 0)
        temp3 = gemm(temp2, self.Hm, True, 1, self.R, 1)
        temp4 = solve_svd(temp3, temp2, trace)
        self.gain = np.ascontiguousarray(temp4.T)
        hx = gemm(self.Hm, self.statePre[:, None], False, 1, None, 0)[:, 0]
        temp5 = z - hx
        self.statePost = gemm(self.gain, temp5[:, None], False, 1, self.statePre[:, None], 1)[:, 0]
        self.errorCovPost = gemm(self.gain, temp2, False, -1, self.errorCovPre, 1)
        return self.statePost[:6].copy()

    def state_in(self):
        return np.concatenate([self.statePost, self.errorCovPost.reshape(-1)]).astype(F32)

    def state_out(self):
        return np.concatenate([self.statePre, self.statePost, self.errorCovPre.reshape(-1), self.errorCovPost.reshape(-1),
                               self.gain.reshape(-1)]).astype(F32)


def run(state_in, start_pose, samples, trace=None):
    """svo_pose_filter_batch of one state: (state_out [456], filtered [len(samples), 6]); a chained sample measures
    the previous filtered pose, the first one start_pose"""
    f = Filter(state_in[:N], state_in[N:])
    prev = np.array(start_pose, F32)
    filtered = np.zeros((len(samples), 6), F32)
    for k, sm in enumerate(samples):
        pose = prev if int(sm["flags"]) & CHAIN else sm["pose"]
        prev = f.update(pose, sm["speed"], sm["pose_var"], sm["speed_var"], float(sm["dt"]), trace)
        filtered[k] = prev
    return f.state_out(), filtered


# ------------------------------------------------------------------ samples

def sample(pose=None, speed=None, pose_var=1000.0, speed_var=(100.0, 100.0, 100.0, 0.1, 0.1, 0.1), dt=1.0 / 104, chain=False):
    s = np.zeros((), SAMPLE_DTYPE)
    if pose is not None:
        s["pose"] = pose
    if speed is not None:
        s["speed"] = speed
    s["pose_var"], s["speed_var"], s["dt"], s["flags"] = pose_var, speed_var, dt, CHAIN if chain else 0
    return s


def app_sample(rng, chain=True, dt=1.0 / 104):
    """one gyro sample of SlamApp::update_pose_from_imu: the app's variances, a rotation rate as the speed"""
    speed = np.zeros(6, F32)
    speed[3:] = (rng.uniform(-40, 40, 3) / 180.0 * math.pi).astype(F32)
    return sample(pose=rng.uniform(-1, 1, 6).astype(F32), speed=speed, dt=dt, chain=chain)


def frame_sample(rng, chain=False):
    """the update of a frame (StereoSlam::new_image): variances 0.1 / 1.0, dt = 0"""
    return sample(pose=rng.uniform(-1, 1, 6).astype(F32), speed=rng.uniform(-2, 2, 6).astype(F32), pose_var=0.1, speed_var=1.0,
                  dt=0.0, chain=chain)


def mixed_samples(rng, count):
    """chained and unchained samples, the app's and the frame path's, dt = 1/104, 0.05 and 0, mixed inside one slot"""
    out = []
    for k in range(count):
        kind = int(rng.integers(0, 4))
        if kind == 0:
            out.append(app_sample(rng, chain=True))
        elif kind == 1:
            out.append(app_sample(rng, chain=False, dt=0.05))
        elif kind == 2:
            out.append(frame_sample(rng, chain=bool(k % 2)))
        else:
            out.append(sample(pose=rng.uniform(-3, 3, 6).astype(F32), speed=rng.uniform(-1, 1, 6).astype(F32),
                              pose_var=rng.uniform(0.01, 10, 6).astype(F32), speed_var=rng.uniform(0.01, 10, 6).astype(F32),
                              dt=float(rng.uniform(0, 0.1)), chain=bool(rng.integers(0, 2))))
    return np.array(out, SAMPLE_DTYPE).reshape(count)


# ------------------------------------------------------------------ states

def fresh_state():
    return Filter().state_in()


_AFTER_50 = []


def state_after_50():
    """a filter after 50 updates of the app's loop and the frame path, interleaved"""
    if not _AFTER_50:
        rng = np.random.default_rng(50)
        f = Filter()
        pose = np.zeros(6, F32)
        for k in range(50):
            sm = frame_sample(rng) if k % 4 == 3 else app_sample(rng)
            pose = f.update(pose if int(sm["flags"]) & CHAIN else sm["pose"], sm["speed"], sm["pose_var"], sm["speed_var"],
                            float(sm["dt"]))
        _AFTER_50.append(f.state_in())
    return _AFTER_50[0].copy()


def singular_state():
    """errorCovPost = diag(-100) on rows 0..2: with dt = 0 and zero variances there (singular_sample) errorCovPre and
    S = errorCovPre + R have three zero rows, so three singular values are 0 and the solve skips them"""
    cov = np.eye(N, dtype=F32)
    for i in range(3):
        cov[i, i] = -100.0
    return np.concatenate([np.linspace(-1, 1, N).astype(F32), cov.reshape(-1)])


def singular_sample(rng, chain=False):
    pv = np.array([0, 0, 0, 0.1, 0.1, 0.1], F32)
    return sample(pose=rng.uniform(-1, 1, 6).astype(F32), speed=rng.uniform(-1, 1, 6).astype(F32), pose_var=pv, speed_var=1.0,
                  dt=0.0, chain=chain)


def coupled_state(seed=7):
    """a symmetric, strongly coupled covariance: random orthogonal basis, spectrum 1e-3 .. 1e3 (condition 1e6)"""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((N, N)))
    cov = (q * np.logspace(-3, 3, N)) @ q.T
    cov = ((cov + cov.T) / 2).astype(F32)
    return np.concatenate([rng.uniform(-2, 2, N).astype(F32), cov.reshape(-1)])


def state_of_kind(kind):
    return (fresh_state, state_after_50, singular_state, coupled_state)[kind]()


def samples_of_kind(kind, rng, count):
    """`count` samples for a state of `kind`: mixed, but the singular state starts with its singular sample"""
    s = mixed_samples(rng, count)
    if kind == 2 and count > 0:
        s[0] = singular_sample(rng)
    return s


def first_launch():
    """6 states (fresh, after 50, singular, coupled, fresh, coupled) with counts 1, 0, 7, 3, 0, 2"""
    rng = np.random.default_rng(101)
    kinds, counts = (0, 1, 2, 3, 0, 3), (1, 0, 7, 3, 0, 2)
    return [(state_of_kind(k), rng.uniform(-1, 1, 6).astype(F32), samples_of_kind(k, rng, c)) for k, c in zip(kinds, counts)]


def second_launch():
    """70 states, kind i % 4, count i % 5: more than one wavefront's worth of lanes, rows or slots"""
    rng = np.random.default_rng(202)
    return [(state_of_kind(i % 4), rng.uniform(-1, 1, 6).astype(F32), samples_of_kind(i % 4, rng, i % 5)) for i in range(70)]


def pack(cases):
    """the arrays of svo_pose_filter_batch for a list of (state_in, start_pose, samples)"""
    state_in = np.stack([c[0] for c in cases]).astype(F32)
    start = np.stack([c[1] for c in cases]).astype(F32)
    first = np.concatenate([[0], np.cumsum([len(c[2]) for c in cases])]).astype(np.int32)
    samples = np.concatenate([c[2] for c in cases]) if cases else np.zeros(0, SAMPLE_DTYPE)
    return state_in, start, first, samples


_REFERENCE = {}


def reference(name):
    """(cases, [(state_out, filtered) per case], Trace) of first_launch / second_launch, computed once"""
    if name not in _REFERENCE:
        cases = {"first": first_launch, "second": second_launch}[name]()
        trace = Trace()
        _REFERENCE[name] = (cases, [run(*c, trace) if len(c[2]) else None for c in cases], trace)
    return _REFERENCE[name]
