"""Plain statements of the two geometry stages that sit between the window kernels (the merge and the line-search
Gauss-Newton of the reprojection refinement; the outlier check, the depth update, the flag write-back and the
inside counter of the depth filter), and the case lists of tests/test_geometry_cpu.py and
tests/test_geometry_gpu.py.

Nothing here calls the HIP library. numpy only, written from the reference's source:

  merge_ref          PoseRefiner::refine_pose, src/lib/pose_refinement.cpp:125-150
  reproj_cost_ref    PoseRefinerCallback::do_calc, :321-348
  reproj_normal_ref  the loop of PoseRefinerCallback::get_gradient, :350-396 (the 36 + 6 sums in keypoint order)
  reproj_gn_ref      PoseRefiner::update_pose, :236-290, with the solve of :398-412
  outlier_ref        DepthFilter::outlier_check, src/lib/depth_filter.cpp:52-128
  update_ref         DepthFilter::update_kps3d, :130-257
  writeback_ref      the loop of StereoSlam::new_image, src/lib/stereo_slam.cpp:205-229, and the counter of
                     KeyFrameManager::keyframe_needed, src/lib/keyframe_manager.cpp:47-74

Every float step is one IEEE operation of the type the reference uses there (np.float32 arrays and scalars, double
where the reference computes in double: cv::projectPoints, fabs(..) > 3.0, < 0.1, 0.5 / sqrt, 1.0 / kx), and every
sum runs in the reference's order. Five primitives come from oracle_py, where tests/test_oracle_cpu.py ties them
down: rodrigues, inv_svd, solve_svd, kf1_update, exponential_map. Everything else, project_keypoints included, is
restated here.

Every statement takes T: np.float32 is the statement proper; np.float64 is its twin, the same expressions with
every value kept in double (the five primitives replaced by numpy's double ones). A twin does not say what the
kernel must give; it says whether the float formula is a sound formula. Every statement also labels, per keypoint
or per run, the branch it took; `at_threshold` marks a comparison whose operand lies within 1e-4 (relative) of its
constant, where the float statement and its twin may rightly decide differently.

No label is left out: the two that may be missing are reached as well (written next to `filter_cases`).
"""
import functools

import numpy as np

import oracle_py as O

F, D = np.float32, np.float64
IGNORE_DURING_REFINEMENT, IGNORE_COMPLETELY, IGNORE_TEMPORARY = 1, 2, 4
_FLAG_LABEL = ((IGNORE_DURING_REFINEMENT, "skipped_by_flag_during_refinement"),
               (IGNORE_COMPLETELY, "skipped_by_flag_completely"), (IGNORE_TEMPORARY, "skipped_by_flag_temporary"))

REPROJ_LABELS = ("merged", "moved_over_9px", "occluded", "err_inf") + tuple(l for _, l in _FLAG_LABEL) + (
    "residual_over_3px_x", "residual_over_3px_y", "took_part", "accepted_first_try", "accepted_after_halving",
    "exit_small", "ran_50", "nan_step", "no_keypoint_takes_part")
FILTER_LABELS = ("outlier", "inlier", "disparity_clamped", "disparity_nan", "ref_in_camera_plane",
                 "both_infinite_is_inlier", "ignored_counts_outlier", "near_skipped", "near_x_only", "near_y_only",
                 "rotated_diff_negative", "updated", "rank_deficient_rays", "zero_depth_measurement",
                 "flag_set_completely", "temporary_cleared", "counts_equal", "inside", "outside_left", "outside_top",
                 "outside_right", "outside_bottom", "inside_but_ignored", "projection_nan")
ALLOWED_MISSING = ("rank_deficient_rays", "both_infinite_is_inlier")
# labels of a case that keep it out of the comparison with the float64 twin
NO_TWIN_LABELS = ("at_threshold", "nan_step", "err_inf", "disparity_nan", "projection_nan", "ref_in_camera_plane",
                  "both_infinite_is_inlier", "zero_depth_measurement", "rank_deficient_rays",
                  "no_keypoint_takes_part", "ran_50", "non_finite", "underdetermined",
                  "starts_at_zero_cost")

CAMERAS = {   # the pinhole part of the synthetic configurations (stereo_svo_slam_amd/synth.py), and one with powers of two
    "euroc": dict(width=752, height=480, fx=435.2046959714599, fy=435.2046959714599, cx=367.4517211914062,
                  cy=252.2008514404297, baseline=47.90639384423901, k1=0.0, k2=0.0, k3=0.0, p1=0.0, p2=0.0),
    "econ": dict(width=752, height=480, fx=743.8041254687444, fy=743.8041254687444, cx=365.86266803741455,
                 cy=238.70182609558105, baseline=45.1932, k1=0.12598132, k2=-0.22447148, k3=0.09229389,
                 p1=0.00074527, p2=0.00802387),
    "pow2": dict(width=320, height=240, fx=256.0, fy=256.0, cx=160.0, cy=120.0, baseline=32.0, k1=0.0, k2=0.0,
                 k3=0.0, p1=0.0, p2=0.0),
}


def same_bits(a, b):
    """element-wise: equal bit patterns, or both NaN"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype.kind != "f":
        return a == b
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return (a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))


def _near(v, c):
    with np.errstate(all="ignore"):
        return np.abs(np.asarray(v, D) - c) <= 1e-4 * abs(c)


# ------------------------------------------------------------------ primitives
def _rodrigues(r, T):
    """cv::Rodrigues, double [3, 3]; r: three values of type T"""
    if T is F:
        return O.rodrigues(np.asarray(r, F))
    r = np.asarray(r, D)
    theta = np.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2])
    if theta < np.finfo(D).eps:
        return np.eye(3)
    c, s = np.cos(theta), np.sin(theta)
    k = r / theta
    kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return c * np.eye(3) + (1 - c) * np.outer(k, k) + s * kx


@functools.lru_cache(maxsize=4096)
def _pose_mats_cached(key, T):
    r = np.frombuffer(key, T)
    return _rodrigues(r, T).astype(T), _rodrigues(-r, T).astype(T)


def pose_mats(pose, T):
    """PoseManager::set_pose (src/lib/pose_manager.cpp:9-17): R(r) and R(-r), rounded to T"""
    r = np.asarray(pose[3:6], T)
    return _pose_mats_cached(r.tobytes(), T)


def _matvec(M, v):
    """Matx33f * Vec3f: s = 0, s += M[i][k] * v[k] for k = 0, 1, 2. M [3, 3] or [n, 3, 3]; v a list of three
    scalars or arrays"""
    out = []
    for i in range(3):
        s = M.dtype.type(0)
        for k in range(3):
            s = s + M[..., i, k] * v[k]
        out.append(s)
    return out


def _cam(cam, T):
    """the camera's float members, as T"""
    return {k: T(F(cam[k])) for k in ("fx", "fy", "cx", "cy", "baseline", "k1", "k2", "k3", "p1", "p2")}


def project_ref(pose, pts, cam, T=F):
    """project_keypoints, src/lib/transform_keypoints.cpp:11-48: the points minus the translation in float, then
    cv::projectPoints(rvec = -r, tvec = 0, K, dist) in double, stored as float"""
    pose = np.asarray(pose, T)
    pts = np.asarray(pts, T).reshape(-1, 3)
    R = _rodrigues(-pose[3:6], T)
    c = _cam(cam, D)
    with np.errstate(all="ignore"):
        X, Y, Z = ((pts[:, k] - pose[k]).astype(D) for k in range(3))
        x = R[0, 0] * X + R[0, 1] * Y + R[0, 2] * Z + 0.0
        y = R[1, 0] * X + R[1, 1] * Y + R[1, 2] * Z + 0.0
        z = R[2, 0] * X + R[2, 1] * Y + R[2, 2] * Z + 0.0
        z = np.where(z != 0, 1.0 / z, 1.0)                 # z ? 1. / z : 1
        x, y = x * z, y * z
        r2 = x * x + y * y
        r4 = r2 * r2
        r6 = r4 * r2
        a1, a2, a3 = 2 * x * y, r2 + 2 * x * x, r2 + 2 * y * y
        cdist = 1 + c["k1"] * r2 + c["k2"] * r4 + c["k3"] * r6
        xd = x * cdist + c["p1"] * a1 + c["p2"] * a2
        yd = y * cdist + c["p1"] * a3 + c["p2"] * a1
        return np.stack([xd * c["fx"] + c["cx"], yd * c["fy"] + c["cy"]], 1).astype(T)


# ------------------------------------------------------------------ reprojection refinement
def merge_ref(kps2d, flags, tracked, err, T=F):
    """(kps2d, flags, labels): entry i of the frame meets its own tracked position and error (the reverse
    iteration and the pop_back of :125-150 are bookkeeping)"""
    k2 = np.array(kps2d, T).reshape(-1, 2)
    tr = np.asarray(tracked, T).reshape(-1, 2)
    fl = np.array(flags, np.uint32)
    labels = []
    for i in range(len(k2)):
        dx, dy = k2[i, 0] - tr[i, 0], k2[i, 1] - tr[i, 1]
        diff = dx * dx + dy * dy
        e = T(err[i])
        lab = set()
        if _near(e, 20) or (not e > 20 and _near(diff, 81)):
            lab.add("at_threshold")
        if e > 20:
            fl[i] |= IGNORE_COMPLETELY
            lab.add("err_inf" if np.isinf(e) else "occluded")
        elif diff > 81:
            fl[i] |= IGNORE_DURING_REFINEMENT
            lab.add("moved_over_9px")
        else:
            fl[i] &= ~np.uint32(IGNORE_DURING_REFINEMENT)
            k2[i] = tr[i]
            lab.add("merged")
        labels.append(lab)
    return k2, fl, labels


def _active(flags):
    return (np.asarray(flags, np.uint32) & 7) == 0


def reproj_cost_ref(kps2d, kps3d, flags, cam, pose, T=F):
    """tot_diff of do_calc: cv::absdiff of the projections and the positions, summed over the keypoints that no
    flag excludes, in keypoint order"""
    k2 = np.asarray(kps2d, T).reshape(-1, 2)
    proj = project_ref(pose, kps3d, cam, T)
    with np.errstate(all="ignore"):
        term = np.abs(proj[:, 0] - k2[:, 0]) + np.abs(proj[:, 1] - k2[:, 1])
        tot = T(0)
        for i in np.nonzero(_active(flags))[0]:
            tot = tot + term[i]
    return tot


def _jacobian(fx, fy, x, y, z):
    """the 2 x 6 Jacobian of :380-381, rows first"""
    zero = np.zeros_like(x)
    one = x.dtype.type(1)
    zz = z * z
    return [-fx / z, zero, fx * x / zz, fx * x * y / zz, -fx * (one + (x * x) / zz), fx * y / z,
            zero, -fy / z, fy * y / zz, fy * (one + (y * y) / zz), -fy * x * y / zz, -fy * x / z]


def reproj_normal_ref(kps2d, kps3d, flags, cam, pose, T=F):
    """(H [36], err [6], labels): hessian += J^T J and err += J^T diff over the keypoints in order, each entry
    s = 0, s += J[0][a] * J[0][b], s += J[1][a] * J[1][b] (Matx product), then added to its sum"""
    k2 = np.asarray(kps2d, T).reshape(-1, 2)
    k3 = np.asarray(kps3d, T).reshape(-1, 3)
    pose = np.asarray(pose, T)
    n = len(k2)
    c = _cam(cam, T)
    proj = project_ref(pose, k3, cam, T)
    _, inv_rot = pose_mats(pose, T)
    flags = np.asarray(flags, np.uint32)
    with np.errstate(all="ignore"):
        x, y, z = _matvec(inv_rot, [k3[:, k] - pose[k] for k in range(3)])
        J = _jacobian(c["fx"], c["fy"], x, y, z)
        d0, d1 = k2[:, 0] - proj[:, 0], k2[:, 1] - proj[:, 1]
        over_x, over_y = np.abs(d0.astype(D)) > 3.0, np.abs(d1.astype(D)) > 3.0
        terms = np.zeros((n, 42), T)
        for a in range(6):
            for b in range(6):
                s = T(0) + J[a] * J[b]
                terms[:, a * 6 + b] = s + J[6 + a] * J[6 + b]
            s = T(0) + J[a] * d0
            terms[:, 36 + a] = s + J[6 + a] * d1
        sums = np.zeros(42, T)
        labels = []
        for i in range(n):
            lab = {l for bit, l in _FLAG_LABEL if flags[i] & bit}
            if not lab:
                if _near(np.abs(d0[i]), 3.0) or _near(np.abs(d1[i]), 3.0):
                    lab.add("at_threshold")
                if over_x[i]:
                    lab.add("residual_over_3px_x")
                if over_y[i]:
                    lab.add("residual_over_3px_y")
                if not (over_x[i] or over_y[i]):
                    lab.add("took_part")
                    sums = sums + terms[i]
            labels.append(lab)
        if 0 < sum("took_part" in l for l in labels) < 3:
            labels[0].add("underdetermined")           # fewer than three points: J^T J has no inverse
    return sums[:36].copy(), sums[36:].copy(), labels


def _exponential_map_d(twist):
    """exponential_map (src/include/exponential_map.hpp:12-37) in double: the norm is hard set to 1"""
    v, w = twist[:3], twist[3:]
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    M = np.eye(3) + K * (1 - np.cos(1.0)) + (K @ K) * (1.0 - np.sin(1.0))
    return np.concatenate([M @ v, w])


def reproj_step_ref(H, err, T=F):
    """hessian.inv(DECOMP_SVD) * err through exponential_map, :398-411"""
    with np.errstate(all="ignore"):
        if T is F:
            Hinv, _ = O.inv_svd(np.asarray(H, F).reshape(6, 6))
            twist = np.zeros(6, F)
            for a in range(6):
                s = F(0)
                for b in range(6):
                    s = s + Hinv[a, b] * err[b]
                twist[a] = s
            return O.exponential_map(twist)
        H = np.asarray(H, D).reshape(6, 6)
        if not np.all(np.isfinite(H)) or not np.all(np.isfinite(err)):
            return np.full(6, np.nan)
        return _exponential_map_d(np.linalg.pinv(H, rcond=1e-15) @ err)


def reproj_gn_ref(kps2d, kps3d, flags, cam, pose_in, T=F):
    """dict(pose, cost, n_gradient, n_cost, n_accepted, exit_small, initial_cost, labels, kp_labels): the
    line-search Gauss-Newton of update_pose. kp_labels are those of the first get_gradient (at pose_in)."""
    max_iter = 50
    x0 = np.array(pose_in, T)
    labels = set()
    n_grad, n_cost, accepted, exit_small = 0, 1, 0, 0
    prev_cost = reproj_cost_ref(kps2d, kps3d, flags, cam, x0, T)
    initial = prev_cost
    if initial == 0:
        labels.add("starts_at_zero_cost")              # (nothing to compare relative to)
    kp_labels = None
    i = 0
    with np.errstate(all="ignore"):
        while i < max_iter:
            H, e, kl = reproj_normal_ref(kps2d, kps3d, flags, cam, x0, T)
            gradient = np.asarray(reproj_step_ref(H, e, T), T)
            if kp_labels is None:
                kp_labels = kl
                if not any("took_part" in l for l in kl):
                    labels.add("no_keypoint_takes_part")
            if np.any(np.isnan(gradient)):
                labels.add("nan_step")
            n_grad += 1
            k = T(1.0)
            while i < max_iter:
                x = x0 + k * gradient
                new_cost = reproj_cost_ref(kps2d, kps3d, flags, cam, x, T)
                n_cost += 1
                if new_cost < prev_cost:
                    x0, prev_cost = x, new_cost
                    accepted += 1
                    labels.add("accepted_first_try" if k == 1 else "accepted_after_halving")
                    break
                elif np.abs(D(new_cost - prev_cost)) < 0.0001:
                    i = max_iter
                    exit_small = 1
                    labels.add("exit_small")
                    break
                else:
                    k = k / T(2)
                i += 1
            i += 1
    if not exit_small:
        labels.add("ran_50")
    return dict(pose=x0, cost=prev_cost, n_gradient=n_grad, n_cost=n_cost, n_accepted=accepted,
                exit_small=exit_small, initial_cost=initial, labels=labels, kp_labels=kp_labels)


# ------------------------------------------------------------------ depth filter
def _vec(a, T):
    return [T(v) for v in a]


def pixel_distance_ref(kp2d, d, cam, frame_pose, ref3d, kf_pose, T=F):
    """(pixel_distance, labels) of one keypoint of outlier_check"""
    c = _cam(cam, T)
    frame_pose, kf_pose = np.asarray(frame_pose, T), np.asarray(kf_pose, T)
    rot, _ = pose_mats(frame_pose, T)
    _, kinv = pose_mats(kf_pose, T)
    lab = set()
    with np.errstate(all="ignore"):
        d = T(d)
        half = T(0.5)
        dd = half if d < half else d                   # std::max<float>(d, 0.5): (a < b) ? b : a, NaN stays
        if np.isnan(d):
            lab.add("disparity_nan")
        elif d < half:
            lab.add("disparity_clamped")
        if _near(d, 0.5) and d != half:
            lab.add("at_threshold")
        _z = c["baseline"] / dd
        _x = (T(kp2d[0]) - c["cx"]) / c["fx"] * _z
        _y = (T(kp2d[1]) - c["cy"]) / c["fy"] * _z
        p = _matvec(rot, [_x, _y, _z])
        p = [p[k] + frame_pose[k] for k in range(3)]
        a = _matvec(kinv, [p[k] - kf_pose[k] for k in range(3)])
        r = _matvec(kinv, [T(ref3d[k]) - kf_pose[k] for k in range(3)])
        disp_ref = c["baseline"] / r[2]
        disp = c["baseline"] / a[2]
        if r[2] == 0:
            lab.add("ref_in_camera_plane")
        if a[2] == 0:
            lab.add("zero_depth_measurement")
        pd = disp - disp_ref
        if np.isinf(disp) and np.isinf(disp_ref) and np.isnan(pd):
            lab.add("both_infinite_is_inlier")
        if not np.isfinite(pd):
            lab.add("non_finite")
        if _near(np.abs(pd), 2.5):
            lab.add("at_threshold")
    return pd, lab


def outlier_ref(kps2d, disparity, cam, frame_pose, ref3d, kf_pose, outlier, inlier, T=F):
    """(outlier_count, inlier_count, labels)"""
    outl, inl = np.array(outlier, np.int32), np.array(inlier, np.int32)
    labels = []
    for i in range(len(outl)):
        pd, lab = pixel_distance_ref(kps2d[i], disparity[i], cam, frame_pose, ref3d[i], kf_pose[i], T)
        deviation = T(0.5)
        if np.abs(pd) > T(5) * deviation:
            outl[i] += 1
            lab.add("outlier")
        else:
            inl[i] += 1
            lab.add("inlier")
        labels.append(lab)
    return outl, inl, labels


def _kf1_update_d(x, P, Q, R, meas):
    """the 1-state cv::KalmanFilter predict() + correct() in double: A = H = 1"""
    pre, cov = x, P + Q
    gain = cov / (cov + R) if cov + R != 0 else 0.0   # (the SVD solve of a zero 1 x 1 system is 0)
    return gain * (meas - pre) + pre, -(gain * cov) + cov


def update_ref(kps2d, kps3d, flags, cam, frame_pose, ref2d, kf_pose, outlier, kf_inv_depth, kf_variance, T=F):
    """(kps3d, outlier_count, kf_inv_depth, kf_variance, labels)"""
    c = _cam(cam, T)
    k3 = np.array(kps3d, T).reshape(-1, 3)
    outl = np.array(outlier, np.int32)
    kx, kP = np.array(kf_inv_depth, T), np.array(kf_variance, T)
    frame_pose = np.asarray(frame_pose, T)
    frot, _ = pose_mats(frame_pose, T)
    labels = []
    with np.errstate(all="ignore"):
        for i in range(len(k3)):
            lab = set()
            labels.append(lab)
            kp = np.asarray(kf_pose[i], T)
            krot, kinv = pose_mats(kp, T)
            c1, c2 = [kp[0], kp[1], kp[2]], [frame_pose[0], frame_pose[1], frame_pose[2]]
            diff = _matvec(kinv, [np.abs(c1[k] - c2[k]) for k in range(3)])
            if flags[i] & (IGNORE_COMPLETELY | IGNORE_DURING_REFINEMENT):
                outl[i] += 1
                lab.add("ignored_counts_outlier")
                continue
            if diff[0] < 0 or diff[1] < 0:
                lab.add("rotated_diff_negative")
            if _near(diff[0], 0.1) or _near(diff[1], 0.1):
                lab.add("at_threshold")
            near_x, near_y = D(diff[0]) < 0.1, D(diff[1]) < 0.1
            if near_x and near_y:
                lab.add("near_skipped")
                continue
            if near_x:
                lab.add("near_x_only")
            if near_y:
                lab.add("near_y_only")
            p1 = _matvec(krot, [T(ref2d[i][0]) - c["cx"], T(ref2d[i][1]) - c["cy"], c["fx"]])
            p2 = _matvec(frot, [T(kps2d[i][0]) - c["cx"], T(kps2d[i][1]) - c["cy"], c["fx"]])
            A = np.array([[p1[0], -p2[0]], [p1[1], -p2[1]], [p1[2], -p2[2]]], T)
            yv = np.array([c2[k] - c1[k] for k in range(3)], T)
            if np.all(np.isfinite(A)):
                sv = np.linalg.svd(A.astype(D), compute_uv=False)
                if sv[1] <= 1e-6 * sv[0]:
                    lab.add("rank_deficient_rays")
            if T is F:
                l0 = O.solve_svd(A, yv)[0]
            else:
                l0 = np.linalg.lstsq(A, yv, rcond=1e-15)[0][0] if np.all(np.isfinite(A)) else np.nan
            s = diff[0] * diff[0] + diff[1] * diff[1]
            deviation = T(0.5 / D(np.sqrt(s)))
            Rm = deviation * deviation
            new_p = _matvec(kinv * l0, [p1[k] - c1[k] for k in range(3)])
            _z = new_p[2]
            if _z == 0:
                lab.add("zero_depth_measurement")
            meas = T(1) / _z
            if T is F:
                x, P = O.kf1_update(float(kx[i]), float(kP[i]), 0.0001, float(Rm), float(meas))
                kx[i], kP[i] = F(x), F(P)
            else:
                kx[i], kP[i] = _kf1_update_d(kx[i], kP[i], D(F(0.0001)), Rm, meas)
            _z = T(1.0 / D(kx[i]))
            _x = (T(ref2d[i][0]) - c["cx"]) / c["fx"] * _z
            _y = (T(ref2d[i][1]) - c["cy"]) / c["fy"] * _z
            cp = _matvec(krot, [_x, _y, _z])
            k3[i] = [c1[k] + cp[k] for k in range(3)]
            lab.add("updated")
            if not (np.all(np.isfinite(k3[i])) and np.isfinite(kx[i]) and np.isfinite(kP[i])):
                lab.add("non_finite")
    return k3, outl, kx, kP, labels


def writeback_ref(flags, outlier, inlier, kps3d, cam, frame_pose, width, height, T=F):
    """(flags, kps2d, inside, labels): the two counter rules of stereo_slam.cpp:212-216, the projection of :228,
    and the counter of keyframe_needed with its five conditions"""
    fl = np.array(flags, np.uint32)
    proj = project_ref(frame_pose, kps3d, cam, T)
    inside = 0
    labels = []
    w, h = T(width), T(height)                         # (kp.x < image_width: the int becomes a float)
    for i in range(len(fl)):
        lab = set()
        if outlier[i] > inlier[i]:
            fl[i] |= IGNORE_COMPLETELY
            lab.add("flag_set_completely")
        if inlier[i] > outlier[i]:
            if fl[i] & IGNORE_TEMPORARY:
                lab.add("temporary_cleared")
            fl[i] &= ~np.uint32(IGNORE_TEMPORARY)
        if outlier[i] == inlier[i]:
            lab.add("counts_equal")
        x, y = proj[i]
        if np.isnan(x) or np.isnan(y):
            lab.add("projection_nan")
        if any(_near(v, c) or abs(D(v)) < 1e-4 for v, c in ((x, D(w)), (y, D(h)))):
            lab.add("at_threshold")
        geom = True
        for cond, name in ((x > 0, "outside_left"), (y > 0, "outside_top"), (x < w, "outside_right"),
                           (y < h, "outside_bottom")):
            if not cond:
                geom = False
                if not (np.isnan(x) or np.isnan(y)):
                    lab.add(name)
        if geom and not (fl[i] & IGNORE_COMPLETELY):
            inside += 1
            lab.add("inside")
        elif geom:
            lab.add("inside_but_ignored")
        labels.append(lab)
    return fl, proj, inside, labels


def all_labels(*label_lists):
    out = set()
    for ll in label_lists:
        for l in ll:
            out |= set(l) if not isinstance(l, str) else {l}
    return out


# ------------------------------------------------------------------ reprojection cases
REPROJ_COUNTS = (1, 2, 27, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300)


def _next(v, up=True):
    return np.nextafter(F(v), F(np.inf if up else -np.inf))


def _scene(rng, n, cam, true_pose, noise):
    """n points in front of the camera and their observations from true_pose"""
    z = rng.uniform(2.0, 9.0, n)
    u, v = rng.uniform(20, cam["width"] - 20, n), rng.uniform(20, cam["height"] - 20, n)
    k3 = np.stack([(u - cam["cx"]) / cam["fx"] * z, (v - cam["cy"]) / cam["fy"] * z, z], 1).astype(F)
    obs = project_ref(np.asarray(true_pose, F), k3, cam) + rng.normal(0, noise, (n, 2)).astype(F) if noise else \
        project_ref(np.asarray(true_pose, F), k3, cam)
    return k3, obs.astype(F)


TRUE_POSE = (0.02, -0.01, 0.03, 0.004, -0.006, 0.002)
ECON_POSE = (0.01, -0.005, 0.015, 0.002, -0.003, 0.001)    # (the focal length is longer: the same 3 px are less motion)


def _reproj_case(name, cam="euroc", n=40, seed=0, noise=0.25, start=(0, 0, 0, 0, 0, 0), true_pose=TRUE_POSE,
                 edit=None, gentle=True):
    """kps2d are the projections from `start` (what the tracker hands to the merge), tracked the observations"""
    camd = CAMERAS[cam]
    rng = np.random.RandomState(1000 + seed)
    k3, tracked = _scene(rng, n, camd, true_pose, noise)
    start = np.asarray(start, F)
    k2 = project_ref(start, k3, camd)
    err = rng.uniform(0, 10, n).astype(F)
    flags = np.zeros(n, np.uint32)
    if gentle and n >= 20:                               # what the parity test has: a few moved, occluded, flagged
        tracked[::17] += F(15.0)
        err[::13] = F(30.0)
        flags[3::11] = rng.randint(1, 8, len(flags[3::11]))
    case = dict(name=name, cam=camd, kps2d=k2, kps3d=k3, flags=flags, tracked=tracked, err=err, start=start)
    if edit:
        edit(case, rng)
    for k in ("kps2d", "kps3d", "tracked", "err", "start"):
        case[k] = np.ascontiguousarray(case[k], F)
    return case


def _edit_offsets(case, rng):
    """tracked offsets of squared length exactly 81 and of the next float above it: (9, 0) and (0, 9) from
    quarter-pixel positions, where the subtraction is exact; (9, dy) with the largest dy whose square is lost in
    the sum and the smallest whose square is not"""
    t, k = case["tracked"], case["kps2d"]
    t[:8] = np.round(t[:8] * 4) / 4
    t[4:8, 1] = 0
    t[6, 0] = 0                                        # (x + nextafter(9) is exact only from 0)
    dy_keep = F(2.0 ** -9)
    while F(F(81) + dy_keep * dy_keep) == F(81):
        dy_keep = _next(dy_keep)
    dy_lost = _next(dy_keep, False)
    assert F(F(81) + dy_keep * dy_keep) == _next(81) and F(F(81) + dy_lost * dy_lost) == F(81)
    nine_up = _next(9)
    for i, (dx, dy) in enumerate(((9, 0), (0, 9), (-9, 0), (0, -9), (9, dy_lost), (9, dy_keep), (nine_up, 0),
                                  (-9, dy_keep))):
        k[i] = t[i] + np.array([dx, dy], F)
        assert k[i, 0] - t[i, 0] == F(dx) and k[i, 1] - t[i, 1] == F(dy)
    case["err"][:8] = 1
    case["flags"][:8] = (0, 1, 0, 1, 0, 0, 1, 0)


def _edit_err(case, rng):
    case["err"][:6] = (20, _next(20), np.inf, np.nan, -np.inf, _next(20, False))
    case["flags"][:6] = 0


def _edit_residuals(case, rng):
    """observations whose residual at the start pose is exactly 3.0 and the next float above, in x alone and in y
    alone, both signs (kps2d are the start pose's projections: the merged offset is 3 px)"""
    k, t = case["kps2d"], case["tracked"]
    for i, (axis, sign, above) in enumerate((a, s, u) for a in (0, 1) for s in (1, -1) for u in (False, True)):
        t[i] = k[i]
        v = F(k[i, axis] + F(3 * sign))
        while abs(F(v - k[i, axis])) > 3:
            v = _next(v, sign < 0)
        while abs(F(v - k[i, axis])) < 3:
            v = _next(v, sign > 0)
        assert abs(F(v - k[i, axis])) == 3
        t[i, axis] = _next(v, sign > 0) if above else v
    case["err"][:8] = 1
    case["flags"][:8] = 0


def _edit_centre(case, rng):
    """keypoint 0 at the camera centre of the start pose, observed 1 px from the principal point: z = 0, the
    Jacobian is inf and NaN, every step is NaN"""
    case["kps3d"][0] = case["start"][:3]
    case["kps2d"][0] = (case["cam"]["cx"], case["cam"]["cy"])
    case["tracked"][0] = case["kps2d"][0] + F(1)
    case["err"][0], case["flags"][0] = 1, 0


def _edit_behind(case, rng):
    case["kps3d"][:3, 2] = (-4.0, -0.5, -40.0)
    case["kps2d"][:3] = project_ref(case["start"], case["kps3d"][:3], case["cam"])
    case["tracked"][:3] = case["kps2d"][:3] + F(0.5)
    case["err"][:3], case["flags"][:3] = 1, 0


def _edit_off_axis(case, rng):
    case["kps3d"][:2] = ((250.0, 3.0, 5.0), (-2.0, -400.0, 3.0))
    case["kps2d"][:2] = project_ref(case["start"], case["kps3d"][:2], case["cam"])
    case["tracked"][:2] = case["kps2d"][:2] + F(0.25)
    case["err"][:2], case["flags"][:2] = 1, 0


def _edit_all_ignored(case, rng):
    case["flags"][:] = rng.randint(1, 8, len(case["flags"]))
    case["flags"][case["flags"] == 1] = 2              # (the merge clears bit 0 of what it merges)


def _edit_far_start(case, rng):
    """the start is 0.3 rad away about the optical axis. Only points within 8 px of the principal point have a
    residual below 3 px there and take part; the positions handed to the merge are next to the observations (the
    9 px rule would flag every keypoint otherwise)"""
    n = len(case["kps3d"])
    cam = case["cam"]
    z = rng.uniform(2.0, 9.0, n // 2)
    ang, rad = rng.uniform(0, 2 * np.pi, n // 2), rng.uniform(0.5, 8.0, n // 2)
    case["kps3d"][:n // 2] = np.stack([rad * np.cos(ang) / cam["fx"] * z, rad * np.sin(ang) / cam["fy"] * z, z], 1)
    obs = project_ref(np.asarray(TRUE_POSE, F), case["kps3d"], cam)
    case["tracked"] = (obs + rng.normal(0, 0.25, obs.shape)).astype(F)
    case["kps2d"] = (case["tracked"] + rng.normal(0, 1.0, obs.shape)).astype(F)
    case["err"][:], case["flags"][:] = 1, 0


def _edit_exact(case, rng):
    case["err"][:] = 1
    case["flags"][:] = 0


@functools.lru_cache(maxsize=None)
def reproj_cases():
    cases = [_reproj_case(f"count{n}", n=n, seed=n) for n in REPROJ_COUNTS]
    cases += [
        _reproj_case("offsets81", n=60, seed=1, edit=_edit_offsets),
        _reproj_case("err_edges", n=60, seed=2, edit=_edit_err),
        _reproj_case("residual3", n=60, seed=3, noise=0.1, edit=_edit_residuals),
        _reproj_case("camera_centre", n=60, seed=4, edit=_edit_centre),
        _reproj_case("behind_camera", n=60, seed=5, edit=_edit_behind),
        _reproj_case("far_off_axis", n=60, seed=6, edit=_edit_off_axis),
        _reproj_case("all_ignored", n=60, seed=7, edit=_edit_all_ignored),
        _reproj_case("zero_noise_at_minimum", n=60, seed=8, noise=0, start=TRUE_POSE, edit=_edit_exact, gentle=False),
        _reproj_case("start_0.3rad", n=80, seed=9, start=(0, 0, 0, 0, 0, 0.3), edit=_edit_far_start),
        _reproj_case("start_0.3rad_200", n=200, seed=10, start=(0, 0, 0, 0, 0, -0.3), edit=_edit_far_start),
        _reproj_case("econ_distortion", cam="econ", n=70, seed=11, true_pose=ECON_POSE),
        _reproj_case("econ_distortion_140", cam="econ", n=140, seed=12, true_pose=ECON_POSE, start=(0.004, 0, 0, 0, 0.001, 0)),
    ]
    assert len({c["name"] for c in cases}) == len(cases)
    return cases


def reproj_results(T=F):
    """name -> dict(merged kps2d, flags, reproj_gn_ref result, sums H, e at the start pose, labels)"""
    return _reproj_results(T)


@functools.lru_cache(maxsize=None)
def _reproj_results(T):
    out = {}
    for c in reproj_cases():
        k2, fl, ml = merge_ref(c["kps2d"], c["flags"], c["tracked"], c["err"], T)
        gn = reproj_gn_ref(k2, c["kps3d"], fl, c["cam"], c["start"], T)
        H, e, _ = reproj_normal_ref(k2, c["kps3d"], fl, c["cam"], c["start"], T)
        out[c["name"]] = dict(kps2d=k2, flags=fl, merge_labels=ml, gn=gn, H=H, e=e,
                              labels=all_labels(ml, gn["kp_labels"], gn["labels"]))
    return out


# ------------------------------------------------------------------ depth filter cases
FILTER_COUNTS = (1, 63, 64, 65, 128, 129)
KF_POSES = ((0.0, 0.0, 0.0, 0.0, 0.0, 0.0), (0.01, 0.0, 0.0, 0.001, 0.0, 0.0), (-0.3, 0.2, 0.1, 0.02, -0.03, 0.01))
FRAME_POSE = (0.15, 0.12, 0.02, 0.01, -0.02, 0.005)


def _filter_case(name, cam="euroc", n=40, seed=0, frame_pose=FRAME_POSE, kf_poses=KF_POSES, edit=None, noise=0.3):
    camd = CAMERAS[cam]
    rng = np.random.RandomState(2000 + seed)
    frame_pose = np.asarray(frame_pose, F)
    kf_pose = np.asarray(kf_poses, F)[rng.randint(0, len(kf_poses), n)]
    ref2d = np.stack([rng.uniform(5, camd["width"] - 5, n), rng.uniform(5, camd["height"] - 5, n)], 1).astype(F)
    z = rng.uniform(2.0, 12.0, n)
    local = np.stack([(ref2d[:, 0] - camd["cx"]) / camd["fx"] * z, (ref2d[:, 1] - camd["cy"]) / camd["fy"] * z, z], 1)
    ref3d = np.stack([_rodrigues(kf_pose[i, 3:], D) @ local[i] + kf_pose[i, :3] for i in range(n)]).astype(F)
    k3 = (ref3d + rng.normal(0, 0.02, (n, 3))).astype(F)
    k2 = (project_ref(frame_pose, ref3d, camd) + rng.normal(0, noise, (n, 2))).astype(F)
    depth = np.stack([_rodrigues(-frame_pose[3:], D) @ (ref3d[i] - frame_pose[:3]) for i in range(n)])[:, 2]
    disp = (camd["baseline"] / depth + rng.normal(0, 0.3, n)).astype(F)
    disp[::11] += F(6.0)
    case = dict(name=name, cam=camd, kps2d=k2, kps3d=k3, flags=rng.choice([0, 0, 0, 0, 1, 2, 4, 6], n).astype(np.uint32),
                frame_pose=frame_pose, disparity=disp, ref3d=ref3d, ref2d=ref2d, kf_pose=kf_pose,
                outlier=rng.randint(0, 3, n).astype(np.int32), inlier=rng.randint(0, 3, n).astype(np.int32),
                kf_inv_depth=(1 / z * rng.uniform(0.9, 1.1, n)).astype(F), kf_variance=rng.uniform(0.001, 0.2, n).astype(F),
                width=camd["width"], height=camd["height"])
    if edit:
        edit(case, rng)
    for k in ("kps2d", "kps3d", "disparity", "ref3d", "ref2d", "kf_pose", "kf_inv_depth", "kf_variance", "frame_pose"):
        case[k] = np.ascontiguousarray(case[k], F)
    return case


def _edit_disparities(case, rng):
    case["disparity"][:9] = (-1, 0, 0.5, _next(0.5), _next(0.5, False), 64, np.inf, np.nan, -np.inf)


def _bits_of(v):
    return int(np.array([v], F).view(np.int32)[0])


def _from_bits(b):
    return np.array([b], np.int32).view(F)[0]


def _edit_straddle(case, rng):
    """pairs of adjacent float disparities on the two sides of |pixel_distance| = 2.5: keypoints 2k and 2k + 1 are
    copies of one keypoint; the boundary is found by bisection over the floats between the disparity that agrees
    with the reference point and one 8 px (or 0.49 of it) away, with the statement as the judge"""
    n = len(case["disparity"])
    k = 0
    for src in range(n // 2, n):
        if k + 1 >= n // 2:
            break

        def out(d):
            pd, _ = pixel_distance_ref(case["kps2d"][src], d, case["cam"], case["frame_pose"], case["ref3d"][src],
                                       case["kf_pose"][src])
            return bool(np.abs(pd) > F(2.5))
        d_in = case["disparity"][src] - (F(6.0) if src % 11 == 0 else F(0))
        for d_out in (d_in + F(8.0), max(d_in * F(0.5), F(0.51))):
            if out(d_in) or not out(d_out):
                continue
            lo, hi = _bits_of(d_in), _bits_of(d_out)     # positive floats order like their bit patterns
            while abs(hi - lo) > 1:
                mid = (lo + hi) // 2
                lo, hi = (lo, mid) if out(_from_bits(mid)) else (mid, hi)
            for j, b in ((k, lo), (k + 1, hi)):
                for key in ("kps2d", "kps3d", "ref3d", "ref2d", "kf_pose", "flags", "outlier", "inlier", "kf_inv_depth",
                            "kf_variance"):
                    case[key][j] = case[key][src]
                case["disparity"][j] = _from_bits(b)
            k += 2
            if k + 1 >= n // 2:
                break
    case["straddle_pairs"] = k // 2
    assert k >= 8


def _edit_planes(case, rng):
    """identity rotations, so that every product is exact: a reference point in the keyframe's camera plane
    (depth 0 there), a measured point in it, and both"""
    b = F(case["cam"]["baseline"])
    case["frame_pose"][:] = 0
    case["kf_pose"][:4] = (0, 0, b, 0, 0, 0)             # the keyframe sits one baseline ahead of the frame
    case["disparity"][:4] = (3.0, 1.0, 1.0, 1.0)         # z = baseline / 1: the measured point has depth 0 there
    case["ref3d"][:4, 2] = (b, b + F(4), b, b)
    case["kps2d"][3] = (case["cam"]["cx"], case["cam"]["cy"])
    case["flags"][:4] = 0


def _edit_offsets01(case, rng):
    """keyframe-to-frame offsets of float32(0.1), which as a double is above 0.1, and of the float below it, in x,
    in y and in both. The frame is at the origin and the keyframes are not rotated: |c1 - c2| = c1 exactly."""
    a, b = F(0.1), _next(0.1, False)
    assert D(a) > 0.1 > D(b)
    case["frame_pose"][:] = (0, 0, 0, 0.01, -0.02, 0.005)
    offs = ((a, 0.05), (b, 0.05), (0.05, a), (0.05, b), (a, a), (b, b), (a, b), (b, a), (-a, 0.05), (0.05, -b))
    for i, (x, y) in enumerate(offs):
        case["kf_pose"][i] = (x, y, 0.3, 0, 0, 0)
    case["flags"][:len(offs)] = 0
    case["n_offsets"] = len(offs)


def _edit_flags_counters(case, rng):
    """every flag combination with counters below, equal and above"""
    n = len(case["flags"])
    case["flags"][:] = np.arange(n) % 8
    case["outlier"][:] = (np.arange(n) // 8) % 3
    case["inlier"][:] = 1


def _edit_filter_state(case, rng):
    case["kf_variance"][:6] = (0, 0, 1e6, 1e6, 0.05, 0)
    case["kf_inv_depth"][:6] = (0.2, 0, 0.2, 0, 0, 0.2)
    case["flags"][:6] = 0


def _edit_parallel(case, rng):
    """the same pixel seen from two poses of one orientation: the two rays are parallel"""
    case["kf_pose"][:] = (0.4, 0.0, 0.0) + tuple(case["frame_pose"][3:])
    case["kps2d"][:8] = case["ref2d"][:8]
    case["flags"][:8] = 0


def _edit_border(case, rng):
    """points whose projection is exactly 0, exactly the width or the height, and the nearest floats that project
    inside (the pow2 camera at the origin: x * 256 + 160 is exact)"""
    cam = case["cam"]
    case["frame_pose"][:] = 0
    pts = []
    for axis, target in ((0, 0.0), (0, float(cam["width"])), (1, 0.0), (1, float(cam["height"]))):
        c, f = (cam["cx"], cam["fx"]) if axis == 0 else (cam["cy"], cam["fy"])
        p = np.array([0.1, 0.1, 1.0], F)
        p[axis] = F((target - c) / f)
        assert project_ref(case["frame_pose"], p, cam)[0, axis] == F(target)
        q = p.copy()
        while project_ref(case["frame_pose"], q, cam)[0, axis] == F(target):
            q[axis] = np.nextafter(q[axis], F(0))
        pts += [p, q]
    pts.append(np.array([0, 0, 0], F))                   # at the camera centre: projects onto the principal point
    pts.append(np.array([np.nan, 0, 1], F))
    pts.append(np.array([0.1, 0.1, -2.0], F))            # behind the camera, projects inside
    pts.append(np.array([np.inf, 0.1, 2.0], F))
    case["kps3d"][:len(pts)] = pts
    case["kf_pose"][:len(pts)] = 0                       # next to the frame: the update leaves these points alone
    case["flags"][:len(pts)] = 0
    case["outlier"][:len(pts)], case["inlier"][:len(pts)] = 0, 1
    case["flags"][len(pts):len(pts) + 4] = 2
    case["n_border"] = len(pts)


@functools.lru_cache(maxsize=None)
def filter_cases():
    """The update runs on every case; test_geometry_gpu.py switches the four stages of the kernel on and off.
    The two labels that may be missing are both reached: `rank_deficient_rays` by `parallel_rays` (the keyframes
    have the frame's orientation and the keypoint sits on its reference pixel: the two rays have the same bits, the
    3 x 2 system has rank 1), `both_infinite_is_inlier` by `camera_planes` (no rotation, the keyframe one baseline
    ahead of the frame, disparity 1: measured and reference point both have depth +0 there, inf - inf is NaN, and
    NaN > 2.5 is false)."""
    rot1 = ((0.3, -0.5, 0.2, 0.9, -0.4, 0.3), (-0.4, 0.3, 0.1, -0.2, 1.0, 0.1), (0.2, 0.6, -0.3, 0.1, 0.2, -1.1))
    cases = [_filter_case(f"count{n}", n=n, seed=n) for n in FILTER_COUNTS]
    cases += [
        _filter_case("disparities", n=60, seed=1, edit=_edit_disparities),
        _filter_case("straddle2.5", n=40, seed=2, edit=_edit_straddle),
        _filter_case("camera_planes", cam="pow2", n=20, seed=3, edit=_edit_planes),
        _filter_case("offsets0.1", n=24, seed=4, edit=_edit_offsets01),
        _filter_case("rotated_keyframes", n=60, seed=5, kf_poses=rot1),
        _filter_case("identical_poses", n=20, seed=6, kf_poses=(FRAME_POSE,)),
        _filter_case("far_in_z_only", n=20, seed=7, kf_poses=((0.15, 0.12, 3.0, 0.0, 0.0, 0.0),),
                     frame_pose=(0.15, 0.12, 0.02, 0, 0, 0)),
        _filter_case("parallel_rays", n=20, seed=8, edit=_edit_parallel),
        _filter_case("filter_state", n=20, seed=9, edit=_edit_filter_state),
        _filter_case("flags_counters", n=72, seed=10, edit=_edit_flags_counters),
        _filter_case("border", cam="pow2", n=24, seed=11, edit=_edit_border),
        _filter_case("econ_distortion", cam="econ", n=70, seed=12),
    ]
    assert len({c["name"] for c in cases}) == len(cases)
    return cases


def filter_ref(c, T=F, do_outlier_check=1, do_update=1):
    """one case through the statements in the kernel's order: dict(outlier, inlier, kps3d, kf_inv_depth,
    kf_variance, flags, kps2d, inside, labels)"""
    outl, inl, k3, kx, kP = c["outlier"], c["inlier"], np.asarray(c["kps3d"], T), c["kf_inv_depth"], c["kf_variance"]
    lo = lu = []
    if do_outlier_check:
        outl, inl, lo = outlier_ref(c["kps2d"], c["disparity"], c["cam"], c["frame_pose"], c["ref3d"], c["kf_pose"],
                                    outl, inl, T)
    if do_update:
        k3, outl, kx, kP, lu = update_ref(c["kps2d"], k3, c["flags"], c["cam"], c["frame_pose"], c["ref2d"],
                                          c["kf_pose"], outl, kx, kP, T)
    fl, k2, inside, lw = writeback_ref(c["flags"], outl, inl, k3, c["cam"], c["frame_pose"], c["width"], c["height"], T)
    return dict(outlier=np.asarray(outl, np.int32), inlier=np.asarray(inl, np.int32), kps3d=np.asarray(k3, T),
                kf_inv_depth=np.asarray(kx, T), kf_variance=np.asarray(kP, T), flags=fl, kps2d=k2, inside=inside,
                labels=all_labels(lo, lu, lw), kp_labels=(lo, lu, lw))


def filter_results(T=F):
    """name -> {(do_outlier_check, do_update): filter_ref}"""
    return _filter_results(T)


@functools.lru_cache(maxsize=None)
def _filter_results(T):
    return {c["name"]: {sw: filter_ref(c, T, *sw) for sw in ((1, 1), (1, 0), (0, 1), (0, 0))} for c in filter_cases()}
