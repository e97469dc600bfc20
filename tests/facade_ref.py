"""Numpy statement of PoseManager::get_robot_angles (reference: src/lib/pose_manager.cpp:45-59) as the C++ facade
(hostcpp/stereo_slam_types.hpp) has to compute it, written from OpenCV's published cv::Rodrigues:

  1. the three single-axis matrices Rodrigues((rx,0,0)), ((0,ry,0)), ((0,0,rz)) from the oracle, rounded to float32
     (the reference keeps them in Matx33f);
  2. the float32 products R_z (R_x R_y) (Matx33f * Matx33f: every entry a float sum taken in k order);
  3. cv::Rodrigues with a matrix input, in double: r = (R21-R12, R02-R20, R10-R01), s = |r| / 2,
     c = (trace - 1) / 2 clamped to [-1, 1], theta = acos(c). Below s = 1e-5 the vector is 0 where c > 0 and otherwise
     theta = pi: the axis comes from the diagonal, sqrt(max((Rii + 1) / 2, 0)), y negated where R01 < 0, z negated
     where R02 < 0, and z negated once more where |x| is the smallest component and the sign of R12 disagrees with
     y * z. Elsewhere the vector is r * theta / (2 s).

cv::Rodrigues first replaces its input by the nearest rotation (an SVD); that step is left out here and in the facade
(parity unpinned). Nothing here imports the library or wire.py."""
import math

import numpy as np

import oracle_py as O

F32 = np.float32

ZERO, GENERIC, PI = "zero", "generic", "pi"          # the arm; the pi arm adds "+y", "+z", "+tie" per sign rule applied


def matrix_to_vector(R):
    """step 3 on a 3x3 array of doubles -> (vector float64[3], label, s)"""
    R = [[float(R[i][j]) for j in range(3)] for i in range(3)]
    rx, ry, rz = R[2][1] - R[1][2], R[0][2] - R[2][0], R[1][0] - R[0][1]
    s = math.sqrt((rx * rx + ry * ry + rz * rz) * 0.25)
    c = (R[0][0] + R[1][1] + R[2][2] - 1) * 0.5
    c = 1.0 if c > 1.0 else (-1.0 if c < -1.0 else c)
    theta = math.acos(c)
    if s < 1e-5:
        if c > 0:
            return np.zeros(3), ZERO, s
        label = PI
        rx = math.sqrt(max((R[0][0] + 1) * 0.5, 0.0))
        ry = math.sqrt(max((R[1][1] + 1) * 0.5, 0.0))
        rz = math.sqrt(max((R[2][2] + 1) * 0.5, 0.0))
        if R[0][1] < 0:
            ry, label = -ry, label + "+y"
        if R[0][2] < 0:
            rz, label = -rz, label + "+z"
        if abs(rx) < abs(ry) and abs(rx) < abs(rz) and (R[1][2] > 0) != (ry * rz > 0):
            rz, label = -rz, label + "+tie"
        theta /= math.sqrt(rx * rx + ry * ry + rz * rz)
        return np.array([rx * theta, ry * theta, rz * theta]), label, s
    vth = 1 / (2 * s) * theta
    return np.array([rx * vth, ry * vth, rz * vth]), GENERIC, s


def _mul33_f32(a, b):
    o = np.zeros((3, 3), F32)
    for i in range(3):
        for j in range(3):
            acc = F32(0)
            for k in range(3):
                acc = F32(acc + F32(a[i, k] * b[k, j]))
            o[i, j] = acc
    return o


def _single_axis(angles):
    a = np.asarray(angles, F32)
    return (O.rodrigues([a[0], 0, 0]), O.rodrigues([0, a[1], 0]), O.rodrigues([0, 0, a[2]]))


def robot_angles(angles):
    """the statement: float32[3] pose angles -> (float32[3], label, s)"""
    fx, fy, fz = (m.astype(F32) for m in _single_axis(angles))
    v, label, s = matrix_to_vector(_mul33_f32(fz, _mul33_f32(fx, fy)).astype(np.float64))
    return v.astype(F32), label, s


def robot_angles64(angles):
    """its float64 twin: the same steps with nothing rounded to float32 -> (float64[3], label, rotation angle)"""
    dx, dy, dz = _single_axis(angles)
    v, label, _ = matrix_to_vector(dz @ (dx @ dy))
    return v, label, float(np.linalg.norm(v))
