// elo_pose_device.h -- what the scan-level kernels share about a pose row (q0 q1 q2 q3 tx ty tz) and the points it carries: R(q), the
// row's loader, p' = R p + t and the two halves of a cell's validity rule.  The
// render (elo_model.hip), the tracker's state (elo_model_state.hip), the map (elo_map.hip), both fits (elo_fit_device.h) and the
// descriptor (elo_place.hip) state these rules through here, so kernels that must agree bit for bit run the same expressions.
#pragma once
#include "elo_common.h"

namespace elo {
namespace {

// R(q) of a normalised quaternion
__device__ __forceinline__ void pose_rotation(double q0, double q1, double q2, double q3, double (&R)[9])
{
    R[0] = 1.0 - 2.0 * (q2 * q2 + q3 * q3); R[1] = 2.0 * (q1 * q2 - q0 * q3);       R[2] = 2.0 * (q1 * q3 + q0 * q2);
    R[3] = 2.0 * (q1 * q2 + q0 * q3);       R[4] = 1.0 - 2.0 * (q1 * q1 + q3 * q3); R[5] = 2.0 * (q2 * q3 - q0 * q1);
    R[6] = 2.0 * (q1 * q3 - q0 * q2);       R[7] = 2.0 * (q2 * q3 + q0 * q1);       R[8] = 1.0 - 2.0 * (q1 * q1 + q2 * q2);
}

// the quaternion of a float or double row, normalised in double; false (q not written): it has no direction -- a zero or
// non-finite norm
template <class T>
__device__ __forceinline__ bool pose_quaternion(const T *row, double (&q)[4])
{
    const double q0 = row[0], q1 = row[1], q2 = row[2], q3 = row[3];
    const double n = sqrt(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3);
    if (!(n > 0.0) || n - n != 0.0) return false;
    q[0] = q0 / n; q[1] = q1 / n; q[2] = q2 / n; q[3] = q3 / n;
    return true;
}

// the row as (R(q), t): what a kernel that carries points loads; false: nothing written, the whole image is skipped
template <class T>
__device__ __forceinline__ bool pose_load(const T *row, double (&R)[9], double (&t)[3])
{
    double q[4];
    if (!pose_quaternion(row, q)) return false;
    pose_rotation(q[0], q[1], q[2], q[3], R);
    t[0] = row[4]; t[1] = row[5]; t[2] = row[6];
    return true;
}

// the row as (q, t), the identity where the quaternion has no direction: elo_pose_fit's rule for the row it is handed
template <class T>
__device__ __forceinline__ void pose_row_or_identity(const T *row, double (&q)[4], double (&t)[3])
{
    if (!pose_quaternion(row, q)) { q[0] = 1.0; q[1] = q[2] = q[3] = 0.0; }
    t[0] = row[4]; t[1] = row[5]; t[2] = row[6];
}

// p' = R p + t in double ...
__device__ __forceinline__ void pose_carry(const double (&R)[9], const double (&t)[3], double x, double y, double z, double (&p)[3])
{
    p[0] = R[0] * x + R[1] * y + R[2] * z + t[0];
    p[1] = R[3] * x + R[4] * y + R[5] * z + t[1];
    p[2] = R[6] * x + R[7] * y + R[8] * z + t[2];
}

// ... and every component rounded to float32 once
__device__ __forceinline__ void pose_carry_f32(const double (&R)[9], const double (&t)[3], float ax, float ay, float az, float &x, float &y,
                                               float &z)
{
    double p[3];
    pose_carry(R, t, ax, ay, az, p);
    x = (float)p[0]; y = (float)p[1]; z = (float)p[2];
}

// the validity rule of a cell, in its two halves: a cell that is exactly (0,0,0) holds no point, and a point with a non-finite
// component is rejected (the render and the map look at the carried, rounded p'; the descriptor at the cell as it stands)
template <class T>
__device__ __forceinline__ bool cell_empty(T x, T y, T z) { return x == T(0) && y == T(0) && z == T(0); }
__device__ __forceinline__ bool point_finite(float x, float y, float z) { return !(x - x != 0.0f || y - y != 0.0f || z - z != 0.0f); }

}  // namespace
}  // namespace elo
