// elo_fit_device.h -- what the point-to-plane fits share (elo_pose_fit, elo_posefit.hip; elo_map_fit, elo_mapfit.hip): the normal of a
// range-image cell, the float32 sums of a term in their fixed order (thread, wave by DPP, workgroup through LDS, one partial row per
// workgroup), the solve launch -- the partial rows added in double, the 6x6 Cholesky, the update of the pose or the report -- and the
// host's loop over the two (fit_run) with the size of its scratch.  The two fits differ in how a term's point finds its target (an
// evaluation kernel each) and in the pose they move: a float32 row about the origin of frame 2 (FitPoseRel), or a double row about the
// sensor's own position (FitPoseWorld).  Pose rows, R(q) and the carried point: elo_pose_device.h.
#pragma once
#include "elo_pose_device.h"

namespace elo {
namespace {

constexpr int FIT_WAVES = ELO_BLOCK / ELO_WAVE;
constexpr int FIT_SUMS = 29;                        // 21 of A (upper triangle, row-major) | 6 of b | cost | sum w
constexpr int FIT_ROW = 32;                         // words of a partial row: FIT_SUMS floats, the count (unsigned), 2 unused
constexpr int FIT_SOLVE_BLOCK = 256;                // FIT_ROW columns x FIT_SOLVE_LANES partial rows in flight
constexpr int FIT_SOLVE_LANES = FIT_SOLVE_BLOCK / FIT_ROW;

// The normal of cell (h,w) of the (H,W,3) image x, whose point is P2, between its neighbours l / r (columns, wrapped at the seam)
// and u / d (rows): false in the edge rows, where the cell or a neighbour is empty, a neighbour's range jumps or the cross product
// has no length.  n: unit, towards the sensor.
__device__ __forceinline__ bool fit_normal(const float *x, const int h, const int w, const int H, const int W, const double jump_rel,
                                           double (&P2)[3], double (&n)[3])
{
    if (h == 0 || h == H - 1) return false;
    const int wl = w == 0 ? W - 1 : w - 1, wr = w == W - 1 ? 0 : w + 1;
    const int m = h * W + w;                                            // (H * W fits an int: fit_sizes_ok)
    const float *c = x + (long)m * 3, *l = x + ((long)h * W + wl) * 3, *r = x + ((long)h * W + wr) * 3;
    const float *u = x + (long)(m - W) * 3, *d = x + (long)(m + W) * 3;
    P2[0] = c[0]; P2[1] = c[1]; P2[2] = c[2];
    const double L[3] = {l[0], l[1], l[2]}, Rt[3] = {r[0], r[1], r[2]};
    const double U[3] = {u[0], u[1], u[2]}, D[3] = {d[0], d[1], d[2]};
    auto empty = [](const double (&v)[3]) { return cell_empty(v[0], v[1], v[2]); };
    if (empty(P2) || empty(L) || empty(Rt) || empty(U) || empty(D)) return false;
    auto range = [](const double (&v)[3]) { return sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); };
    const double r2 = range(P2), jump = jump_rel * r2;
    if (fabs(range(L) - r2) > jump || fabs(range(Rt) - r2) > jump || fabs(range(U) - r2) > jump || fabs(range(D) - r2) > jump) return false;
    const double e[3] = {Rt[0] - L[0], Rt[1] - L[1], Rt[2] - L[2]}, f[3] = {D[0] - U[0], D[1] - U[1], D[2] - U[2]};
    n[0] = e[1] * f[2] - e[2] * f[1]; n[1] = e[2] * f[0] - e[0] * f[2]; n[2] = e[0] * f[1] - e[1] * f[0];
    const double len = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    if (!(len > 0.0) || len - len != 0.0) return false;
    const double sgn = (n[0] * P2[0] + n[1] * P2[1] + n[2] * P2[2]) > 0.0 ? -1.0 / len : 1.0 / len;     // towards the sensor
    n[0] *= sgn; n[1] *= sgn; n[2] *= sgn;
    return true;
}

// one term (J, res) under the Huber weight: every product rounded to float32 once and added to the thread's sums
__device__ __forceinline__ void fit_accumulate(const double (&J)[6], const double res, const double huber, float (&acc)[FIT_SUMS],
                                               unsigned &count)
{
    const double ar = fabs(res), wt = ar <= huber ? 1.0 : huber / ar;
    int k = 0;
    for (int i = 0; i < 6; ++i) {
        const double wj = wt * J[i];
        for (int j = i; j < 6; ++j, ++k) acc[k] = __fadd_rn(acc[k], (float)(wj * J[j]));
    }
    for (int i = 0; i < 6; ++i) acc[21 + i] = __fadd_rn(acc[21 + i], (float)(wt * J[i] * res));
    acc[27] = __fadd_rn(acc[27], (float)(wt * res * res));
    acc[28] = __fadd_rn(acc[28], (float)wt);
    ++count;
}

// the threads' sums -> the workgroup's partial row: wave by DPP, the waves through LDS in order.  (Every lane of every wave arrives
// here: the DPP steps read all 64 lanes.)
__device__ __forceinline__ void fit_store_row(const float (&acc)[FIT_SUMS], const unsigned count, float (*part)[FIT_ROW], unsigned *row)
{
    const int wave = threadIdx.x / ELO_WAVE, lane = threadIdx.x % ELO_WAVE;
    for (int k = 0; k < FIT_SUMS; ++k) {
        const float s = wave_sum_f32(acc[k]);
        if (lane == 0) part[wave][k] = s;
    }
    const unsigned cs = wave_sum_u32(count);
    if (lane == 0) part[wave][FIT_SUMS] = __uint_as_float(cs);
    __syncthreads();
    if (threadIdx.x < FIT_SUMS) {
        float s = part[0][threadIdx.x];
        for (int w = 1; w < FIT_WAVES; ++w) s = __fadd_rn(s, part[w][threadIdx.x]);
        row[threadIdx.x] = __float_as_uint(s);
    } else if (threadIdx.x == FIT_SUMS) {
        unsigned s = 0;
        for (int w = 0; w < FIT_WAVES; ++w) s += __float_as_uint(part[w][FIT_SUMS]);
        row[FIT_SUMS] = s;
    } else if (threadIdx.x < FIT_ROW) {
        row[threadIdx.x] = 0u;
    }
}

// 6x6 Cholesky solve of M d = -g in double; false where a pivot is not positive or d is not finite
__device__ inline bool solve6(double (&M)[6][6], const double (&g)[6], double (&d)[6])
{
    for (int j = 0; j < 6; ++j) {
        double s = M[j][j];
        for (int k = 0; k < j; ++k) s -= M[j][k] * M[j][k];
        if (!(s > 0.0) || s - s != 0.0) return false;
        const double piv = sqrt(s);
        M[j][j] = piv;
        for (int i = j + 1; i < 6; ++i) {
            double v = M[i][j];
            for (int k = 0; k < j; ++k) v -= M[i][k] * M[j][k];
            M[i][j] = v / piv;
        }
    }
    double y[6];
    for (int i = 0; i < 6; ++i) {
        double v = -g[i];
        for (int k = 0; k < i; ++k) v -= M[i][k] * y[k];
        y[i] = v / M[i][i];
    }
    for (int i = 5; i >= 0; --i) {
        double v = y[i];
        for (int k = i + 1; k < 6; ++k) v -= M[k][i] * d[k];
        d[i] = v / M[i][i];
    }
    for (int i = 0; i < 6; ++i)
        if (d[i] - d[i] != 0.0) return false;
    return true;
}

// The pose a fit moves.  FitPoseRel: elo_pose_fit's float32 row, frame 1 -> frame 2, perturbed about the origin of frame 2:
// t <- R(dq) t + v.  FitPoseWorld: elo_map_fit's double row, scan -> world, perturbed about the sensor's position: t <- t + v.
struct FitPoseRel {
    typedef float scalar;
    static constexpr bool about_sensor = false;
    static __device__ __forceinline__ bool load(const float *row, double (&t)[3], double (&q)[4]) { return pose_row_or_identity(row, q, t), true; }
    static __device__ __forceinline__ bool finite(double v) { return (float)v - (float)v == 0.0f; }
};

struct FitPoseWorld {
    typedef double scalar;
    static constexpr bool about_sensor = true;
    static __device__ __forceinline__ bool load(const double *row, double (&t)[3], double (&q)[4])
    {
        if (!pose_quaternion(row, q)) return false;
        for (int i = 0; i < 3; ++i) t[i] = row[4 + i];
        return true;
    }
    static __device__ __forceinline__ bool finite(double v) { return v - v == 0.0; }
};

template <class Pose>
struct FitSolve {
    typedef typename Pose::scalar scalar;
    int parts;                      // partial rows per image
    const unsigned *rows;           // (batch, parts, FIT_ROW)
    unsigned *status;               // (batch): the flags so far
    const scalar *pose_in;          // (batch,7): what a flagged image gets back
    const scalar *pose;             // (batch,7): the pose the evaluation ran at
    scalar *pose_out;               // (batch,7)
    float *info, *grad, *stats;     // report form only
    int min_count;
    double damping;
    int first;                      // 1: no solve ran before this launch (the status words are not read)
    int report;                     // 1: write info / grad / stats of this evaluation, no step
};

template <class Pose>
__global__ __launch_bounds__(FIT_SOLVE_BLOCK) void fit_solve_kernel(const FitSolve<Pose> a)
{
    typedef typename Pose::scalar scalar;
    // The partial rows in a fixed order, in double: thread (k, j) adds rows k, k + LANES, k + 2 LANES, ... of column j (one row per load
    // instruction of a 32-thread group, FIT_SOLVE_LANES rows in flight -- one thread per column walking all the rows one after the other
    // was a chain of `parts` dependent cross-XCD reads, 35 us at 64x1800), then thread j adds the LANES subtotals in order.
    __shared__ double sub[FIT_SOLVE_LANES][FIT_ROW];
    __shared__ double sum[FIT_SUMS];
    __shared__ unsigned long long total;
    const int b = blockIdx.x;
    const unsigned *rows = a.rows + (long)b * a.parts * FIT_ROW;
    {
        const int j = threadIdx.x % FIT_ROW, k = threadIdx.x / FIT_ROW;
        double s = 0.0;                                 // (the count column: integers below 2^53, exact in a double)
        for (int g = k; g < a.parts; g += FIT_SOLVE_LANES) {
            const unsigned v = rows[(long)g * FIT_ROW + j];
            s += j == FIT_SUMS ? (double)v : (double)__uint_as_float(v);
        }
        sub[k][j] = s;
    }
    __syncthreads();
    if (threadIdx.x <= FIT_SUMS) {
        double s = sub[0][threadIdx.x];
        for (int k = 1; k < FIT_SOLVE_LANES; ++k) s += sub[k][threadIdx.x];
        if (threadIdx.x == FIT_SUMS) total = (unsigned long long)s;
        else sum[threadIdx.x] = s;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const scalar *in = a.pose_in + b * 7, *cur = a.pose + b * 7;
    scalar *out = a.pose_out + b * 7;
    unsigned status = a.first ? 0u : a.status[b];
    const long count = (long)total;
    if (a.report) {
        if (count < a.min_count) status |= ELO_FIT_FEW_FINAL;
        int k = 0;
        for (int i = 0; i < 6; ++i)
            for (int j = i; j < 6; ++j, ++k) a.info[b * 36 + i * 6 + j] = a.info[b * 36 + j * 6 + i] = (float)sum[k];
        for (int i = 0; i < 6; ++i) a.grad[b * 6 + i] = (float)sum[21 + i];
        float *st = a.stats + b * 4;
        st[0] = (float)count;
        st[1] = (float)sum[27];
        st[2] = sum[28] > 0.0 ? (float)sqrt(sum[27] / sum[28]) : 0.0f;
        st[3] = (float)status;
        if (a.first)                                    // iters = 0: no solve wrote pose_out
            for (int i = 0; i < 7; ++i) out[i] = in[i];
        a.status[b] = status;
        return;
    }
    bool ok = status == 0u;                             // flagged before: the row stays pose_in's
    double d[6];
    if (ok && count < a.min_count) { status |= ELO_FIT_FEW; ok = false; }
    if (ok) {
        double M[6][6], g[6];
        int k = 0;
        for (int i = 0; i < 6; ++i)
            for (int j = i; j < 6; ++j, ++k) M[i][j] = M[j][i] = sum[k];
        for (int i = 0; i < 6; ++i) { M[i][i] += a.damping * M[i][i]; g[i] = sum[21 + i]; }
        if (!solve6(M, g, d)) { status |= ELO_FIT_SINGULAR; ok = false; }
    }
    double nq[4], nt[3], t[3], q[4];
    if (ok && !Pose::load(cur, t, q)) { status |= ELO_FIT_SINGULAR; ok = false; }
    if (ok) {
        const double th2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2], th = sqrt(th2);
        // dq = (cos(th / 2), sin(th / 2) omega / th); the series where th is tiny
        const double c = cos(0.5 * th), sc = th > 1e-8 ? sin(0.5 * th) / th : 0.5 - th2 / 48.0;
        const double e0 = c, e1 = sc * d[0], e2 = sc * d[1], e3 = sc * d[2];
        nq[0] = e0 * q[0] - e1 * q[1] - e2 * q[2] - e3 * q[3];
        nq[1] = e0 * q[1] + e1 * q[0] + e2 * q[3] - e3 * q[2];
        nq[2] = e0 * q[2] - e1 * q[3] + e2 * q[0] + e3 * q[1];
        nq[3] = e0 * q[3] + e1 * q[2] - e2 * q[1] + e3 * q[0];
        const double nn = sqrt(nq[0] * nq[0] + nq[1] * nq[1] + nq[2] * nq[2] + nq[3] * nq[3]);
        if (Pose::about_sensor) {
            for (int i = 0; i < 3; ++i) nt[i] = t[i] + d[3 + i];
        } else {
            // R(dq) t + v, by the quaternion sandwich t + 2 e0 (e x t) + 2 e x (e x t)
            const double cx = e2 * t[2] - e3 * t[1], cy = e3 * t[0] - e1 * t[2], cz = e1 * t[1] - e2 * t[0];
            const double dx = e2 * cz - e3 * cy, dy = e3 * cx - e1 * cz, dz = e1 * cy - e2 * cx;
            nt[0] = t[0] + 2.0 * e0 * cx + 2.0 * dx + d[3];
            nt[1] = t[1] + 2.0 * e0 * cy + 2.0 * dy + d[4];
            nt[2] = t[2] + 2.0 * e0 * cz + 2.0 * dz + d[5];
        }
        if (!(nn > 0.0) || nn - nn != 0.0) { status |= ELO_FIT_SINGULAR; ok = false; }
        else
            for (int i = 0; i < 4; ++i) nq[i] /= nn;
        for (int i = 0; ok && i < 3; ++i)
            if (!Pose::finite(nt[i])) { status |= ELO_FIT_SINGULAR; ok = false; }
    }
    if (ok) {
        for (int i = 0; i < 4; ++i) out[i] = (scalar)nq[i];
        for (int i = 0; i < 3; ++i) out[4 + i] = (scalar)nt[i];
    } else {
        for (int i = 0; i < 7; ++i) out[i] = in[i];
    }
    a.status[b] = status;
}

// ---- host: what elo_pose_fit and elo_map_fit share around their evaluation launch
inline bool fit_sizes_ok(int batch, int H, int W) { return image_sizes_ok(batch, H, W, 3, 65535); }

// partial rows per image, one per workgroup of `tile` cells; -1: sizes no fit takes
inline int fit_parts(int H, int W, int tile) { return fit_sizes_ok(1, H, W) ? (int)(((long)H * W + tile - 1) / tile) : -1; }

// words of [partial rows (batch, parts, FIT_ROW) | status (batch)]
inline long fit_scratch_words(int batch, int H, int W, int tile)
{
    return fit_sizes_ok(batch, H, W) ? (long)batch * fit_parts(H, W, tile) * FIT_ROW + batch : -1;
}

// The launches of a fit on a checked, non-empty argument block (elo_pose_fit_args or elo_map_fit_args: the fields named here are
// in both): evaluate at pose_in, solve into pose_out, evaluate there, ... -- iters steps, then one evaluation more that only reports.
// eval(pose): launches the evaluation of all images at the (batch,7) rows `pose`, partial rows to a->scratch.
template <class Pose, class Args, class Eval>
int fit_run(const Args *a, const int parts, hipStream_t s, const char *who, Eval eval)
{
    FitSolve<Pose> so = {parts, a->scratch, a->scratch + (long)a->batch * parts * FIT_ROW, a->pose_in, a->pose_in, a->pose_out,
                         a->info, a->grad, a->stats, a->min_count, (double)a->damping, 1, 0};
    for (int it = 0; it <= a->iters; ++it) {
        so.pose = it == 0 ? a->pose_in : a->pose_out;
        eval(so.pose);
        so.first = it == 0;
        so.report = it == a->iters;
        hipLaunchKernelGGL(fit_solve_kernel<Pose>, dim3((unsigned)a->batch), dim3(FIT_SOLVE_BLOCK), 0, s, so);
    }
    return check_launch(who);
}

}  // namespace
}  // namespace elo
