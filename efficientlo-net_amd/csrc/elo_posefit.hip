// elo_posefit.hip -- point-to-plane fit of a relative pose on the two range images of a pair (include/elo.h, elo_pose_fit):
// residual, 6x6 normal equations, optional Gauss-Newton steps.  Outside the fused chain: appended after the l0 pose head, on request.
//
// Two kernels.  fit_eval_kernel: one thread per strip of FIT_STRIP frame-1 cells; the geometry of a term in double (the residual is
// a difference of nearby points), every product rounded to fp32 once and added in fp32 in a fixed order -- thread, wave (DPP),
// workgroup (LDS) -- into ONE partial row per workgroup.  fit_solve_kernel: one workgroup per image adds the partial rows in a fixed
// order in double; one thread solves and updates the pose, or (report form) writes info / grad / stats.  The sums cross from one kernel
// to the other at the launch boundary: an in-launch combine by the last workgroup to arrive would pay an agent-scope release and
// acquire -- about what the boundary costs on this part -- to save it.
#include "elo_project_device.h"

namespace elo {
namespace {

constexpr int FIT_STRIP = 2;                        // cells per thread: 64x1800 is 225 workgroups, one per CU, two dependent gather chains each
constexpr int FIT_TILE = ELO_BLOCK * FIT_STRIP;     // cells per workgroup: consecutive, thread t takes t, t + 256, ...
constexpr int FIT_WAVES = ELO_BLOCK / ELO_WAVE;
constexpr int FIT_SUMS = 29;                        // 21 of A (upper triangle, row-major) | 6 of b | cost | sum w
constexpr int FIT_ROW = 32;                         // words of a partial row: FIT_SUMS floats, the count (unsigned), 2 unused
constexpr int FIT_SOLVE_BLOCK = 256;                // FIT_ROW columns x FIT_SOLVE_LANES partial rows in flight
constexpr int FIT_SOLVE_LANES = FIT_SOLVE_BLOCK / FIT_ROW;

// wave-wide fp32 sum in the fixed order of the DPP reduction (wave_sum_u32's steps); every lane returns lane 63's total
template <int CTRL>
__device__ __forceinline__ float dpp_fadd_step(float v)
{
    return __fadd_rn(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false)));
}

__device__ __forceinline__ float wave_sum_f32(float v)
{
    v = dpp_fadd_step<0xb1>(v);     // quad_perm:[1,0,3,2]
    v = dpp_fadd_step<0x4e>(v);     // quad_perm:[2,3,0,1]
    v = dpp_fadd_step<0x114>(v);    // row_shr:4
    v = dpp_fadd_step<0x118>(v);    // row_shr:8
    v = dpp_fadd_step<0x142>(v);    // row_bcast:15
    v = dpp_fadd_step<0x143>(v);    // row_bcast:31
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

// R(q), q normalised here, in double from the row's floats (a zero quaternion: the identity)
__device__ __forceinline__ void pose_double(const float *row, double (&R)[9], double (&t)[3], double (&q)[4])
{
    double q0 = row[0], q1 = row[1], q2 = row[2], q3 = row[3];
    const double n = sqrt(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3);
    if (n > 0.0 && n - n == 0.0) { q0 /= n; q1 /= n; q2 /= n; q3 /= n; } else { q0 = 1.0; q1 = q2 = q3 = 0.0; }
    q[0] = q0; q[1] = q1; q[2] = q2; q[3] = q3;
    R[0] = 1.0 - 2.0 * (q2 * q2 + q3 * q3); R[1] = 2.0 * (q1 * q2 - q0 * q3);       R[2] = 2.0 * (q1 * q3 + q0 * q2);
    R[3] = 2.0 * (q1 * q2 + q0 * q3);       R[4] = 1.0 - 2.0 * (q1 * q1 + q3 * q3); R[5] = 2.0 * (q2 * q3 - q0 * q1);
    R[6] = 2.0 * (q1 * q3 - q0 * q2);       R[7] = 2.0 * (q2 * q3 + q0 * q1);       R[8] = 1.0 - 2.0 * (q1 * q1 + q2 * q2);
    t[0] = row[4]; t[1] = row[5]; t[2] = row[6];
}

struct FitEval {
    int H, W;
    float az_res;
    const float *xyz1, *xyz2;       // (batch,H,W,3)
    double gate, huber, jump_rel;
    unsigned *parts;                // (batch, gridDim.x, FIT_ROW)
};

// the term of frame-1 cell i of image b, added to acc / count; x2: the image's frame-2 cells
template <class Rows>
__device__ __forceinline__ void fit_term(const FitEval &a, const Rows &rows, const float *x1, const float *x2, const double (&R)[9],
                                         const double (&t)[3], float (&acc)[FIT_SUMS], unsigned &count)
{
    const float ax = x1[0], ay = x1[1], az = x1[2];
    if (ax == 0.0f && ay == 0.0f && az == 0.0f) return;
    const double p[3] = {R[0] * ax + R[1] * ay + R[2] * az + t[0], R[3] * ax + R[4] * ay + R[5] * az + t[1],
                         R[6] * ax + R[7] * ay + R[8] * az + t[2]};
    // the cell of p: the projections' own float32 rule on p rounded to float32 (bin_point_by, elo_features.hip)
    const float x = (float)p[0], y = (float)p[1], z = (float)p[2];
    const float rf = sqrtf(x * x + y * y + z * z);
    if (!(rf > 0.0f) || rf - rf != 0.0f) return;                        // the origin has no direction; a non-finite pose has no cell
    const int m = rows.cell(atan2f(y, x), z, rf, a.H, a.W, a.az_res);   // clipped to the image by the rule
    const int h = m / a.W, w = m - h * a.W;
    if (h == 0 || h == a.H - 1) return;                                 // no normal in the edge rows
    const int wl = w == 0 ? a.W - 1 : w - 1, wr = w == a.W - 1 ? 0 : w + 1;     // the seam
    const float *c = x2 + (long)m * 3, *l = x2 + ((long)h * a.W + wl) * 3, *r = x2 + ((long)h * a.W + wr) * 3;
    const float *u = x2 + (long)(m - a.W) * 3, *d = x2 + (long)(m + a.W) * 3;
    const double P2[3] = {c[0], c[1], c[2]}, L[3] = {l[0], l[1], l[2]}, Rt[3] = {r[0], r[1], r[2]};
    const double U[3] = {u[0], u[1], u[2]}, D[3] = {d[0], d[1], d[2]};
    auto empty = [](const double (&v)[3]) { return v[0] == 0.0 && v[1] == 0.0 && v[2] == 0.0; };
    if (empty(P2) || empty(L) || empty(Rt) || empty(U) || empty(D)) return;
    auto range = [](const double (&v)[3]) { return sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); };
    const double r2 = range(P2), jump = a.jump_rel * r2;
    if (fabs(range(L) - r2) > jump || fabs(range(Rt) - r2) > jump || fabs(range(U) - r2) > jump || fabs(range(D) - r2) > jump) return;
    const double e[3] = {Rt[0] - L[0], Rt[1] - L[1], Rt[2] - L[2]}, f[3] = {D[0] - U[0], D[1] - U[1], D[2] - U[2]};
    double n[3] = {e[1] * f[2] - e[2] * f[1], e[2] * f[0] - e[0] * f[2], e[0] * f[1] - e[1] * f[0]};
    const double len = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    if (!(len > 0.0) || len - len != 0.0) return;
    const double sgn = (n[0] * P2[0] + n[1] * P2[1] + n[2] * P2[2]) > 0.0 ? -1.0 / len : 1.0 / len;     // towards the sensor
    n[0] *= sgn; n[1] *= sgn; n[2] *= sgn;
    const double dv[3] = {p[0] - P2[0], p[1] - P2[1], p[2] - P2[2]};
    if (!(sqrt(dv[0] * dv[0] + dv[1] * dv[1] + dv[2] * dv[2]) <= a.gate)) return;
    const double res = n[0] * dv[0] + n[1] * dv[1] + n[2] * dv[2];
    const double J[6] = {p[1] * n[2] - p[2] * n[1], p[2] * n[0] - p[0] * n[2], p[0] * n[1] - p[1] * n[0], n[0], n[1], n[2]};
    const double ar = fabs(res), wt = ar <= a.huber ? 1.0 : a.huber / ar;
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

template <class Rows>
__device__ __forceinline__ void fit_eval_block(const FitEval &a, const float *pose, const Rows &rows, float (*part)[FIT_ROW])
{
    const int b = blockIdx.y;
    const long cells = (long)a.H * a.W;
    double R[9], t[3], q[4];
    pose_double(pose + b * 7, R, t, q);
    const float *x1 = a.xyz1 + (long)b * cells * 3, *x2 = a.xyz2 + (long)b * cells * 3;
    float acc[FIT_SUMS];
    for (int k = 0; k < FIT_SUMS; ++k) acc[k] = 0.0f;
    unsigned count = 0;
    const long first = (long)blockIdx.x * FIT_TILE + threadIdx.x;
    for (int s = 0; s < FIT_STRIP; ++s) {
        const long i = first + (long)s * ELO_BLOCK;
        if (i < cells) fit_term(a, rows, x1 + i * 3, x2, R, t, acc, count);
    }
    // (every lane of every wave arrives here: the DPP steps read all 64 lanes)
    const int wave = threadIdx.x / ELO_WAVE, lane = threadIdx.x % ELO_WAVE;
    for (int k = 0; k < FIT_SUMS; ++k) {
        const float s = wave_sum_f32(acc[k]);
        if (lane == 0) part[wave][k] = s;
    }
    const unsigned cs = wave_sum_u32(count);
    if (lane == 0) part[wave][FIT_SUMS] = __uint_as_float(cs);
    __syncthreads();
    unsigned *row = a.parts + ((long)b * gridDim.x + blockIdx.x) * FIT_ROW;
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

__global__ __launch_bounds__(ELO_BLOCK) void fit_eval_kernel(const FitEval a, const float *pose, const float vert_res, const float vert_off)
{
    __shared__ float part[FIT_WAVES][FIT_ROW];
    fit_eval_block(a, pose, RowsByFormula{vert_res, vert_off}, part);
}

__global__ __launch_bounds__(ELO_BLOCK) void fit_eval_beams_kernel(const FitEval a, const float *pose, const float *beam_elev, const int half)
{
    __shared__ float part[FIT_WAVES][FIT_ROW];
    __shared__ float mid[ELO_MAX_BEAMS];
    stage_beam_midpoints(mid, beam_elev, a.H, half);
    __syncthreads();
    fit_eval_block(a, pose, RowsByBeams{mid, half}, part);
}

struct FitSolve {
    int parts;                      // partial rows per image
    const unsigned *rows;           // (batch, parts, FIT_ROW)
    unsigned *status;               // (batch): the flags so far
    const float *pose_in;           // (batch,7): what a flagged image gets back
    const float *pose;              // (batch,7): the pose the evaluation ran at
    float *pose_out;                // (batch,7)
    float *info, *grad, *stats;     // report form only
    int min_count;
    double damping;
    int first;                      // 1: no solve ran before this launch (the status words are not read)
    int report;                     // 1: write info / grad / stats of this evaluation, no step
};

// 6x6 Cholesky solve of M d = -g in double; false where a pivot is not positive or d is not finite
__device__ bool solve6(double (&M)[6][6], const double (&g)[6], double (&d)[6])
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

__global__ __launch_bounds__(FIT_SOLVE_BLOCK) void fit_solve_kernel(const FitSolve a)
{
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
    const float *in = a.pose_in + b * 7, *cur = a.pose + b * 7;
    float *out = a.pose_out + b * 7;
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
    double nq[4], nt[3];
    if (ok) {
        double R[9], t[3], q[4];
        pose_double(cur, R, t, q);
        const double th2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2], th = sqrt(th2);
        // dq = (cos(th / 2), sin(th / 2) omega / th); the series where th is tiny
        const double c = cos(0.5 * th), sc = th > 1e-8 ? sin(0.5 * th) / th : 0.5 - th2 / 48.0;
        const double e0 = c, e1 = sc * d[0], e2 = sc * d[1], e3 = sc * d[2];
        nq[0] = e0 * q[0] - e1 * q[1] - e2 * q[2] - e3 * q[3];
        nq[1] = e0 * q[1] + e1 * q[0] + e2 * q[3] - e3 * q[2];
        nq[2] = e0 * q[2] - e1 * q[3] + e2 * q[0] + e3 * q[1];
        nq[3] = e0 * q[3] + e1 * q[2] - e2 * q[1] + e3 * q[0];
        const double nn = sqrt(nq[0] * nq[0] + nq[1] * nq[1] + nq[2] * nq[2] + nq[3] * nq[3]);
        // R(dq) t + v, by the quaternion sandwich t + 2 e0 (e x t) + 2 e x (e x t)
        const double cx = e2 * t[2] - e3 * t[1], cy = e3 * t[0] - e1 * t[2], cz = e1 * t[1] - e2 * t[0];
        const double dx = e2 * cz - e3 * cy, dy = e3 * cx - e1 * cz, dz = e1 * cy - e2 * cx;
        nt[0] = t[0] + 2.0 * e0 * cx + 2.0 * dx + d[3];
        nt[1] = t[1] + 2.0 * e0 * cy + 2.0 * dy + d[4];
        nt[2] = t[2] + 2.0 * e0 * cz + 2.0 * dz + d[5];
        if (!(nn > 0.0) || nn - nn != 0.0) { status |= ELO_FIT_SINGULAR; ok = false; }
        else
            for (int i = 0; i < 4; ++i) nq[i] /= nn;
        for (int i = 0; ok && i < 3; ++i)
            if ((float)nt[i] - (float)nt[i] != 0.0f) { status |= ELO_FIT_SINGULAR; ok = false; }
    }
    if (ok) {
        for (int i = 0; i < 4; ++i) out[i] = (float)nq[i];
        for (int i = 0; i < 3; ++i) out[4 + i] = (float)nt[i];
    } else {
        for (int i = 0; i < 7; ++i) out[i] = in[i];
    }
    a.status[b] = status;
}

#define ELO_REQUIRE(cond, who, what) \
    do { if (!(cond)) return fail(ELO_ERR_ARG, "%s: %s", who, what); } while (0)

bool fit_sizes_ok(int batch, int H, int W)
{
    return batch >= 0 && H >= 3 && W >= 1 && (long)H * W <= (1l << 31) - 1 && (long)batch * H * W <= (1l << 31) - 1 && batch <= 65535;
}

}  // namespace
}  // namespace elo

using namespace elo;

extern "C" int elo_pose_fit_parts(int H, int W)
{
    if (!fit_sizes_ok(1, H, W)) return -1;
    return (int)(((long)H * W + FIT_TILE - 1) / FIT_TILE);
}

// [partial rows (batch, parts, FIT_ROW) | status (batch)]
extern "C" long elo_pose_fit_scratch_words(int batch, int H, int W)
{
    if (!fit_sizes_ok(batch, H, W)) return -1;
    return (long)batch * elo_pose_fit_parts(H, W) * FIT_ROW + batch;
}

extern "C" int elo_pose_fit(const elo_pose_fit_args *a, elo_stream_t stream)
{
    const char *who = "elo_pose_fit";
    ELO_REQUIRE(a, who, "null argument block");
    ELO_REQUIRE(a->H >= 3, who, "a normal needs three rows: H >= 3");
    ELO_REQUIRE(fit_sizes_ok(a->batch, a->H, a->W), who, "bad sizes");
    ELO_REQUIRE(a->iters >= 0, who, "negative iters");
    ELO_REQUIRE(a->gate > 0.0f && a->gate - a->gate == 0.0f, who, "gate must be positive and finite");
    ELO_REQUIRE(a->huber > 0.0f && a->huber - a->huber == 0.0f, who, "huber must be positive and finite");
    ELO_REQUIRE(a->jump_rel >= 0.0f && a->damping >= 0.0f && a->damping - a->damping == 0.0f, who, "jump_rel / damping must be >= 0");
    ELO_REQUIRE(!a->beam_elev || a->H <= ELO_MAX_BEAMS, who, "more beams than ELO_MAX_BEAMS");
    ELO_REQUIRE(a->az_res > 0.0f && (a->beam_elev || a->vert_res > 0.0f), who, "bad projection constants");
    ELO_REQUIRE(a->xyz1 && a->xyz2 && a->pose_in, who, "null image or pose");
    ELO_REQUIRE(a->pose_out && a->info && a->grad && a->stats && a->scratch, who, "null output or scratch pointer");
    ELO_REQUIRE(a->pose_out != a->pose_in, who, "pose_out aliases pose_in");
    if (a->batch == 0) return ELO_OK;
    hipStream_t s = (hipStream_t)stream;
    const int parts = elo_pose_fit_parts(a->H, a->W);
    const FitEval ev = {a->H, a->W, a->az_res, a->xyz1, a->xyz2, (double)a->gate, (double)a->huber, (double)a->jump_rel, a->scratch};
    FitSolve so = {parts, a->scratch, a->scratch + (long)a->batch * parts * FIT_ROW, a->pose_in, a->pose_in, a->pose_out,
                   a->info, a->grad, a->stats, a->min_count, (double)a->damping, 1, 0};
    const int half = a->beam_elev ? beam_search_half(a->H) : 0;
    const dim3 grid((unsigned)parts, (unsigned)a->batch);
    for (int it = 0; it <= a->iters; ++it) {
        const float *pose = it == 0 ? a->pose_in : a->pose_out;
        if (a->beam_elev)
            hipLaunchKernelGGL(fit_eval_beams_kernel, grid, dim3(ELO_BLOCK), 0, s, ev, pose, a->beam_elev, half);
        else
            hipLaunchKernelGGL(fit_eval_kernel, grid, dim3(ELO_BLOCK), 0, s, ev, pose, a->vert_res, a->vert_off);
        so.pose = pose;
        so.first = it == 0;
        so.report = it == a->iters;
        hipLaunchKernelGGL(fit_solve_kernel, dim3((unsigned)a->batch), dim3(FIT_SOLVE_BLOCK), 0, s, so);
    }
    return check_launch(who);
}
