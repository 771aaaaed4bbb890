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
#include "elo_fit_device.h"

namespace elo {
namespace {

constexpr int FIT_STRIP = 2;                        // cells per thread: 64x1800 is 225 workgroups, one per CU, two dependent gather chains each
constexpr int FIT_TILE = ELO_BLOCK * FIT_STRIP;     // cells per workgroup: consecutive, thread t takes t, t + 256, ...

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
    if (cell_empty(ax, ay, az)) return;
    double p[3];
    pose_carry(R, t, ax, ay, az, p);
    // the cell of p: the projections' own float32 rule on p rounded to float32 (bin_point_by, elo_features.hip)
    const float x = (float)p[0], y = (float)p[1], z = (float)p[2];
    const float rf = sqrtf(x * x + y * y + z * z);
    if (!(rf > 0.0f) || rf - rf != 0.0f) return;                        // the origin has no direction; a non-finite pose has no cell
    const int m = rows.cell(atan2f(y, x), z, rf, a.H, a.W, a.az_res);   // clipped to the image by the rule
    const int h = m / a.W;
    double P2[3], n[3];
    if (!fit_normal(x2, h, m - h * a.W, a.H, a.W, a.jump_rel, P2, n)) return;
    const double dv[3] = {p[0] - P2[0], p[1] - P2[1], p[2] - P2[2]};
    if (!(sqrt(dv[0] * dv[0] + dv[1] * dv[1] + dv[2] * dv[2]) <= a.gate)) return;
    const double res = n[0] * dv[0] + n[1] * dv[1] + n[2] * dv[2];
    const double J[6] = {p[1] * n[2] - p[2] * n[1], p[2] * n[0] - p[0] * n[2], p[0] * n[1] - p[1] * n[0], n[0], n[1], n[2]};
    fit_accumulate(J, res, a.huber, acc, count);
}

template <class Rows>
__device__ __forceinline__ void fit_eval_block(const FitEval &a, const float *pose, const Rows &rows, float (*part)[FIT_ROW])
{
    const int b = blockIdx.y;
    const long cells = (long)a.H * a.W;
    double R[9], t[3], q[4];
    pose_row_or_identity(pose + b * 7, q, t);
    pose_rotation(q[0], q[1], q[2], q[3], R);
    const float *x1 = a.xyz1 + (long)b * cells * 3, *x2 = a.xyz2 + (long)b * cells * 3;
    float acc[FIT_SUMS];
    for (int k = 0; k < FIT_SUMS; ++k) acc[k] = 0.0f;
    unsigned count = 0;
    const long first = (long)blockIdx.x * FIT_TILE + threadIdx.x;
    for (int s = 0; s < FIT_STRIP; ++s) {
        const long i = first + (long)s * ELO_BLOCK;
        if (i < cells) fit_term(a, rows, x1 + i * 3, x2, R, t, acc, count);
    }
    fit_store_row(acc, count, part, a.parts + ((long)b * gridDim.x + blockIdx.x) * FIT_ROW);
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

}  // namespace
}  // namespace elo

using namespace elo;

extern "C" int elo_pose_fit_parts(int H, int W) { return fit_parts(H, W, FIT_TILE); }
extern "C" long elo_pose_fit_scratch_words(int batch, int H, int W) { return fit_scratch_words(batch, H, W, FIT_TILE); }

extern "C" int elo_pose_fit(const elo_pose_fit_args *a, elo_stream_t stream)
{
    const char *who = "elo_pose_fit";
    ELO_REQUIRE(a, who, "null argument block");
    ELO_REQUIRE(a->H >= 3, who, "a normal needs three rows: H >= 3");
    ELO_REQUIRE(fit_sizes_ok(a->batch, a->H, a->W), who, "bad sizes");
    ELO_REQUIRE(a->iters >= 0, who, "negative iters");
    ELO_REQUIRE(positive_finite(a->gate), who, "gate must be positive and finite");
    ELO_REQUIRE(positive_finite(a->huber), who, "huber must be positive and finite");
    ELO_REQUIRE(a->jump_rel >= 0.0f && a->damping >= 0.0f && a->damping - a->damping == 0.0f, who, "jump_rel / damping must be >= 0");
    ELO_REQUIRE(!a->beam_elev || a->H <= ELO_MAX_BEAMS, who, "more beams than ELO_MAX_BEAMS");
    ELO_REQUIRE(a->az_res > 0.0f && (a->beam_elev || a->vert_res > 0.0f), who, "bad projection constants");
    ELO_REQUIRE(a->xyz1 && a->xyz2 && a->pose_in, who, "null image or pose");
    ELO_REQUIRE(a->pose_out && a->info && a->grad && a->stats && a->scratch, who, "null output or scratch pointer");
    ELO_REQUIRE(a->pose_out != a->pose_in, who, "pose_out aliases pose_in");
    if (a->batch == 0) return ELO_OK;
    hipStream_t s = (hipStream_t)stream;
    const int parts = fit_parts(a->H, a->W, FIT_TILE);
    const FitEval ev = {a->H, a->W, a->az_res, a->xyz1, a->xyz2, (double)a->gate, (double)a->huber, (double)a->jump_rel, a->scratch};
    const int half = a->beam_elev ? beam_search_half(a->H) : 0;
    const dim3 grid((unsigned)parts, (unsigned)a->batch);
    return fit_run<FitPoseRel>(a, parts, s, who, [&](const float *pose) {
        if (a->beam_elev)
            hipLaunchKernelGGL(fit_eval_beams_kernel, grid, dim3(ELO_BLOCK), 0, s, ev, pose, a->beam_elev, half);
        else
            hipLaunchKernelGGL(fit_eval_kernel, grid, dim3(ELO_BLOCK), 0, s, ev, pose, a->vert_res, a->vert_off);
    });
}
