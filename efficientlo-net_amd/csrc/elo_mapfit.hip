// elo_mapfit.hip -- SCAN-TO-MAP registration (include/elo.h, elo_map_fit): the point-to-plane fit of a scan's world pose against the
// centroids of the voxel map (elo_map.hip), the first reader of the hash table on a hot path.
//
// mapfit_eval_kernel: one thread per scan cell.  The normal comes first -- five neighbouring points of the scan, loads the lanes of
// a wave share -- so a cell without one never touches the table.  Then the 27 candidate voxels of the carried point, one x-plane
// of nine at a time: nine keys and nine home slots, the nine first-probe key loads issued together, the rare later probes
// resolved, then the 32-byte acc rows of the HITS only, two 16-byte loads each, again issued together; centroids and distances in
// ascending key order, so a strict `<` leaves ties with the smaller key.  A candidate whose voxel box lies further than the gate
// from the point (plus a margin for the roundings, PRUNE_*) is not looked up at all: with gate = voxel that is about half of the
// 27, with a gate of a quarter voxel all but ~4.  The table is only ever read here, by plain loads.
// Forms.  Built and measured: this one -- nine candidates at a time, unrolled, three rounds of (<= 9 key loads, <= 9 row pairs) per
// cell: 195 VGPRs, 26 SGPRs spilled to VGPR lanes, 32 bytes of scratch a lane, two waves a SIMD at __launch_bounds__(ELO_BLOCK).
// Not built: all 27 first probes in flight (keys, slots and first words of 27 candidates are 162 more registers across the
// resolve: beyond what this form leaves), and one candidate after the other (27 dependent round trips of two loads each: what a
// latency-bound gather must not do).  One cell per thread (MAPFIT_STRIP): a second cell would double the live double-precision
// state for loads that only queue behind the first cell's; 64x1800 is 450 workgroups.  A strip of 2 was not measured.
// The sums leave as elo_pose_fit's do (elo_fit_device.h): thread, wave, workgroup, one partial row; the solve launch is
// fit_solve_kernel<FitPoseWorld>: a double pose row, moved about the sensor's own position.
#include "elo_fit_device.h"
#include "elo_map_device.h"

namespace elo {
namespace {

constexpr int MAPFIT_STRIP = 1;                             // cells per thread
constexpr int MAPFIT_TILE = ELO_BLOCK * MAPFIT_STRIP;       // cells per workgroup: consecutive
// A candidate is skipped where the distance from p to its voxel's box exceeds gate + margin.  The box holds the centroid up to
// its float32 rounding, and the box is placed by the float32 rounding of p while the distance is taken from the double p: both
// are within 2^-23 of the coordinate's magnitude (which is below |p| + 2 voxels), and 2^-21 of it covers them with room.
constexpr double PRUNE_REL = 1e-6;                          // of the gate
constexpr double PRUNE_ULP = 4.76837158203125e-07;          // 2^-21 of (|coordinate| + 2 voxel)

struct MapFitEval {
    int H, W;
    double voxel, gate, huber, jump_rel;
    unsigned long long mask;            // C - 1
    unsigned long long min_points;
    const unsigned long long *keys, *acc;
    const float *xyz;                   // (batch,H,W,3)
    long long *match;                   // (batch,H,W) or NULL
    unsigned *parts;                    // (batch, gridDim.x, FIT_ROW)
};

// the lower bound of |p - c| along one axis for a centroid c in the box of index field + d - 2^20: 0 for the point's own voxel
__device__ __forceinline__ double mapfit_axis_gap(double p, unsigned long long field, int d, double voxel)
{
    const double lo = ((double)(long long)field - MAP_HALF) * voxel;        // the lower face of the point's voxel
    const double g = d < 0 ? p - lo : d > 0 ? (lo + voxel) - p : 0.0;
    return g > 0.0 ? g : 0.0;
}

// the term of scan cell (h,w) of one image, added to acc / count; returns the key of its target voxel, -1: no term
__device__ __forceinline__ long long mapfit_term(const MapFitEval &a, const float *x, const int h, const int w, const double (&R)[9],
                                                 const double (&t)[3], float (&acc)[FIT_SUMS], unsigned &count)
{
    double P[3], ns[3];
    if (!fit_normal(x, h, w, a.H, a.W, a.jump_rel, P, ns)) return -1;
    const double n[3] = {R[0] * ns[0] + R[1] * ns[1] + R[2] * ns[2], R[3] * ns[0] + R[4] * ns[1] + R[5] * ns[2],
                         R[6] * ns[0] + R[7] * ns[1] + R[8] * ns[2]};
    double p[3];
    pose_carry(R, t, P[0], P[1], P[2], p);
    // the voxel of p: the insert's rule on p rounded to float32
    const float xf = (float)p[0], yf = (float)p[1], zf = (float)p[2];
    if (!point_finite(xf, yf, zf)) return -1;
    unsigned long long f[3];
    unsigned g;
    if (!map_axis(xf, a.voxel, f[0], g) || !map_axis(yf, a.voxel, f[1], g) || !map_axis(zf, a.voxel, f[2], g)) return -1;
    // which of the 27 are candidates at all: indices in range, the box within reach
    double gap2[3][3];
    bool in[3][3];
    for (int ax = 0; ax < 3; ++ax)
        for (int dd = -1; dd <= 1; ++dd) {
            const double gp = mapfit_axis_gap(p[ax], f[ax], dd, a.voxel);
            gap2[ax][dd + 1] = gp * gp;
            in[ax][dd + 1] = !(dd < 0 && f[ax] == 0ull) && !(dd > 0 && f[ax] == 0x1fffffull);
        }
    const double amax = fmax(fabs(p[0]), fmax(fabs(p[1]), fabs(p[2])));
    const double reach = a.gate + PRUNE_REL * a.gate + PRUNE_ULP * (amax + 2.0 * a.voxel);
    const double reach2 = reach * reach;
    double best = __builtin_inf(), bc[3] = {0.0, 0.0, 0.0};
    unsigned long long bkey = MAP_EMPTY;
    for (int dx = 0; dx < 3; ++dx) {
        if (!in[0][dx] || gap2[0][dx] > reach2) continue;
        unsigned long long key[9], slot[9], k0[9];
        bool want[9];
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            const int dy = j / 3, dz = j % 3;
            want[j] = in[1][dy] && in[2][dz] && gap2[0][dx] + gap2[1][dy] + gap2[2][dz] <= reach2;
            key[j] = (f[0] + dx - 1ull) << 42 | (f[1] + dy - 1ull) << 21 | (f[2] + dz - 1ull);
            slot[j] = map_home(key[j]) & a.mask;
            k0[j] = MAP_EMPTY;
            if (want[j]) k0[j] = a.keys[slot[j]];
        }
        bool hit[9];
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            hit[j] = want[j] && k0[j] == key[j];
            if (want[j] && !hit[j] && k0[j] != MAP_EMPTY) {                        // another key sits in the home slot: walk on
                for (int q = 1; q < ELO_MAP_MAX_PROBE; ++q) {
                    const unsigned long long s = (slot[j] + (unsigned long long)q) & a.mask;
                    const unsigned long long cur = a.keys[s];
                    if (cur == key[j]) { hit[j] = true; slot[j] = s; break; }
                    if (cur == MAP_EMPTY) break;
                }
            }
        }
        ulonglong2 r0[9], r1[9];
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            r0[j] = make_ulonglong2(0ull, 0ull);
            r1[j] = make_ulonglong2(0ull, 0ull);
            if (hit[j]) {
                const ulonglong2 *row = reinterpret_cast<const ulonglong2 *>(a.acc + slot[j] * 4ull);
                r0[j] = row[0];
                r1[j] = row[1];
            }
        }
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            if (!hit[j] || r0[j].x < a.min_points) continue;
            const double cx = (double)map_centroid(key[j] >> 42 & 0x1fffffull, r0[j].y, r0[j].x, a.voxel);
            const double cy = (double)map_centroid(key[j] >> 21 & 0x1fffffull, r1[j].x, r0[j].x, a.voxel);
            const double cz = (double)map_centroid(key[j] & 0x1fffffull, r1[j].y, r0[j].x, a.voxel);
            const double ex = p[0] - cx, ey = p[1] - cy, ez = p[2] - cz;
            const double d2 = ex * ex + ey * ey + ez * ez;
            if (d2 < best) { best = d2; bkey = key[j]; bc[0] = cx; bc[1] = cy; bc[2] = cz; }      // (ascending keys: ties stay)
        }
    }
    if (!(sqrt(best) <= a.gate)) return -1;
    const double dv[3] = {p[0] - bc[0], p[1] - bc[1], p[2] - bc[2]};
    const double res = n[0] * dv[0] + n[1] * dv[1] + n[2] * dv[2];
    const double s[3] = {bc[0] - t[0], bc[1] - t[1], bc[2] - t[2]};       // the target as the sensor sees it
    const double J[6] = {s[1] * n[2] - s[2] * n[1], s[2] * n[0] - s[0] * n[2], s[0] * n[1] - s[1] * n[0], n[0], n[1], n[2]};
    fit_accumulate(J, res, a.huber, acc, count);
    return (long long)bkey;
}

__global__ __launch_bounds__(ELO_BLOCK) void mapfit_eval_kernel(const MapFitEval a, const double *pose)
{
    __shared__ float part[FIT_WAVES][FIT_ROW];
    const int b = blockIdx.y;
    const long cells = (long)a.H * a.W;
    double R[9], t[3];
    bool live = pose_load(pose + (long)b * 7, R, t);                    // (uniform over the workgroup)
    live = live && t[0] - t[0] == 0.0 && t[1] - t[1] == 0.0 && t[2] - t[2] == 0.0;
    const float *x = a.xyz + (long)b * cells * 3;
    float acc[FIT_SUMS];
    for (int k = 0; k < FIT_SUMS; ++k) acc[k] = 0.0f;
    unsigned count = 0;
    const long first = (long)blockIdx.x * MAPFIT_TILE + threadIdx.x;
    for (int s = 0; s < MAPFIT_STRIP; ++s) {
        const long i = first + (long)s * ELO_BLOCK;
        if (i >= cells) continue;
        long long key = -1;
        if (live) {
            const int h = (int)(i / a.W);
            key = mapfit_term(a, x, h, (int)(i - (long)h * a.W), R, t, acc, count);
        }
        if (a.match) a.match[(long)b * cells + i] = key;
    }
    fit_store_row(acc, count, part, a.parts + ((long)b * gridDim.x + blockIdx.x) * FIT_ROW);
}

}  // namespace
}  // namespace elo

using namespace elo;

extern "C" int elo_map_fit_parts(int H, int W) { return fit_parts(H, W, MAPFIT_TILE); }
extern "C" long elo_map_fit_scratch_words(int batch, int H, int W) { return fit_scratch_words(batch, H, W, MAPFIT_TILE); }

extern "C" int elo_map_fit(const elo_map_fit_args *a, elo_stream_t stream)
{
    const char *who = "elo_map_fit";
    ELO_REQUIRE(a, who, "null argument block");
    ELO_REQUIRE(a->H >= 3, who, "a normal needs three rows: H >= 3");
    ELO_REQUIRE(fit_sizes_ok(a->batch, a->H, a->W), who, "bad sizes");
    ELO_REQUIRE(map_table_ok(a->voxel, a->log2_capacity), who, "voxel is positive and finite, log2_capacity ELO_MAP_MIN_LOG2 .. ELO_MAP_MAX_LOG2");
    ELO_REQUIRE(a->iters >= 0, who, "negative iters");
    ELO_REQUIRE(a->gate > 0.0f && a->gate <= a->voxel, who, "gate must be positive and at most the voxel");
    ELO_REQUIRE(positive_finite(a->huber), who, "huber must be positive and finite");
    ELO_REQUIRE(a->jump_rel >= 0.0f && a->damping >= 0.0f && a->damping - a->damping == 0.0f, who, "jump_rel / damping must be >= 0");
    ELO_REQUIRE(a->min_points >= 1, who, "min_points is >= 1");
    ELO_REQUIRE(a->keys && a->acc && a->xyz && a->pose_in, who, "null table, image or pose");
    ELO_REQUIRE(a->pose_out && a->info && a->grad && a->stats && a->scratch, who, "null output or scratch pointer");
    ELO_REQUIRE(a->pose_out != a->pose_in, who, "pose_out aliases pose_in");
    ELO_REQUIRE(aligned(a->keys, 8) && aligned(a->acc, 8) && aligned(a->pose_in, 8) && aligned(a->pose_out, 8) && aligned(a->match, 8), who,
                "keys, acc, pose_in, pose_out and match must be 8-byte aligned");
    if (a->batch == 0) return ELO_OK;
    hipStream_t s = (hipStream_t)stream;
    const int parts = fit_parts(a->H, a->W, MAPFIT_TILE);
    const MapFitEval ev = {a->H, a->W, (double)a->voxel, (double)a->gate, (double)a->huber, (double)a->jump_rel,
                           (1ull << a->log2_capacity) - 1ull, (unsigned long long)a->min_points, a->keys, a->acc, a->xyz, a->match,
                           a->scratch};
    const dim3 grid((unsigned)parts, (unsigned)a->batch);
    return fit_run<FitPoseWorld>(a, parts, s, who, [&](const double *pose) {
        hipLaunchKernelGGL(mapfit_eval_kernel, grid, dim3(ELO_BLOCK), 0, s, ev, pose);
    });
}
