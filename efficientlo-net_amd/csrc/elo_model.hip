// elo_model.hip -- the LOCAL MODEL of a frame-to-model pose fit (include/elo.h, elo_model_render): K range images, each carried by
// its own pose into one frame, rendered into ONE range image by nearest range.  Outside the fused chain, like the pose fit it feeds.
//
// Three kernels.  model_clear_kernel: one 64-bit key per target cell <- all ones.  model_splat_kernel: a streaming pass over the 12
// bytes of every source cell -- a workgroup works inside one (b, k), so R(q) is formed once per thread; a thread takes MODEL_STRIP
// consecutive cells by 16-byte loads, carries each point in double, rounds it to float32 once, takes its cell by the projections'
// float32 rule and sends ONE 64-bit integer atomicMin of (range bits << 32 | source index) -- none where a plain load of the key
// already beats the candidate (keys only fall, so a stale read costs an atomic, never a winner).  model_resolve_kernel: one thread
// per target cell recomputes the winner's point from its index by the very same instructions (splat stores no points) and writes
// both outputs in full.  No floating-point atomic: the minimum of a set of integers does not depend on the order of arrival.
#include "elo_project_device.h"
#include "elo_pose_device.h"

namespace elo {
namespace {

constexpr int MODEL_STRIP = 4;                          // cells per thread: 48 bytes, three 16-byte loads
constexpr int MODEL_TILE = ELO_BLOCK * MODEL_STRIP;     // cells per workgroup: consecutive, thread t takes 4 t .. 4 t + 3
constexpr int MODEL_CLEAR_BLOCKS = 1024;                // the clear walks its words with a grid stride beyond this
constexpr unsigned long long MODEL_EMPTY = ~0ull;

struct ModelRender {
    int K, H, W;
    float az_res;
    const float *src;               // (batch,K,H,W,3)
    const float *pose;              // (batch,K,7)
    unsigned long long *keys;       // (batch,H,W)
    unsigned tiles;                 // workgroups per source image
    int vec;                        // 1: H*W is a multiple of 4 and src is 16-byte aligned -- a strip is three aligned float4
};

// p' = R p + t in double, every component rounded to float32 once, and its float32 range; false: the point is dropped (an empty
// cell, a non-finite or all-zero p', a range that is not positive and finite).  Splat and resolve both come through here.
__device__ __forceinline__ bool model_carry(const double (&R)[9], const double (&t)[3], float ax, float ay, float az, float &x, float &y,
                                            float &z, float &rf)
{
    if (cell_empty(ax, ay, az)) return false;
    pose_carry_f32(R, t, ax, ay, az, x, y, z);
    if (x - x != 0.0f || y - y != 0.0f || z - z != 0.0f) return false;      // (!point_finite, spelled out: through the call the
                                                                            //  splat and resolve kernels allocate other registers)
    if (cell_empty(x, y, z)) return false;
    rf = sqrtf(x * x + y * y + z * z);                                  // the projections' own sequence (bin_point_by, elo_features.hip)
    return rf > 0.0f && rf - rf == 0.0f;
}

__global__ __launch_bounds__(ELO_BLOCK) void model_clear_kernel(unsigned *words, const unsigned n)
{
    fill_words(words, n, 0xffffffffu, blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
}

template <class Rows>
__device__ __forceinline__ void model_splat_block(const ModelRender &a, const Rows &rows)
{
    const unsigned bk = blockIdx.x / a.tiles, tile = blockIdx.x - bk * a.tiles;         // bk = b * K + k
    const unsigned b = bk / (unsigned)a.K, k = bk - b * (unsigned)a.K;
    const long cells = (long)a.H * a.W;
    const long i0 = ((long)tile * ELO_BLOCK + threadIdx.x) * MODEL_STRIP;
    if (i0 >= cells) return;
    double R[9], t[3];
    if (!pose_load(a.pose + (long)bk * 7, R, t)) return;                              // the whole source is skipped
    const float *s = a.src + ((long)bk * cells + i0) * 3;
    float v[3 * MODEL_STRIP];
    if (a.vec) {                                                                        // (cells % 4 == 0: the strip is inside the image)
        const float4 *s4 = reinterpret_cast<const float4 *>(s);
        const float4 u0 = s4[0], u1 = s4[1], u2 = s4[2];
        v[0] = u0.x; v[1] = u0.y; v[2] = u0.z; v[3] = u0.w; v[4] = u1.x; v[5] = u1.y; v[6] = u1.z; v[7] = u1.w;
        v[8] = u2.x; v[9] = u2.y; v[10] = u2.z; v[11] = u2.w;
    } else {
        for (int c = 0; c < MODEL_STRIP; ++c) {
            const bool in = i0 + c < cells;
            for (int j = 0; j < 3; ++j) v[c * 3 + j] = in ? s[c * 3 + j] : 0.0f;
        }
    }
    unsigned long long *keys = a.keys + (long)b * cells;
    const unsigned first = (unsigned)((long)k * cells + i0);                            // K * H * W < 2^31
    for (int c = 0; c < MODEL_STRIP; ++c) {
        float x, y, z, rf;
        if (!model_carry(R, t, v[c * 3], v[c * 3 + 1], v[c * 3 + 2], x, y, z, rf)) continue;
        const int m = rows.cell(atan2f(y, x), z, rf, a.H, a.W, a.az_res);               // clipped to the image by the rule
        const unsigned long long key = ((unsigned long long)__float_as_uint(rf) << 32) | (first + (unsigned)c);
        if (keys[m] > key) atomicMin(keys + m, key);
    }
}

__global__ __launch_bounds__(ELO_BLOCK) void model_splat_kernel(const ModelRender a, const float vert_res, const float vert_off)
{
    model_splat_block(a, RowsByFormula{vert_res, vert_off});
}

__global__ __launch_bounds__(ELO_BLOCK) void model_splat_beams_kernel(const ModelRender a, const float *beam_elev, const int half)
{
    __shared__ float mid[ELO_MAX_BEAMS];
    stage_beam_midpoints(mid, beam_elev, a.H, half);
    __syncthreads();
    model_splat_block(a, RowsByBeams{mid, half});
}

// one thread per target cell g = b * H * W + m
__global__ __launch_bounds__(ELO_BLOCK) void model_resolve_kernel(const ModelRender a, const unsigned total, float *out_xyz, int *out_src)
{
    const unsigned g = blockIdx.x * ELO_BLOCK + threadIdx.x;
    if (g >= total) return;
    const unsigned cells = (unsigned)a.H * (unsigned)a.W;
    const unsigned long long key = a.keys[g];
    float x = 0.0f, y = 0.0f, z = 0.0f, rf;
    int idx = -1;
    if (key != MODEL_EMPTY) {
        const unsigned i = (unsigned)key, b = g / cells, k = i / cells;
        const long bk = (long)b * a.K + k;
        const float *p = a.src + (bk * cells + (i - k * cells)) * 3;
        double R[9], t[3];
        if (pose_load(a.pose + bk * 7, R, t) && model_carry(R, t, p[0], p[1], p[2], x, y, z, rf)) idx = (int)i;
        else x = y = z = 0.0f;                                                          // (not reached: the key came from this point)
    }
    out_xyz[(long)g * 3 + 0] = x;
    out_xyz[(long)g * 3 + 1] = y;
    out_xyz[(long)g * 3 + 2] = z;
    out_src[g] = idx;
}

}  // namespace
}  // namespace elo

using namespace elo;

// one 64-bit key per target cell
extern "C" long elo_model_render_scratch_words(int batch, int H, int W)
{
    if (!image_sizes_ok(batch, H, W, 1)) return -1;
    return 2l * batch * H * W;
}

extern "C" int elo_model_render(const elo_model_render_args *a, elo_stream_t stream)
{
    const char *who = "elo_model_render";
    ELO_REQUIRE(a, who, "null argument block");
    ELO_REQUIRE(a->K >= 1 && a->K <= ELO_MODEL_MAX_SCANS, who, "K is 1 .. ELO_MODEL_MAX_SCANS");
    ELO_REQUIRE(image_sizes_ok(a->batch, a->H, a->W, 1), who, "bad sizes");
    ELO_REQUIRE((long)a->K * a->H * a->W <= (1l << 31) - 1, who, "K * H * W beyond 2^31");
    ELO_REQUIRE(!a->beam_elev || a->H <= ELO_MAX_BEAMS, who, "more beams than ELO_MAX_BEAMS");
    ELO_REQUIRE(a->az_res > 0.0f && (a->beam_elev || a->vert_res > 0.0f), who, "bad projection constants");
    ELO_REQUIRE(a->src && a->pose, who, "null image or pose");
    ELO_REQUIRE(a->out_xyz && a->out_src && a->scratch, who, "null output or scratch pointer");
    ELO_REQUIRE(aligned(a->scratch, 8), who, "scratch must be 8-byte aligned");
    const long cells = (long)a->H * a->W;
    ELO_REQUIRE(a->batch == 0 ? a->out_xyz != a->src                                     // (an empty batch: only the very same address)
                              : !ranges_meet(a->src, (size_t)a->batch * a->K * cells * 12, a->out_xyz, (size_t)a->batch * cells * 12),
                who, "out_xyz aliases src");
    if (a->batch == 0) return ELO_OK;
    hipStream_t s = (hipStream_t)stream;
    const unsigned total = (unsigned)(a->batch * cells);
    const unsigned tiles = (unsigned)((cells + MODEL_TILE - 1) / MODEL_TILE);
    const ModelRender r = {a->K, a->H, a->W, a->az_res, a->src, a->pose, reinterpret_cast<unsigned long long *>(a->scratch), tiles,
                           (cells % MODEL_STRIP == 0 && aligned(a->src, 16)) ? 1 : 0};
    const unsigned quads = (2u * total + 3u) / 4u, want = (quads + ELO_BLOCK - 1) / ELO_BLOCK;
    hipLaunchKernelGGL(model_clear_kernel, dim3(want < MODEL_CLEAR_BLOCKS ? want : MODEL_CLEAR_BLOCKS), dim3(ELO_BLOCK), 0, s,
                       a->scratch, 2u * total);
    const dim3 grid(tiles * (unsigned)a->K * (unsigned)a->batch);       // < 2^31: batch * H * W < 2^31, K <= 16, 1024 cells a tile
    if (a->beam_elev)
        hipLaunchKernelGGL(model_splat_beams_kernel, grid, dim3(ELO_BLOCK), 0, s, r, a->beam_elev, beam_search_half(a->H));
    else
        hipLaunchKernelGGL(model_splat_kernel, grid, dim3(ELO_BLOCK), 0, s, r, a->vert_res, a->vert_off);
    hipLaunchKernelGGL(model_resolve_kernel, dim3((total + ELO_BLOCK - 1) / ELO_BLOCK), dim3(ELO_BLOCK), 0, s, r, total, a->out_xyz,
                       a->out_src);
    return check_launch(who);
}
