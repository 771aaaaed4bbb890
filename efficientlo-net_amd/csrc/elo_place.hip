// elo_place.hip -- PLACE RECOGNITION (include/elo.h, elo_scan_descriptor / elo_descriptor_search): a scan's descriptor -- per azimuth
// sector and range ring the integer level of the highest point -- and the brute-force search of a database of descriptors over every
// entry and every column shift.  Integers wherever the rule allows it: the descriptor is a max of integers, the column products
// of the search are 32-bit integer sums, and the distance is a fixed sequence of IEEE double operations, so every result is a
// function of its inputs alone.
//
// place_descriptor_kernel: a workgroup owns ONE sector of one image -- a range image's column is the azimuth, so the sector's cells
// are a contiguous run of columns over all H rows -- and with it that sector's bins alone: `rings` words of LDS, integer atomicMax
// on them, `rings` plain stores.  The ring edges are copied to LDS first (a by-value array indexed by a loop variable would live
// in scratch).
// place_search_kernel: a workgroup takes one (query, entry) pair.  Both descriptors are staged in LDS as 32-bit words with an ODD
// row stride (lane s reads row (j + s) mod sectors: neighbouring lanes, neighbouring rows.  A 32-bit LDS read is served in two
// groups of 32 lanes with the bank (address / 4) mod 32, so with an odd stride the 32 rows of a group fall on 32 different banks --
// except in the group where the row index wraps, which may meet a bank twice), the two norm vectors are formed once, and lane s
// then walks ITS shift serially over j: the fixed ascending-j order of the rule for free.  Q[j][r] is one address for the whole
// wave (a broadcast), D's word is the lane's own.  The column products are formed where they are used instead of in a sectors x
// sectors matrix in LDS: the same multiply-adds, 12 KB instead of 26 KB of LDS at 60 x 20, and at 128 sectors the matrix alone is
// 64 KB: more than a launch may ask for without raising the kernel's dynamic-LDS limit by a function attribute, and two
// workgroups a CU at most.  The best shift by (dist, shift) is a shuffle reduction in the first wave.
// place_rank_kernel: a workgroup per query, k passes of an argmin by (dist, entry) over the entries that lie above the last
// winner: no sort, no ties left to chance.
#include "elo_pose_device.h"

namespace elo {
namespace {

constexpr int PLACE_WAVE = 64;
constexpr int PLACE_MAX_R = ELO_PLACE_MAX_RINGS, PLACE_MAX_S = ELO_PLACE_MAX_SECTORS;

struct PlaceDescriptor {
    int H, W, rings, sectors;
    double z_min, z_step, min_range2;
    double edge2[PLACE_MAX_R + 1];
    const float *xyz;
    unsigned short *desc;
};

__global__ __launch_bounds__(ELO_BLOCK) void place_descriptor_kernel(const PlaceDescriptor a)
{
    __shared__ double edge2[PLACE_MAX_R + 1];
    __shared__ unsigned bins[PLACE_MAX_R];
    const int s = (int)blockIdx.x, b = (int)blockIdx.y;
    if (threadIdx.x <= (unsigned)PLACE_MAX_R) edge2[threadIdx.x] = a.edge2[threadIdx.x];
    if (threadIdx.x < (unsigned)PLACE_MAX_R) bins[threadIdx.x] = 0u;
    __syncthreads();
    // the columns w with (w * sectors) / W == s: [ceil(s W / sectors), ceil((s + 1) W / sectors))
    const long S = a.sectors, W = a.W;
    const int w0 = (int)((s * W + S - 1) / S), w1 = (int)(((s + 1) * W + S - 1) / S);
    const int run = w1 - w0;                                                            // >= 1: W >= sectors
    const long cells = (long)a.H * run;
    const float *img = a.xyz + (long)b * a.H * W * 3;
    const double top = (double)(ELO_PLACE_LEVELS - 1);
    for (long i = threadIdx.x; i < cells; i += ELO_BLOCK) {
        const int h = (int)(i / run), w = w0 + (int)(i - (long)h * run);
        const float *p = img + ((long)h * W + w) * 3;
        const float x = p[0], y = p[1], z = p[2];
        if (cell_empty(x, y, z) || !point_finite(x, y, z)) continue;
        const double r2 = (double)x * (double)x + (double)y * (double)y;
        if (r2 < a.min_range2 || r2 >= edge2[a.rings]) continue;
        int ring = 0;
        for (int j = 1; j <= PLACE_MAX_R; ++j) ring += (j <= a.rings && edge2[j] <= r2) ? 1 : 0;
        double f = floor(((double)z - a.z_min) / a.z_step);
        f = f < 0.0 ? 0.0 : (f > top ? top : f);
        atomicMax(&bins[ring], (unsigned)(int)f + 1u);                                  // ring < rings: r2 < edge2[rings]
    }
    __syncthreads();
    if ((int)threadIdx.x < a.rings)
        a.desc[((long)b * a.sectors + s) * a.rings + threadIdx.x] = (unsigned short)bins[threadIdx.x];
}

struct PlaceSearch {
    int n, m, rings, sectors, k;
    const unsigned short *query, *db;
    int *entry, *shift;
    double *dist;
    int *best_shift;
    double *best_dist;
};

// (d1, s1) before (d0, s0): the smaller dist, then the smaller index
__device__ __forceinline__ bool place_before(double d1, int s1, double d0, int s0) { return d1 < d0 || (d1 == d0 && s1 < s0); }

__device__ __forceinline__ void place_wave_min(double &d, int &s)
{
    for (int step = PLACE_WAVE / 2; step >= 1; step >>= 1) {
        const double od = __shfl_xor(d, step, PLACE_WAVE);
        const int os = __shfl_xor(s, step, PLACE_WAVE);
        if (place_before(od, os, d, s)) { d = od; s = os; }
    }
}

constexpr int PLACE_NONE = 0x7fffffff;                  // the index of a lane that holds no candidate: after every real one

// block: 64 threads where sectors <= 64, else 128.  Dynamic LDS: dist (128 doubles), Q and D (sectors * stride words each), the two
// norm vectors (sectors words each); stride = rings | 1.
__global__ __launch_bounds__(2 * PLACE_WAVE) void place_search_kernel(const PlaceSearch a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char place_lds[];
    const int S = a.sectors, R = a.rings, stride = R | 1;
    double *dists = reinterpret_cast<double *>(place_lds);
    unsigned *Q = reinterpret_cast<unsigned *>(place_lds + PLACE_MAX_S * sizeof(double));
    unsigned *D = Q + S * stride;
    unsigned *na = D + S * stride, *nb = na + S;
    const int e = (int)blockIdx.x, q = (int)blockIdx.y, t = (int)threadIdx.x, threads = (int)blockDim.x;
    const unsigned short *gq = a.query + (long)q * S * R, *gd = a.db + (long)e * S * R;
    for (int i = t; i < S * R; i += threads) {
        const int c = i / R, r = i - c * R;
        Q[c * stride + r] = gq[i];
        D[c * stride + r] = gd[i];
    }
    __syncthreads();
    if (t < S) {
        unsigned sa = 0u, sb = 0u;
        for (int r = 0; r < R; ++r) {
            const unsigned u = Q[t * stride + r], v = D[t * stride + r];
            sa += u * u; sb += v * v;
        }
        na[t] = sa; nb[t] = sb;
    }
    __syncthreads();
    double mine = __builtin_inf();
    if (t < S) {
        double sum = 0.0;
        int pairs = 0, c = t;                                                           // c = (j + t) mod S
        for (int j = 0; j < S; ++j) {
            const unsigned aa = na[j], bb = nb[c];
            if (aa != 0u && bb != 0u) {
                const unsigned *qr = Q + j * stride, *dr = D + c * stride;
                unsigned d = 0u;
                for (int r = 0; r < R; ++r) d += qr[r] * dr[r];
                sum = sum + (1.0 - (double)d / sqrt((double)((unsigned long long)aa * (unsigned long long)bb)));
                pairs += 1;
            }
            c = c + 1 == S ? 0 : c + 1;
        }
        if (pairs) mine = sum / (double)pairs;
    }
    dists[t] = mine;                                                                    // t < 128 = PLACE_MAX_S
    __syncthreads();
    if (t < PLACE_WAVE) {
        double d = t < S ? dists[t] : __builtin_inf();
        int s = t < S ? t : PLACE_NONE;
        if (t + PLACE_WAVE < S && place_before(dists[t + PLACE_WAVE], t + PLACE_WAVE, d, s)) { d = dists[t + PLACE_WAVE]; s = t + PLACE_WAVE; }
        place_wave_min(d, s);
        if (t == 0) {
            a.best_shift[(long)q * a.m + e] = s;
            a.best_dist[(long)q * a.m + e] = d;
        }
    }
}

__global__ __launch_bounds__(ELO_BLOCK) void place_rank_kernel(const PlaceSearch a)
{
    __shared__ double wd[ELO_BLOCK / PLACE_WAVE];
    __shared__ int we[ELO_BLOCK / PLACE_WAVE];
    const int q = (int)blockIdx.x, t = (int)threadIdx.x;
    const double *bd = a.best_dist + (long)q * a.m;
    double last_d = 0.0;
    int last_e = -1;                                                                    // -1: no winner yet, every entry is above
    for (int pass = 0; pass < a.k; ++pass) {
        double d = __builtin_inf();
        int e = PLACE_NONE;
        for (int i = t; i < a.m; i += ELO_BLOCK) {
            const double v = bd[i];
            const bool above = last_e < 0 || place_before(last_d, last_e, v, i);
            if (above && place_before(v, i, d, e)) { d = v; e = i; }
        }
        place_wave_min(d, e);
        if ((t & (PLACE_WAVE - 1)) == 0) { wd[t / PLACE_WAVE] = d; we[t / PLACE_WAVE] = e; }
        __syncthreads();
        d = wd[0]; e = we[0];
        for (int w = 1; w < ELO_BLOCK / PLACE_WAVE; ++w)
            if (place_before(wd[w], we[w], d, e)) { d = wd[w]; e = we[w]; }
        __syncthreads();
        const bool found = e != PLACE_NONE;
        if (t == 0) {
            const long o = (long)q * a.k + pass;
            a.entry[o] = found ? e : -1;
            a.shift[o] = found ? a.best_shift[(long)q * a.m + e] : -1;
            a.dist[o] = found ? d : __builtin_inf();
        }
        if (!found) {                                                                   // (uniform) the rest is padding
            for (int rest = pass + 1 + t; rest < a.k; rest += ELO_BLOCK) {
                const long o = (long)q * a.k + rest;
                a.entry[o] = -1; a.shift[o] = -1; a.dist[o] = __builtin_inf();
            }
            return;
        }
        last_d = d; last_e = e;
    }
}

inline bool place_shape_ok(int rings, int sectors)
{
    return rings >= 1 && rings <= PLACE_MAX_R && sectors >= 1 && sectors <= PLACE_MAX_S;
}

}  // namespace
}  // namespace elo

using namespace elo;

extern "C" int elo_scan_descriptor(const elo_scan_descriptor_args *a, elo_stream_t stream)
{
    const char *who = "elo_scan_descriptor";
    ELO_REQUIRE(a, who, "null argument block");
    ELO_REQUIRE(place_shape_ok(a->rings, a->sectors), who, "rings is 1 .. ELO_PLACE_MAX_RINGS, sectors 1 .. ELO_PLACE_MAX_SECTORS");
    ELO_REQUIRE(a->batch >= 0 && a->H >= 1 && a->W >= a->sectors, who, "bad sizes: batch >= 0, H >= 1, W >= sectors");
    ELO_REQUIRE(image_sizes_ok(a->batch, a->H, a->W, 1), who, "batch * H * W beyond 2^31");
    ELO_REQUIRE(a->batch <= 65535, who, "batch beyond 65535");
    ELO_REQUIRE(positive_finite(a->z_step) && a->z_min - a->z_min == 0.0, who,
                "z_step is positive and finite, z_min finite");
    ELO_REQUIRE(a->min_range2 >= 0.0, who, "min_range2 is >= 0");
    double below = 0.0;
    for (int j = 1; j <= a->rings; ++j) {
        ELO_REQUIRE(a->edge2[j] > below && positive_finite(a->edge2[j]), who, "edge2[1 .. rings] is positive, finite and ascending");
        below = a->edge2[j];
    }
    ELO_REQUIRE(a->xyz && a->desc, who, "null pointer");
    if (a->batch == 0) return ELO_OK;
    PlaceDescriptor d = {a->H, a->W, a->rings, a->sectors, a->z_min, a->z_step, a->min_range2, {0.0}, a->xyz, a->desc};
    for (int j = 1; j <= a->rings; ++j) d.edge2[j] = a->edge2[j];
    hipLaunchKernelGGL(place_descriptor_kernel, dim3((unsigned)a->sectors, (unsigned)a->batch), dim3(ELO_BLOCK), 0, (hipStream_t)stream, d);
    return check_launch(who);
}

extern "C" int elo_descriptor_search(const elo_descriptor_search_args *a, elo_stream_t stream)
{
    const char *who = "elo_descriptor_search";
    ELO_REQUIRE(a, who, "null argument block");
    ELO_REQUIRE(place_shape_ok(a->rings, a->sectors), who, "rings is 1 .. ELO_PLACE_MAX_RINGS, sectors 1 .. ELO_PLACE_MAX_SECTORS");
    ELO_REQUIRE(a->n >= 0 && a->n <= 65535 && a->m >= 0, who, "bad sizes: n is 0 .. 65535, m >= 0");
    ELO_REQUIRE(a->k >= 1 && a->k <= ELO_PLACE_MAX_K, who, "k is 1 .. ELO_PLACE_MAX_K");
    ELO_REQUIRE(a->query && a->db && a->entry && a->shift && a->dist, who, "null pointer");
    ELO_REQUIRE(a->m == 0 || (a->best_shift && a->best_dist), who, "null pointer");
    ELO_REQUIRE(aligned(a->dist, 8) && aligned(a->best_dist, 8), who, "dist and best_dist must be 8-byte aligned");
    if (a->n == 0) return ELO_OK;
    const PlaceSearch s = {a->n, a->m, a->rings, a->sectors, a->k, a->query, a->db, a->entry, a->shift, a->dist, a->best_shift, a->best_dist};
    hipStream_t st = (hipStream_t)stream;
    if (a->m > 0) {
        const int stride = a->rings | 1;
        const size_t lds = PLACE_MAX_S * sizeof(double) + (size_t)(2 * a->sectors * stride + 2 * a->sectors) * sizeof(unsigned);   // <= 35 840
        const unsigned threads = a->sectors <= PLACE_WAVE ? PLACE_WAVE : 2 * PLACE_WAVE;
        hipLaunchKernelGGL(place_search_kernel, dim3((unsigned)a->m, (unsigned)a->n), dim3(threads), lds, st, s);
    }
    hipLaunchKernelGGL(place_rank_kernel, dim3((unsigned)a->n), dim3(ELO_BLOCK), 0, st, s);
    return check_launch(who);
}
