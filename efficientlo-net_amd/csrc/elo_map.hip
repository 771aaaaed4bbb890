// elo_map.hip -- the WORLD MAP (include/elo.h, elo_map_insert / elo_map_extract): a voxel-hashed point map, every scan carried by its
// scan -> world pose and summed per voxel into 64-bit INTEGERS: count and the three sums of the points' 16-bit offsets inside the
// voxel.  Sums of integers do not depend on the order of arrival, so the content of the map is a function of the points put in.
//
// map_insert_kernel: a streaming pass like model_splat_kernel -- a workgroup works inside one scan, so R(q) is formed once per
// thread; a thread takes MAP_STRIP consecutive cells by 16-byte loads.  Neighbouring cells of a range image often share a voxel:
// a thread first folds RUNS of equal keys inside its strip (cells without a point pass a run along), then the wave folds runs of
// equal keys across its lanes -- heads where the key changes, a segmented scan of the four integers, six shuffle steps whatever the
// keys -- and the last lane of every run probes and adds: ONE probe / claim and four adds per run.  Equal keys that are not neighbours
// are sent apart; the sums are integers, so the table ends up the same.  (The loop over the wave's DISTINCT keys -- first lane's key,
// ballot, butterfly sum -- costs 24 shuffles per key: slower than one add per point below ~8 cells a key; tools/micro/map_atomics.hip
// holds all three forms.)  The counters go the same way: ballots and one add per wave and counter.
// map_extract_kernel: one thread per slot, ballot compaction, one atomic on the cursor per wave.
// map_merge_kernel (elo_map_merge): source rows (key, four integers) filtered and added into a table through the insert's own
// probe / claim / add (map_add, elo_map_device.h): the sliding window, growth, a loaded state and the union of two maps.
#include "elo_map_device.h"

namespace elo {
namespace {

constexpr int MAP_STRIP = 4;                            // cells per thread: 48 bytes, three 16-byte loads
constexpr int MAP_TILE = ELO_BLOCK * MAP_STRIP;         // cells per workgroup
constexpr int MAP_WAVE = 64;

struct MapInsert {
    int H, W;
    float voxel, min_range, max_range;
    unsigned long long mask;        // C - 1
    const float *xyz;               // (batch,H,W,3)
    const double *pose;             // (batch,7)
    unsigned long long *keys, *acc, *stats;
    unsigned tiles;                 // workgroups per scan
    int vec;                        // 1: H*W is a multiple of 4 and xyz is 16-byte aligned
};

enum { MAP_NONE = 0, MAP_FILTERED = 1, MAP_REJECTED = 2, MAP_POINT = 3 };

// the per-point rule of include/elo.h -> MAP_NONE / FILTERED / REJECTED / POINT (then key and g are set)
__device__ __forceinline__ int map_point(const MapInsert &a, const double (&R)[9], const double (&t)[3], float ax, float ay, float az,
                                         unsigned long long &key, unsigned (&g)[3])
{
    if (cell_empty(ax, ay, az)) return MAP_NONE;
    const float rf = sqrtf(ax * ax + ay * ay + az * az);
    if (rf < a.min_range || rf > a.max_range) return MAP_FILTERED;
    float x, y, z;
    pose_carry_f32(R, t, ax, ay, az, x, y, z);
    if (!point_finite(x, y, z)) return MAP_REJECTED;
    const double voxel = (double)a.voxel;
    unsigned long long fx, fy, fz;
    if (!map_axis(x, voxel, fx, g[0]) || !map_axis(y, voxel, fy, g[1]) || !map_axis(z, voxel, fz, g[2])) return MAP_REJECTED;
    key = fx << 42 | fy << 21 | fz;
    return MAP_POINT;
}

__device__ __forceinline__ unsigned wave_sum(unsigned v)
{
    for (int d = MAP_WAVE / 2; d >= 1; d >>= 1) v += __shfl_xor(v, d, MAP_WAVE);
    return v;
}

__global__ __launch_bounds__(ELO_BLOCK) void map_insert_kernel(const MapInsert a)
{
    const unsigned b = blockIdx.x / a.tiles, tile = blockIdx.x - b * a.tiles;
    double R[9], t[3];
    if (!pose_load(a.pose + (long)b * 7, R, t)) return;                                 // the whole scan, by the whole workgroup
    const long cells = (long)a.H * a.W;
    const long i0 = ((long)tile * ELO_BLOCK + threadIdx.x) * MAP_STRIP;
    float v[3 * MAP_STRIP];
    if (i0 >= cells) {                                                                  // (the lane stays for the wave's ballots)
        for (int j = 0; j < 3 * MAP_STRIP; ++j) v[j] = 0.0f;
    } else {
        const float *s = a.xyz + ((long)b * cells + i0) * 3;
        if (a.vec) {                                                                    // (cells % 4 == 0: the strip is inside the image)
            const float4 *s4 = reinterpret_cast<const float4 *>(s);
            const float4 u0 = s4[0], u1 = s4[1], u2 = s4[2];
            v[0] = u0.x; v[1] = u0.y; v[2] = u0.z; v[3] = u0.w; v[4] = u1.x; v[5] = u1.y; v[6] = u1.z; v[7] = u1.w;
            v[8] = u2.x; v[9] = u2.y; v[10] = u2.z; v[11] = u2.w;
        } else {
            for (int c = 0; c < MAP_STRIP; ++c) {
                const bool in = i0 + c < cells;
                for (int j = 0; j < 3; ++j) v[c * 3 + j] = in ? s[c * 3 + j] : 0.0f;
            }
        }
    }
    const unsigned lane = threadIdx.x & (MAP_WAVE - 1);
    const unsigned long long upto = (2ull << lane) - 1ull;                              // lanes 0 .. lane (lane 63: all)
    unsigned long long key[MAP_STRIP];
    unsigned cnt[MAP_STRIP], sx[MAP_STRIP], sy[MAP_STRIP], sz[MAP_STRIP];
    unsigned filtered = 0, rejected = 0;                                                // wave-uniform: ballots
    for (int c = 0; c < MAP_STRIP; ++c) {
        unsigned g[3] = {0u, 0u, 0u};
        key[c] = MAP_EMPTY;
        const int kind = map_point(a, R, t, v[c * 3], v[c * 3 + 1], v[c * 3 + 2], key[c], g);
        filtered += (unsigned)__popcll(__ballot(kind == MAP_FILTERED));
        rejected += (unsigned)__popcll(__ballot(kind == MAP_REJECTED));
        cnt[c] = kind == MAP_POINT ? 1u : 0u;
        sx[c] = cnt[c] ? g[0] : 0u; sy[c] = cnt[c] ? g[1] : 0u; sz[c] = cnt[c] ? g[2] : 0u;
        if (c > 0) {
            // a run inside the strip moves on to its last cell; a cell without a point passes the run before it along (a hole in a
            // wall does not end the wall's run)
            if (!cnt[c]) key[c] = key[c - 1];
            if (key[c] == key[c - 1]) {
                cnt[c] += cnt[c - 1]; sx[c] += sx[c - 1]; sy[c] += sy[c - 1]; sz[c] += sz[c - 1];
                cnt[c - 1] = 0u; sx[c - 1] = 0u; sy[c - 1] = 0u; sz[c - 1] = 0u;
            }
        }
    }
    unsigned inserted = 0, dropped = 0, claimed = 0;                                    // this lane's
    for (int c = 0; c < MAP_STRIP; ++c) {
        // ... and across the lanes, cell c of every strip: a lane with nothing in cell c takes the key of the nearest lane below
        // that has, so runs pass over it; a run of lanes with one key is a segment, summed by a segmented scan (six steps, whatever
        // the keys), and the segment's last lane sends the sums.  <= 256 points a wave: a sum stays below 2^24.
        const unsigned long long have = __ballot(cnt[c] != 0u) & upto;
        const unsigned long long k = __shfl(key[c], have ? 63 - __clzll((long long)have) : (int)lane, MAP_WAVE);
        const unsigned long long mine = have ? k : MAP_EMPTY;
        const unsigned long long below = __shfl_up(mine, 1, MAP_WAVE);
        const unsigned long long heads = __ballot(lane == 0u || mine != below);
        const unsigned start = 63u - (unsigned)__clzll((long long)(heads & upto));      // (lane 0 is a head)
        unsigned n = cnt[c], gx = sx[c], gy = sy[c], gz = sz[c];
        for (unsigned d = 1; d < MAP_WAVE; d <<= 1) {
            const unsigned tn = __shfl_up(n, d, MAP_WAVE), tx = __shfl_up(gx, d, MAP_WAVE);
            const unsigned ty = __shfl_up(gy, d, MAP_WAVE), tz = __shfl_up(gz, d, MAP_WAVE);
            if (lane >= start + d) { n += tn; gx += tx; gy += ty; gz += tz; }
        }
        const bool last = lane == MAP_WAVE - 1 || (heads >> (lane + 1u) & 1ull) != 0ull;
        if (last && n != 0u) {
            if (map_add(a.keys, a.acc, a.mask, mine, (unsigned long long)n, (unsigned long long)gx, (unsigned long long)gy,
                        (unsigned long long)gz, claimed))
                inserted += n;
            else
                dropped += n;
        }
    }
    inserted = wave_sum(inserted);
    dropped = wave_sum(dropped);
    claimed = wave_sum(claimed);
    if (lane == 0u) {
        if (inserted) atomicAdd(a.stats + 0, (unsigned long long)inserted);
        if (filtered) atomicAdd(a.stats + 1, (unsigned long long)filtered);
        if (rejected) atomicAdd(a.stats + 2, (unsigned long long)rejected);
        if (dropped) atomicAdd(a.stats + 3, (unsigned long long)dropped);
        if (claimed) atomicAdd(a.stats + 4, (unsigned long long)claimed);
    }
}

__global__ void map_cursor_kernel(unsigned long long *cursor)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) *cursor = 0ull;
}

struct MapExtract {
    float voxel;
    unsigned long long slots;       // C
    unsigned long long max_out;
    const unsigned long long *keys, *acc;
    long long *out_key, *out_count;
    float *out_xyz;
    unsigned long long *cursor;
};

// one thread per slot; the grid covers C exactly (C is a multiple of the block)
__global__ __launch_bounds__(ELO_BLOCK) void map_extract_kernel(const MapExtract a)
{
    const unsigned long long s = (unsigned long long)blockIdx.x * ELO_BLOCK + threadIdx.x;
    const unsigned lane = threadIdx.x & (MAP_WAVE - 1);
    const unsigned long long key = s < a.slots ? a.keys[s] : MAP_EMPTY;
    const bool full = key != MAP_EMPTY;
    const unsigned long long m = __ballot(full);
    if (m == 0ull) return;
    unsigned long long base = 0ull;
    if (lane == 0u) base = atomicAdd(a.cursor, (unsigned long long)__popcll(m));
    base = __shfl(base, 0, MAP_WAVE);
    if (!full) return;
    const unsigned long long row = base + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull));
    if (row >= a.max_out) return;
    const unsigned long long *acc = a.acc + s * 4ull;
    const unsigned long long count = acc[0];
    const double voxel = (double)a.voxel;
    a.out_key[row] = (long long)key;
    a.out_count[row] = (long long)count;
    a.out_xyz[row * 3 + 0] = map_centroid(key >> 42 & 0x1fffffull, acc[1], count, voxel);
    a.out_xyz[row * 3 + 1] = map_centroid(key >> 21 & 0x1fffffull, acc[2], count, voxel);
    a.out_xyz[row * 3 + 2] = map_centroid(key & 0x1fffffull, acc[3], count, voxel);
}

constexpr int MERGE_STRIP = 2;                          // source rows per lane and step: their keys are one 16-byte load
constexpr int MERGE_STEPS = 8;                          // steps per wave: 1024 neighbouring rows
constexpr int MERGE_TILE = ELO_BLOCK * MERGE_STRIP * MERGE_STEPS;      // source rows per workgroup

struct MapMerge {
    unsigned long long rows;
    const unsigned long long *src_keys, *src_acc;
    float voxel, radius;
    unsigned long long mask;        // C - 1, the destination's
    unsigned long long *keys, *acc, *stats;
    const double *centre;           // NULL: no window
    unsigned long long min_count;
    unsigned long long *report;
    int vec_keys, vec_acc;          // 1: src_keys / src_acc is 16-byte aligned
};

enum { MERGE_SKIP = 0, MERGE_REJECTED = 1, MERGE_FILTERED = 2, MERGE_ROW = 3 };

// the per-row rule of include/elo.h for an occupied source row (key is not all ones) -> MERGE_REJECTED / FILTERED / ROW
__device__ __forceinline__ int merge_row(const MapMerge &a, const double (&centre)[3], unsigned long long key,
                                         const unsigned long long (&r)[4])
{
    const unsigned long long n = r[0];
    if (key >> 63 != 0ull || n == 0ull || n >= 1ull << 40) return MERGE_REJECTED;
    const unsigned long long most = 65535ull * n;                                       // < 2^56
    if (r[1] > most || r[2] > most || r[3] > most) return MERGE_REJECTED;
    if (n < a.min_count) return MERGE_FILTERED;
    if (a.centre) {
        const double voxel = (double)a.voxel, radius = (double)a.radius;
        for (int axis = 0; axis < 3; ++axis) {
            const unsigned long long field = key >> (42 - 21 * axis) & 0x1fffffull;
            const double c = ((double)((long long)field - (1ll << 20)) + 0.5) * voxel;
            const double d = fabs(c - centre[axis]);
            if (!(d <= radius)) return MERGE_FILTERED;                                  // (a NaN centre keeps nothing)
        }
    }
    return MERGE_ROW;
}

__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long v)
{
    for (int d = MAP_WAVE / 2; d >= 1; d >>= 1) v += __shfl_xor(v, d, MAP_WAVE);
    return v;
}

// a stream over src_keys, 8 bytes a source row.  A wave takes MERGE_STEPS * 128 neighbouring rows, 128 a step (a lane two
// neighbours: one 16-byte load), all its key loads issued before the first is looked at; a step whose 128 slots are all empty -- most
// steps over a table -- costs no more.  The 32 bytes of an acc row are read for occupied rows only.  Every kept row is one map_add: a
// source has a key once (a table) or a few times (concatenated states), so there are no runs to fold.  The counters are the wave's,
// one add per wave and counter: with one step a wave, a table of 2^22 slots made 32 768 waves add to the same few words and those
// adds, not the probes, were the kernel's time (profiles/map_merge.txt).
__global__ __launch_bounds__(ELO_BLOCK) void map_merge_kernel(const MapMerge a)
{
    const unsigned lane = threadIdx.x & (MAP_WAVE - 1);
    const unsigned long long wave = (unsigned long long)blockIdx.x * (ELO_BLOCK / MAP_WAVE) + threadIdx.x / MAP_WAVE;
    const unsigned long long first = (wave * MERGE_STEPS * MAP_WAVE + lane) * MERGE_STRIP;      // this lane's rows of step 0
    unsigned long long key[MERGE_STEPS][MERGE_STRIP];
    for (int step = 0; step < MERGE_STEPS; ++step) {
        const unsigned long long i0 = first + (unsigned long long)step * (MAP_WAVE * MERGE_STRIP);
        if (a.vec_keys && i0 + MERGE_STRIP <= a.rows) {
            const ulonglong2 u = *reinterpret_cast<const ulonglong2 *>(a.src_keys + i0);
            key[step][0] = u.x; key[step][1] = u.y;
        } else {
            for (int c = 0; c < MERGE_STRIP; ++c) key[step][c] = i0 + c < a.rows ? a.src_keys[i0 + c] : MAP_EMPTY;
        }
    }
    double centre[3] = {0.0, 0.0, 0.0};
    if (a.centre) { centre[0] = a.centre[0]; centre[1] = a.centre[1]; centre[2] = a.centre[2]; }
    unsigned v_merged = 0, v_filtered = 0, v_rejected = 0, v_dropped = 0;               // wave-uniform: ballots
    unsigned long long p_merged = 0, p_filtered = 0, p_dropped = 0;                     // this lane's
    unsigned claimed = 0;
    for (int step = 0; step < MERGE_STEPS; ++step) {
        if (__ballot(key[step][0] != MAP_EMPTY || key[step][1] != MAP_EMPTY) == 0ull) continue;
        const unsigned long long i0 = first + (unsigned long long)step * (MAP_WAVE * MERGE_STRIP);
        for (int c = 0; c < MERGE_STRIP; ++c) {
            int kind = MERGE_SKIP;
            bool dropped = false;
            if (key[step][c] != MAP_EMPTY) {
                const unsigned long long *s = a.src_acc + (i0 + c) * 4ull;
                unsigned long long r[4];
                if (a.vec_acc) {
                    const ulonglong2 u0 = reinterpret_cast<const ulonglong2 *>(s)[0], u1 = reinterpret_cast<const ulonglong2 *>(s)[1];
                    r[0] = u0.x; r[1] = u0.y; r[2] = u1.x; r[3] = u1.y;
                } else {
                    for (int j = 0; j < 4; ++j) r[j] = s[j];
                }
                kind = merge_row(a, centre, key[step][c], r);
                if (kind == MERGE_ROW) {
                    if (map_add(a.keys, a.acc, a.mask, key[step][c], r[0], r[1], r[2], r[3], claimed)) p_merged += r[0];
                    else { dropped = true; p_dropped += r[0]; }
                } else if (kind == MERGE_FILTERED) {
                    p_filtered += r[0];
                }
            }
            v_merged += (unsigned)__popcll(__ballot(kind == MERGE_ROW && !dropped));
            v_filtered += (unsigned)__popcll(__ballot(kind == MERGE_FILTERED));
            v_rejected += (unsigned)__popcll(__ballot(kind == MERGE_REJECTED));
            v_dropped += (unsigned)__popcll(__ballot(dropped));
        }
    }
    if ((v_merged | v_filtered | v_rejected | v_dropped) == 0u) return;                 // (wave-uniform) only empty slots
    p_merged = wave_sum64(p_merged);
    p_filtered = wave_sum64(p_filtered);
    p_dropped = wave_sum64(p_dropped);
    claimed = wave_sum(claimed);
    if (lane == 0u) {
        if (v_merged) atomicAdd(a.report + 0, (unsigned long long)v_merged);
        if (v_filtered) atomicAdd(a.report + 1, (unsigned long long)v_filtered);
        if (v_rejected) atomicAdd(a.report + 2, (unsigned long long)v_rejected);
        if (v_dropped) atomicAdd(a.report + 3, (unsigned long long)v_dropped);
        if (p_merged) { atomicAdd(a.report + 4, p_merged); atomicAdd(a.stats + 0, p_merged); }
        if (p_filtered) atomicAdd(a.report + 5, p_filtered);
        if (p_dropped) { atomicAdd(a.report + 6, p_dropped); atomicAdd(a.stats + 3, p_dropped); }
        if (claimed) { atomicAdd(a.report + 7, (unsigned long long)claimed); atomicAdd(a.stats + 4, (unsigned long long)claimed); }
    }
}

}  // namespace
}  // namespace elo

using namespace elo;

extern "C" int elo_map_insert(const elo_map_insert_args *a, elo_stream_t stream)
{
    const char *who = "elo_map_insert";
    ELO_REQUIRE(a, who, "null argument block");
    ELO_REQUIRE(a->batch >= 0 && a->H >= 1 && a->W >= 1, who, "bad sizes");
    ELO_REQUIRE(image_sizes_ok(a->batch, a->H, a->W, 1), who, "batch * H * W beyond 2^31");
    ELO_REQUIRE(map_table_ok(a->voxel, a->log2_capacity), who, "voxel is positive and finite, log2_capacity ELO_MAP_MIN_LOG2 .. ELO_MAP_MAX_LOG2");
    ELO_REQUIRE(a->min_range >= 0.0f, who, "min_range is >= 0");
    ELO_REQUIRE(a->max_range > a->min_range, who, "max_range lies above min_range");
    ELO_REQUIRE(a->xyz && a->pose && a->keys && a->acc && a->stats, who, "null pointer");
    ELO_REQUIRE(aligned(a->pose, 8) && aligned(a->keys, 8) && aligned(a->acc, 8) && aligned(a->stats, 8), who,
                "pose, keys, acc and stats must be 8-byte aligned");
    if (a->batch == 0) return ELO_OK;
    const long cells = (long)a->H * a->W;
    const unsigned tiles = (unsigned)((cells + MAP_TILE - 1) / MAP_TILE);
    const MapInsert m = {a->H, a->W, a->voxel, a->min_range, a->max_range, (1ull << a->log2_capacity) - 1ull, a->xyz, a->pose, a->keys,
                         a->acc, a->stats, tiles, (cells % MAP_STRIP == 0 && aligned(a->xyz, 16)) ? 1 : 0};
    const dim3 grid(tiles * (unsigned)a->batch);                        // < 2^21: batch * H * W < 2^31, 1024 cells a tile
    hipLaunchKernelGGL(map_insert_kernel, grid, dim3(ELO_BLOCK), 0, (hipStream_t)stream, m);
    return check_launch(who);
}

extern "C" int elo_map_extract(const elo_map_extract_args *a, elo_stream_t stream)
{
    const char *who = "elo_map_extract";
    ELO_REQUIRE(a, who, "null argument block");
    ELO_REQUIRE(map_table_ok(a->voxel, a->log2_capacity), who, "voxel is positive and finite, log2_capacity ELO_MAP_MIN_LOG2 .. ELO_MAP_MAX_LOG2");
    ELO_REQUIRE(a->max_out >= 0, who, "max_out is >= 0");
    ELO_REQUIRE(a->keys && a->acc && a->out_key && a->out_count && a->out_xyz && a->cursor, who, "null pointer");
    ELO_REQUIRE(aligned(a->keys, 8) && aligned(a->acc, 8) && aligned(a->out_key, 8) && aligned(a->out_count, 8) && aligned(a->cursor, 8), who,
                "keys, acc, out_key, out_count and cursor must be 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const unsigned long long slots = 1ull << a->log2_capacity;
    const MapExtract e = {a->voxel, slots, (unsigned long long)a->max_out, a->keys, a->acc, a->out_key, a->out_count, a->out_xyz, a->cursor};
    hipLaunchKernelGGL(map_cursor_kernel, dim3(1), dim3(MAP_WAVE), 0, s, a->cursor);
    hipLaunchKernelGGL(map_extract_kernel, dim3((unsigned)(slots / ELO_BLOCK)), dim3(ELO_BLOCK), 0, s, e);    // <= 2^20 workgroups
    return check_launch(who);
}

extern "C" int elo_map_merge(const elo_map_merge_args *a, elo_stream_t stream)
{
    const char *who = "elo_map_merge";
    ELO_REQUIRE(a, who, "null argument block");
    ELO_REQUIRE(a->rows >= 0 && a->rows < (1l << 31), who, "rows is 0 .. 2^31 - 1");
    ELO_REQUIRE(map_table_ok(a->voxel, a->log2_capacity), who, "voxel is positive and finite, log2_capacity ELO_MAP_MIN_LOG2 .. ELO_MAP_MAX_LOG2");
    ELO_REQUIRE(a->min_count >= 1, who, "min_count is >= 1");
    ELO_REQUIRE(!a->centre || positive_finite(a->radius), who, "with a centre, radius is positive and finite");
    ELO_REQUIRE(a->src_keys && a->src_acc && a->keys && a->acc && a->stats && a->report, who, "null pointer");
    ELO_REQUIRE(aligned(a->src_keys, 8) && aligned(a->src_acc, 8) && aligned(a->keys, 8) && aligned(a->acc, 8) && aligned(a->stats, 8) &&
                aligned(a->centre, 8) && aligned(a->report, 8), who, "src_keys, src_acc, keys, acc, stats, centre and report must be 8-byte aligned");
    const unsigned long long rows = (unsigned long long)a->rows, slots = 1ull << a->log2_capacity;
    ELO_REQUIRE(rows == 0ull ||                                                         // (no row: nothing overlaps, whatever the pointers)
                (!ranges_meet(a->src_keys, rows * 8ull, a->keys, slots * 8ull) && !ranges_meet(a->src_keys, rows * 8ull, a->acc, slots * 32ull) &&
                 !ranges_meet(a->src_acc, rows * 32ull, a->keys, slots * 8ull) && !ranges_meet(a->src_acc, rows * 32ull, a->acc, slots * 32ull)),
                who, "the source rows overlap the destination table");
    if (a->rows == 0) return ELO_OK;
    const MapMerge m = {rows, a->src_keys, a->src_acc, a->voxel, a->radius, slots - 1ull, a->keys, a->acc, a->stats, a->centre,
                        (unsigned long long)a->min_count, a->report, aligned(a->src_keys, 16) ? 1 : 0,
                        aligned(a->src_acc, 16) ? 1 : 0};
    const dim3 grid((unsigned)((rows + MERGE_TILE - 1) / MERGE_TILE));                  // < 2^19: rows < 2^31, 4096 rows a workgroup
    hipLaunchKernelGGL(map_merge_kernel, grid, dim3(ELO_BLOCK), 0, (hipStream_t)stream, m);
    return check_launch(who);
}
