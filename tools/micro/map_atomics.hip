// map_atomics.hip -- the A/B behind elo_map_insert's shape (csrc/elo_map.hip): the SAME keys and offsets sent to the voxel table
//   plain        every point probes for its slot and sends its own four 64-bit integer adds;
//   keys         equal keys are folded inside a thread's strip of 4 cells and then across the wave by a loop over its DISTINCT keys (first
//                lane's key, ballot, butterfly sums): ONE lane per distinct key probes and adds;
//   runs         RUNS of equal keys are folded inside the strip and then across the lanes by a segmented scan (heads where the key
//                changes, six shuffle steps whatever the keys): one lane per run probes and adds -- the form the library ships.
// All count their points per wave.  The keys are those of a 64 x 1800 range image whose neighbouring cells share a voxel in runs of
// `run` cells (run = 1: every cell its own voxel; a KITTI scan at voxel 0.5 m has runs of ~5 .. 20, at 0.1 m of ~1 .. 3), equal
// keys also meeting `rows` apart as a wall seen by neighbouring beams does.  Timed: COLD (the table was just reset: every key is
// claimed) and WARM (the keys are there: probe + adds), device events around every launch, the median of `reps`.  The forms'
// tables are compared (count and sums per key, by a checksum that does not depend on placement).
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -o tools/micro/build/map_atomics tools/micro/map_atomics.hip
//   tools/micro/build/map_atomics [reps]
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

typedef unsigned long long u64;
constexpr int BLOCK = 256, STRIP = 4, WAVE = 64, MAX_PROBE = 128;
constexpr u64 EMPTY = ~0ull;

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

__device__ __forceinline__ u64 home_of(u64 h)
{
    h ^= h >> 30; h *= 0xbf58476d1ce4e5b9ull;
    h ^= h >> 27; h *= 0x94d049bb133111ebull;
    h ^= h >> 31;
    return h;
}

__device__ __forceinline__ bool slot_of(u64 *keys, u64 mask, u64 key, u64 &slot, unsigned &claimed)
{
    const u64 home = home_of(key);
    for (int j = 0; j < MAX_PROBE; ++j) {
        const u64 s = (home + (u64)j) & mask;
        u64 cur = __atomic_load_n(keys + s, __ATOMIC_RELAXED);
        if (cur == EMPTY) {
            cur = atomicCAS(keys + s, EMPTY, key);
            if (cur == EMPTY) { claimed += 1u; cur = key; }
        }
        if (cur == key) { slot = s; return true; }
    }
    return false;
}

__device__ __forceinline__ unsigned wave_sum(unsigned v)
{
    for (int d = WAVE / 2; d >= 1; d >>= 1) v += __shfl_xor(v, d, WAVE);
    return v;
}

__device__ __forceinline__ void send(u64 *keys, u64 *acc, u64 mask, u64 key, unsigned n, unsigned gx, unsigned gy, unsigned gz,
                                     unsigned &inserted, unsigned &dropped, unsigned &claimed)
{
    u64 slot;
    if (slot_of(keys, mask, key, slot, claimed)) {
        u64 *row = acc + slot * 4ull;
        atomicAdd(row + 0, (u64)n); atomicAdd(row + 1, (u64)gx); atomicAdd(row + 2, (u64)gy); atomicAdd(row + 3, (u64)gz);
        inserted += n;
    } else {
        dropped += n;
    }
}

__device__ __forceinline__ void count(u64 *stats, unsigned inserted, unsigned dropped, unsigned claimed)
{
    inserted = wave_sum(inserted); dropped = wave_sum(dropped); claimed = wave_sum(claimed);
    if ((threadIdx.x & (WAVE - 1)) == 0) {
        if (inserted) atomicAdd(stats + 0, (u64)inserted);
        if (dropped) atomicAdd(stats + 3, (u64)dropped);
        if (claimed) atomicAdd(stats + 4, (u64)claimed);
    }
}

// key (n), g (n) = gx | gy << 16 | gz << 32; n is a multiple of 4
__global__ __launch_bounds__(BLOCK) void plain_kernel(const u64 *key, const u64 *g, long n, u64 *keys, u64 *acc, u64 *stats, u64 mask)
{
    const long i0 = ((long)blockIdx.x * BLOCK + threadIdx.x) * STRIP;
    unsigned inserted = 0, dropped = 0, claimed = 0;
    for (int c = 0; c < STRIP; ++c) {
        if (i0 + c >= n) break;
        const u64 k = key[i0 + c], o = g[i0 + c];
        send(keys, acc, mask, k, 1u, (unsigned)(o & 0xffff), (unsigned)(o >> 16 & 0xffff), (unsigned)(o >> 32 & 0xffff), inserted, dropped, claimed);
    }
    count(stats, inserted, dropped, claimed);
}

__global__ __launch_bounds__(BLOCK) void aggregated_kernel(const u64 *key, const u64 *g, long n, u64 *keys, u64 *acc, u64 *stats, u64 mask)
{
    const long i0 = ((long)blockIdx.x * BLOCK + threadIdx.x) * STRIP;
    const unsigned lane = threadIdx.x & (WAVE - 1);
    u64 k[STRIP];
    unsigned cnt[STRIP], sx[STRIP], sy[STRIP], sz[STRIP];
    for (int c = 0; c < STRIP; ++c) {
        const bool in = i0 + c < n;
        const u64 o = in ? g[i0 + c] : 0ull;
        k[c] = in ? key[i0 + c] : EMPTY;
        cnt[c] = in ? 1u : 0u;
        sx[c] = (unsigned)(o & 0xffff); sy[c] = (unsigned)(o >> 16 & 0xffff); sz[c] = (unsigned)(o >> 32 & 0xffff);
        if (c > 0 && cnt[c] && cnt[c - 1] && k[c] == k[c - 1]) {
            cnt[c] += cnt[c - 1]; sx[c] += sx[c - 1]; sy[c] += sy[c - 1]; sz[c] += sz[c - 1];
            cnt[c - 1] = 0u;
        }
    }
    unsigned inserted = 0, dropped = 0, claimed = 0;
    for (int c = 0; c < STRIP; ++c) {
        u64 todo = __ballot(cnt[c] != 0u), mine = EMPTY;
        unsigned m = 0, gx = 0, gy = 0, gz = 0;
        for (int trip = 0; trip < WAVE && todo != 0ull; ++trip) {
            const int first = __ffsll((long long)todo) - 1;
            const u64 kk = __shfl(k[c], first, WAVE);
            const bool same = cnt[c] != 0u && k[c] == kk;
            const u64 group = __ballot(same);
            const unsigned tn = wave_sum(same ? cnt[c] : 0u), tx = wave_sum(same ? sx[c] : 0u);
            const unsigned ty = wave_sum(same ? sy[c] : 0u), tz = wave_sum(same ? sz[c] : 0u);
            if ((int)lane == first) { mine = kk; m = tn; gx = tx; gy = ty; gz = tz; }
            todo &= ~group;
        }
        if (m != 0u) send(keys, acc, mask, mine, m, gx, gy, gz, inserted, dropped, claimed);
    }
    count(stats, inserted, dropped, claimed);
}

__global__ __launch_bounds__(BLOCK) void runs_kernel(const u64 *key, const u64 *g, long n, u64 *keys, u64 *acc, u64 *stats, u64 mask)
{
    const long i0 = ((long)blockIdx.x * BLOCK + threadIdx.x) * STRIP;
    const unsigned lane = threadIdx.x & (WAVE - 1);
    const u64 upto = (2ull << lane) - 1ull;
    u64 k[STRIP];
    unsigned cnt[STRIP], sx[STRIP], sy[STRIP], sz[STRIP];
    for (int c = 0; c < STRIP; ++c) {
        const bool in = i0 + c < n;
        const u64 o = in ? g[i0 + c] : 0ull;
        k[c] = in ? key[i0 + c] : EMPTY;
        cnt[c] = in ? 1u : 0u;
        sx[c] = (unsigned)(o & 0xffff); sy[c] = (unsigned)(o >> 16 & 0xffff); sz[c] = (unsigned)(o >> 32 & 0xffff);
        if (c > 0) {
            if (!cnt[c]) k[c] = k[c - 1];
            if (k[c] == k[c - 1]) {
                cnt[c] += cnt[c - 1]; sx[c] += sx[c - 1]; sy[c] += sy[c - 1]; sz[c] += sz[c - 1];
                cnt[c - 1] = 0u; sx[c - 1] = 0u; sy[c - 1] = 0u; sz[c - 1] = 0u;
            }
        }
    }
    unsigned inserted = 0, dropped = 0, claimed = 0;
    for (int c = 0; c < STRIP; ++c) {
        const u64 have = __ballot(cnt[c] != 0u) & upto;
        const u64 kk = __shfl(k[c], have ? 63 - __clzll((long long)have) : (int)lane, WAVE);
        const u64 mine = have ? kk : EMPTY;
        const u64 below = __shfl_up(mine, 1, WAVE);
        const u64 heads = __ballot(lane == 0u || mine != below);
        const unsigned start = 63u - (unsigned)__clzll((long long)(heads & upto));
        unsigned m = cnt[c], gx = sx[c], gy = sy[c], gz = sz[c];
        for (unsigned d = 1; d < WAVE; d <<= 1) {
            const unsigned tn = __shfl_up(m, d, WAVE), tx = __shfl_up(gx, d, WAVE), ty = __shfl_up(gy, d, WAVE), tz = __shfl_up(gz, d, WAVE);
            if (lane >= start + d) { m += tn; gx += tx; gy += ty; gz += tz; }
        }
        const bool last = lane == WAVE - 1 || (heads >> (lane + 1u) & 1ull) != 0ull;
        if (last && m != 0u) send(keys, acc, mask, mine, m, gx, gy, gz, inserted, dropped, claimed);
    }
    count(stats, inserted, dropped, claimed);
}

// a sum over the occupied slots that does not depend on where a key sits
__global__ void checksum_kernel(const u64 *keys, const u64 *acc, u64 slots, u64 *out)
{
    const u64 s = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= slots || keys[s] == EMPTY) return;
    const u64 *r = acc + s * 4;
    atomicAdd(out + 0, 1ull);
    atomicAdd(out + 1, r[0]);
    atomicAdd(out + 2, home_of(keys[s] ^ home_of(r[0] + 3 * r[1] + 5 * r[2] + 7 * r[3])));
}

int main(int argc, char **argv)
{
    const int reps = argc > 1 ? atoi(argv[1]) : 31;
    const int H = 64, W = 1800, LOG2 = 22;
    const long n = (long)H * W;
    const u64 slots = 1ull << LOG2;
    u64 *d_key, *d_g, *keys, *acc, *stats, *sum;
    CHECK(hipMalloc(&d_key, n * 8)); CHECK(hipMalloc(&d_g, n * 8));
    CHECK(hipMalloc(&keys, slots * 8)); CHECK(hipMalloc(&acc, slots * 32)); CHECK(hipMalloc(&stats, 64)); CHECK(hipMalloc(&sum, 24));
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
    const dim3 grid((unsigned)((n + BLOCK * STRIP - 1) / (BLOCK * STRIP)));
    printf("%ld points (a %d x %d image), table 2^%d slots, median of %d launches, us\n", n, H, W, LOG2, reps);
    printf("%6s %9s | %10s %10s | %10s %10s | %10s %10s | %s\n", "run", "voxels", "plain cold", "warm", "keys cold", "warm", "runs cold", "warm",
           "tables");
    auto launch = [&](int form) {
        if (form == 0) hipLaunchKernelGGL(plain_kernel, grid, dim3(BLOCK), 0, 0, d_key, d_g, n, keys, acc, stats, slots - 1);
        else if (form == 1) hipLaunchKernelGGL(aggregated_kernel, grid, dim3(BLOCK), 0, 0, d_key, d_g, n, keys, acc, stats, slots - 1);
        else hipLaunchKernelGGL(runs_kernel, grid, dim3(BLOCK), 0, 0, d_key, d_g, n, keys, acc, stats, slots - 1);
    };
    for (int run : {1, 2, 4, 8, 16, 64}) {
        std::vector<u64> key(n), g(n);
        u64 rng = 88172645463325252ull;
        for (long i = 0; i < n; ++i) {
            const long h = i / W, w = i % W;
            const u64 vx = (u64)(w / run), vy = (u64)(h / 2);                   // neighbouring beams see the same voxel: runs `rows` apart
            key[i] = (vx + (1ull << 20)) << 42 | (vy + (1ull << 20)) << 21 | (1ull << 20);
            rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17;
            g[i] = (rng & 0xffff) | (rng >> 16 & 0xffff) << 16 | (rng >> 32 & 0xffff) << 32;
        }
        CHECK(hipMemcpy(d_key, key.data(), n * 8, hipMemcpyHostToDevice));
        CHECK(hipMemcpy(d_g, g.data(), n * 8, hipMemcpyHostToDevice));
        double med[3][2];
        u64 sums[3][3], st[3][8];
        for (int form = 0; form < 3; ++form) {
            for (int warm = 0; warm < 2; ++warm) {
                std::vector<float> t;
                for (int r = 0; r < reps + 2; ++r) {
                    if (!warm || r == 0) {
                        CHECK(hipMemset(keys, 0xff, slots * 8)); CHECK(hipMemset(acc, 0, slots * 32)); CHECK(hipMemset(stats, 0, 64));
                        if (warm) launch(0);
                    }
                    CHECK(hipDeviceSynchronize());
                    CHECK(hipEventRecord(e0, 0));
                    launch(form);
                    CHECK(hipEventRecord(e1, 0));
                    CHECK(hipEventSynchronize(e1));
                    float ms;
                    CHECK(hipEventElapsedTime(&ms, e0, e1));
                    if (r >= 2) t.push_back(ms * 1e3f);
                }
                std::sort(t.begin(), t.end());
                med[form][warm] = t[t.size() / 2];
            }
            // the table of ONE cold launch of this form
            CHECK(hipMemset(keys, 0xff, slots * 8)); CHECK(hipMemset(acc, 0, slots * 32)); CHECK(hipMemset(stats, 0, 64)); CHECK(hipMemset(sum, 0, 24));
            launch(form);
            hipLaunchKernelGGL(checksum_kernel, dim3((unsigned)(slots / 256)), dim3(256), 0, 0, keys, acc, slots, sum);
            CHECK(hipDeviceSynchronize());
            CHECK(hipMemcpy(sums[form], sum, 24, hipMemcpyDeviceToHost));
            CHECK(hipMemcpy(st[form], stats, 64, hipMemcpyDeviceToHost));
        }
        bool same = st[0][0] == (u64)n;
        for (int form = 1; form < 3; ++form)
            same = same && sums[0][0] == sums[form][0] && sums[0][1] == sums[form][1] && sums[0][2] == sums[form][2] &&
                   st[0][0] == st[form][0] && st[0][3] == st[form][3] && st[0][4] == st[form][4];
        printf("%6d %9llu | %10.1f %10.1f | %10.1f %10.1f | %10.1f %10.1f | %s\n", run, sums[0][0], med[0][0], med[0][1], med[1][0], med[1][1],
               med[2][0], med[2][1], same ? "equal" : "DIFFERENT");
        if (!same) return 1;
    }
    return 0;
}
