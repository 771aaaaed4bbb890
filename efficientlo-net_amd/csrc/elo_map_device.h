// elo_map_device.h -- the world map's rules that more than one file states (include/elo.h, WORLD MAP): the voxel index of a rounded
// coordinate, the hash, the probe / claim / add, the centroid.  elo_map.hip writes the table by them (the insert and the merge
// through the same map_add) and elo_mapfit.hip reads it by them.  The pose row and a cell's validity rule (cell_empty, point_finite)
// come with elo_pose_device.h, included here.
#pragma once
#include "elo_pose_device.h"

namespace elo {
namespace {

constexpr unsigned long long MAP_EMPTY = ~0ull;
constexpr double MAP_HALF = 1048576.0;                  // 2^20: indices lie in [-2^20, 2^20)

// one axis of the rounded p': its 21-bit field of the key and its offset inside the voxel; false: the index is out of range
__device__ __forceinline__ bool map_axis(float c, double voxel, unsigned long long &field, unsigned &g)
{
    const double u = (double)c / voxel;
    const double i = floor(u);
    if (!(i >= -MAP_HALF && i < MAP_HALF)) return false;
    const double f = floor((u - i) * 65536.0);          // u - i lies in [0, 1]: 1 where u is a tiny negative number
    const unsigned o = (unsigned)f;
    g = o < 65535u ? o : 65535u;
    field = (unsigned long long)((long long)i + (1ll << 20));
    return true;
}

__device__ __forceinline__ unsigned long long map_home(unsigned long long h)
{
    h ^= h >> 30; h *= 0xbf58476d1ce4e5b9ull;
    h ^= h >> 27; h *= 0x94d049bb133111ebull;
    h ^= h >> 31;
    return h;
}

__device__ __forceinline__ float map_centroid(unsigned long long field, unsigned long long s, unsigned long long count, double voxel)
{
    const double i = (double)((long long)field - (1ll << 20));
    return (float)((i + ((double)s / (double)count + 0.5) / 65536.0) * voxel);
}

// the slot of `key`, claimed where it has none yet; false: none within ELO_MAP_MAX_PROBE.  A slot only ever turns from empty into
// one key, so a plain load that shows another key is final and one that shows empty is settled by the CAS.
__device__ __forceinline__ bool map_slot(unsigned long long *keys, const unsigned long long mask, const unsigned long long key,
                                         unsigned long long &slot, unsigned &claimed)
{
    const unsigned long long home = map_home(key);
    for (int j = 0; j < ELO_MAP_MAX_PROBE; ++j) {
        const unsigned long long s = (home + (unsigned long long)j) & mask;
        unsigned long long cur = __atomic_load_n(keys + s, __ATOMIC_RELAXED);
        if (cur == MAP_EMPTY) {
            cur = atomicCAS(keys + s, MAP_EMPTY, key);
            if (cur == MAP_EMPTY) { claimed += 1u; cur = key; }
        }
        if (cur == key) { slot = s; return true; }
    }
    return false;
}

// probe / claim / add: {n, sx, sy, sz} into the voxel `key` of the table; false: no slot within the limit, nothing touched.  The
// ONE writer of a table's rows: elo_map_insert sends a run's sums through it, elo_map_merge a source row's.
__device__ __forceinline__ bool map_add(unsigned long long *keys, unsigned long long *acc, const unsigned long long mask,
                                        const unsigned long long key, const unsigned long long n, const unsigned long long sx,
                                        const unsigned long long sy, const unsigned long long sz, unsigned &claimed)
{
    unsigned long long slot;
    if (!map_slot(keys, mask, key, slot, claimed)) return false;
    unsigned long long *row = acc + slot * 4ull;
    atomicAdd(row + 0, n);
    atomicAdd(row + 1, sx);
    atomicAdd(row + 2, sy);
    atomicAdd(row + 3, sz);
    return true;
}

inline bool map_table_ok(float voxel, int log2_capacity)
{
    return positive_finite(voxel) && log2_capacity >= ELO_MAP_MIN_LOG2 && log2_capacity <= ELO_MAP_MAX_LOG2;
}

}  // namespace
}  // namespace elo
