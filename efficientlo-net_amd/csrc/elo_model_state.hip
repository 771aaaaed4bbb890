// elo_model_state.hip -- the STATE MACHINE of a frame-to-model tracker on the device (include/elo.h, elo_model_begin /
// elo_model_advance): which slot of the ring a scan enters, whether the first frame 2 enters, and the re-basing of the held poses
// by the pose the fit returned.  The host decides nothing from device state, so a tracker step is a fixed launch sequence that a
// hipGraph records once.
//
// Two kernels.  model_enter_kernel: a streaming copy of one (H,W,3) image into the slot the state words name -- 16-byte accesses
// where the image is a whole number of them and both pointers are aligned, one float at a time otherwise; it READS the state.
// model_update_kernel: one workgroup, thread j owns row j of the poses: P_j <- T^-1 o P_j in double, the entered row <- the
// identity, every component rounded to float32 once into the copy the render reads, then thread 0 writes the state -- the only
// store to it anywhere, behind a barrier that follows every read of it.  No atomic.
#include "elo_pose_device.h"

namespace elo {
namespace {

constexpr int STATE_COPY_BLOCKS = 1024;                 // the copy walks its words with a grid stride beyond this
constexpr int STATE_UPDATE_BLOCK = ELO_WAVE;            // one wave: K <= ELO_MODEL_MAX_SCANS = 16 rows

// {next, held} inside their domain; a state outside it (memory nobody reset) moves nothing and is left as it is
__device__ __forceinline__ bool state_ok(int next, int held, int K) { return next >= 0 && next < K && held >= 0 && held <= K; }

// the slot a scan enters and the count it finds: an empty model takes its first frame 2 in slot 0 first (elo_model_begin)
__device__ __forceinline__ void state_entry(int next, int held, int K, int &slot, int &count)
{
    slot = held == 0 ? 1 % K : next;
    count = held == 0 ? 1 : held;
}

// begin = 1: slot 0, and only while the model is empty.  begin = 0: the slot of state_entry.  n: float4s (vec) or floats of one image
__global__ __launch_bounds__(ELO_BLOCK) void model_enter_kernel(float *ring, const float *image, const int *state, const int K,
                                                                const unsigned long n, const int vec, const int begin)
{
    const int next = state[0], held = state[1];
    if (!state_ok(next, held, K)) return;
    int slot = 0, count;
    if (begin) {
        if (held != 0) return;
    } else {
        state_entry(next, held, K, slot, count);
    }
    const unsigned long stride = (unsigned long)gridDim.x * ELO_BLOCK;
    unsigned long i = (unsigned long)blockIdx.x * ELO_BLOCK + threadIdx.x;
    if (vec) {
        float4 *d = reinterpret_cast<float4 *>(ring) + (unsigned long)slot * n;
        const float4 *s = reinterpret_cast<const float4 *>(image);
        for (; i < n; i += stride) d[i] = s[i];
    } else {
        float *d = ring + (unsigned long)slot * n;
        for (; i < n; i += stride) d[i] = image[i];
    }
}

__global__ __launch_bounds__(STATE_UPDATE_BLOCK) void model_update_kernel(double *poses64, float *poses32, int *state, const float *T,
                                                                          const int K)
{
    const int next = state[0], held = state[1];
    const bool ok = state_ok(next, held, K);
    int slot = 0, count = 0;
    if (ok) state_entry(next, held, K, slot, count);
    const int j = threadIdx.x;
    if (ok && j < K) {
        double *row = poses64 + j * 7;
        double p[7];
        if (j == slot) {
            p[0] = 1.0;
            for (int i = 1; i < 7; ++i) p[i] = 0.0;
        } else {
            // q_T normalised where it is used; a non-finite T is not special-cased: the rows become non-finite
            double w = T[0], x = T[1], y = T[2], z = T[3];
            const double n = sqrt(w * w + x * x + y * y + z * z);
            w /= n; x /= n; y /= n; z /= n;
            const double a = row[0], b = row[1], c = row[2], d = row[3];
            // conj(q_T) (x) q_j
            double q0 = w * a + x * b + y * c + z * d;
            double q1 = w * b - x * a - y * d + z * c;
            double q2 = w * c + x * d - y * a - z * b;
            double q3 = w * d - x * c + y * b - z * a;
            const double m = sqrt(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3);
            p[0] = q0 / m; p[1] = q1 / m; p[2] = q2 / m; p[3] = q3 / m;
            // R(q_T)^T (t_j - t_T)
            double R[9];
            pose_rotation(w, x, y, z, R);
            const double v0 = row[4] - (double)T[4], v1 = row[5] - (double)T[5], v2 = row[6] - (double)T[6];
            p[4] = R[0] * v0 + R[3] * v1 + R[6] * v2;
            p[5] = R[1] * v0 + R[4] * v1 + R[7] * v2;
            p[6] = R[2] * v0 + R[5] * v1 + R[8] * v2;
        }
        for (int i = 0; i < 7; ++i) {
            row[i] = p[i];
            poses32[j * 7 + i] = (float)p[i];
        }
    }
    __syncthreads();                                    // every thread has read the state
    if (ok && j == 0) {
        state[0] = (slot + 1) % K;
        state[1] = count + 1 < K ? count + 1 : K;
    }
}

void launch_enter(float *ring, const float *image, const int *state, int K, long cells, int begin, hipStream_t s)
{
    const int vec = (cells % 4 == 0 && aligned(ring, 16) && aligned(image, 16)) ? 1 : 0;
    const unsigned long n = vec ? (unsigned long)cells * 3 / 4 : (unsigned long)cells * 3;
    const unsigned long want = (n + ELO_BLOCK - 1) / ELO_BLOCK;
    hipLaunchKernelGGL(model_enter_kernel, dim3((unsigned)(want < STATE_COPY_BLOCKS ? want : STATE_COPY_BLOCKS)), dim3(ELO_BLOCK), 0, s,
                       ring, image, state, K, n, vec, begin);
}

}  // namespace
}  // namespace elo

using namespace elo;

extern "C" int elo_model_begin(const elo_model_begin_args *a, elo_stream_t stream)
{
    const char *who = "elo_model_begin";
    ELO_REQUIRE(a, who, "null argument block");
    ELO_REQUIRE(a->K >= 1 && a->K <= ELO_MODEL_MAX_SCANS, who, "K is 1 .. ELO_MODEL_MAX_SCANS");
    ELO_REQUIRE(a->H >= 3, who, "a fit's normal needs three rows: H >= 3");
    ELO_REQUIRE(image_sizes_ok(a->K, a->H, a->W, 3), who, "bad sizes");    // one image as a fit takes it, the K of the ring as the render does
    ELO_REQUIRE(a->ring && a->state && a->first, who, "null ring, state or image");
    const long cells = (long)a->H * a->W;
    ELO_REQUIRE(!ranges_meet(a->ring, (size_t)a->K * cells * 12, a->first, (size_t)cells * 12), who, "first overlaps ring");
    launch_enter(a->ring, a->first, a->state, a->K, cells, 1, (hipStream_t)stream);
    return check_launch(who);
}

extern "C" int elo_model_advance(const elo_model_advance_args *a, elo_stream_t stream)
{
    const char *who = "elo_model_advance";
    ELO_REQUIRE(a, who, "null argument block");
    ELO_REQUIRE(a->K >= 1 && a->K <= ELO_MODEL_MAX_SCANS, who, "K is 1 .. ELO_MODEL_MAX_SCANS");
    ELO_REQUIRE(a->H >= 3, who, "a fit's normal needs three rows: H >= 3");
    ELO_REQUIRE(image_sizes_ok(a->K, a->H, a->W, 3), who, "bad sizes");    // one image as a fit takes it, the K of the ring as the render does
    ELO_REQUIRE(a->ring && a->state && a->scan, who, "null ring, state or image");
    ELO_REQUIRE(a->poses64 && a->poses32 && a->T, who, "null poses or T");
    ELO_REQUIRE(aligned(a->poses64, 8), who, "poses64 must be 8-byte aligned");
    const long cells = (long)a->H * a->W;
    ELO_REQUIRE(!ranges_meet(a->ring, (size_t)a->K * cells * 12, a->scan, (size_t)cells * 12), who, "scan overlaps ring");
    hipStream_t s = (hipStream_t)stream;
    launch_enter(a->ring, a->scan, a->state, a->K, cells, 0, s);
    hipLaunchKernelGGL(model_update_kernel, dim3(1), dim3(STATE_UPDATE_BLOCK), 0, s, a->poses64, a->poses32, a->state, a->T, a->K);
    return check_launch(who);
}
