/*
 * include/elo.h -- C ABI of libelo_hip.so, the MI355X (gfx950) implementation of
 * EfficientLO-Net's projection-aware 3D feature hot path.
 *
 * Plain pointers and sizes only (no torch / TF types).  Every pointer is a
 * DEVICE pointer on the current HIP device unless stated otherwise; `stream`
 * is a hipStream_t passed as void* (NULL = the null stream).  Nothing here
 * allocates, synchronises or keeps global state, so every entry point is
 * re-entrant and safe to call while a hipGraph is being captured on `stream`.
 * All entry points return ELO_OK or a negative elo_status; elo_last_error()
 * gives the message for the calling thread.
 *
 * Each entry point names the reference interface it replaces
 * (paths relative to the upstream repository IRMVLab/EfficientLO-Net).
 */
#ifndef ELO_H_
#define ELO_H_

#ifdef __cplusplus
extern "C" {
#endif

typedef void *elo_stream_t; /* hipStream_t */

typedef enum elo_status {
    ELO_OK = 0,
    ELO_ERR_ARG = -1,    /* null pointer / non-positive size / inconsistent shapes      */
    ELO_ERR_LIMIT = -2,  /* outside the supported envelope (e.g. kernel window > 5000)  */
    ELO_ERR_LAUNCH = -3  /* hipGetLastError() after the launch                          */
} elo_status;

int elo_abi_version(void);          /* bumps when a struct below changes layout */
int elo_dense_f32(void);            /* 1: built with -DELO_DENSE_F32 (elo_dense.w_packed holds fp32 weights), 0: fp16 hi|lo */
const char *elo_last_error(void);   /* thread-local, never NULL                 */
/* Range check of the fp16-split operands (a debugging switch, process-wide; also ELO_RANGE_CHECK=1 in the environment):
 * while enabled, the fused kernels run instances that COUNT every activation / gathered feature with |x| >= 65504 or
 * NaN on its way into a matrix-core operand (where the fp16 split saturates instead of raising).
 * elo_range_check(1 / 0) switches it and returns the previous setting (-1: only query);
 * elo_range_violations() takes the count since the last call out of the device counter with ONE atomic exchange (a
 * violation recorded meanwhile by a checked launch on another stream is kept for the next call), synchronises `stream`
 * and returns it.  That counter is process-wide; a caller with several streams in flight gives every fused argument block its
 * own word instead (ABI 26: `range_counter` in elo_setconv_args / elo_mlp_args / elo_cv1_args / elo_cv2_args -- the checked instances
 * add there when it is not NULL): efficientlo-net_amd/model.py bakes a lane's word into the lane's checked graph, so a violation is
 * that lane's alone. */
int elo_range_check(int enable);
int elo_range_violations(unsigned long long *count, elo_stream_t stream);

/* Host runtime: one step of a captured forward (a "lane": a hipGraphExec_t with fixed input / output buffers) as one call --
 * if bytes != 0 a device-to-device hipMemcpyAsync(dst <- src) of the lane's input, then hipGraphLaunch, both on `stream`.
 * graph_exec: the hipGraphExec_t (torch: CUDAGraph.raw_cuda_graph_exec()).
 * ORDERING (ABI 23; the contract replaced is the reference's synchronous sess.run(feed_dict=...), main.py:372-381): with
 * order_event != NULL (a hipEvent_t the lane owns) the call records it on `producer` -- the stream whose work so far produced
 * src, or wrote the lane's input buffer in place (0 = the null stream) -- and makes `stream` wait for it before the copy and
 * the graph, so a caller may submit right behind the kernels that fill src (a producer found idle by hipStreamQuery has nothing
 * to wait for: no event is recorded then).  order_event == NULL: no ordering -- the caller
 * guarantees src (or the in-place input) is complete before `stream` reaches this step (inputs resident and synchronised,
 * or produced on `stream` itself).
 * LIFETIME: the caller keeps src alive until `stream` has run the copy, as with any asynchronous copy (torch: record_stream).
 * device >= 0: the lane's device; made current for the call when the calling thread's current device differs (and put back). */
int elo_graph_submit(void *graph_exec, elo_stream_t stream, void *dst, const void *src, unsigned long bytes,
                     elo_stream_t producer, void *order_event, int device);

/* The library's tuning: every choice of KERNEL FORM that is not a function of the arguments alone, as ONE value.  The library
 * itself reads no environment variable; the host fills this once (efficientlo-net_amd/_lib.py maps the ELO_* variables named
 * below onto it when it loads the library) and may change it between launches.  A form baked into a captured hipGraph stays
 * what it was at capture time: the host hashes the tuning into its capture generation and refuses to replay a graph under
 * another tuning (efficientlo-net_amd/model.py).  Every form of an entry point computes the same function (bit for bit, or to
 * fp32 summation order where a comment says so): these are speed choices.  The elo_debug_* hooks further down are
 * single-field shorthands for elo_set_tuning. */
typedef struct elo_tuning {
    int chain_forms;            /* 1: the register-resident ("chain") kernels may be taken, 0: tile kernels only   [ELO_CV1_RR]            */
    int narrow_mfma;            /* narrow set-conv layers: 0 VALU kernel, 1 matrix cores for 19 -> 16 -> 16 -> 32  [ELO_SETCONV_NARROW_MFMA] */
    int range_check;            /* 1: the fused kernels run their operand-range-checked instances (elo_range_check) [ELO_RANGE_CHECK]       */
    int select_dense_waves;     /* elo_fused_conv_select_k_dense: 4 / 8 / 16 waves per tile, 0 = by grid size     [ELO_SELECT_DENSE_WAVES]  */
    int random_dense_rows;      /* elo_fused_conv_random_k_dense: 2 / 4 rows per tile, 0 = by grid size            [ELO_DENSE_ROWS]          */
    long setconv_chain_rows;    /* rows per launch from which elo_setconv_fused2 takes the chain form; -1: 20 000 (below batch
                                   ELO_THROUGHPUT_BATCH: 100 000 until round 5)                                    [ELO_SETCONV_RR_ROWS]     */
    long mlp_chain_rows;        /* ... elo_mlp_fused2; -1: 2048 / 8192                                            [ELO_MLP_RR_ROWS]         */
    long small_tile_units;      /* 16-row tiles while 32-row tiles would give fewer workgroups than this (64)      [ELO_SMALL_TILE_UNITS]    */
    int pool_wave;              /* elo_masked_softmax_pool with C = 64, K <= 32: 1 (default) one WAVE per point, one or two light nontemporal
                                   loads per lane and tensor (HBM-cold streaming: tools/micro/hbm_probe.hip), 0 the quarter-wave form  [ELO_POOL_WAVE] */
} elo_tuning;
int elo_get_tuning(elo_tuning *out);             /* what the launchers read now: elo_set_tuning's value with pending elo_debug_* overrides on top */
int elo_get_tuning_base(elo_tuning *out);        /* what elo_set_tuning installed (no elo_debug_* override): the value a read-modify-write starts from */
int elo_set_tuning(const elo_tuning *in);      /* ELO_ERR_ARG on a field outside its domain (nothing is changed then) */

/* ------------------------------------------------------------------------- *
 * Neighbour grouping on the H x W range image.
 *
 * Replaces the launchers
 *   void FusedConvRandomKLauncher(int batch_size, int H, int W, int npoints,
 *        int kernel_size_H, int kernel_size_W, int K, int flag_copy,
 *        float distance, int stride_h, int stride_w, const float *xyz1,
 *        const float *xyz2, const int *idx_n2, const int *random_hw,
 *        int *selected_bhw_idx, float *valid_idx, float *valid_in_dis_idx,
 *        float *selected_mask, int small_h, int small_w)
 *     -- tf_ops/2d_conv_random_k/fused_conv_g.cu:162, declared fused_conv.cpp:73
 *   void FusedConvSelectKLauncher(... same 21 arguments ...)
 *     -- tf_ops/2d_conv_select_k/fused_conv_g.cu:215
 * and the four cudaMemset zero-fills of the op glue (fused_conv.cpp:154-166):
 * the kernels write every element of every output, so the caller passes
 * uninitialised buffers.
 *
 * Shapes (row-major, contiguous):
 *   xyz1 (batch,H,W,3) f32        centres' grid
 *   xyz2 (batch,H2,W2,3) f32      queried grid, H2=ceil(H/stride_h), W2=ceil(W/stride_w)
 *   idx_n2 (batch,npoints,2) i32  (h,w) of each centre in xyz1
 *   random_hw (kernel_h*kernel_w) i32   visiting order, a permutation of 0..KT-1
 *   selected_bhw_idx (batch,npoints,K,3) i32   OUT
 *   valid_idx, valid_in_dis_idx (batch,npoints,KT,1) f32   OUT, either may be NULL
 *        (no caller in the model reads them: pointnet_util.py:49,106,197,272)
 *   selected_mask (batch,npoints,K,1) f32   OUT
 * Preconditions mirrored from the op (fused_conv.cpp:78-123) and from the
 * kernel's own bounds: sizes > 0, flag_copy in {0,1}, KT <= 5000
 * (fused_conv_g.cu:42-43), kernel_w/2 <= W2 (single cylindrical wrap, :89-97),
 * H2 < 32768, W2 < 65536.  random_hw being a permutation is NOT checked.
 * ------------------------------------------------------------------------- */
typedef struct elo_group_args {
    int batch, H, W;            /* xyz1 grid                               */
    int H2, W2;                 /* xyz2 grid ("small_h", "small_w")        */
    int npoints;
    int kernel_h, kernel_w;
    int K;
    int flag_copy;
    float distance;
    int stride_h, stride_w;
    const float *xyz1;
    const float *xyz2;
    const int *idx_n2;
    const int *random_hw;
    int *selected_bhw_idx;
    float *valid_idx;           /* nullable */
    float *valid_in_dis_idx;    /* nullable */
    float *selected_mask;
} elo_group_args;

int elo_fused_conv_random_k(const elo_group_args *a, elo_stream_t stream);
int elo_fused_conv_select_k(const elo_group_args *a, elo_stream_t stream);
/* elo_fused_conv_random_k for the call shape "EVERY pixel of xyz1 is a centre, in row-major order" -- idx_n2 =
 * get_hw_idx(...) (utils/pointnet_util.py:23-30), npoints == H*W: the cost-volume stage 2 and set-upconv calls
 * (:106-108, :272-274) and BASELINE configs[0].  a->idx_n2 is IGNORED (may be NULL); same outputs bit for bit.
 * The window union of a tile of 4 x 64 centres is staged once in LDS and every centre walks its window from there.
 * ELO_ERR_LIMIT when the window / K do not fit the 64 KB tile: call the general entry point. */
int elo_fused_conv_random_k_dense(const elo_group_args *a, elo_stream_t stream);
/* elo_fused_conv_select_k for the same call shape (every pixel a centre, row-major; a->idx_n2 ignored) with K <= 7,
 * flag_copy == 0 and a window of at most 512 slots -- the select-k of the refinement cost volumes
 * (utils/pointnet_util.py:49-51: K = 6 of 5x15 / 7x25 / 11x41).  The window union of 64 consecutive centres of a grid row
 * is staged once in LDS; a lane per centre walks it (no visiting order needed: the K smallest distances in increasing
 * order are unique unless two of them are EQUAL, and exactly then the centre is redone by the wave-per-centre form in
 * the reference's visiting order).  Same outputs bit for bit.  ELO_ERR_LIMIT outside those bounds. */
int elo_fused_conv_select_k_dense(const elo_group_args *a, elo_stream_t stream);
/* Does a window fit the dense forms AS THIS BUILD sizes their LDS tiles?  1 / 0; host arithmetic only (no device, no stream
 * work, elo_last_error untouched: legal during graph capture).  A host that picks a grouping entry point asks here instead of
 * restating the tile geometry.  random_k: the smaller (2 x 64 centres) tile fits, i.e. elo_fused_conv_random_k_dense does not
 * answer ELO_ERR_LIMIT.  select_k: K <= 7, flag_copy == 0, at most 512 slots and the form's largest configuration (16 waves
 * per tile, both prefix masks) fits -- stricter than the launcher, which sizes LDS for the outputs and tile count of the call. */
int elo_fused_conv_random_k_dense_fits(int kernel_h, int kernel_w, int K, int stride_h, int stride_w);
int elo_fused_conv_select_k_dense_fits(int kernel_h, int kernel_w, int K, int flag_copy, int stride_h, int stride_w);
/* debugging hook: force 4, 8 or 16 waves per tile in elo_fused_conv_select_k_dense (0 = chosen by grid size; also
 * ELO_SELECT_DENSE_WAVES); returns the previous setting */
int elo_debug_select_dense_waves(int waves);
/* WHICH KERNEL FORM the four grouping entry points take for an argument block.  Host arithmetic only: nothing is launched and no
 * memory behind the block's pointers is read (only their being NULL or not); the two dense queries also read the current
 * elo_tuning (random_dense_rows / select_dense_waves).  Each entry point switches on the same function as its query, so the answer
 * is what a launch with this block takes.  Return: an enumerator below, or the negative elo_status with which the entry point
 * would refuse the block.  All forms of an entry point compute the same outputs bit for bit.
 *   elo_fused_conv_random_k: G<lanes per centre>U<window slots per lane and step>: up to 16 slots G16U1, up to 32 G32U1, above
 *     that G16U4 for K <= 16 and G32U2 for a larger K.
 *   elo_fused_conv_random_k_dense: ROWS<rows of 64 centres per workgroup>: the forced elo_tuning.random_dense_rows, else 4 from
 *     1024 four-row tiles on; 2 wherever the four-row tile does not fit 64 KB of LDS (ELO_ERR_LIMIT where 2 rows do not either).
 *   elo_fused_conv_select_k: ELO_SELECT_FORM(store, path).  store: REG<J> -- the window in J registers per lane (flag_copy 0 and
 *     K <= 8 with at most 512 slots, or K <= 32 with at most 192; J = 2 up to 128 slots, 3 up to 192, else 8) -- or LDS<waves per
 *     block> (4 while 4 * (order + 4 waves' window state) fits 64 KB: up to 1820 slots; 2 up to 3276; else 1).  path (REG only; the
 *     LDS forms answer ELO_SELECT_PATH_SWAPS): with rounds = min(K, slots), SMALL for rounds <= 7 (candidates below the largest of
 *     eight lane-group minima, ranked), MID for J <= 3 (candidates below the (rounds+1)-th lane minimum, ranked; the whole window
 *     ranked when that gives up), ROUNDS for J = 8 with K = 8 (the swap rounds in registers).  SMALL and MID fall back to the swap
 *     rounds on an exact tie that touches the selected elements or the first one left out; a centre at the origin is zero-filled
 *     by every form.
 *   elo_fused_conv_select_k_dense: ELO_SELECT_DENSE_FORM(waves, counts): W4 / W8 / W16 waves per 64-centre tile (the forced
 *     elo_tuning.select_dense_waves, else by the tile count), counts = 1 where valid_idx or valid_in_dis_idx is asked for. */
enum { ELO_RANDOM_G16U1 = 0, ELO_RANDOM_G32U1 = 1, ELO_RANDOM_G16U4 = 2, ELO_RANDOM_G32U2 = 3 };
enum { ELO_RANDOM_DENSE_ROWS2 = 0, ELO_RANDOM_DENSE_ROWS4 = 1 };
enum { ELO_SELECT_REG2 = 0, ELO_SELECT_REG3 = 1, ELO_SELECT_REG8 = 2, ELO_SELECT_LDS4 = 3, ELO_SELECT_LDS2 = 4, ELO_SELECT_LDS1 = 5 };
enum { ELO_SELECT_PATH_SWAPS = 0, ELO_SELECT_PATH_SMALL = 1, ELO_SELECT_PATH_MID = 2, ELO_SELECT_PATH_ROUNDS = 3 };
#define ELO_SELECT_FORM(store, path) ((store) | (path) << 4)
enum { ELO_SELECT_DENSE_W4 = 0, ELO_SELECT_DENSE_W8 = 1, ELO_SELECT_DENSE_W16 = 2 };
#define ELO_SELECT_DENSE_FORM(waves, counts) ((waves) | (counts) << 4)
int elo_fused_conv_random_k_form(const elo_group_args *a);
int elo_fused_conv_select_k_form(const elo_group_args *a);
int elo_fused_conv_random_k_dense_form(const elo_group_args *a);
int elo_fused_conv_select_k_dense_form(const elo_group_args *a);

/* ------------------------------------------------------------------------- *
 * Feature path: fused gather / encode / pool kernels.  These replace chains of
 * stock TF ops (tf.gather_nd, tf.tile, tf.concat, tf.where, tf.nn.softmax,
 * tf.reduce_max/sum, tf.scatter_nd, ...) in utils/pointnet_util.py and
 * model_util.py; each comment names the lines it covers.  "idx" is always the
 * (batch,npoints,K,3) int32 (b,h,w) tensor produced by the grouping ops and
 * "mask" its (batch,npoints,K) float 0/1 mask.  Features are fp32, row-major,
 * channels last.  A masked slot gathers idx (0,0,0) and is multiplied by 0,
 * exactly like `tf.gather_nd(...) * mask` (Appendix A.4 of SURVEY.md).
 * ------------------------------------------------------------------------- */

/* set-conv / set-upconv input:  out[b,n,k,:] = [ src_xyz[idx]*m - centre_xyz[b,n] , src_feat[idx]*m ]
 * utils/pointnet_util.py:203-213 (down_conv) and :277-284 (up_conv). */
typedef struct elo_group_concat_args {
    int batch, npoints, K;
    int H2, W2, C;                /* source grid and its feature channels */
    const float *centre_xyz;      /* (batch,npoints,3) */
    const float *src_xyz;         /* (batch,H2,W2,3)   */
    const float *src_feat;        /* (batch,H2,W2,C)   */
    const int *idx;
    const float *mask;
    float *out;                   /* (batch,npoints,K,3+C) */
} elo_group_concat_args;
int elo_group_concat(const elo_group_concat_args *a, elo_stream_t stream);

/* out[b,n,c] = max_k x[b,n,k,c] * mask[b,n,k]     utils/pointnet_util.py:224-230, :295-298 */
typedef struct elo_masked_maxpool_args {
    int batch, npoints, K, C;
    const float *x;               /* (batch,npoints,K,C) */
    const float *mask;
    float *out;                   /* (batch,npoints,C)   */
} elo_masked_maxpool_args;
int elo_masked_maxpool(const elo_masked_maxpool_args *a, elo_stream_t stream);

/* Storage type of the FEATURE tensors of the three cost-volume kernels below (fields typed `void *`): fp32, or fp16
 * storage with fp32 arithmetic (BASELINE configs[2]; SURVEY.md section 8(d): s = 2).  Geometry inputs (xyz), indices
 * and masks are always fp32 / int32. */
enum { ELO_F32 = 0, ELO_F16 = 1 };

/* Cost volume, stage 1 (point -> patch of frame 2), utils/pointnet_util.py:54-66:
 *   q = xyz2[idx]*m, diff = q - p, euc = sqrt(sum(diff^2) + 1e-20)
 *   out[b,n,k,:] = [ p(3), q(3), diff(3), euc(1), feat1[b,n](C), feat2[idx]*m (C) ]      (10+2C channels) */
typedef struct elo_cv_encode1_args {
    int batch, npoints, K;
    int H2, W2, C;
    const float *xyz1;            /* (batch,npoints,3)  warped frame-1 points      */
    const void *feat1;            /* (batch,npoints,C)        dtype                */
    const float *xyz2;            /* (batch,H2,W2,3)                               */
    const void *feat2;            /* (batch,H2,W2,C)          dtype                */
    const int *idx;
    const float *mask;
    void *out;                    /* (batch,npoints,K,10+2C)  dtype                */
    int dtype;                    /* ELO_F32 / ELO_F16 */
} elo_cv_encode1_args;
int elo_cv_encode1(const elo_cv_encode1_args *a, elo_stream_t stream);

/* Cost volume, stage 2 (patch -> patch inside frame 1), utils/pointnet_util.py:110-129:
 *   g = xyz1_grid[idx]*m, diff = g - p, euc as above
 *   xyz_cat[b,n,k,:] = [ p, g, diff, euc ]                       (10 channels)
 *   rest[b,n,k,:]    = [ feat1[b,n] (C), cost[idx]*m (Cc) ]      (C+Cc channels)
 * (the reference concatenates conv(xyz_cat) in front of `rest`; the caller
 *  does that product as a split GEMM, see pointnet_util.cost_volume) */
typedef struct elo_cv_encode2_args {
    int batch, npoints, K;
    int H, W, C, Cc;              /* xyz1 grid (npoints == H*W), feat1 and cost channels */
    const float *xyz1;            /* (batch,H,W,3)  */
    const void *feat1;            /* (batch,H,W,C)   dtype */
    const void *cost;             /* (batch,H,W,Cc)  dtype: stage-1 output */
    const int *idx;
    const float *mask;
    void *xyz_cat;                /* (batch,npoints,K,10)    dtype */
    void *rest;                   /* (batch,npoints,K,C+Cc)  dtype */
    int dtype;                    /* ELO_F32 / ELO_F16 */
} elo_cv_encode2_args;
int elo_cv_encode2(const elo_cv_encode2_args *a, elo_stream_t stream);

/* out[b,n,c] = sum_k softmax_k( mask==1 ? logits : -1e10 )[k,c] * values[b,n,k,c]
 * utils/pointnet_util.py:92-98 and :137-146.  `values` rows may be a channel
 * slice of a wider tensor: element (row,c) is values[row*values_stride + c]. */
typedef struct elo_softmax_pool_args {
    int batch, npoints, K, C;
    const void *logits;           /* (batch,npoints,K,C)  dtype */
    const void *values;           /*                      dtype */
    int values_stride;            /* elements between consecutive (b,n,k) rows, >= C */
    const float *mask;
    void *out;                    /* (batch,npoints,C)    dtype; the softmax itself runs in fp32 */
    int dtype;                    /* ELO_F32 / ELO_F16 */
} elo_softmax_pool_args;
int elo_masked_softmax_pool(const elo_softmax_pool_args *a, elo_stream_t stream);

/* WHICH KERNEL the three entry points above launch for an argument block (host-only queries: nothing is launched, no tensor pointer is
 * dereferenced -- only the pointers' VALUES are read, for their alignment -- and elo_masked_softmax_pool_form also reads the current
 * elo_tuning.pool_wave).  Each entry point switches on the same function, so the answer is what a launch with these arguments takes.
 * All forms of an entry point compute the same function; the storage type (fp32 / fp16 instance) is the block's `dtype`.
 * Return: one of the enumerators below, or the negative elo_status with which the entry point would refuse the block (bad sizes, a
 * NULL pointer, fp16 storage with a channel count or an alignment its vector forms cannot take: fp16 has no scalar form).
 * With batch == 0 the entry points launch nothing and the answer is the scalar enumerator.
 *   elo_cv_encode1: VEC<R> / COL<R> / STAGED<R> work on R-row workgroups (R by the row count batch*npoints*K: 32 below 64 Ki rows,
 *     64 from there, 128 above 512 Ki).  STAGED (the tile built in LDS, 16-byte accesses): >= 8192 rows, 16-byte aligned feature
 *     tensors, C a multiple of 16 bytes' worth of elements, and the tile within 40 KB (128 rows, else 64).  COL (a thread owns a slot
 *     column): where whole rows tile the 256 threads with at most 1/16 of them idle.  VEC otherwise; SCALAR (fp32 only): odd C,
 *     C >= 500, K >= 32768 or feature tensors off 8-byte alignment.
 *   elo_cv_encode2: VEC<R> with C and Cc multiples of 16 bytes' worth of elements and 16-byte aligned tensors, else SCALAR (fp32 only).
 *   elo_masked_softmax_pool: WAVE<J> (fp32, C = 64, K <= 32, 16-byte aligned, pool_wave on; J = 1, 2, 4, 8 >= ceil(K / 4) neighbour rows
 *     per lane group), VEC6 / VEC4 (C % 4 == 0, 256 % (C / 4) == 0, C <= 1024, values_stride % 4 == 0, tensors aligned to four elements;
 *     six rows in flight when K % 6 == 0, else four), SCALAR (fp32 only) otherwise. */
enum { ELO_ENCODE1_SCALAR = 0, ELO_ENCODE1_VEC32 = 1, ELO_ENCODE1_VEC64 = 2, ELO_ENCODE1_VEC128 = 3, ELO_ENCODE1_COL64 = 4,
       ELO_ENCODE1_COL128 = 5, ELO_ENCODE1_STAGED128 = 6, ELO_ENCODE1_STAGED64 = 7 };
enum { ELO_ENCODE2_SCALAR = 0, ELO_ENCODE2_VEC32 = 1, ELO_ENCODE2_VEC64 = 2, ELO_ENCODE2_VEC128 = 3 };
enum { ELO_POOL_SCALAR = 0, ELO_POOL_VEC6 = 1, ELO_POOL_VEC4 = 2, ELO_POOL_WAVE1 = 3, ELO_POOL_WAVE2 = 4, ELO_POOL_WAVE4 = 5,
       ELO_POOL_WAVE8 = 6 };
int elo_cv_encode1_form(const elo_cv_encode1_args *a);
int elo_cv_encode2_form(const elo_cv_encode2_args *a);
int elo_masked_softmax_pool_form(const elo_softmax_pool_args *a);

/* Fresh visiting orders per replay of a captured forward (tf.random_shuffle inside every operator on every sess.run:
 * utils/pointnet_util.py:45,104,193,270).  All order tensors of a forward are slices of `flat` (their decoded (dh, dw)
 * forms, elo_group_spec.decoded_hw, slices of `decoded`); `pool` holds `versions` pre-drawn contents of `flat`.  One
 * launch copies version (*cursor % versions) into flat, decodes it and advances the device-side cursor -- captured at the
 * head of a hipGraph it gives every replay its own orders at unchanged addresses.
 *   table (n_entries,4) i32: (offset, KT, kernel_h, kernel_w) per order tensor; entry_of (total) i32: slot -> entry. */
typedef struct elo_perm_refresh_args {
    const int *pool;            /* (versions, total) */
    int versions, total;
    int *cursor;                /* (1) device counter */
    int *flat, *decoded;        /* (total) each */
    const int *entry_of;        /* (total) */
    const int *table;           /* (n_entries, 4) */
    int n_entries;
} elo_perm_refresh_args;
int elo_perm_refresh(const elo_perm_refresh_args *a, elo_stream_t stream);

/* model_util.py:319-343 softmax_valid: per batch element, softmax over the
 * VALID points (xyz != (0,0,0)) per channel, out[b,0,c] = sum_n softmax*feature.
 * Two launches: `parts` blocks per batch element reduce slices of the point axis
 * with an online softmax, a second kernel merges the partials.
 * scratch: 3 * batch * ELO_SV_MAX_PARTS * C floats, laid out (3, batch, ELO_SV_MAX_PARTS, C): [maximum | denominator |
 * weighted sum] of slice `part` of batch element b (the partial launch writes at most 64 slices; a row-wise MLP launch that
 * computes the partial sums itself -- elo_mlp_args.sv_* -- one slice per row tile, up to ELO_SV_MAX_PARTS). */
#define ELO_SV_MAX_PARTS 512
typedef struct elo_softmax_valid_args {
    int batch, npoints, C;
    const float *feature;         /* (batch,npoints,C) */
    const float *weight;          /* (batch,npoints,C) */
    const float *xyz;             /* (batch,npoints,3): a point is valid unless all three are exactly 0 */
    float *out;                   /* (batch,1,C); all-invalid batch element -> 0 */
    float *scratch;
    float *stats;                 /* (batch,2,C) OUT or NULL: [maximum | denominator] of the masked softmax per channel (what
                                     elo_softmax_valid_backward needs besides `out`; denominator 0 = no valid point) */
} elo_softmax_valid_args;
int elo_softmax_valid(const elo_softmax_valid_args *a, elo_stream_t stream);

/* Pose head of one pyramid level, inference form (pwclo_model.py:194-208 at l3,
 * :262-280 / :338-356 / :406-425 at the refinement levels), fused:
 *   f      = softmax_valid(feature, weight, xyz)                       (B,C)
 *   big    = f @ W_big + b_big                                         (B,hidden)   conv1d, no activation
 *   q_det  = normalise(big @ W_q + b_q),  t_det = big @ W_t + b_t      normalise: q / (sqrt(sum q^2 + 1e-10) + 1e-10)
 *   coarse == NULL :  q = q_det, t = t_det                             (l3)
 *   else           :  q = q_det (x) q_coarse,
 *                     t = (q_det (x) [0,t_coarse] (x) q_det^-1)[1:] + t_det
 *   q_norm = normalise(q)                                              (:427-430)
 * Weights are row-major (in,out).  Dropout (training only) is not part of this kernel.
 * scratch: as elo_softmax_valid. */
typedef struct elo_pose_head_args {
    int batch, npoints, C, hidden;
    const void *feature, *weight; /* (batch,npoints,C) feat_dtype */
    const float *xyz;
    const float *W_big, *b_big;   /* (C,hidden), (hidden) */
    const float *W_q, *b_q;       /* (hidden,4), (4)      */
    const float *W_t, *b_t;       /* (hidden,3), (3)      */
    const float *q_coarse;        /* (batch,4) or NULL    */
    const float *t_coarse;        /* (batch,3) or NULL    */
    float *q, *t, *q_norm;        /* (batch,4), (batch,3), (batch,4) OUT */
    float *scratch;
    float *pose7;                 /* (batch,7) [q_norm | t] OUT, or NULL: the pose as one row a caller can log */
    /* Optional side job for the workgroups of the first launch: clear the buffers of the elo_warp_project call
     * that will consume this pose (its scratch min-range words and its two outputs), so that call can set
     * `prepared` and skip its own init launch.  clear_scratch == NULL: no side job. */
    unsigned *clear_scratch;      /* the warp call's `scratch`: its first clear_cells + 4*batch words are set to 0x7f7f7f7f */
    float *clear_xyz;             /* its out_xyz  (clear_cells*3 floats  <- 0) */
    void *clear_feat;             /* its out_feat (clear_cells*clear_C elements of feat_dtype <- 0), NULL when clear_C == 0 */
    long clear_cells;             /* batch*H*W of that call */
    int clear_C;
    int feat_dtype;               /* ELO_F32 / ELO_F16: storage of feature, weight and of clear_feat (C, clear_C even for fp16) */
    /* pose7 as a RING, for a launch that is replayed from a captured graph (fixed pointers): with pose7_slots > 1 and
     * pose7_cursor != NULL, pose7 is (pose7_slots,batch,7); batch element b's row goes to slot pose7_cursor[b] % pose7_slots
     * and pose7_cursor[b] is incremented (by the one thread that writes the row).  A stream of frame pairs then needs no
     * copy-out per pair: the caller drains the ring every pose7_slots replays (and may reset the cursors to 0). */
    int pose7_slots;
    unsigned *pose7_cursor;       /* (batch) or NULL */
    /* Optional side job for the LAST launch of a captured forward (the l0 pose head): load the next pooled set of window
     * visiting orders (elo_perm_refresh semantics) once this pose is written -- the NEXT replay of the graph then walks
     * fresh orders without a launch of its own.  next_orders.pool == NULL: no side job. */
    elo_perm_refresh_args next_orders;
    /* ready_parts > 0: the partial sums of softmax_valid are ALREADY in `scratch`, ready_parts slices per batch element, written
     * by the launch that produced `feature` / `weight` (elo_mlp_fused / elo_mlp_fused2 with sv_scratch == scratch;
     * elo_mlp_sv_parts gives the count): no partial-sums launch here -- one launch less per pyramid level.  The clear_* buffers
     * are then not cleared by this call (elo_mlp_args.clear_* did it). */
    int ready_parts;
} elo_pose_head_args;
int elo_pose_head(const elo_pose_head_args *a, elo_stream_t stream);

/* Pose warp + spherical re-projection.
 *   warp : p' = ((q (x) [0,p]) (x) q^-1)[1:] + t, zeroed where p == (0,0,0)
 *          (pwclo_model.py:213-227; model_util.py:17-69), skipped when q == NULL
 *   project : model_util.py:181-292 ProjectPC2SphericalRing -- per point
 *          r = |p'|, col = int((pi - atan2(y,x)) / az_res), row = H - int(asin(z/r)/vert_res + vert_off)
 *          (NaN -> 0, the GPU float->int convention), both clipped; the point(s)
 *          with the minimum r of a cell are SUMMED into it (tf.scatter_nd adds).
 * az_res / vert_res / vert_off are computed by the caller exactly as
 * model_util.py:189-200 does (python double -> float32).
 * scratch: (batch*H*W) + 4*batch + 2*(batch*npoints) 32-bit device words
 *          [min range per cell | 4 zero-point flags per image | cell of point | range bits of point]. */
typedef struct elo_warp_project_args {
    int batch, npoints, C;        /* C may be 0 (no features) */
    int H, W;
    float az_res, vert_res, vert_off;
    const float *xyz;             /* (batch,npoints,3) */
    const void *feat;             /* (batch,npoints,C) feat_dtype, or NULL */
    const float *q;               /* (batch,4) or NULL = no warp */
    const float *t;               /* (batch,3) */
    float *warped;                /* (batch,npoints,3) OUT (nullable when q == NULL) */
    float *out_xyz;               /* (batch,H,W,3) OUT */
    void *out_feat;               /* (batch,H,W,C) feat_dtype OUT, or NULL */
    unsigned *scratch;
    int prepared;                 /* 1: scratch / out_xyz / out_feat were cleared by elo_pose_head (clear_*): no init launch */
    int feat_dtype;               /* ELO_F32 / ELO_F16 storage of feat / out_feat (fp16: C even; duplicates are summed with
                                     packed fp16 atomics, i.e. rounded per addition) */
} elo_warp_project_args;
int elo_warp_project(const elo_warp_project_args *a, elo_stream_t stream);

/* Raw-cloud input stage: PreProcess (model_util.py:346-445; the point part) + the input ProjectPC2SphericalRing of
 * BOTH frames (pwclo_model.py:54-67) in three launches (clear, per-point pass, scatter).  Per point p of frame f:
 *   valid = any(p != 0);  p4 = [p, 1], zeroed (all four) where sqrt(x^2 + y^2) > crop_xy  (model_util.py:380-383);
 *   p4 <- T_trans[b] . p4  when aug_frame[b] == f  (:392-394, :408-410);  out = p4[:3] * valid  (:421-422)
 * then the projection of elo_warp_project (no warp).  Outputs are STACKED over frames, frame 1 of every batch element
 * first: points (2*batch, npoints, 3), out_xyz (2*batch, H, W, 3) -- the layout the Siamese pyramid runs as one batch.
 * q_gt / t_gt of PreProcess (a 4x4 product and an Euler round trip per batch element) are elo_preprocess_gt below.
 * scratch: (2*batch*H*W) + 4*(2*batch) + 2*(2*batch*npoints) 32-bit device words. */
typedef struct elo_input_stage_args {
    int batch, npoints;           /* points per frame */
    int point_stride;             /* floats per point in `cloud` (>= 3: x, y, z first; main.py feeds 6) */
    int H, W;
    float az_res, vert_res, vert_off;   /* as in elo_warp_project_args */
    float crop_xy;                /* 35 (model_util.py:380) */
    const float *cloud;           /* (batch, 2*npoints, point_stride): frame 1's points, then frame 2's (pwclo_model.py:56-57) */
    const float *T_trans;         /* (batch,4,4) row-major, or NULL = no augmentation */
    const int *aug_frame;         /* (batch) 1 or 2: the frame T_trans applies to (NULL with T_trans == NULL) */
    float *points;                /* (2*batch, npoints, 3) OUT */
    float *out_xyz;               /* (2*batch, H, W, 3) OUT */
    unsigned *scratch;
} elo_input_stage_args;
int elo_input_stage(const elo_input_stage_args *a, elo_stream_t stream);

/* elo_input_stage for a sensor with a calibrated BEAM TABLE: the same three launches, crop, T_trans / aug_frame, point_stride,
 * minimum-range winner per cell with duplicates summed, scratch layout and stacked outputs -- only the ROW of a point differs.
 * Instead of the uniform formula (which lets the beams of an unevenly spaced sensor share rows and leaves other rows empty)
 *   row = the beam nearest in elevation to beta = asin(z / r)
 *       = the number of midpoints  m_k = (beam_elev[k] + beam_elev[k+1]) / 2,  k = 0 .. H-2,  that lie above beta:
 * above the top midpoint row 0, below the bottom one row H-1.  The kernel compares z / r with sin(m_k) (monotone, no asinf),
 * H-1 sines staged per workgroup in LDS, by a branch-free binary search; a point within 4 float32 ulps (of z / r) of a midpoint
 * may take either neighbouring row.  A zero point (r = 0, z / r = NaN) counts every midpoint as above it -- the comparison is
 * written !(s >= m_k) -- and lands in row H-1, where the formula's NaN -> 0 conversion puts it too; its column follows atan2 as
 * before, so the three zero cells and the blanking convention of elo_warp_project hold unchanged.
 * beam_elev: H floats in DEVICE memory, radians, strictly descending (row 0 is the highest beam); the order is the caller's to
 * guarantee (efficientlo-net_amd/sensor.py validates the table it is built from), the entry checks what the host can see:
 * H <= ELO_MAX_BEAMS, a non-NULL table, the sizes and pairings elo_input_stage checks.  On ELO_ERR_ARG nothing is launched.
 * LIFETIME: the launches read beam_elev when they RUN.  A captured graph bakes the pointer in: the table stays alive and
 * unchanged for as long as a graph recorded with it may be replayed -- the rule of every other buffer a captured launch names
 * (elo_graph_submit); efficientlo-net_amd keeps it as a tensor owned by the net / trainer whose graphs read it.
 * Additive to ABI 26: no existing struct changes. */
#define ELO_MAX_BEAMS 256
typedef struct elo_input_stage_beams_args {
    int batch, npoints;           /* points per frame */
    int point_stride;             /* floats per point in `cloud` (>= 3) */
    int H, W;                     /* H = number of beams, 1 .. ELO_MAX_BEAMS */
    float az_res;                 /* as in elo_warp_project_args */
    float crop_xy;
    const float *cloud;           /* (batch, 2*npoints, point_stride) */
    const float *T_trans;         /* (batch,4,4) row-major, or NULL = no augmentation */
    const int *aug_frame;         /* (batch) 1 or 2 (NULL with T_trans == NULL) */
    float *points;                /* (2*batch, npoints, 3) OUT */
    float *out_xyz;               /* (2*batch, H, W, 3) OUT */
    unsigned *scratch;            /* as elo_input_stage_args.scratch */
    const float *beam_elev;       /* (H) radians, strictly descending */
} elo_input_stage_beams_args;
int elo_input_stage_beams(const elo_input_stage_beams_args *a, elo_stream_t stream);

/* elo_input_stage / elo_input_stage_beams for a scan that is NOT motion-compensated: every point is first carried from the
 * instant it was acquired to one reference instant of its sweep, by a constant-velocity model of the sensor's motion during that
 * sweep; the stage then runs on the corrected cloud.  The same three launches, scratch layout and stacked outputs.
 * A MOTION is a row [q0 q1 q2 q3 | t0 t1 t2] per image: the rigid transform that carries coordinates from the sensor frame at the
 * END of the sweep (phase 1) to the sensor frame at its START (phase 0),  p_start = R(q) p_end + t.  The kernel normalises q and,
 * where q0 < 0, negates it (the shorter arc); theta = 2 atan2(|v|, q0), u = v / |v| with v = (q1, q2, q3); |v| = 0 (and a zero
 * quaternion): no rotation.  A point p acquired at phase s becomes
 *   a = s - phase_ref;   p' = Rot(u, a theta) p + a t        (slerp from the identity + a linear translation; a may be negative)
 * and the entry is DEFINED as elo_input_stage (beam_elev == NULL) / elo_input_stage_beams (beam_elev != NULL, vert_res / vert_off
 * unused) applied to the cloud whose non-zero points were replaced by p': the crop, T_trans / aug_frame, the validity re-mask, the
 * binning and the scatter all see p'.  A point whose x, y, z are all zero (padding) is not touched and keeps its bits, signs
 * included.  With the identity row, or where s == phase_ref, p' == p bit for bit unless p has a -0 component (which becomes +0).
 * invert = 1: the inverse of the given transform is used, (q^-1, -q^-1 t q) -- the [q_norm | t] row a net writes for the PREVIOUS
 * pair (frame 1 -> frame 2: elo_pose_head_args.pose7) can be named as it stands.
 * phase_mode ELO_PHASE_CHANNEL: s = float number phase_channel of the point (3 <= phase_channel < point_stride), used as given,
 * not clamped.  ELO_PHASE_AZIMUTH: s = (pi - atan2f(y, x)) / 2 pi of the RAW point, the fraction of the row at which the
 * projection puts its column (a sensor that starts its sweep at azimuth pi and turns towards -pi).
 * motion: (batch, 7) in DEVICE memory, the motion of both frames of a batch element; motion2 (or NULL): (batch, 7) for frame 2,
 * motion then serving frame 1 only.  Every workgroup of the per-point launch first stages (u, theta, t) of the 2 * batch images in
 * LDS, 28 bytes each: batch <= ELO_DESKEW_MAX_BATCH.  Per point: one sincosf and the quaternion sandwich, in float32.
 * The entry checks what elo_input_stage / elo_input_stage_beams check, and: a non-NULL motion, a known phase_mode, the channel
 * bound, a finite phase_ref, the batch bound.  On ELO_ERR_ARG nothing is launched.
 * LIFETIME: as beam_elev -- the launches read motion / motion2 when they RUN.  A captured graph bakes the pointers in and sees at
 * every replay what the rows hold THEN: a producer (the pose head of the previous pair, a copy on the replaying stream) may
 * rewrite them between replays; the buffers stay alive for as long as the graph may be replayed.
 * Additive to ABI 26: no existing struct changes. */
#define ELO_PHASE_CHANNEL 0
#define ELO_PHASE_AZIMUTH 1
#define ELO_DESKEW_MAX_BATCH 512
typedef struct elo_input_stage_deskew_args {
    int batch, npoints;           /* points per frame */
    int point_stride;             /* floats per point in `cloud` (>= 3) */
    int H, W;
    float az_res, vert_res, vert_off;   /* as in elo_input_stage_args (vert_res / vert_off: only with beam_elev == NULL) */
    float crop_xy;
    const float *cloud;           /* (batch, 2*npoints, point_stride) */
    const float *T_trans;         /* (batch,4,4) row-major, or NULL = no augmentation */
    const int *aug_frame;         /* (batch) 1 or 2 (NULL with T_trans == NULL) */
    float *points;                /* (2*batch, npoints, 3) OUT */
    float *out_xyz;               /* (2*batch, H, W, 3) OUT */
    unsigned *scratch;            /* as elo_input_stage_args.scratch */
    const float *beam_elev;       /* NULL: the uniform row formula; else (H) radians, strictly descending, H <= ELO_MAX_BEAMS */
    const float *motion;          /* (batch,7) [q | t], end of sweep -> start of sweep */
    const float *motion2;         /* (batch,7) for frame 2, or NULL = frame 2 uses `motion` */
    int invert;                   /* 1: use the inverse of every row */
    int phase_mode;               /* ELO_PHASE_CHANNEL / ELO_PHASE_AZIMUTH */
    int phase_channel;            /* ELO_PHASE_CHANNEL: which float of a point holds its phase */
    float phase_ref;              /* the phase every point is carried to (0: start of the sweep, 1: its end) */
} elo_input_stage_deskew_args;
int elo_input_stage_deskew(const elo_input_stage_deskew_args *a, elo_stream_t stream);

/* The ground-truth half of PreProcess (model_util.py:403, :419, :427-445) in ONE launch, one thread per batch element:
 *   T = T_trans . T_gt      where aug_frame[b] == 2  (:403)
 *   T = T_gt . T_trans_inv  where aug_frame[b] == 1  (:419)
 *   T = T_gt                otherwise (also: T_trans == NULL)
 *   (z, y, x) = mat2euler(T[:3,:3]) (:130-142, no branch: cy = sqrt(r33^2 + r23^2), three atan2);
 *   q_gt = euler2quat(z, y, x) (:112-127), t_gt = T[:3,3].
 * The inputs are fp32; the arithmetic in between is double and each output is rounded to fp32 once (one thread per batch
 * element, so the cost is nil: the targets of the loss are then the correctly rounded ones, not what a chain of fp32 roundings
 * leaves; they may differ from model_util.preprocess_gt's fp32 chain by an ulp or so).
 * aug_frame is DEVICE memory, as every pointer here: a captured training step draws a fresh augmentation per replay by
 * rewriting it (and the matrices) between replays.  Additive to ABI 26: no existing struct changes. */
typedef struct elo_preprocess_gt_args {
    int batch;
    const float *T_gt;            /* (batch,4,4) row-major */
    const float *T_trans;         /* (batch,4,4) row-major, or NULL = no augmentation */
    const float *T_trans_inv;     /* (batch,4,4) row-major (NULL with T_trans == NULL) */
    const int *aug_frame;         /* (batch) (NULL with T_trans == NULL) */
    float *q_gt;                  /* (batch,4) OUT: w, x, y, z */
    float *t_gt;                  /* (batch,3) OUT */
} elo_preprocess_gt_args;
int elo_preprocess_gt(const elo_preprocess_gt_args *a, elo_stream_t stream);

/* elo_pose_head followed by elo_warp_project of the NEXT level's cloud by the pose it just computed
 * (pwclo_model.py:211-236 after :194-208 / :262-280), in three launches instead of five: the projection's buffers
 * are cleared by the pose head's first launch (a->clear_* must name w's scratch / out_xyz / out_feat), every workgroup
 * of the second launch recomputes the head (block 0 stores it) and warps + bins its 256 points with the (q, t) it holds,
 * the third launch is the projection's scatter.  w->q / w->t are ignored (the pose is a->q, a->t); w->warped is required. */
int elo_pose_head_warp(const elo_pose_head_args *a, const elo_warp_project_args *w, elo_stream_t stream);

/* WHAT THE POSE TAIL LAUNCHES for an argument block.  Host-only queries: nothing is launched, no tensor is dereferenced (only the
 * pointers' values are read: NULL or not, equal or not).  Additive: no struct changed.
 * elo_softmax_valid_parts(npoints): the slices per batch element of the partial-sums launch of elo_softmax_valid and of
 *   elo_pose_head / elo_pose_head_warp without ready_parts -- ceil(npoints / 64), at least 1, at most 64.
 * elo_pose_head_form(a, w): elo_pose_head (w == NULL) / elo_pose_head_warp itself, run up to the point where it would launch:
 *   ELO_TAIL_FORM(partials, merge, head, wide, warp, parts) of the enumerators below, or the negative elo_status with which the
 *   entry point would refuse the block.
 *     partials: READY (ready_parts > 0: no partial-sums launch), F32 / F16 (softmax_valid_partial_kernel in that storage type);
 *     merge:    TRIPS16 (parts <= 64: each of a channel's four threads takes its slices in one trip of 16) / TRIPS32 (trips of 32);
 *     head:     MODEL (C == 64 and hidden == 256: one hidden unit per thread, weights requested ahead of the merge) / GENERIC;
 *     wide:     1 when C > 64: channels 64.. are merged by elo_softmax_valid's own sequential merge inside the head;
 *     warp:     1 when the warp and pass A of the projection ride in the head's launch (w != NULL);
 *     parts:    the slices per batch element the head merges (ready_parts, or elo_softmax_valid_parts(npoints)).
 *   With batch == 0 nothing is launched; the query still answers the form of the block's sizes.
 * The LDS limit: the head keeps C + hidden + 808 floats in dynamic LDS; a head with C + hidden > 15576 (more than 64 KiB) is refused
 * with ELO_ERR_LIMIT before any HIP call (an empty batch launches nothing and stays ELO_OK). */
enum { ELO_TAIL_PARTIALS_READY = 0, ELO_TAIL_PARTIALS_F32 = 1, ELO_TAIL_PARTIALS_F16 = 2 };
enum { ELO_TAIL_TRIPS16 = 0, ELO_TAIL_TRIPS32 = 1 };
enum { ELO_TAIL_HEAD_MODEL = 0, ELO_TAIL_HEAD_GENERIC = 1 };
#define ELO_TAIL_FORM(partials, merge, head, wide, warp, parts) \
    ((partials) | (merge) << 2 | (head) << 3 | (wide) << 4 | (warp) << 5 | (parts) << 8)
#define ELO_TAIL_PARTIALS(form) ((form) & 3)
#define ELO_TAIL_MERGE(form) ((form) >> 2 & 1)
#define ELO_TAIL_HEAD(form) ((form) >> 3 & 1)
#define ELO_TAIL_WIDE(form) ((form) >> 4 & 1)
#define ELO_TAIL_WARP(form) ((form) >> 5 & 1)
#define ELO_TAIL_PARTS(form) ((form) >> 8)
int elo_softmax_valid_parts(int npoints);
int elo_pose_head_form(const elo_pose_head_args *a, const elo_warp_project_args *w);

/* POSE FIT on the two range images of a pair (csrc/elo_posefit.hip): how well a relative pose registers them, the 6x6
 * information matrix of that pose, and -- on request -- a few Gauss-Newton steps on it ("polish").
 * pose_in: (batch,7) [q | t], frame 1 -> frame 2, p' = R(q) p + t: the layout and convention of elo_pose_head_args.pose7.  q is
 * normalised in the kernel.  xyz1 / xyz2: (batch,H,W,3) range images as the input stage writes them; an all-zero cell is empty.
 * ONE EVALUATION at a pose (R, t):
 *   normal of a frame-2 cell (h,w):  n = normalise((x[h,w+1] - x[h,w-1]) x (x[h+1,w] - x[h-1,w])), columns wrap (the cylinder's
 *     seam); invalid in rows 0 and H-1, where the cell or one of the four neighbours is empty, where a neighbour's range differs
 *     from the cell's range r by more than jump_rel * r, and where the cross product has no length; oriented towards the sensor
 *     (n . x <= 0).  Computed on the fly at the matched cell.
 *   term of a non-empty frame-1 cell p1:  p = R p1 + t;  m = the cell of p in frame 2 -- cell_of_point at (az_res, vert_res,
 *     vert_off), exactly as elo_warp_project takes it, or (beam_elev != NULL) the beam-table row of elo_input_stage_beams --;
 *     p2 = xyz2[m].  No term where p2 is empty, its normal is invalid or |p - p2| > gate.  Else
 *       r = n . (p - p2),   J = [p x n | n]  (left perturbation: rotation first, then translation),
 *       w = 1 where |r| <= huber, else huber / |r|
 *   sums per image:  A = sum w J J^T,  b = sum w J r,  cost = sum w r^2,  sum w,  count (an integer).
 * ARITHMETIC: the geometry of a term (p, the normal, r, J, w and their products) is double precision from the float32 inputs --
 * r is a difference of nearby points, which float32 would leave with a relative error of |p| / |r| ulps --; the cell of p is taken
 * from p rounded to float32, by the float32 rule the projections use.  Each product is rounded to float32 ONCE and summed in
 * float32 in a FIXED order: a thread over its strip of cells, a wave by DPP, the four waves of a workgroup through LDS; the
 * workgroup stores one partial row.  The partial rows of an image are then added in a fixed order, in double.  No floating-point atomic:
 * two runs, and an eager run and a graph replay, agree bit for bit.  The grid is a fixed function of (batch, H, W).
 * SOLVE (a second, one-workgroup-per-image launch after an evaluation): (A + damping * diag(A)) d = -b by Cholesky in double, one
 * thread; d = (omega, v);  q <- dq(omega) (x) q, normalised,  t <- R(dq) t + v.  Where count < min_count (ELO_FIT_FEW) or the
 * factorisation fails / d is not finite (ELO_FIT_SINGULAR) the image is FLAGGED: its pose_out row is pose_in's, every bit, from
 * then on (later steps do not move it), and the status says why.  No NaN leaves these kernels.
 * iters = 0: one evaluation at pose_in; pose_out = pose_in (bits).  iters = k: k times (evaluate, solve), then one evaluation at
 * the updated pose.  The sums of the LAST evaluation are added up and written by the solve kernel in its report form (no pose
 * update; count < min_count there sets ELO_FIT_FEW_FINAL and leaves pose_out alone): 2 (k + 1) launches, all enqueued by this
 * one call, capturable.
 * OUT: pose_out (batch,7); info (batch,6,6) = A at pose_out (all 36 entries, symmetric); grad (batch,6) = b;
 *      stats (batch,4) = [count, cost, rms = sqrt(cost / sum w) (0 where count = 0), status], float32 roundings of the doubles.
 * scratch: elo_pose_fit_scratch_words(batch, H, W) 32-bit device words (ask: the host does not restate the launch geometry).
 * ELO_ERR_ARG (nothing is launched): a NULL image / pose / output / scratch, H < 3, W < 1, gate or huber not positive, a negative
 * or NaN jump_rel or damping, H > ELO_MAX_BEAMS with a table, iters < 0, batch * H * W beyond 2^31.
 * LIFETIME: the launches read pose_in, the images and beam_elev when they RUN: a captured graph sees at every replay the row the
 * pose head has just written; every buffer named here stays alive for as long as a graph recorded with it may be replayed.
 * pose_out must not alias pose_in.  Additive to ABI 26: no existing struct changes. */
#define ELO_FIT_FEW 1            /* status bits: a solve step met count < min_count */
#define ELO_FIT_SINGULAR 2       /*   a solve step's factorisation failed */
#define ELO_FIT_FEW_FINAL 4      /*   the last evaluation (the one reported) has count < min_count */
typedef struct elo_pose_fit_args {
    int batch, H, W;
    float az_res, vert_res, vert_off;   /* as in elo_warp_project_args (vert_res / vert_off: only with beam_elev == NULL) */
    const float *xyz1, *xyz2;     /* (batch,H,W,3) */
    const float *pose_in;         /* (batch,7) [q | t] */
    const float *beam_elev;       /* NULL: the uniform row formula; else (H) radians, strictly descending, H <= ELO_MAX_BEAMS */
    int iters;                    /* Gauss-Newton steps, >= 0 */
    float gate;                   /* m: no term beyond this distance to the matched point */
    float huber;                  /* m */
    float jump_rel;               /* a normal's neighbours lie within jump_rel * range of its cell's range */
    int min_count;
    float damping;                /* Levenberg factor on diag(A), >= 0 */
    float *pose_out;              /* (batch,7) OUT */
    float *info;                  /* (batch,6,6) OUT */
    float *grad;                  /* (batch,6) OUT */
    float *stats;                 /* (batch,4) OUT */
    unsigned *scratch;
} elo_pose_fit_args;
long elo_pose_fit_scratch_words(int batch, int H, int W);   /* < 0: sizes the entry refuses */
int elo_pose_fit_parts(int H, int W);                       /* partial rows (workgroups) per image of an evaluation */
int elo_pose_fit(const elo_pose_fit_args *a, elo_stream_t stream);

/* LOCAL MODEL for a frame-to-model pose fit (csrc/elo_model.hip): K range images, each carried into ONE frame by its own pose,
 * rendered into one range image by nearest range -- what elo_pose_fit takes as xyz2 when a scan is fitted against the last K scans
 * instead of the last one.
 * src: (batch,K,H,W,3) range images as the input stage writes them; an all-zero cell is empty.  pose: (batch,K,7) [q | t], source
 * k -> the model's frame, p' = R(q) p + t: the layout and convention of elo_pose_fit_args.pose_in.
 * ONE POINT: a non-empty source point p is carried in double from the float32 inputs, q normalised in double; each component of p'
 *   is rounded to float32 ONCE.  A point whose rounded p' has a non-finite component, or is exactly (0,0,0), is dropped (so is
 *   one whose float32 range below is not positive and finite: components that underflow or overflow in the square).  A source whose
 *   quaternion has zero or non-finite norm is skipped whole.  No NaN leaves these kernels.
 *   The cell of p' comes from the ROUNDED point by the float32 sequence of the projections and of elo_pose_fit:
 *     rf = sqrtf(x*x + y*y + z*z);  m = cell(atan2f(y, x), z, rf) -- cell_of_point at (az_res, vert_res, vert_off), or (beam_elev
 *     != NULL) the beam-table row of elo_input_stage_beams --, clipped to the image by the rule.  A point the input stage stored in
 *     cell m therefore lands in cell m again under the identity pose 1 0 0 0 0 0 0, with the bits it had (but for a component
 *     that is -0.0 beside non-zero ones: the sum returns it as +0.0).
 * ONE CELL: the winner is the point with the smallest rf (its float32 bits order it: rf is positive); among equal rf the smallest
 *   source index (k*H + h)*W + w wins.  out_xyz = the winner's rounded p', out_src = its index; a cell nobody reached is zeros and
 *   -1.  EVERY cell of both outputs is written: the caller need not clear them.
 * DETERMINISM: one 64-bit integer atomicMin of (rf bits << 32 | index) per surviving point, no floating-point atomic; the point is
 *   recomputed from the winning index by the same instructions.  Two calls, and an eager call and a graph replay, agree bit for
 *   bit.  The grid is a fixed function of (batch, K, H, W).
 * Three launches (clear the keys, splat, resolve), all enqueued by this one call; no host synchronisation; capturable.
 * scratch: elo_model_render_scratch_words(batch, H, W) 32-bit device words, 8-byte aligned (ask: the host does not restate it).
 * ELO_ERR_ARG (nothing is launched): a NULL src / pose / output / scratch, K < 1 or K > ELO_MODEL_MAX_SCANS, H < 1, W < 1, H >
 * ELO_MAX_BEAMS with a table, K*H*W or batch*H*W at or beyond 2^31, out_xyz overlapping src, bad projection constants.
 * LIFETIME: the launches read pose, src and beam_elev when they RUN: a captured graph renders at every replay what the buffers
 * hold then; every buffer named here stays alive for as long as a graph recorded with it may be replayed.
 * Additive to ABI 26: no existing struct changes. */
#define ELO_MODEL_MAX_SCANS 16
typedef struct elo_model_render_args {
    int batch, K, H, W;
    float az_res, vert_res, vert_off;   /* as elo_pose_fit_args */
    const float *src;             /* (batch,K,H,W,3) range images; an all-zero cell is empty */
    const float *pose;            /* (batch,K,7) [q | t]: source k -> the model's frame, p' = R(q) p + t */
    const float *beam_elev;       /* NULL: the uniform row formula; else (H) radians as in elo_pose_fit */
    float *out_xyz;               /* (batch,H,W,3) OUT */
    int *out_src;                 /* (batch,H,W) OUT: (k*H + h)*W + w of the winner, -1 for an empty cell */
    unsigned *scratch;            /* elo_model_render_scratch_words(batch,H,W) 32-bit words */
} elo_model_render_args;
long elo_model_render_scratch_words(int batch, int H, int W);   /* < 0: refused sizes */
int elo_model_render(const elo_model_render_args *a, elo_stream_t stream);

/* TRACKER STATE on the device (csrc/elo_model_state.hip): the state machine of a frame-to-model tracker -- which slot of the ring
 * a scan enters, whether the first frame 2 enters, the re-basing of the held poses -- as launches that read their decisions from
 * device memory, so that one tracker step (begin, elo_model_render, elo_pose_fit, advance) is a FIXED launch sequence: a hipGraph
 * records it once and replays it per scan.
 * STATE of one tracker, four device buffers the caller owns:
 *   ring    (K,H,W,3) float32: the held scans; an unused slot is all empty cells (zeros) and gives the render nothing;
 *   poses64 (K,7) double [q | t]: scan of the slot -> the model's frame (the frame of the newest scan held);
 *   poses32 (K,7) float32: every component of poses64 rounded to float32 once -- what elo_model_render takes as `pose`;
 *   state   int32[2] = {next in 0 .. K-1: the slot the next scan enters;  held in 0 .. K: how many scans the ring holds}.
 *   RESET (the caller's, by device-side fills): ring zero, every pose row 1 0 0 0 0 0 0 in both copies, state {0, 0}.
 * elo_model_begin, ONE launch: where held == 0 the image `first` (H,W,3) -- the pair's frame 2, which starts an empty model at the
 *   identity -- is copied into slot 0; otherwise nothing is written.  It reads `state` and never writes it.
 * elo_model_advance, TWO launches, in this order; (next', held') = held == 0 ? (1 % K, 1) : (next, held) -- an empty model has just
 *   taken its frame 2 in slot 0 --:
 *   1. enter: the image `scan` (H,W,3) is copied into slot next'.  It only reads `state`.
 *   2. update, one workgroup: every row P_j <- T^-1 o P_j, where T (7) float32 [q | t] carries the NEW model frame (that of `scan`)
 *      into the old one, p_old = R(q) p_new + t -- the pose_out row of the fit of `scan` against the model --:
 *        q_new = conj(q_T) (x) q_j, renormalised;  t_new = R(q_T)^T (t_j - t_T);  q_T normalised where it is used; all in double
 *        from the float32 T and the double rows;
 *      then row next' <- the identity 1 0 0 0 0 0 0, exactly; poses32 <- every component of poses64 rounded to float32 once;
 *      state <- {(next' + 1) % K, min(held' + 1, K)}.  Only this launch writes `state`, and it is ordered after every launch that
 *      reads it.
 *   A non-finite T is not special-cased: the re-based rows become non-finite, elo_model_render skips such sources, and a reset
 *   recovers.  A `state` outside its domain (memory nobody reset) makes all three launches write nothing.
 * COPIES: 16-byte accesses where H * W is a multiple of 4 and ring and the image are 16-byte aligned; one float at a time
 *   otherwise.  Empty cells stay the zeros they are.  No atomic anywhere; two runs, and an eager run and a graph replay, agree bit
 *   for bit.  The grids are fixed functions of (H, W).
 * No host synchronisation; capturable.  The launches read `state`, `T` and the images when they RUN: a captured graph acts at every
 *   replay on what the buffers hold then; every buffer named here stays alive for as long as a graph recorded with it may be
 *   replayed.
 * ELO_ERR_ARG (nothing is launched): a NULL pointer, K < 1 or K > ELO_MODEL_MAX_SCANS, H < 3, W < 1, H * W or K * H * W at or
 *   beyond 2^31 (the bounds of elo_pose_fit on an image and of elo_model_render on the ring), `first` / `scan` overlapping `ring`,
 *   poses64 not 8-byte aligned.
 * Additive to ABI 26: no existing struct changes. */
typedef struct elo_model_begin_args {
    int K, H, W;
    float *ring;                  /* (K,H,W,3) IN/OUT: slot 0 <- first where the model is empty */
    const int *state;             /* int32[2] {next, held}: read only */
    const float *first;           /* (H,W,3): the pair's frame 2; must not overlap ring */
} elo_model_begin_args;
int elo_model_begin(const elo_model_begin_args *a, elo_stream_t stream);
typedef struct elo_model_advance_args {
    int K, H, W;
    float *ring;                  /* (K,H,W,3) IN/OUT: slot next' <- scan */
    double *poses64;              /* (K,7) IN/OUT */
    float *poses32;               /* (K,7) OUT */
    int *state;                   /* int32[2] {next, held} IN/OUT */
    const float *scan;            /* (H,W,3): the scan that enters (the pair's frame 1); must not overlap ring */
    const float *T;               /* (7) [q | t]: elo_pose_fit's pose_out row of scan against the model */
} elo_model_advance_args;
int elo_model_advance(const elo_model_advance_args *a, elo_stream_t stream);

/* WORLD MAP (csrc/elo_map.hip): a voxel-hashed point map of a trajectory, built on the device -- every scan's range image carried
 * by its scan -> world pose and summed, per voxel, into INTEGERS, so that the map does not depend on the order of arrival.
 * STATE of one map of capacity C = 1 << log2_capacity, three device buffers the caller owns:
 *   keys   unsigned long long[C]: the voxel a slot holds; all ones = empty;
 *   acc    unsigned long long[C][4] = {count, sx, sy, sz}: the points of the slot's voxel and the sums of their offsets g (below);
 *   stats  unsigned long long[8] = {inserted, filtered, rejected, dropped_full, occupied, 0, 0, 0}, running totals.
 *   RESET (the caller's, by device-side fills): keys to 0xFF bytes, acc and stats to zero.
 * elo_map_insert, ONE launch.  xyz: (batch,H,W,3) range images; a cell that is exactly (0,0,0) is empty and counts nowhere.  pose:
 *   (batch,7) DOUBLE [q | t], scan -> world, p' = R(q) p + t.
 * ONE POINT p = (x, y, z), in this order:
 *   pose       q is normalised in double; a scan whose quaternion has zero or non-finite norm is skipped whole and counts nothing
 *              (elo_model_render's rule, taken from a double row);
 *   range gate on the SOURCE point, in float32: rf = sqrtf(x*x + y*y + z*z) (summed left to right); rf < min_range or rf >
 *              max_range -> `filtered` (a NaN rf is neither: the point goes on and is rejected below);
 *   carry      in double from the float32 inputs, p'_i = ((R_i0 x + R_i1 y) + R_i2 z) + t_i, R(q) as elo_model_render forms it;
 *              each component is rounded to float32 ONCE;
 *   rejection  a non-finite component of the rounded p' -> `rejected`;
 *   index      per axis u = (double)x' / (double)voxel (a division, not a reciprocal multiply), i = floor(u) (floor, not
 *              truncation: negative coordinates work); i must lie in [-2^20, 2^20) -- checked in double before any integer
 *              conversion --, else -> `rejected`;
 *   offset     g = min((unsigned)floor((u - i) * 65536.0), 65535) per axis;
 *   Every step after the one rounding to float32 is a single IEEE operation with no multiply-add to contract: a float64 / uint64
 *   restatement reproduces it bit for bit.
 *   key        (ix + 2^20) << 42 | (iy + 2^20) << 21 | (iz + 2^20); its top bit is clear, so all ones is never a key;
 *   home slot  the splitmix64 finaliser of the key, & (C - 1):  h = key; h ^= h >> 30; h *= 0xbf58476d1ce4e5b9; h ^= h >> 27;
 *              h *= 0x94d049bb133111eb; h ^= h >> 31;
 *   probing    linear: slot (home + j) & (C - 1), j = 0 .. ELO_MAP_MAX_PROBE - 1.  A slot holding the key is found.  An empty slot
 *              is claimed by a 64-bit atomicCAS(empty -> key), won if the CAS returns empty or the key; the thread that turns an
 *              empty slot into the key adds 1 to `occupied`.  No slot within the limit -> `dropped_full`, nothing else touched;
 *   sums       the found slot gets integer atomic adds count += 1, sx += gx, sy += gy, sz += gz; the point counts in `inserted`.
 *   Neighbouring cells of one wave that share a key (a run; cells without a point do not end it) are summed in registers first and
 *   sent as ONE probe and four adds (and are dropped together where the table is full); the counters are summed per wave.  Sums of
 *   integers: the result is that of one add per point.
 * DETERMINED: as long as dropped_full == 0, the CONTENT of the map -- the set of keys, each with its four integers -- and `stats`
 *   are a function of the multiset of points inserted: not of launch order, scan order, batch split or races.  Two runs, and an
 *   eager run and a graph replay, agree bit for bit in content.  NOT DETERMINED: the PLACEMENT of keys in slots (which of two
 *   colliding keys sits nearer its home); nothing may depend on it -- compare maps after sorting by key.  With dropped_full > 0
 *   which points were dropped depends on the races too; what is stored is still consistent (no key twice, every count that of the
 *   points inserted for it).
 * Every loop in the kernels has a static trip bound; nothing waits on another thread.  No host synchronisation; capturable.  The
 *   grid is a fixed function of (batch, H, W).  16-byte loads where H * W is a multiple of 4 and xyz is 16-byte aligned, one float
 *   at a time otherwise.
 * ELO_ERR_ARG (nothing is launched): a NULL pointer, H < 1, W < 1, batch < 0, batch * H * W at or beyond 2^31, a voxel that is not
 *   positive and finite, a negative or NaN min_range, max_range <= min_range (or NaN), log2_capacity outside ELO_MAP_MIN_LOG2 ..
 *   ELO_MAP_MAX_LOG2, keys / acc / stats / pose not 8-byte aligned.  An empty batch launches nothing and is ELO_OK.
 * elo_map_extract: the occupied slots compacted into rows, in ARBITRARY order (ballot compaction within a wave, one integer atomic
 *   on the cursor per wave).  cursor: one device word, cleared by the call itself (its first launch), which ends at the number of
 *   occupied slots even where that exceeds max_out; only rows < max_out are written.  Row of a slot: out_key = its key, out_count =
 *   its count, out_xyz = the centroid, per axis, every step one IEEE operation in double,
 *     c = ((double)i + ((double)s / (double)count + 0.5) / 65536.0) * (double)voxel,   i = the key's field - 2^20,
 *   rounded to float32 once.  Two launches; capturable.  ELO_ERR_ARG: a NULL pointer, max_out < 0, a bad voxel or log2_capacity,
 *   keys / acc / cursor / out_key / out_count not 8-byte aligned.
 * elo_map_merge, ONE launch: source ROWS (key, {count, sx, sy, sz}) from anywhere -- the keys / acc of another table, rows = its C,
 *   or the m rows of a saved state -- filtered and added into the destination table.  A sliding window (rebuild into a second
 *   table under a box about the vehicle), growth (rebuild into a larger table), loading a state and joining two maps are all this.
 *   The source's keys are taken to mean the destination's voxel.  ONE SOURCE ROW with key k and count n, in this order:
 *   empty      k all ones: skipped, counts nowhere;
 *   malformed  k's top bit set, n == 0, n >= 2^40, or a sum above 65535 * n -> `voxels_rejected`: no division by zero and no
 *              overflowing sum can enter a table from rows that are not trusted;
 *   min_count  n < min_count -> filtered.  The SOURCE ROW's count, not the destination's total;
 *   window     with centre (3 device doubles, read when the launch RUNS): per axis c = ((double)i + 0.5) * (double)voxel, i = the
 *              key's field - 2^20, d = fabs(c - centre[axis]); the row is kept where d <= (double)radius on all three axes (a BOX;
 *              a voxel whose centre lies exactly at the radius is kept), else filtered.  A NaN centre keeps nothing.  Every step is
 *              one IEEE operation in double;
 *   add        elo_map_insert's home slot, probing and atomicCAS claim -- the same device function --; the found slot gets count +=
 *              n, sx += sx, sy += sy, sz += sz.  No slot within ELO_MAP_MAX_PROBE -> dropped, nothing touched.
 *   report, eight words the launch ADDS to (the caller zeroes them): {voxels_merged, voxels_filtered, voxels_rejected,
 *   voxels_dropped, points_merged, points_filtered, points_dropped, claimed}, points being the rows' counts; summed per wave, one add
 *   per wave and counter.  The destination's stats get inserted += points_merged, dropped_full += points_dropped, occupied +=
 *   claimed: the sum of all counts of a table stays equal to its `inserted`.  Filtered and rejected rows were never offered to the
 *   table and do not touch its stats.  A key may stand in several source rows (concatenated states): the result is that of one add
 *   per row.
 *   DETERMINED as for the insert: with nothing dropped, the destination's content, its stats and the report are a function of the
 *   multiset of rows merged and of what the table held before -- not of row order, split into launches, launch order or races;
 *   an eager run and a graph replay agree bit for bit in content.  PLACEMENT is not determined.  With rows dropped, which ones
 *   depends on the races; what is stored is still consistent.
 *   The grid is a fixed function of rows (not of alignment: the keys are taken by 16-byte loads where src_keys is 16-byte aligned,
 *   one word at a time otherwise; likewise the acc rows, which are read for occupied rows only).  Static trip bounds, nothing
 *   waits on another thread, integer atomics only; no host synchronisation; capturable.
 *   ELO_ERR_ARG (nothing is launched): a NULL pointer other than centre, rows < 0 or >= 2^31, a bad voxel or log2_capacity,
 *   min_count < 1, with a centre a radius that is not positive and finite, a pointer that is not 8-byte aligned, a source range
 *   ([rows] keys, [rows][4] acc) that overlaps the destination's keys or acc.  rows == 0 launches nothing and is ELO_OK.
 * LIFETIME as elo_model_render's.  Additive to ABI 26: no existing struct changes. */
#define ELO_MAP_MAX_PROBE 128
#define ELO_MAP_MIN_LOG2 10
#define ELO_MAP_MAX_LOG2 28
typedef struct elo_map_insert_args {
    int batch, H, W;
    float voxel, min_range, max_range;  /* m; max_range may be +inf */
    int log2_capacity;
    const float *xyz;             /* (batch,H,W,3); an all-zero cell is empty */
    const double *pose;           /* (batch,7) [q | t] DOUBLE: scan -> world */
    unsigned long long *keys;     /* [C] IN/OUT */
    unsigned long long *acc;      /* [C][4] IN/OUT */
    unsigned long long *stats;    /* [8] IN/OUT */
} elo_map_insert_args;
int elo_map_insert(const elo_map_insert_args *a, elo_stream_t stream);
typedef struct elo_map_extract_args {
    float voxel;
    int log2_capacity;
    long max_out;                 /* rows the outputs hold, >= 0 */
    const unsigned long long *keys;
    const unsigned long long *acc;
    long long *out_key;           /* [max_out] OUT */
    long long *out_count;         /* [max_out] OUT */
    float *out_xyz;               /* [max_out][3] OUT */
    unsigned long long *cursor;   /* one word OUT: the number of occupied slots */
} elo_map_extract_args;
int elo_map_extract(const elo_map_extract_args *a, elo_stream_t stream);
typedef struct elo_map_merge_args {
    long rows;                    /* source rows, >= 0: ANY number (a table's C, or a saved state's m) */
    const unsigned long long *src_keys;  /* [rows]; all ones = an empty slot: skipped, counts nowhere */
    const unsigned long long *src_acc;   /* [rows][4] {count, sx, sy, sz} */
    float voxel;                  /* the DESTINATION table's; the source's keys are taken to mean the same voxel */
    int log2_capacity;
    unsigned long long *keys;     /* [C] IN/OUT: the destination, as elo_map_insert_args */
    unsigned long long *acc;      /* [C][4] IN/OUT */
    unsigned long long *stats;    /* [8] IN/OUT */
    const double *centre;         /* NULL: no window.  Else 3 device doubles, read when the launch RUNS */
    float radius;                 /* with centre: finite, > 0 (m) */
    long long min_count;          /* >= 1 */
    unsigned long long *report;   /* [8] device words, ADDED to (the caller zeroes them) */
} elo_map_merge_args;
int elo_map_merge(const elo_map_merge_args *a, elo_stream_t stream);

/* SCAN-TO-MAP REGISTRATION (csrc/elo_mapfit.hip): the point-to-plane fit of a scan's WORLD pose against the voxel map above -- every
 * cell of a range image carried by the scan -> world pose, matched to the nearest voxel centroid of the map, and -- on request -- a
 * few Gauss-Newton steps on the pose.  The table (keys, acc; voxel and log2_capacity as elo_map_insert_args) is only READ.
 * xyz: (batch,H,W,3) range images, an all-zero cell is empty.  pose_in: (batch,7) DOUBLE [q | t], scan -> world, p' = R(q) p + t:
 * the layout and convention of elo_map_insert_args.pose.
 * ONE EVALUATION at a pose (R, t), per cell (h,w) of a scan, in this order:
 *   pose row   q is normalised in double, R(q) as elo_map_insert forms it.  A row whose quaternion has zero or non-finite norm, or
 *              whose t has a non-finite component, gives NO terms at all (the insert's rule for a scan, not elo_pose_fit's identity).
 *   normal     elo_pose_fit's rule for a frame-2 cell, applied to xyz at the cell ITSELF, in the scan's frame, in double:
 *              n_s = normalise((x[h,w+1] - x[h,w-1]) x (x[h+1,w] - x[h-1,w])), columns wrap; none in rows 0 and H-1, where the cell
 *              or one of the four neighbours is empty, where a neighbour's range differs from the cell's range r by more than
 *              jump_rel * r, where the cross product has no length; oriented towards the sensor (n_s . x <= 0).  n = R n_s.
 *              A cell without a normal gives no term and makes no table access.
 *   carry      p_i = ((R_i0 x + R_i1 y) + R_i2 z) + t_i in double from the float32 cell: elo_map_insert's carry.
 *   voxel      (ix, iy, iz) from p rounded to float32 ONCE per component, by the insert's rule: u = (double)p32 / (double)voxel,
 *              i = floor(u), in [-2^20, 2^20).  A non-finite rounded component or an index out of range: no term.  A scan inserted
 *              at a pose therefore finds its own voxels at that pose.
 *   candidates the 27 voxels (ix + dx, iy + dy, iz + dz), d* in {-1, 0, 1}, whose indices lie in [-2^20, 2^20).
 *   lookup     read only: key as elo_map_insert packs it, home slot = the splitmix64 finaliser & (C - 1), slots (home + j) & (C - 1),
 *              j = 0 .. ELO_MAP_MAX_PROBE - 1; found where a slot holds the key, absent at the first empty slot or after the last
 *              probe.  A slot only ever turns from empty into one key, so this finds every key an insert stored.  A voxel whose
 *              count < min_points is no candidate.
 *   centroid   the float32 value elo_map_extract writes for the voxel, per axis, widened to double: the rows of the extract are
 *              exactly the targets of the fit.
 *   choice     the candidate with the smallest d2 = ((px - cx)^2 + (py - cy)^2) + (pz - cz)^2, in double from the unrounded p;
 *              equal d2: the smaller key.  No term unless sqrt(d2) <= gate.
 *   gate       gate <= voxel is REQUIRED: a centroid lies inside its voxel, and every voxel outside the 3x3x3 block is at least one
 *              voxel away from p.  The target is therefore the nearest centroid OF THE WHOLE MAP within the gate (among voxels of
 *              min_points points or more), not merely of the block.  (Candidates whose voxel box lies beyond the gate are not looked
 *              up; the margin of that test covers every rounding, so the result is this rule's.)
 *   term       with c the chosen centroid:  r = n . (p - c),   J = [ (c - t) x n | n ],   w = 1 where |r| <= huber, else huber / |r|.
 *              The perturbation d = (omega, v) is about the SENSOR's position t, not the world origin: p(d) = R(dq) (p - t) + t + v
 *              and the normal turns with the scan, n(d) = R(dq) n; so dr/domega = (c - t) x n and the numbers of a term are sensor-
 *              relative however far the drive is from the world origin (about the origin the rotation block grows with |t|^2 and
 *              float32 sums lose the fit after a few kilometres).
 *   sums per image:  A = sum w J J^T,  b = sum w J r,  cost = sum w r^2,  sum w,  count (an integer).
 * ARITHMETIC: as elo_pose_fit's.  The geometry of a term is double precision; each product is rounded to float32 ONCE and summed in
 * float32 in a FIXED order: a thread over its strip of cells, a wave by DPP, the four waves of a workgroup through LDS; the workgroup
 * stores one partial row; the elo_map_fit_parts(H, W) partial rows of an image are added in a fixed order, in double.  No
 * floating-point atomic: two runs, and an eager run and a graph replay, agree bit for bit.  The grid is a fixed function of
 * (batch, H, W).
 * SOLVE, FLAGS, iters, REPORT: elo_pose_fit's, by the same code, on a double pose:  (A + damping * diag(A)) d = -b by Cholesky in
 * double;  q <- dq(omega) (x) q, normalised,  t <- t + v.  ELO_FIT_FEW / ELO_FIT_SINGULAR flag an image: its pose_out row is
 * pose_in's, every bit of the doubles, from then on.  pose_out is double and is NOT rounded to float32 between steps.  iters = 0:
 * one evaluation at pose_in, pose_out = pose_in (bits); iters = k: k times (evaluate, solve), then one evaluation at pose_out,
 * reported (ELO_FIT_FEW_FINAL where its count < min_count): 2 (k + 1) launches from this one call, capturable.  No NaN leaves the
 * kernels.
 * OUT: pose_out (batch,7) double; info (batch,6,6), grad (batch,6), stats (batch,4) = [count, cost, rms, status] as elo_pose_fit's;
 * match (batch,H,W) or NULL: the key of the voxel the cell's term went to, -1 where the cell gave none; written by EVERY
 * evaluation, so it holds the association of the last one, which ran at pose_out.
 * scratch: elo_map_fit_scratch_words(batch, H, W) 32-bit device words.
 * ELO_ERR_ARG (nothing is launched): a NULL pointer other than match, H < 3, W < 1, batch * H * W beyond 2^31, a bad voxel or
 * log2_capacity (as elo_map_insert), gate not positive or gate > voxel, huber not positive, a negative or NaN jump_rel or damping,
 * iters < 0, min_points < 1, pose_out == pose_in, keys / acc / pose_in / pose_out / match not 8-byte aligned.  An empty batch
 * launches nothing and is ELO_OK.
 * LIFETIME AND ORDER: the launches read the table, xyz and pose_in when they RUN; the caller orders them against inserts into the
 * same table (one stream does).  Every buffer named here stays alive for as long as a graph recorded with it may be replayed.
 * Additive to ABI 26: no existing struct changes. */
typedef struct elo_map_fit_args {
    int batch, H, W;
    float voxel;                  /* the table's, as elo_map_insert_args */
    int log2_capacity;
    const unsigned long long *keys;     /* [C] READ ONLY */
    const unsigned long long *acc;      /* [C][4] READ ONLY */
    const float *xyz;             /* (batch,H,W,3); an all-zero cell is empty */
    const double *pose_in;        /* (batch,7) [q | t] DOUBLE: scan -> world */
    int iters;                    /* Gauss-Newton steps, >= 0 */
    float gate;                   /* m: no term beyond this distance to the centroid; <= voxel */
    float huber;                  /* m */
    float jump_rel;               /* as elo_pose_fit_args */
    int min_count;
    float damping;                /* Levenberg factor on diag(A), >= 0 */
    int min_points;               /* a voxel with fewer points is no target, >= 1 */
    double *pose_out;             /* (batch,7) OUT */
    float *info;                  /* (batch,6,6) OUT */
    float *grad;                  /* (batch,6) OUT */
    float *stats;                 /* (batch,4) OUT */
    long long *match;             /* (batch,H,W) OUT, or NULL */
    unsigned *scratch;
} elo_map_fit_args;
long elo_map_fit_scratch_words(int batch, int H, int W);    /* < 0: sizes the entry refuses */
int elo_map_fit_parts(int H, int W);                        /* partial rows (workgroups) per image of an evaluation */
int elo_map_fit(const elo_map_fit_args *a, elo_stream_t stream);

/* PLACE RECOGNITION (csrc/elo_place.hip): a descriptor of a scan that does not depend on the vehicle's heading -- a grid of
 * `sectors` azimuth sectors by `rings` range rings that holds, per bin, the height of its highest point as an INTEGER level -- and
 * the search of a database of such descriptors over every entry and every column shift.  Integers throughout: the descriptor and
 * every inner product of the search are exact, the distance is a fixed sequence of IEEE double operations.
 * elo_scan_descriptor, ONE launch.  xyz: (batch,H,W,3) range images, W >= sectors.  desc: (batch,sectors,rings) unsigned 16-bit,
 *   sector-major (one sector's rings are contiguous), written in full.  A stored level is 1 .. ELO_PLACE_LEVELS; 0 = no point.
 * ONE CELL (h, w) with p = (x, y, z), in this order:
 *   validity   elo_map_insert's rule for a cell at the identity pose, without its range gate: a cell that is exactly (0,0,0) is
 *              empty, a cell with a non-finite component is left out (the same device functions, csrc/elo_map_device.h);
 *   sector     (w * sectors) / W in integers: the columns of a sector are a contiguous run, of two lengths where sectors does not
 *              divide W;
 *   r2         (double)x * (double)x + (double)y * (double)y: both products are exact in double, the sum is ONE rounding;
 *   ring       the number of j in 1 .. rings with edge2[j] <= r2 (a point exactly on an edge lies in the ring above it).  edge2[j]
 *              = e_j * e_j with e_j = (double)max_range * j / rings is formed by the CALLER in double and passed in, so that the
 *              kernel and a restatement compare against the same numbers; edge2[0] is not read;
 *   range      r2 < min_range2 or r2 >= edge2[rings]: left out (min_range2 = min_range * min_range, the caller's, in double);
 *   level      q = ((double)z - z_min) / z_step (a division), f = floor(q), clamped IN DOUBLE to [0, ELO_PLACE_LEVELS - 1];
 *              level = (int)f + 1.  Both ends clamp; nothing is counted;
 *   bin        desc[sector][ring] = the largest level of its points (an integer max: no order of arrival).
 *   An image without points gives all zeros.  A workgroup owns one sector of one image: `rings` words of LDS, integer atomicMax on
 *   them, `rings` plain stores; no global atomics, no scratch buffer.
 * elo_descriptor_search, TWO launches (one where m == 0).  query: (n,sectors,rings), db: (cap,sectors,rings), both as desc above;
 *   the entries [0, m) are searched, m BY VALUE (the caller counts its entries on the host).
 * THE DISTANCE of a query Q, an entry D and a shift s in 0 .. sectors - 1:
 *   pairing    column j of Q goes with column c = (j + s) mod sectors of D;
 *   integers   a = sum_r Q[j][r]^2, b = sum_r D[c][r]^2, d = sum_r Q[j][r] * D[c][r]  (each below 2^31: 4095^2 * 32);
 *   skipped    a pair with a == 0 or b == 0 (an empty column) gives no term and does not count in `pairs`;
 *   term       1.0 - (double)d / sqrt((double)((unsigned long long)a * b)): product in 64-bit integers, ONE conversion, IEEE sqrt
 *              and division;
 *   dist       (sum of the terms) / (double)pairs, the terms added in ASCENDING j, one after the other, in double, from 0.0;
 *              no pair at all: +inf.
 *   A function of (Q, D, s) alone: not of where the entry sits or which lane computed it -- equal entries give equal bits.
 *   best_shift[q][e], best_dist[q][e]: the shift with the smallest dist, the SMALLER shift winning a tie, and that dist.
 *   ranking    the entries by (best_dist, entry) ascending; for r < k: entry[q][r], shift[q][r] = its best shift, dist[q][r].  Rows
 *              r >= m are padded with -1, -1, +inf; m == 0 is legal and gives padding only.
 *   THE YAW a shift stands for: the query's heading relative to the entry's, about the scan's z axis, is MINUS s * 2 pi / sectors
 *   (mod 2 pi).  The columns of a range image run AGAINST the azimuth (column w looks along pi - (w + 0.5) 2 pi / W): a vehicle
 *   turned by +yaw sees the place in columns moved up by yaw W / 2 pi, so its column j pairs with the entry's column j - yaw
 *   sectors / 2 pi = j + s.  The guess of a fit is the entry's world pose composed with R_z(-s 2 pi / sectors)
 *   (sensor.ScanContext.yaw_of is this rule on the host, wrapped to [-pi, pi)).
 * Static trip bounds, nothing waits on another thread, no atomics in the search; no host synchronisation; capturable.  Two runs,
 *   and an eager run and a graph replay, agree bit for bit.
 * ELO_ERR_ARG (nothing is launched): a NULL pointer (best_shift / best_dist may be NULL only where m == 0), batch or n < 0, H < 1,
 *   W < sectors, batch * H * W at or beyond 2^31, rings outside 1 .. ELO_PLACE_MAX_RINGS, sectors outside 1 ..
 *   ELO_PLACE_MAX_SECTORS, z_step not positive and finite, z_min not finite, min_range2 negative or NaN, edge2[1 .. rings] not
 *   positive, finite and ascending, m < 0, k outside 1 .. ELO_PLACE_MAX_K, dist / best_dist not 8-byte aligned.  An empty batch
 *   (n == 0) launches nothing and is ELO_OK.
 * LIFETIME as elo_model_render's.  Additive to ABI 26: no existing struct changes. */
#define ELO_PLACE_MAX_RINGS 32
#define ELO_PLACE_MAX_SECTORS 128
#define ELO_PLACE_LEVELS 4095
#define ELO_PLACE_MAX_K 8
typedef struct elo_scan_descriptor_args {
    int batch, H, W;
    int rings, sectors;
    double z_min, z_step;         /* m */
    double min_range2;            /* m^2 */
    double edge2[ELO_PLACE_MAX_RINGS + 1];  /* m^2: [1 .. rings] are read */
    const float *xyz;             /* (batch,H,W,3); an all-zero cell is empty */
    unsigned short *desc;         /* (batch,sectors,rings) OUT */
} elo_scan_descriptor_args;
int elo_scan_descriptor(const elo_scan_descriptor_args *a, elo_stream_t stream);
typedef struct elo_descriptor_search_args {
    int n, m;                     /* queries; entries searched, 0 .. the rows db holds */
    int rings, sectors, k;
    const unsigned short *query;  /* (n,sectors,rings) */
    const unsigned short *db;     /* (>= m,sectors,rings) */
    int *entry;                   /* (n,k) OUT */
    int *shift;                   /* (n,k) OUT */
    double *dist;                 /* (n,k) OUT */
    int *best_shift;              /* (n,m) OUT */
    double *best_dist;            /* (n,m) OUT */
} elo_descriptor_search_args;
int elo_descriptor_search(const elo_descriptor_search_args *a, elo_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Backward passes of the feature kernels above, for TRAINING (csrc/elo_backward.hip).
 * The reference trains through TensorFlow's autodiff of its stock ops (main.py:171-176): gather_nd -> scatter-add of
 * the incoming gradient (utils/pointnet_util.py:54-55, :110-111, :203-204, :277-278; masks are stop_gradient, indices
 * integer), reduce_max -> the maximal entries (even split among exact ties), softmax, scatter_nd -> gather
 * (model_util.py:264-273).  Each entry point is the adjoint of ONE forward entry point: same shapes, `grad_x` has the
 * shape of `x`.  fp32.  Outputs marked ACC receive atomic adds and must be ZERO on entry; the others are written in full.
 * Any gradient output may be NULL (not wanted).  Masked slots add nothing anywhere.
 * ------------------------------------------------------------------------- */
typedef struct elo_group_concat_bwd_args {
    int batch, npoints, K;
    int H2, W2, C;
    const float *grad_out;        /* (batch,npoints,K,3+C) */
    const int *idx;
    const float *mask;
    float *grad_centre;           /* (batch,npoints,3)  = -sum_k grad_out[..., :3]        */
    float *grad_src_xyz;          /* (batch,H2,W2,3)  ACC                                  */
    float *grad_src_feat;         /* (batch,H2,W2,C)  ACC                                  */
} elo_group_concat_bwd_args;
int elo_group_concat_backward(const elo_group_concat_bwd_args *a, elo_stream_t stream);

typedef struct elo_masked_maxpool_bwd_args {
    int batch, npoints, K, C;
    const float *x;               /* the forward input (batch,npoints,K,C) */
    const float *mask;
    const float *grad_out;        /* (batch,npoints,C) */
    float *grad_x;                /* (batch,npoints,K,C) */
} elo_masked_maxpool_bwd_args;
int elo_masked_maxpool_backward(const elo_masked_maxpool_bwd_args *a, elo_stream_t stream);

typedef struct elo_cv_encode1_bwd_args {
    int batch, npoints, K;
    int H2, W2, C;
    const float *xyz1;            /* forward inputs: the geometry code's norm needs them */
    const float *xyz2;
    const int *idx;
    const float *mask;
    const float *grad_out;        /* (batch,npoints,K,10+2C) */
    float *grad_xyz1;             /* (batch,npoints,3) */
    float *grad_feat1;            /* (batch,npoints,C) */
    float *grad_xyz2;             /* (batch,H2,W2,3)  ACC */
    float *grad_feat2;            /* (batch,H2,W2,C)  ACC */
} elo_cv_encode1_bwd_args;
int elo_cv_encode1_backward(const elo_cv_encode1_bwd_args *a, elo_stream_t stream);

typedef struct elo_cv_encode2_bwd_args {
    int batch, npoints, K;
    int H, W, C, Cc;
    const float *xyz1;            /* (batch,H,W,3) */
    const int *idx;
    const float *mask;
    const float *grad_xyz_cat;    /* (batch,npoints,K,10)   */
    const float *grad_rest;       /* (batch,npoints,K,C+Cc) */
    float *grad_xyz1;             /* (batch,H,W,3)   ACC (centre and neighbours live in the same grid) */
    float *grad_feat1;            /* (batch,H,W,C)   */
    float *grad_cost;             /* (batch,H,W,Cc)  ACC */
} elo_cv_encode2_bwd_args;
int elo_cv_encode2_backward(const elo_cv_encode2_bwd_args *a, elo_stream_t stream);

typedef struct elo_softmax_pool_bwd_args {
    int batch, npoints, K, C;
    const float *logits;          /* forward inputs */
    const float *values;
    int values_stride;
    const float *mask;
    const float *grad_out;        /* (batch,npoints,C) */
    float *grad_logits;           /* (batch,npoints,K,C); 0 at masked slots (tf.where feeds a constant there) */
    float *grad_values;           /* (batch,npoints,K,C) contiguous, whatever values_stride was */
} elo_softmax_pool_bwd_args;
int elo_masked_softmax_pool_backward(const elo_softmax_pool_bwd_args *a, elo_stream_t stream);

typedef struct elo_softmax_valid_bwd_args {
    int batch, npoints, C;
    const float *feature, *weight, *xyz;     /* forward inputs */
    const float *grad_out;        /* (batch,1,C) */
    float *grad_feature;          /* (batch,npoints,C) */
    float *grad_weight;           /* (batch,npoints,C) */
    const float *out, *stats;     /* the forward's out (batch,1,C) and stats (batch,2,C): with them the adjoint is one
                                     element-wise pass; both NULL: the kernel recomputes them (one block per batch element
                                     and 64 channels, three serial passes over the points -- 300 us at 3600 points) */
} elo_softmax_valid_bwd_args;
int elo_softmax_valid_backward(const elo_softmax_valid_bwd_args *a, elo_stream_t stream);

/* Adjoint of elo_warp_project.  `scratch` is the forward call's scratch as it left it (per-cell minimum range, zero-point
 * flags, per-point cell and range bits: who won each cell); the forward's projection constants come along because the
 * cells a zero point can fall in are recomputed from them.  Gradients never reach the cell indices (model_util.py:255-273). */
typedef struct elo_warp_project_bwd_args {
    int batch, npoints, C;
    int H, W;
    float az_res, vert_res, vert_off;
    const float *xyz;             /* forward input (batch,npoints,3) */
    const float *q, *t;           /* forward inputs, or NULL = the forward did not warp */
    const unsigned *scratch;
    const float *grad_out_xyz;    /* (batch,H,W,3) or NULL */
    const float *grad_out_feat;   /* (batch,H,W,C) or NULL */
    const float *grad_warped;     /* (batch,npoints,3) or NULL: gradient on the forward's `warped` output */
    float *grad_xyz;              /* (batch,npoints,3) */
    float *grad_feat;             /* (batch,npoints,C) */
    float *grad_q;                /* (batch,4)  ACC */
    float *grad_t;                /* (batch,3)  ACC */
} elo_warp_project_bwd_args;
int elo_warp_project_backward(const elo_warp_project_bwd_args *a, elo_stream_t stream);

/* ---------------------------------------------------------------------------
 * Training layer: the ROW REDUCTIONS of conv2d -> batch norm (batch statistics) -> ReLU
 * (utils/tf_util.py:120-185 conv2d, :512-563 batch_norm_template) on a (rows, C) fp32 matrix, rows = B*N*K.
 * The dense products themselves (z = x W + b, dx = dz W^T) stay library GEMMs; these entry points are the passes over
 * the rows around them.  C: a power of two in 4..256 (every batch-normalised width of the model); all tensors fp32,
 * 16-byte aligned.  Reductions are per-block partial sums in caller-provided scratch, combined in a fixed order (fp64
 * for the batch-norm sums): no atomics, bit-reproducible.
 * ------------------------------------------------------------------------- */
#define ELO_BN_MAX_PARTS 512      /* partial rows of the batch-norm reductions: scratch = 2 * C * ELO_BN_MAX_PARTS floats */
typedef struct elo_bn_stats_args {
    long rows; int C;
    const float *z;               /* (rows,C) */
    float *scratch;               /* (ELO_BN_MAX_PARTS, 2, C) */
    float eps, momentum;          /* 1e-3; 1 - bn_decay */
    float *mean, *invstd;         /* (C) OUT: batch mean, 1/sqrt(biased batch variance + eps) */
    float *running_mean, *running_var;   /* (C) IN/OUT or both NULL: r <- (1-momentum) r + momentum * (mean | unbiased var) */
    int groups;                   /* > 1: the rows are `groups` equal contiguous blocks with their OWN batch statistics (the two frames of a
                                   * Siamese batch in one launch: utils/tf_util.py's layer called twice with shared variables): mean, invstd
                                   * are (groups,C), the moving averages take the groups' moments one after the other; 0 / 1: one group */
} elo_bn_stats_args;
int elo_bn_stats(const elo_bn_stats_args *a, elo_stream_t stream);
long elo_bn_scratch_floats(int C, int groups);  /* the scratch of elo_bn_stats / elo_bn_backward AS THIS BUILD sizes it (a host that mirrors the #define
                                             * and a stale library disagree silently: ask) */

typedef struct elo_bn_apply_args {
    long rows; int C;
    const float *z, *mean, *invstd, *gamma, *beta;
    int relu;                     /* 1: y = max(., 0) */
    float *y;                     /* (rows,C) OUT (may alias z) */
    int groups;                   /* as elo_bn_stats_args: mean, invstd (groups,C) */
} elo_bn_apply_args;
int elo_bn_apply(const elo_bn_apply_args *a, elo_stream_t stream);

/* g = dy * [gamma*xhat + beta > 0] (relu = 1) or dy;  sums <- [sum g | sum g*xhat] = [d beta | d gamma];
 * dz = gamma * invstd * (g - sum g / rows - xhat * sum g*xhat / rows)        (three launches) */
typedef struct elo_bn_backward_args {
    long rows; int C;
    const float *dy, *z, *mean, *invstd, *gamma, *beta;
    int relu;
    float *scratch;               /* (ELO_BN_MAX_PARTS, 2, C) */
    float *sums;                  /* (2*C) OUT [d beta | d gamma] */
    float *dz;                    /* (rows,C) OUT (may alias dy); NULL: the sums only (two launches) -- dz is then formed by elo_dense_rows */
    int groups;                   /* as elo_bn_stats_args: mean, invstd (groups,C), sums (groups,2*C) -- d beta / d gamma are their sums over the groups */
} elo_bn_backward_args;
int elo_bn_backward(const elo_bn_backward_args *a, elo_stream_t stream);

/* dW = x^T g (Cin,Cout row-major), db = column sums of g (or NULL): fp32 operands on v_mfma_f32_16x16x4_f32, fp32
 * accumulation per row slice, slices summed in order.  Any Cin, Cout.
 * scratch: elo_weight_grad_slices(rows, Cin, Cout) * (Cin*Cout + Cout) floats. */
typedef struct elo_weight_grad_args {
    long rows; int Cin, Cout;
    const float *x;               /* (rows,Cin)  */
    const float *g;               /* (rows,Cout) */
    float *dW;                    /* (Cin,Cout) OUT */
    float *db;                    /* (Cout) OUT or NULL */
    float *scratch;
} elo_weight_grad_args;
int elo_weight_grad_slices(long rows, int Cin, int Cout);
int elo_dense_weight_grad(const elo_weight_grad_args *a, elo_stream_t stream);

/* WHICH KERNELS the entry points above launch (host-only queries: nothing is launched, no tensor pointer is dereferenced -- only the
 * pointers' VALUES are read, for null and for their alignment).  Each launcher calls the same function, so the answer is what a launch
 * takes.  All forms of an entry point compute the same function.
 * elo_dense_weight_grad_form(a): ELO_WGRAD_FORM(CI, CO, xv, gv, waves, gy, gz), or the negative elo_status with which
 *   elo_dense_weight_grad would refuse the block (ELO_ERR_ARG: a NULL block or tensor pointer other than db, a size <= 0; ELO_ERR_LIMIT:
 *   rows * max(Cin, Cout) >= 2^31, or more than 2047 x 4095 -- 262140 in all -- blocks of dW).
 *     CI x CO: the 16 x 16 tiles of dW one wave owns (a block).  CO = 4 from 4 column tiles on, 2 from 2, else 1; CI = the count in
 *       1..4 that pads the ceil(Cin / 16) row tiles least, the larger on a tie or while the padding stays <= 25 %.
 *     xv / gv: x / g is loaded as CI / CO consecutive channels per lane in one instruction (Cin % (16 CI) == 0 resp. Cout % (16 CO) == 0,
 *       the tensor 16-byte aligned, CI != 3), else one channel per tile.  Same products in the same order: the same bits.
 *     gy x gz: the grid of blocks; waves: per workgroup, min(gy * gz, 4) -- the workgroups are (slices, ceil(gy * gz / waves)).
 *   One of 42 compiled kernels: CI in 1..4, CO in {1, 2, 4}, xv (never with CI = 3), gv.
 * elo_bn_parts(rows_per_group, C): the partial rows (workgroups per group) of the reductions of elo_bn_stats and elo_bn_backward:
 *   ceil(ceil(rows_per_group / (1024 / C)) / 8), at least 1, at most ELO_BN_MAX_PARTS; or the negative elo_status with which those
 *   refuse the sizes (ELO_ERR_ARG: no rows; ELO_ERR_LIMIT: C not a power of two in 4..256). */
#define ELO_WGRAD_FORM(CI, CO, xv, gv, waves, gy, gz) \
    (((CI) - 1) | ((CO) >> 1) << 2 | (xv) << 4 | (gv) << 5 | ((waves) - 1) << 6 | (gz) << 8 | (gy) << 20)
#define ELO_WGRAD_CI(form) (((form) & 3) + 1)
#define ELO_WGRAD_CO(form) (1 << ((form) >> 2 & 3))
#define ELO_WGRAD_XV(form) ((form) >> 4 & 1)
#define ELO_WGRAD_GV(form) ((form) >> 5 & 1)
#define ELO_WGRAD_WAVES(form) (((form) >> 6 & 3) + 1)
#define ELO_WGRAD_GZ(form) ((form) >> 8 & 4095)
#define ELO_WGRAD_GY(form) ((form) >> 20)
int elo_dense_weight_grad_form(const elo_weight_grad_args *a);
int elo_bn_parts(long rows_per_group, int C);

/* out = x W (+ bias) over the rows of a training layer (utils/tf_util.py:120-185: conv2d 1x1 and its adjoint dx = dz W^T with
 * transposed = 1), fp32 on v_mfma_f32_16x16x4_f32: one pass over x, W staged once per workgroup in LDS.  Any Cin; Cout <= 192
 * and ceil(Cin/16) * ceil(Cout/16) <= 160 (elo_dense_rows_supported).  scratch != NULL: ALSO the batch-norm moments of out, from the
 * accumulators (what elo_bn_stats computes with one more pass over out): mean, invstd and the moving averages as there. */
#define ELO_DENSE_MAX_PARTS 2048  /* scratch = 2 * Cout * ELO_DENSE_MAX_PARTS floats */
typedef struct elo_dense_rows_args {
    long rows; int Cin, Cout;
    const float *x;               /* (rows,Cin), 16-byte aligned */
    const float *W;               /* (Cin,Cout) row-major; transposed = 1: (Cout,Cin) row-major */
    int transposed;
    const float *bias;            /* (Cout) or NULL */
    float *out;                   /* (rows,Cout) OUT, 16-byte aligned */
    float *scratch;               /* NULL: no moments */
    float eps, momentum;
    float *mean, *invstd;         /* (Cout) OUT when scratch != NULL */
    float *running_mean, *running_var;   /* (Cout) IN/OUT or both NULL */
    /* bn_z != NULL (dx = dz W^T of a batch-normalised layer; Cin = that layer's width, % 4 == 0; no moments): x holds dy and the operand
     * is dz = gamma invstd (g - sum_g / rows - xhat sum_gxhat / rows), formed on the load and ALSO written to bn_dz (rows,Cin) --
     * elo_bn_backward's third launch inside this pass.  bn_sums: its (2*Cin) [sum g | sum g xhat]. */
    const float *bn_z, *bn_mean, *bn_invstd, *bn_gamma, *bn_beta, *bn_sums;
    int bn_relu;
    float *bn_dz;
    int groups;                   /* as elo_bn_stats_args, for the moments (mean, invstd (groups,Cout)) and for the bn_* operand
                                   * (bn_mean, bn_invstd (groups,Cin), bn_sums (groups,2*Cin)); the plain product ignores it */
} elo_dense_rows_args;
int elo_dense_rows_supported(long rows, int Cin, int Cout);
long elo_dense_rows_scratch_floats(int Cout, int groups);
int elo_dense_rows(const elo_dense_rows_args *a, elo_stream_t stream);

/* Adam (torch.optim.Adam's arithmetic; the reference trains with tf.train.AdamOptimizer, main.py:171-176) over ONE flat
 * fp32 parameter buffer in one launch: every variable, its gradient and its two moments are views of four buffers of n
 * floats.  hyper (device, 4 floats, written by the host before the step): [lr / (1 - beta1^t), 1 / sqrt(1 - beta2^t), eps, -]. */
typedef struct elo_adam_flat_args {
    long n;
    float *param;                 /* (n) IN/OUT */
    const float *grad;            /* (n)        */
    float *exp_avg;               /* (n) IN/OUT */
    float *exp_avg_sq;            /* (n) IN/OUT */
    const float *hyper;           /* (4) device */
    float beta1, beta2;
    float one_minus_beta1, one_minus_beta2;   /* (float)(1.0 - beta) from the caller's doubles */
} elo_adam_flat_args;
int elo_adam_flat(const elo_adam_flat_args *a, elo_stream_t stream);

/* The per-pair pose algebra of a TRAINING step in one launch each way (inference has it inside pose_head_kernel):
 * q_det = normalise(q_raw); coarse level (q_coarse == NULL): q = q_det, t = t_det; refinement level: q = q_det (x) q_coarse,
 * t = (q_det (x) [0, t_coarse] (x) q_det^-1)[1:] + t_det; q_norm = normalise(q)   (pwclo_model.py:197-208, :262-280;
 * model_util.py:17-69).  Forward: grad_q == NULL, writes q, t, q_norm.  Backward: grad_q / grad_t / grad_q_norm given (all
 * three), writes grad_q_raw, grad_t_det and (refinement level) grad_q_coarse, grad_t_coarse.  All tensors (batch,4) / (batch,3) fp32. */
typedef struct elo_pose_compose_args {
    int batch;
    const float *q_raw, *t_det, *q_coarse, *t_coarse;
    float *q, *t, *q_norm;
    const float *grad_q, *grad_t, *grad_q_norm;
    float *grad_q_raw, *grad_t_det, *grad_q_coarse, *grad_t_coarse;
} elo_pose_compose_args;
int elo_pose_compose(const elo_pose_compose_args *a, elo_stream_t stream);

/* get_loss (pwclo_model.py:437-481): per level L_q = mean_b |q_gt - normalise(q)|_2 (+1e-10 under the root), L_x = mean
 * sqrt((t - t_gt)^2 + 1e-10), level = L_x e^-w_x + w_x + L_q e^-w_q + w_q; loss = 0.2 l0 + 0.4 l1 + 0.8 l2 + 1.6 l3.
 * q[lv] / t[lv]: level lv = 0..3 (batch,4) / (batch,3).  Forward: grad_out == NULL, writes *loss.  Backward: grad_out (the
 * incoming scalar gradient, device) given, writes grad_q[lv], grad_t[lv], *grad_w_x, *grad_w_q. */
typedef struct elo_pose_loss_args {
    int batch;
    const float *q[4], *t[4];
    const float *q_gt, *t_gt;     /* (batch,4), (batch,3) */
    const float *w_x, *w_q;       /* scalars (device) */
    float *loss;
    const float *grad_out;
    float *grad_q[4], *grad_t[4];
    float *grad_w_x, *grad_w_q;
} elo_pose_loss_args;
int elo_pose_loss(const elo_pose_loss_args *a, elo_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Fused inference kernels: gather/encode -> chain of 1x1 convolutions (BN and
 * bias folded, ReLU) -> pooling, in ONE launch with the activations of a
 * 16/32-row tile resident in LDS and the contractions on the matrix cores.
 * They compute what the unfused kernels above + the hipBLASLt GEMMs compute,
 * for the launch-bound small-batch regime.
 *
 * A layer is  y = act(x[K] @ W[K,N] + b[N]).  `w_packed` is W zero-padded to (Kp = ceil16(K), Np = ceil16(N)) and stored
 * in MFMA fragment order, every weight SPLIT into fp16 hi + lo (hi = fp16(w), lo = fp16(w - hi)): the kernels compute
 * hi*hi + hi*lo + lo*hi on the fp16 matrix cores with fp32 accumulation (2^-20 relative per product; fp16 range:
 * |x| < 65504 saturates -- see ELO_RANGE_CHECK below).  With KS = Kp / 16 blocks of 16 k and lane = 16*kq + n, the
 * fragment element (cb, ks, lane, s) is  W[ks*16 + 4*kq + s][cb*16 + n],  s = 0..3.  Per column block cb (contiguous,
 * KS * 1 KiB) the K axis is laid out as
 *     KS / 2 PAIRS of 32 k  (v_mfma_f32_16x16x32_f16), pair p = blocks 2p and 2p+1:
 *         1 KiB of hi8: per lane the eight halves  hi(cb, 2p, lane, 0..3), hi(cb, 2p+1, lane, 0..3)   (16 bytes),
 *         1 KiB of lo8: the same eight elements' lo halves,
 *     then, for odd KS, one TAIL of 16 k  (v_mfma_f32_16x16x16_f16), block KS-1:
 *         1 KiB: per lane  [hi0 hi1 hi2 hi3 | lo0 lo1 lo2 lo3]  (16 bytes),
 * so that every wave-wide 16-byte load is a contiguous 1 KiB.  ELO_PRODUCTS_HALF keeps only the round-to-nearest
 * halves: 1 KiB per pair (8 halves per lane), 512 bytes per tail.  Activations are split the same way ONCE, by the
 * layer (or the gather) that produces them, and live in the LDS tile as [hi x4 | lo x4] per four consecutive columns.
 * (A library built with -DELO_DENSE_F32 expects KS blocks of four fp32 weights per lane instead -- element order as
 * above, no pairs -- and uses v_mfma_f32_16x16x4_f32.)
 * `bias` has Np fp32 entries (zero padded).  Packing is done once per parameter update by the host
 * (efficientlo-net_amd/fused.py).
 *
 * Feature storage.  Every FEATURE tensor these kernels read or write in HBM (fields typed `void *`) is fp32 or fp16
 * according to the call's `feat_dtype` (ELO_F32 / ELO_F16; BASELINE configs[2]: s = 2 in SURVEY.md section 8(d)).
 * Geometry (xyz, centres, new_xyz), indices and masks are always fp32 / int32; all arithmetic is as described above
 * whatever the storage (an fp16 input is an exact operand: hi = x, lo = 0).  fp16 rows are read 16 bytes at a time:
 * channel counts must be multiples of 8 (fp32: of 4) for the vector paths; other widths take an element-wise path
 * where one exists (set-conv, row-wise MLP) and are an ELO_ERR_LIMIT otherwise (cost volume).
 * Masks are 0/1 by contract: `x * mask` is implemented as a select.
 *
 * Operands beyond the fp16 range saturate: elo_range_check() above counts them in a debugging run.
 *
 * The LDS limit.  A tile launch keeps `rows` (16 or 32) tile rows of S words in dynamic LDS, S = the widest of the call's
 * concatenated input and its layer widths, each rounded up to 16 columns (plus a few words of bank padding), beside 768
 * bytes of per-row metadata and, with in-kernel grouping, the visiting order.  A call whose tile would need more than
 * 64 KiB -- a row-wise MLP or a set-conv over a concatenation of more than 496 columns (32-row tile; 992 where the launcher
 * takes the 16-row tile) -- is refused with ELO_ERR_LIMIT before any HIP call, pre-grouped calls included.  The elo_*_form
 * queries below answer the same code; for such a row-wise MLP elo_mlp_sv_parts and elo_cv_stage2_upconv_form answer 0 (it cannot be
 * launched, so nothing can ride on it).  A call without rows or points launches nothing and is ELO_OK whatever its widths.
 * ------------------------------------------------------------------------- */
enum { ELO_PRODUCTS_SPLIT = 0,      /* fp32-class: hi/lo split operands, three fp16 MFMA products (default)     */
       ELO_PRODUCTS_HALF = 1 };     /* fp16 arithmetic: operands rounded to nearest fp16, ONE product, fp32 accumulate;
                                       `w_packed` then holds the halves only (pairs / tail as above, half the bytes).
                                       All layers of one launch must use the same mode.  (BASELINE configs[2].)   */

typedef struct elo_dense {
    const float *w_packed;
    const float *bias;
    int K, N;
    int relu;
    const float *w_plain;         /* optional: the same folded W as plain row-major (K,N); lets narrow chains
                                     (all widths <= 32) run on the wave-per-point VALU kernel (fp32 in either mode) */
    int products;                 /* ELO_PRODUCTS_SPLIT / ELO_PRODUCTS_HALF */
} elo_dense;

#define ELO_MAX_CHAIN 3

/* Optional in-kernel neighbour grouping for the fused kernels: with random_hw != NULL the kernel
 * runs the grouping itself (same semantics as elo_fused_conv_random_k / _select_k with flag_copy = 0,
 * one wave per centre) and the idx / mask INPUTS of the argument block are ignored (may be NULL).
 * idx_out / mask_out, when given, receive the (batch,npoints,K,3) indices and (batch,npoints,K) mask
 * exactly as the stand-alone ops would write them (used by the parity tests). */
typedef struct elo_group_spec {
    const int *random_hw;         /* (kernel_h*kernel_w) visiting order, or NULL = use idx/mask inputs */
    int kernel_h, kernel_w;
    float distance;
    int stride_h, stride_w;
    int *idx_out;                 /* nullable */
    float *mask_out;              /* nullable */
    const int *decoded_hw;        /* nullable: random_hw already decoded, entry i = (dh << 16) | (dw & 0xffff) with
                                   * dh = random_hw[i] / kernel_w - kernel_h/2, dw = random_hw[i] % kernel_w - kernel_w/2;
                                   * spares every tile two integer divisions per window slot */
} elo_group_spec;

/* set-conv / set-upconv stage 1:  group_concat -> chain -> masked max over K.
 * utils/pointnet_util.py:197-230 (down_conv) and :272-298 (up_conv). K <= 32.
 * centre_hw != NULL: centre = xyz1_grid[b, centre_hw[b,n,0], centre_hw[b,n,1]] and is also
 * written to new_xyz (the `new_xyz_proj` output of down_conv, :206); else centre = centre_xyz[b,n].
 * layers[0] expects its input rows ordered [features (C), xyz difference (3)] (the reference concatenates
 * [xyz_diff, features], :213: the host permutes the weight rows when packing; `w_plain` likewise). */
typedef struct elo_setconv_args {
    int batch, npoints, K;
    int H, W;                     /* xyz1 grid (only with centre_hw)        */
    int H2, W2, C;                /* gathered grid and its feature channels */
    const float *xyz1_grid;       /* (batch,H,W,3) or NULL                  */
    const int *centre_hw;         /* (batch,npoints,2) or NULL              */
    const float *centre_xyz;      /* (batch,npoints,3) or NULL              */
    const float *src_xyz;         /* (batch,H2,W2,3)                        */
    const void *src_feat;         /* (batch,H2,W2,C)   feat_dtype           */
    const int *idx;
    const float *mask;
    int n_layers;
    elo_dense layers[ELO_MAX_CHAIN];
    void *out;                    /* (batch,npoints,layers[last].N) feat_dtype */
    float *new_xyz;               /* (batch,npoints,3) or NULL              */
    elo_group_spec group;         /* random-k; needs xyz1_grid; centre_hw == NULL: centre n is pixel (n / W, n % W) */
    int feat_dtype;               /* ELO_F32 / ELO_F16 */
    unsigned long long *range_counter;   /* the CHECKED instances (elo_range_check) add their count of out-of-range operands here (a lane's own
                                          * device word: a violation is then that lane's, not every lane's); NULL: the process-wide counter of
                                          * elo_range_violations() */
} elo_setconv_args;
int elo_setconv_fused(const elo_setconv_args *a, elo_stream_t stream);
/* two independent jobs of identical shape in ONE launch (b may be NULL): the embedding and the embedding-mask
 * set-upconv of a refinement level (pwclo_model.py:247,250) share everything but weights and one input */
int elo_setconv_fused2(const elo_setconv_args *a, const elo_setconv_args *b, elo_stream_t stream);

/* Row-wise MLP over the concatenation of up to three row-aligned sources:
 * flow_predictor (utils/pointnet_util.py:153-175) and set-upconv stage 2 (:303-311). */
typedef struct elo_mlp_args {
    long rows;
    int n_sources;
    const void *src[3];           /* (rows, src_width[i]) feat_dtype */
    int src_width[3];
    int n_layers;
    elo_dense layers[ELO_MAX_CHAIN];
    void *out;                    /* (rows, layers[last].N) feat_dtype */
    /* Optional SECOND row-wise MLP in the same launch (n_layers2 > 0), fed by the first one's output: its input rows
     * are  [ out | before (w_before) | after (w_after) ]  -- flow_predictor's concat [points_f1, upsampled_feat,
     * cost_volume] (utils/pointnet_util.py:161-166) with the set-upconv stage 2 (:303-311) as the first MLP and its
     * output moved to the front (the host permutes the rows of layers2[0] when packing; layers[last].N % 4 == 0).
     * `out` is still written; the second output goes to out2. */
    int n_layers2;
    elo_dense layers2[ELO_MAX_CHAIN];
    const void *before;           /* (rows, w_before) feat_dtype, or NULL with w_before == 0 */
    int w_before;
    const void *after;            /* (rows, w_after)  feat_dtype, or NULL with w_after == 0  */
    int w_after;
    void *out2;                   /* (rows, layers2[last].N) feat_dtype */
    int feat_dtype;               /* ELO_F32 / ELO_F16 */
    /* Optional side job (job 0 of a paired launch only): the launch's workgroups also clear the buffers of an
     * elo_warp_project / elo_pose_head_warp call further down the stream -- elo_pose_head_args.clear_* semantics, for a
     * pose head run with ready_parts (which has no partial-sums launch of its own left to do it).  clear_scratch == NULL: no side job. */
    unsigned *clear_scratch;      /* first clear_cells + 4*clear_images words <- 0x7f7f7f7f */
    float *clear_xyz;             /* clear_cells*3 floats <- 0 */
    void *clear_feat;             /* clear_cells*clear_C elements of feat_dtype <- 0, NULL when clear_C == 0 */
    long clear_cells;             /* images*H*W of the projection */
    int clear_C;
    int clear_images;
    /* Batch size the rows came from (rows = batch x points), 0 = unknown: from ELO_THROUGHPUT_BATCH on the launcher takes the
     * register-resident kernel for every launch of 2048 rows or more (the GPU is full: a kernel costs its CU-time), below
     * that only from 8192 rows (a forward is a latency chain there and the tile kernel is faster). */
    int batch_hint;
    /* Optional (sv_scratch != NULL, the first job of a launch): the launch ALSO computes the first half of softmax_valid
     * (model_util.py:319-343) over its final output -- per row tile and channel the (maximum, denominator, weighted sum) triple
     * of the masked softmax over the tile's points, in elo_softmax_valid's scratch layout -- so the pose head that follows needs
     * no partial-sums launch (elo_pose_head_args.ready_parts = elo_mlp_sv_parts(a, b)).  The final output (out2, or out of a
     * one-stage MLP) must be 64 wide.
     *   paired launch (elo_mlp_fused2):  job a's final output are the LOGITS (`weight`), job b's the FEATURES; sv_feature NULL;
     *   single launch (elo_mlp_fused):   the final output are the logits, the features are sv_feature.
     * Rows are (batch, sv_npoints): a row tile never straddles two batch elements.  Taken by the tile kernel only: call
     * elo_mlp_sv_parts first -- 0 means this launch would run as a register-resident chain (or has another shape) and the
     * sv_* fields must stay NULL. */
    float *sv_scratch;            /* 3 * batch * ELO_SV_MAX_PARTS * 64 floats */
    const float *sv_xyz;          /* (batch, sv_npoints, 3): a row is a valid point unless all three are exactly 0 */
    const void *sv_feature;       /* single launch: (rows, 64) feat_dtype; paired launch: NULL */
    int sv_npoints;               /* rows per batch element (rows % sv_npoints == 0) */
    unsigned long long *range_counter;   /* the CHECKED instances (elo_range_check) add their count of out-of-range operands here (a lane's own
                                          * device word: a violation is then that lane's, not every lane's); NULL: the process-wide counter of
                                          * elo_range_violations() */
} elo_mlp_args;
#define ELO_THROUGHPUT_BATCH 4
int elo_mlp_fused(const elo_mlp_args *a, elo_stream_t stream);
int elo_mlp_fused2(const elo_mlp_args *a, const elo_mlp_args *b, elo_stream_t stream);   /* paired launch, as above */
/* Slices per batch element the launch (a, b) -- b NULL: a single launch -- would write with sv_scratch set (the sv_* fields
 * of `a` need not be filled yet, sv_npoints must be); 0: it cannot (chain-kernel regime, shape, more than ELO_SV_MAX_PARTS tiles). */
int elo_mlp_sv_parts(const elo_mlp_args *a, const elo_mlp_args *b);

/* Attentive cost volume, stage 1 (utils/pointnet_util.py:54-100) in one launch:
 * encode -> CV_0..2 -> CV_xyz -> sum_CV_0..1 -> masked softmax over K -> weighted sum.
 * cv0 expects its input rows ordered [feat1 (C), feat2 grouped (C), geometry (10)] (reference: [geometry, feat1,
 * feat2], :62-66) and sum_cv0 [x (64), xyz-encoding (64)] (reference: [encoding, x], :84): the host permutes the
 * weight rows when packing.  K <= 32, C % 4 == 0 (fp16 storage: C % 8 == 0). */
typedef struct elo_cv1_args {
    int batch, npoints, K;
    int H2, W2, C;
    const float *xyz1;            /* (batch,npoints,3) */
    const void *feat1;            /* (batch,npoints,C)  feat_dtype */
    const float *xyz2;            /* (batch,H2,W2,3)   */
    const void *feat2;            /* (batch,H2,W2,C)    feat_dtype */
    const int *idx;
    const float *mask;
    elo_dense cv0, cv1, cv2, cv_xyz, sum_cv0, sum_cv1;     /* N: 128,64,64,64,128,64 */
    void *out;                    /* (batch,npoints,64) feat_dtype */
    elo_group_spec group;         /* select-k of xyz2 around every pixel of xyz1 (npoints == H2*W2, stride 1) */
    int feat_dtype;               /* ELO_F32 / ELO_F16 */
    unsigned long long *range_counter;   /* the CHECKED instances (elo_range_check) add their count of out-of-range operands here (a lane's own
                                          * device word: a violation is then that lane's, not every lane's); NULL: the process-wide counter of
                                          * elo_range_violations() */
} elo_cv1_args;
int elo_cv_stage1_fused(const elo_cv1_args *a, elo_stream_t stream);
/* debugging hooks of the register-resident ("chain") kernel forms -- cv1_rr_kernel, cv2_rr_kernel, setconv_rr_kernel,
 * mlp2_rr_kernel: the forms elo_cv_stage1_fused / elo_cv_stage2_fused (pre-grouped calls), elo_setconv_fused2 and
 * elo_mlp_fused2 take from their row thresholds on.  Both forms of an entry point give the same bits.
 * elo_debug_cv1_rr(0) keeps ALL FOUR entry points on their tile kernels, 1 allows the chain forms (the default, also
 * ELO_CV1_RR), -1 = back to the environment's choice; returns the previous setting.  (The name is round 3's, when the
 * switch covered cost-volume stage 1 only.)
 * elo_debug_rr_rows(setconv_rows, mlp_rows): rows per launch from which elo_setconv_fused2 / elo_mlp_fused2 take the chain
 * form; -1 = the built-in regimes (or ELO_SETCONV_RR_ROWS / ELO_MLP_RR_ROWS, read once per process).
 * elo_debug_rr_launches(counts4, reset): launches of [cv1_rr, cv2_rr, setconv_rr, mlp2_rr] since the last reset. */
int elo_debug_cv1_rr(int on);
int elo_debug_rr_rows(long setconv_rows, long mlp_rows);
int elo_debug_rr_launches(unsigned long long *counts4, int reset);
int elo_debug_sv_ride_launches(unsigned long long *count, int reset);     /* ... and of mlp_sv_kernel (elo_mlp_args.sv_*) */
int elo_debug_chain_pair_launches(unsigned long long *count, int reset);  /* ... and of cv1_setconv_rr_kernel (elo_cv_stage1_setconv_chain) */
int elo_debug_upconv_ride_launches(unsigned long long *count, int reset); /* ... and of cv2_upconv_kernel (elo_cv_stage2_upconv_fused) */
/* the two narrow set-conv layers of the pyramid (6 -> 8 -> 8 -> 16 and 19 -> 16 -> 16 -> 32, K = 32; elo_setconv_fused with
 * elo_dense.w_plain given): 1 = setconv_narrow_kernel, the MLP on the matrix cores, for the 19-channel layer (the default;
 * also ELO_SETCONV_NARROW_MFMA; the 6-channel layer stays on the VALU kernel: slower on the matrix cores, measured), 0 =
 * setconv_small_kernel, the fp32 VALU form, for both (the only one in the fp32-MFMA build), -1 = back to the environment's
 * choice; returns the previous setting.  Results agree to fp32-class rounding. */
int elo_debug_narrow_mfma(int on);
/* elo_debug_narrow_launches(counts2, reset): launches of [setconv_narrow_kernel, setconv_small_kernel] since the last reset
 * (the oracle test of the matrix-core form asserts through it which kernel produced the tensor) */
int elo_debug_narrow_launches(unsigned long long *counts2, int reset);
/* elo_cv_stage1_fused AND one or two set-conv jobs (elo_setconv_fused / elo_setconv_fused2 semantics, tile-kernel form;
 * jb may be NULL) in ONE launch: the first workgroups of the grid run cost-volume tiles, the rest set-conv tiles.
 * For branches that only share inputs -- the cost volume and the two set-upconvs of a refinement level
 * (pwclo_model.py:242-250), the initial cost volume and the layer-3 set-conv of the pyramid (:138, :170) -- so that a
 * small-batch forward pays one launch boundary and keeps both branches in flight together.  Same results bit for bit. */
int elo_cv_stage1_setconv_fused(const elo_cv1_args *a, const elo_setconv_args *ja, const elo_setconv_args *jb, elo_stream_t stream);
/* The same move on the register-resident kernels (round 5): the cost volume PRE-GROUPED (idx / mask of the select-k pre-pass), two
 * set-conv jobs of the set-upconv shape (64 + 3 -> 128 -> 64, in-kernel random-k): one launch of 512-thread chain workgroups, the
 * first ones on the cost volume, then job a, then job b -- the bits of elo_cv_stage1_fused + elo_setconv_fused2.
 * elo_cv_stage1_setconv_chain_form: 1 when (a's C and layers, the jobs' shape / size / products mode) take it; `a` need not carry
 * idx / mask or a grouping spec yet. */
int elo_cv_stage1_setconv_chain_form(const elo_cv1_args *a, const elo_setconv_args *ja, const elo_setconv_args *jb);
int elo_cv_stage1_setconv_chain(const elo_cv1_args *a, const elo_setconv_args *ja, const elo_setconv_args *jb, elo_stream_t stream);

/* Attentive cost volume, stage 2 (utils/pointnet_util.py:104-146) in one launch.
 * sum_cost0 expects input rows ordered [cost[idx]*m (64), xyz-encoding (64), feat1 (C)]
 * (reference order [encoding, feat1, grouped], :129). K <= 32, npoints == H*W, C % 4 == 0 (fp16: % 8), C <= 64. */
typedef struct elo_cv2_args {
    int batch, npoints, K;
    int H, W, C;
    const float *xyz1;            /* (batch,H,W,3)  */
    const void *feat1;            /* (batch,H,W,C)  feat_dtype */
    const void *cost;             /* (batch,H,W,64) feat_dtype */
    const int *idx;
    const float *mask;
    elo_dense xyz_enc, sum_cost0, sum_cost1;               /* N: 64,128,64 */
    void *out;                    /* (batch,npoints,64) feat_dtype */
    elo_group_spec group;         /* random-k of xyz1 around every pixel of xyz1 (stride 1) */
    int feat_dtype;               /* ELO_F32 / ELO_F16 */
    unsigned long long *range_counter;   /* the CHECKED instances (elo_range_check) add their count of out-of-range operands here (a lane's own
                                          * device word: a violation is then that lane's, not every lane's); NULL: the process-wide counter of
                                          * elo_range_violations() */
} elo_cv2_args;
int elo_cv_stage2_fused(const elo_cv2_args *a, elo_stream_t stream);
/* elo_cv_stage2_fused AND the two set-upconv stage-2 MLPs of the level (elo_mlp_fused2(ja, jb) semantics; one-stage jobs:
 * n_layers2 = 0, no clear_* / sv_* side jobs) in ONE launch: the first workgroups run cost-volume tiles, the rest MLP row
 * tiles of ja, then jb.  The set-upconvs read only the stage-1 output of the launch in front, so they leave the critical
 * path of the predictors, which then run on [out | points_f1 | cost] alone.  Tile-kernel form only: the cost volume groups in
 * the kernel and the two-stage pair these jobs would begin is below the chain kernel's rows (elo_mlp_fused2).
 * elo_cv_stage2_upconv_form: 1 when the launch takes them (else the separate entry points).  Same results bit for bit. */
int elo_cv_stage2_upconv_form(const elo_cv2_args *a, const elo_mlp_args *ja, const elo_mlp_args *jb);
int elo_cv_stage2_upconv_fused(const elo_cv2_args *a, const elo_mlp_args *ja, const elo_mlp_args *jb, elo_stream_t stream);

/* WHICH KERNEL elo_setconv_fused2 / elo_mlp_fused2 / elo_cv_stage1_fused / elo_cv_stage2_fused launch for an argument block
 * (b may be NULL: a single job).  Host-only queries: nothing is launched and no tensor is dereferenced -- only the pointers'
 * VALUES are read (NULL or not, alignment) -- and the current elo_tuning is read as the launcher reads it.  Each entry point
 * switches on the same function, so the answer is what a launch with these arguments takes.
 * Return: ELO_FUSED_FORM(family, rows, products) of the enumerators below, or the negative elo_status with which the entry
 * point would refuse the block (the LDS limit above included).  With no points / rows the entry points launch nothing and the
 * answer is ELO_FUSED_FORM(ELO_FUSED_TILE, 32, ELO_FUSED_SPLIT).
 *   family:   TILE (setconv_kernel, mlp_kernel, cv1_kernel / cv1_meta_kernel, cv2_kernel), CHAIN (the register-resident kernels),
 *             NARROW_MFMA / NARROW_VALU (the wave-per-point set-conv kernels), SV_RIDE (mlp_sv_kernel: sv_scratch is set);
 *   rows:     16 or 32, the tile height (TILE and SV_RIDE; 0 for the other families, which have no tile of their own);
 *   products: SPLIT, HALF, or CHECKED (the split instances that also count out-of-range operands: elo_range_check).  The narrow
 *             VALU kernel computes in fp32 whatever the layers say: it answers SPLIT. */
enum { ELO_FUSED_TILE = 0, ELO_FUSED_CHAIN = 1, ELO_FUSED_NARROW_MFMA = 2, ELO_FUSED_NARROW_VALU = 3, ELO_FUSED_SV_RIDE = 4 };
enum { ELO_FUSED_SPLIT = 0, ELO_FUSED_HALF = 1, ELO_FUSED_CHECKED = 2 };
#define ELO_FUSED_FORM(family, rows, products) ((family) | (rows) << 4 | (products) << 12)
#define ELO_FUSED_FAMILY(form) ((form) & 15)
#define ELO_FUSED_ROWS(form) ((form) >> 4 & 255)
#define ELO_FUSED_PRODUCTS(form) ((form) >> 12 & 15)
int elo_setconv_fused_form(const elo_setconv_args *a, const elo_setconv_args *b);
int elo_mlp_fused_form(const elo_mlp_args *a, const elo_mlp_args *b);
int elo_cv_stage1_form(const elo_cv1_args *a);
int elo_cv_stage2_form(const elo_cv2_args *a);

#ifdef __cplusplus
}
#endif
#endif /* ELO_H_ */
