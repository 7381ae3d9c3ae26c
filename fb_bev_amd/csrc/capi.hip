// capi.hip -- extern "C" entry points of libfbbev_hip.so (include/fbbev.h): argument checks,
// launch geometry, workspace carving.  No torch, no host synchronisation, caller's stream.
#include <stdio.h>
#include <stdlib.h>
#include <mutex>
#include "rt.h"
#include "pool_kernels.h"
#include "pool_bwd_kernels.h"
#include "rank_kernels.h"
#include "sort_kernels.h"
#include "msda_kernels.h"
#include "geom_kernels.h"
#include "da_kernels.h"
#include "history_kernels.h"
#include "norm_kernels.h"
#include "history_conv_kernels.h"
#include "history_fused_kernels.h"
#include "history_conv_x3_kernels.h"
#include "history_fused_x3_kernels.h"
#include "rows_linear_kernels.h"
#include "rows_linear_f32_kernels.h"
#include "da_fused_kernels.h"
#include "da_bwd_planes_kernels.h"
#include "msda_bwd_kernels.h"
#include "conv3d_kernels.h"
#include "det_kernels.h"
#include "occ_kernels.h"
#include "occ_loss_kernels.h"
#include "occ_fscore_kernels.h"
#include "../../include/fbbev.h"

#include "capi_common.h"

extern "C" int fbbev_version(void) { return 100; }

// ------------------------------------------------------------------------------ bev_pool_v2 fwd
extern "C" int fbbev_bev_pool_v2_fwd(int c, int n_intervals, const float* depth, const float* feat,
                                     const int32_t* ranks_depth, const int32_t* ranks_feat,
                                     const int32_t* ranks_bev, const int32_t* interval_starts,
                                     const int32_t* interval_lengths, float* out,
                                     fbbev_stream_t stream_) {
    if (c <= 0 || n_intervals < 0) return FBBEV_E_BADARG;
    if (n_intervals == 0) return 0;
    if (!depth || !feat || !ranks_depth || !ranks_feat || !ranks_bev || !interval_starts ||
        !interval_lengths || !out) return FBBEV_E_BADARG;
    fbbev_rt_stream stream = (fbbev_rt_stream)stream_;
    if (c % 4 == 0 && aligned16(feat) && aligned16(out)) {
        const long long threads = (long long)n_intervals * (c / 4);
        FBBEV_LAUNCH(k_pool_fwd_rows<4>, (threads + 255) / 256, 256, 0, stream, c, n_intervals, depth,
                     feat, ranks_depth, ranks_feat, ranks_bev, interval_starts, interval_lengths, out);
    } else {
        const long long threads = (long long)n_intervals * c;
        FBBEV_LAUNCH(k_pool_fwd_rows<1>, (threads + 255) / 256, 256, 0, stream, c, n_intervals, depth,
                     feat, ranks_depth, ranks_feat, ranks_bev, interval_starts, interval_lengths, out);
    }
    FBBEV_CHECK_LAUNCH();
    return 0;
}

// ------------------------------------------------------------------------------ bev_pool_v2 bwd
extern "C" int fbbev_bev_pool_v2_bwd(int c, int n_intervals, const float* out_grad,
                                     const float* depth, const float* feat,
                                     const int32_t* ranks_depth, const int32_t* ranks_feat,
                                     const int32_t* ranks_bev, const int32_t* interval_starts,
                                     const int32_t* interval_lengths, float* depth_grad,
                                     float* feat_grad, fbbev_stream_t stream_) {
    if (c <= 0 || n_intervals < 0) return FBBEV_E_BADARG;
    if (c > 256) return FBBEV_E_UNSUPPORTED;
    if (n_intervals == 0) return 0;
    if (!out_grad || !depth || !feat || !ranks_depth || !ranks_feat || !ranks_bev ||
        !interval_starts || !interval_lengths || !depth_grad || !feat_grad) return FBBEV_E_BADARG;
    fbbev_rt_stream stream = (fbbev_rt_stream)stream_;
    const long long blocks = ((long long)n_intervals * 64 + 255) / 256;  // one wave64 per interval
    const int nch = (c + 63) / 64;
#define FBBEV_BWD(NCH)                                                                             \
    FBBEV_LAUNCH(k_pool_bwd<NCH>, blocks, 256, 0, stream, c, n_intervals, out_grad, depth, feat,   \
                 ranks_depth, ranks_feat, ranks_bev, interval_starts, interval_lengths, depth_grad, \
                 feat_grad)
    switch (nch) {
        case 1: FBBEV_BWD(1); break;
        case 2: FBBEV_BWD(2); break;
        case 3: FBBEV_BWD(3); break;
        default: FBBEV_BWD(4); break;
    }
#undef FBBEV_BWD
    FBBEV_CHECK_LAUNCH();
    return 0;
}

// ------------------------------------------------------------------------------ frustum geometry
extern "C" int fbbev_lidar_coor(const float* xs, const float* ys, const float* ds, const float* rots,
                                const float* trans, const float* intrins, const float* post_rots,
                                const float* post_trans, const float* bda, int B, int N, int D, int H,
                                int W, float* coor, fbbev_stream_t stream_) {
    if (B <= 0 || N <= 0 || D <= 0 || H <= 0 || W <= 0) return FBBEV_E_BADARG;
    if (!xs || !ys || !ds || !rots || !trans || !intrins || !post_rots || !post_trans || !bda || !coor)
        return FBBEV_E_BADARG;
    const long long dhw = (long long)D * H * W;
    const long long chunks = (dhw + 255) / 256;
    if (chunks * B * N >= (1ll << 31)) return FBBEV_E_UNSUPPORTED;
    fbbev_cam_ptrs g;
    g.xs = xs; g.ys = ys; g.ds = ds; g.rots = rots; g.trans = trans; g.intrins = intrins; g.post_rots = post_rots;
    g.post_trans = post_trans; g.bda = bda; g.N = N; g.D = D; g.H = H; g.W = W;
    FBBEV_LAUNCH(k_lidar_coor, chunks * B * N, 256, 0, (fbbev_rt_stream)stream_, g, (int)chunks, coor);
    FBBEV_CHECK_LAUNCH();
    return 0;
}

extern "C" int fbbev_nchw_to_nhwc(const float* in, float* out, int n_images, int C, int HW, fbbev_stream_t stream_) {
    return fbbev_tokens_from_nchw(in, out, n_images, C, HW, (long long)C * HW, 0, nullptr, 0, stream_);
}

static int tokens_from_nchw_impl(const float* in, float* out, int n_images, int C, int HW, long long out_image_stride,
                                 long long out_offset, const float* bias, int bias_rows, const float* pos_bias,
                                 fbbev_stream_t stream_) {
    if (n_images < 0 || C <= 0 || HW <= 0 || out_offset < 0 || out_image_stride < (long long)C * HW) return FBBEV_E_BADARG;
    if (bias && bias_rows <= 0) return FBBEV_E_BADARG;
    if (n_images == 0) return 0;
    if (!in || !out) return FBBEV_E_BADARG;
    const int tc = (C + 31) / 32, th = (HW + 31) / 32;
    const long long blocks = (long long)n_images * tc * th;
    if (blocks >= (1ll << 31)) return FBBEV_E_UNSUPPORTED;
    FBBEV_LAUNCH(k_nchw_to_nhwc, blocks, 256, 0, (fbbev_rt_stream)stream_, in, out, C, HW, tc, th, out_image_stride,
                 out_offset, bias, bias ? bias_rows : 1, pos_bias);
    FBBEV_CHECK_LAUNCH();
    return 0;
}

extern "C" int fbbev_tokens_from_nchw(const float* in, float* out, int n_images, int C, int HW,
                                      long long out_image_stride, long long out_offset, const float* bias,
                                      int bias_rows, fbbev_stream_t stream_) {
    return tokens_from_nchw_impl(in, out, n_images, C, HW, out_image_stride, out_offset, bias, bias_rows, nullptr, stream_);
}

// every level of the camera-token pyramid in one launch: level l = in[l] (n_images, C, hw[l]) -> rows [start_l, start_l + hw[l]) of
// every image's (sum hw, C) token block in `out`, start_l = hw[0] + .. + hw[l-1]; + bias[(img % bias_rows), c] when bias is given
extern "C" int fbbev_tokens_from_nchw_levels(const float* const* in, const int32_t* hw, int n_levels, float* out, int n_images, int C,
                                             const float* bias, int bias_rows, fbbev_stream_t stream_) {
    if (n_levels <= 0 || n_levels > 8 || n_images < 0 || C <= 0 || !in || !hw) return FBBEV_E_BADARG;
    if (bias && bias_rows <= 0) return FBBEV_E_BADARG;
    if (n_images == 0) return 0;
    if (!out) return FBBEV_E_BADARG;
    fbbev_token_levels lv;
    const int tc = (C + 31) / 32;
    long long start = 0, blocks = 0;
    for (int l = 0; l < 8; ++l) { lv.in[l] = nullptr; lv.out_off[l] = 0; lv.hw[l] = 1; lv.blk0[l] = 0; }
    for (int l = 0; l < n_levels; ++l) {
        if (hw[l] <= 0 || !in[l]) return FBBEV_E_BADARG;
        lv.in[l] = in[l]; lv.hw[l] = hw[l]; lv.out_off[l] = start * C; lv.blk0[l] = (int)blocks;
        start += hw[l];
        blocks += (long long)n_images * tc * ((hw[l] + 31) / 32);
        if (blocks >= (1ll << 31)) return FBBEV_E_UNSUPPORTED;
    }
    lv.blk0[n_levels] = (int)blocks;
    lv.n = n_levels;
    FBBEV_LAUNCH(k_nchw_to_nhwc_levels, blocks, 256, 0, (fbbev_rt_stream)stream_, lv, out, C, tc, start * C, bias, bias ? bias_rows : 1);
    FBBEV_CHECK_LAUNCH();
    return 0;
}

// out[img, p, c] = in[img, c, p] + pos_bias[p, c]: the BEV queries of the backward projection (backward_projection.py:96-99:
// lss_bev flattened to tokens + the learned bev_embedding) in one transposing pass
extern "C" int fbbev_tokens_from_nchw_pos(const float* in, float* out, int n_images, int C, int HW, long long out_image_stride,
                                          long long out_offset, const float* pos_bias, fbbev_stream_t stream_) {
    if (!pos_bias) return FBBEV_E_BADARG;
    return tokens_from_nchw_impl(in, out, n_images, C, HW, out_image_stride, out_offset, nullptr, 0, pos_bias, stream_);
}

extern "C" int fbbev_point_sampling(const float* xs, const float* ys, const float* zs, const float* rots,
                                    const float* trans, const float* intrins, const float* post_rots,
                                    const float* post_trans, const float* bda, int B, int N, int Y, int X,
                                    int Za, float ogfH, float ogfW, float* ref_cam, uint8_t* mask,
                                    float* qdepth, fbbev_stream_t stream_) {
    if (B <= 0 || N <= 0 || Y <= 0 || X <= 0 || Za <= 0 || !(ogfH > 0.f) || !(ogfW > 0.f)) return FBBEV_E_BADARG;
    if (!xs || !ys || !zs || !rots || !trans || !intrins || !post_rots || !post_trans || !bda || !ref_cam ||
        !mask || !qdepth) return FBBEV_E_BADARG;
    const long long npts = (long long)Y * X * Za;
    int ppt = 8;                                            // points per thread: the most that leaves >= 1024 workgroups
    while (ppt > 1 && (npts + 256 * ppt - 1) / (256 * ppt) * B * N < 1024) ppt >>= 1;
    const long long chunks = (npts + 256 * ppt - 1) / (256 * ppt);
    if (chunks * B * N >= (1ll << 31) || ((uintptr_t)ref_cam & 7) != 0) return FBBEV_E_UNSUPPORTED;
    FBBEV_LAUNCH(k_point_sampling, chunks * B * N, 256, 0, (fbbev_rt_stream)stream_, xs, ys, zs, rots, trans,
                 intrins, post_rots, post_trans, bda, B, N, Y, X, Za, ogfH, ogfW, (int)chunks, ref_cam, mask,
                 qdepth, ppt);
    FBBEV_CHECK_LAUNCH();
    return 0;
}

// ------------------------------------------------------------------------------ voxel ranking
static inline int key_bits(long long total_voxels) {
    int bits = 1;
    while ((1ll << bits) < total_voxels) ++bits;   // every rank < total_voxels <= 2^bits
    return bits;
}

// Chunk shapes of the ranking chain.  A workgroup owns one chunk; fat chunks keep the count matrix (chunks x digits)
// small enough to be summed directly by every scatter workgroup, and the chunk is the smallest one whose workgroup count
// still fits ONE round on the 256 CUs (a 1024-thread workgroup is alone on its CU: a second, partly filled round doubles
// the kernel's time -- measured: 325 workgroups 56 us, the same work in 146 workgroups 29 us).
//   variant: 0 = 4 waves x 8 (2048), 1 = 16 x 4 (4096), 2 = 16 x 8 (8192), 3 = 16 x 12 (12288), 4 = 16 x 16 (16384)
//            5 = 8 waves x 8 (4096), 6 = 8 x 16 (8192): 512-thread workgroups, TWO per CU -- the phases of a scatter workgroup
//            (column sums -> key loads -> ballot ranking -> scatter) are serial and barrier-separated; a second workgroup on
//            the CU fills them (round 3; chosen only through FBBEV_RANK_SHAPE until measured better)
static const int kSortTile[7] = {2048, 4096, 8192, 12288, 16384, 4096, 8192};
static int sort_variant_for(long long items) {
    for (int v = 0; v < 5; ++v)
        if ((items + kSortTile[v] - 1) / kSortTile[v] <= 256) return v;
    // more than one round of the fattest chunks: 512-thread workgroups of 8192 pairs, two per CU, interleave their phases
    // (measured at the shipped grid, B = 16, 5.4 M points: 0.262 -> 0.239 ms per build, profiles/r03_time_rank_shapes.jsonl)
    return 6;
}
//   interval kernels: 0 = 4 waves x 4 (1024), 1 = 16 x 4 (4096), 2 = 16 x 8 (8192)
static const int kIvTile[3] = {1024, 4096, 8192};
static int iv_variant_for(long long items) {
    for (int v = 0; v < 3; ++v)
        if ((items + kIvTile[v] - 1) / kIvTile[v] <= 256) return v;
    return 2;
}

// (m, sh) of fbbev_div for an invariant divisor d (Granlund & Montgomery, N = 32): l = ceil(log2 d),
// m = floor(2^32 (2^l - d) / d) + 1, sh = l - 1
static fbbev_fastdiv make_fastdiv(unsigned int d) {
    fbbev_fastdiv f;
    f.d = d; f.m = 0; f.sh = 0;
    if (d <= 1) { f.d = 1; return f; }
    unsigned int l = 0;
    while ((1ull << l) < d) ++l;
    f.m = (unsigned int)((((1ull << l) - d) << 32) / d + 1);
    f.sh = l - 1;
    return f;
}

struct rank_ws_layout {
    size_t keys_a, keys_t, vals_t, matrix, ctot, chunk_info, boff, hb, total;
    int v0, wgs0;          // pass 0 (keys + scatter over all n points)
    int v1, wgs1;          // later passes (over the P kept pairs; P is only known on the device: sized for about n/2,
                           // the grid covers the worst case P = n and surplus workgroups leave at once)
    int vi, wgsi;          // interval kernels
};

static rank_ws_layout rank_layout(long long n) {
    rank_ws_layout L;
    L.v0 = sort_variant_for(n);
    L.v1 = sort_variant_for((n + 1) / 2);
    L.vi = iv_variant_for((n + 1) / 2);
    // tuning / test knob: FBBEV_RANK_SHAPE="v0,v1,vi" forces the chunk variants (results do not depend on them)
    if (const char* env = fbbev_env_str("FBBEV_RANK_SHAPE")) {
        int a = -1, b = -1, c = -1;
        if (sscanf(env, "%d,%d,%d", &a, &b, &c) == 3 && a >= 0 && a < 7 && b >= 0 && b < 7 && c >= 0 && c < 3) {
            L.v0 = a; L.v1 = b; L.vi = c;
        }
    }
    L.wgs0 = (int)((n + kSortTile[L.v0] - 1) / kSortTile[L.v0]);
    L.wgs1 = (int)((n + kSortTile[L.v1] - 1) / kSortTile[L.v1]);
    L.wgsi = (int)((n + kIvTile[L.vi] - 1) / kIvTile[L.vi]);
    size_t off = 0;
    L.keys_a = off; off = align_up(off + (size_t)n * 4, 256);
    L.keys_t = off; off = align_up(off + (size_t)n * 4, 256);
    L.vals_t = off; off = align_up(off + (size_t)n * 4, 256);
    const int rows = L.wgs0 > L.wgs1 ? L.wgs0 : L.wgs1;
    // the segmented (per-sample) sort: at most n / TILE + 256 sample-aligned chunks (<= 256 samples), 2^10 digit columns, + ctot
    const size_t seg_rows = (size_t)(n / FBBEV_SEG_TILE) + 256 + 1;
    size_t mbytes = (size_t)rows * FBBEV_SORT_MAX_NB * 4;
    if (seg_rows * FBBEV_SEG_NB * 4 > mbytes) mbytes = seg_rows * FBBEV_SEG_NB * 4;
    L.matrix = off; off = align_up(off + mbytes, 256);
    L.ctot = off; off = align_up(off + seg_rows * 4, 256);
    L.chunk_info = off; off = align_up(off + (size_t)L.wgsi * 8, 256);
    // the high-digit-first route (FBBEV_RANK_FINISH): bucket offsets (+ the closing P) and run heads per bucket, at most
    // 2^10 buckets for each of min(n, 256) samples
    const size_t fin_buckets = (size_t)(n < 256 ? n : 256) * FBBEV_SEG_NB;
    L.boff = off; off = align_up(off + (fin_buckets + 1) * 4, 256);
    L.hb = off; off = align_up(off + fin_buckets * 4, 256);
    L.total = off;                                        // no per-build state: nothing to clear, no kernel waits for another
    return L;
}

// one launch of KERNEL<threads or waves, per-thread items> for chunk variant v
#define FBBEV_SORT_DISPATCH(KERNEL, v, by_waves, grid, stream, ...)                                             \
    do {                                                                                                        \
        switch (v) {                                                                                            \
            case 0: FBBEV_LAUNCH((KERNEL<(by_waves) ? 4 : 256, 8>), grid, 256, 0, stream, __VA_ARGS__); break;   \
            case 1: FBBEV_LAUNCH((KERNEL<(by_waves) ? 16 : 1024, 4>), grid, 1024, 0, stream, __VA_ARGS__); break; \
            case 2: FBBEV_LAUNCH((KERNEL<(by_waves) ? 16 : 1024, 8>), grid, 1024, 0, stream, __VA_ARGS__); break; \
            case 3: FBBEV_LAUNCH((KERNEL<(by_waves) ? 16 : 1024, 12>), grid, 1024, 0, stream, __VA_ARGS__); break; \
            case 5: FBBEV_LAUNCH((KERNEL<(by_waves) ? 8 : 512, 8>), grid, 512, 0, stream, __VA_ARGS__); break;     \
            case 6: FBBEV_LAUNCH((KERNEL<(by_waves) ? 8 : 512, 16>), grid, 512, 0, stream, __VA_ARGS__); break;    \
            default: FBBEV_LAUNCH((KERNEL<(by_waves) ? 16 : 1024, 16>), grid, 1024, 0, stream, __VA_ARGS__); break; \
        }                                                                                                       \
    } while (0)

extern "C" size_t fbbev_rank_workspace_bytes(int64_t n_points) {
    if (n_points <= 0) return 256;
    return rank_layout(n_points).total;
}

static int rank_seg_mode() { FBBEV_KNOB_ONCE(int, m, fbbev_env_int("FBBEV_RANK_SEG", -1)); return m; }
static int rank_finish_mode() { FBBEV_KNOB_ONCE(int, m, fbbev_env_int("FBBEV_RANK_FINISH", -1)); return m; }
// auto rule of the high-digit-first route, on what the host knows (key bits of a sample, frustum points per sample, samples): on
// where it measured faster than the two-pass route beyond that route's own spread, whole build, eager, p50 of 60
// (profiles/r19_rank_finish.md) --
//   20 key bits (10 + 10; the 200 x 200 x 16 grid), 249 k points per sample: B = 16  0.143 -> 0.122 ms, B = 4  0.108 -> 0.088 ms
//   17 key bits (10 + 7; the shipped 100 x 100 x 8 grid), 338 k points per sample, B = 16: 0.176 -> 0.170 ms, inside the spread: off
// Nothing between 17 and 20 bits has been measured, so only full 10-bit low digits take the route; B and the points per sample
// are already bounded by the segmented route's own rule (at least 96 chunks, at most 64 per sample).
static bool rank_finish_auto(int lbits, long long npb, int B) {
    (void)npb; (void)B;
    return lbits >= 2 * FBBEV_SEG_RB;
}

static int rank_build_impl(const float* coor, const fbbev_cam_ptrs* cams, const float* frustum, int B, int N, int D,
                           int H, int W,
                           const float* lower3, const float* interval3, const float* grid_size3,
                           int32_t* ranks_bev, int32_t* ranks_depth, int32_t* ranks_feat,
                           int32_t* interval_starts, int32_t* interval_lengths, int32_t* interval_rank,
                           int32_t* counts, void* workspace, size_t workspace_bytes, fbbev_rt_stream stream,
                           const float* point_depth = nullptr, float depth_thr = 0.f, const int* skip = nullptr) {
    if (B <= 0 || N <= 0 || D <= 0 || H <= 0 || W <= 0) return FBBEV_E_BADARG;
    if (point_depth && cams) return FBBEV_E_UNSUPPORTED;      // the depth filter belongs to the coor-based (two-step) contract
    if ((!coor && !cams) || !lower3 || !interval3 || !grid_size3 || !ranks_bev || !ranks_depth || !ranks_feat ||
        !interval_starts || !interval_lengths || !counts || !workspace) return FBBEV_E_BADARG;
    const long long n = (long long)B * N * D * H * W;
    if (n >= (1ll << 30)) return FBBEV_E_UNSUPPORTED;          // 30-bit counts in the look-back words
    const rank_ws_layout L = rank_layout(n);
    if (workspace_bytes < L.total) return FBBEV_E_WORKSPACE;
    unsigned char* ws = static_cast<unsigned char*>(workspace);
    unsigned int* keys_a = reinterpret_cast<unsigned int*>(ws + L.keys_a);
    unsigned int* keys_t = reinterpret_cast<unsigned int*>(ws + L.keys_t);
    unsigned int* vals_t = reinterpret_cast<unsigned int*>(ws + L.vals_t);
    int* matrix = reinterpret_cast<int*>(ws + L.matrix);
    int2* chunk_info = reinterpret_cast<int2*>(ws + L.chunk_info);

    fbbev_grid_params gp;
    gp.lx = lower3[0]; gp.ly = lower3[1]; gp.lz = lower3[2];
    gp.ix = interval3[0]; gp.iy = interval3[1]; gp.iz = interval3[2];
    gp.gx = grid_size3[0]; gp.gy = grid_size3[1]; gp.gz = grid_size3[2];
    // the 0-dim fp32 products of view_transformer.py:586-588, rounded step by step like torch
    volatile float zy = gp.gz * gp.gy;
    volatile float zyx = zy * gp.gx;
    volatile float yx = gp.gy * gp.gx;
    gp.f_zyx = zyx; gp.f_yx = yx;
    const long long total_voxels = (long long)B * (long long)gp.gz * (long long)gp.gy * (long long)gp.gx;
    if (total_voxels <= 0 || total_voxels >= (1ll << 30)) return FBBEV_E_UNSUPPORTED;
    // fp32 rank evaluation can round UP above 2^24 voxels: one spare bit covers total_voxels itself
    const int bits = key_bits(total_voxels + 128);
    struct { int passes, rb; } plan;
    plan.passes = (bits + FBBEV_SORT_MAX_RB - 1) / FBBEV_SORT_MAX_RB;
    plan.rb = (bits + plan.passes - 1) / plan.passes;          // digits as even as possible, <= 8 bits
    if (plan.rb < 4) plan.rb = 4;
    const int rb = plan.rb;
    // Per-sample (segmented) sort: B V <= 2^24 (the fp32 rank arithmetic is exact, so the keys of sample b lie in [b V, (b+1) V))
    // and V fits two 10-bit digits -- two passes instead of three, 6 launches instead of 9 (sort_kernels.h).  FBBEV_RANK_SEG=0
    // keeps the global sort (A/B timing, tests); the index tensors are the same either way.
    const int seg_mode = rank_seg_mode();                   // -1 auto | 0 never | 2 whenever legal (tests)
    const long long vps = total_voxels / B;
    const long long npb = n / B;
    const int lbits = key_bits(vps);
    const bool seg_legal = B <= 256 && total_voxels <= (1ll << 24) && lbits <= 2 * FBBEV_SEG_RB;
    // auto: when it saves a pass AND the launch has the shape the kernels are good at -- enough sample-aligned chunks to fill
    // the part (>= 96 workgroups) and few chunks per sample (every scatter workgroup sums the <= 64 count rows of its sample).
    // Measured (profiles/r03_time_rank_seg*.jsonl, whole build, eager): shipped grid B = 16  0.258 -> 0.190 ms, BL2 B = 16
    // 0.182 -> 0.175 ms, BL2 B = 4  0.133 -> 0.122 ms; it LOSES for one fat sample (BL1 B = 1: 487 chunks per sample,
    // 0.152 -> 0.258 ms) and for a single small sample (shipped grid B = 1: 42 workgroups), which keep the global sort.
    const long long seg_cps = (npb + FBBEV_SEG_TILE - 1) / FBBEV_SEG_TILE;
    const bool seg = seg_legal && seg_mode != 0 &&
                     (seg_mode == 2 || ((lbits + FBBEV_SEG_RB - 1) / FBBEV_SEG_RB < plan.passes && seg_cps <= 64 && B * seg_cps >= 96));
    if (seg) {
        fbbev_seg sg;
        sg.npb = (int)npb; sg.cps = (int)((npb + FBBEV_SEG_TILE - 1) / FBBEV_SEG_TILE); sg.vps = (unsigned int)vps; sg.nseg = B;
        const int passes = (lbits + FBBEV_SEG_RB - 1) / FBBEV_SEG_RB;                     // 1 or 2
        const int srb = (lbits + passes - 1) / passes < 4 ? 4 : (lbits + passes - 1) / passes;
        const int wgs = B * sg.cps;
        int* ctot = reinterpret_cast<int*>(ws + L.ctot);
        fbbev_geom_src gs;
        if (cams) { gs.cam = *cams; gs.frustum = frustum; gs.gp = gp; }
        else { gs.cam = fbbev_cam_ptrs(); gs.frustum = nullptr; gs.gp = gp; }
        // High digit first (FBBEV_RANK_FINISH, two-digit plans only): ONE scatter by (key - b V) >> low_bits, then every bucket is
        // finished by one wave (k_bucket_finish) and the intervals follow from the buckets' head counts (k_bucket_intervals):
        // 4 launches instead of 6, the same index tensors bit for bit (sort_kernels.h).  0 = never, 1 = wherever legal (tests),
        // unset = auto: see rank_finish_auto.
        const int fin_mode = rank_finish_mode();
        const bool finish = passes == 2 && fin_mode != 0 && (fin_mode == 1 || rank_finish_auto(lbits, npb, B));
        const int high_bits = FBBEV_SEG_RB, low_bits = lbits - FBBEV_SEG_RB;        // passes == 2: 1 <= low_bits <= 10
        const int rb0 = finish ? high_bits : srb, dshift0 = finish ? low_bits : 0;
        if (cams) FBBEV_LAUNCH((k_keys_hist_seg<true>), wgs, FBBEV_SEG_NT, 0, stream, gs, (const float*)nullptr, gp, (const float*)nullptr, 0.f,
                               sg, rb0, dshift0, skip, keys_a, matrix, ctot);
        else FBBEV_LAUNCH((k_keys_hist_seg<false>), wgs, FBBEV_SEG_NT, 0, stream, gs, coor, gp, point_depth, depth_thr, sg, rb0, dshift0, skip,
                          keys_a, matrix, ctot);
        FBBEV_CHECK_LAUNCH();
        if (finish) {
            int* boff = reinterpret_cast<int*>(ws + L.boff);
            int* hb = reinterpret_cast<int*>(ws + L.hb);
            const int nbk = (int)((vps + (1ll << low_bits) - 1) >> low_bits);       // buckets a sample can fill (<= 2^high_bits)
            const int buckets = B * nbk;
            static const int swz = fbbev_env_int("FBBEV_RANK_XCD_SWIZZLE", 1);   // as the two-pass route below
            const int sw = (swz && B >= 8) ? 1 : 0;
            // the compacted (key, point id) pairs in keys_t | vals_t (adjacent: one array of pairs), bucket after bucket
            FBBEV_LAUNCH(k_sort_scatter_seg, sw ? (wgs + 7) / 8 * 8 : wgs, FBBEV_SEG_NT, 0, stream, (const unsigned int*)keys_a,
                         (const unsigned int*)nullptr, (const int*)matrix, (const int*)ctot, sg, 0, high_bits, skip, keys_t, vals_t, counts, sw, 2,
                         low_bits, boff, nbk);
            FBBEV_CHECK_LAUNCH();
            const fbbev_fastdiv div_dhw = make_fastdiv((unsigned int)((long long)D * H * W)), div_hw = make_fastdiv((unsigned int)(H * W));
            // short buckets: one wave per bucket while they fit the part (8 four-wave workgroups per CU), then a wave walks several;
            // long buckets: two workgroups per CU in front of them, each looking at every 512th bucket
            int short_wgs = (buckets + FBBEV_FIN_WAVES - 1) / FBBEV_FIN_WAVES;
            if (short_wgs > 2048) short_wgs = 2048;
            const int long_wgs = buckets < 512 ? buckets : 512;
            FBBEV_LAUNCH(k_bucket_finish, long_wgs + short_wgs, FBBEV_FIN_WAVES * 64, 0, stream, reinterpret_cast<const uint2*>(keys_t),
                         (const int*)boff, buckets, nbk, sg.vps, low_bits, long_wgs, div_dhw, div_hw, skip,
                         reinterpret_cast<unsigned int*>(ranks_bev), reinterpret_cast<unsigned int*>(ranks_depth), ranks_feat, hb);
            FBBEV_CHECK_LAUNCH();
            const int per_wg = (buckets + 255) / 256;                               // one round of 1024-thread workgroups on the part
            FBBEV_LAUNCH((k_bucket_intervals<16, 4>), (buckets + per_wg - 1) / per_wg, 1024, (size_t)2 * 4 * 1024 * 4, stream,
                         reinterpret_cast<const unsigned int*>(ranks_bev), (const int*)boff, (const int*)hb, buckets, per_wg, skip,
                         interval_starts, interval_lengths, interval_rank, counts);
            FBBEV_CHECK_LAUNCH();
            return 0;
        }
        const unsigned int* kin = keys_a;
        const unsigned int* vin = nullptr;
        static const int pairs = fbbev_env_int("FBBEV_RANK_PAIRS", 1);   // A/B knob, read once
        for (int p = 0; p < passes; ++p) {
            const bool to_out = p == passes - 1;
            // the intermediate (pass 0 -> pass 1) lives in keys_t | vals_t, which are adjacent: as ONE array of (key, value) pairs
            const int pm = pairs ? ((p > 0 ? 1 : 0) | (to_out ? 0 : 2)) : 0;
            unsigned int* ko = to_out ? reinterpret_cast<unsigned int*>(ranks_bev) : keys_t;
            unsigned int* vo = to_out ? reinterpret_cast<unsigned int*>(ranks_depth) : vals_t;
            if (p > 0) {
                FBBEV_LAUNCH(k_sort_hist_seg, wgs, FBBEV_SEG_NT, 0, stream, kin, (const int*)ctot, sg, p * srb, srb, skip, matrix,
                             (pm & 1) ? 2 : 1);
                FBBEV_CHECK_LAUNCH();
            }
            static const int swz = fbbev_env_int("FBBEV_RANK_XCD_SWIZZLE", 1);   // A/B knob, read once
            // XCD-contiguous chunk order when every XCD then owns whole samples' worth of chunks (B >= 8): measured 0.174 -> 0.156 ms
            // per build at BL2 B = 16, 0.192 -> 0.184 at the shipped grid B = 16; with few samples the round-robin order is faster
            // (BL2 B = 4: 0.123 vs 0.129) -- profiles/r04_time_rank_swizzle.jsonl
            const int sw = (swz && B >= 8) ? 1 : 0;
            FBBEV_LAUNCH(k_sort_scatter_seg, sw ? (wgs + 7) / 8 * 8 : wgs, FBBEV_SEG_NT, 0, stream, kin, vin, (const int*)matrix,
                         (const int*)ctot, sg, p, srb, skip, ko, vo, counts, sw, pm, -1, (int*)nullptr, 0);
            FBBEV_CHECK_LAUNCH();
            kin = ko; vin = vo;
        }
    } else {
    if (cams) {
            fbbev_geom_src gs;
            gs.cam = *cams; gs.frustum = frustum; gs.gp = gp;
            FBBEV_SORT_DISPATCH(k_keys_hist_geom, L.v0, false, L.wgs0, stream, gs, n, rb, skip, keys_a, matrix);
        } else {
            FBBEV_SORT_DISPATCH(k_keys_hist_coor, L.v0, false, L.wgs0, stream, coor, n, n / B, gp, point_depth, depth_thr, rb, keys_a, matrix);
        }
        FBBEV_CHECK_LAUNCH();
        const unsigned int* kin = keys_a;
        const unsigned int* vin = nullptr;                         // pass 0: value = position = point id
        for (int p = 0; p < plan.passes; ++p) {
            const bool to_out = ((plan.passes - 1 - p) % 2) == 0;  // the last pass always writes the outputs
            unsigned int* ko = to_out ? reinterpret_cast<unsigned int*>(ranks_bev) : keys_t;
            unsigned int* vo = to_out ? reinterpret_cast<unsigned int*>(ranks_depth) : vals_t;
            const int v = p == 0 ? L.v0 : L.v1, wgs = p == 0 ? L.wgs0 : L.wgs1;
            if (p > 0) {                                           // count matrix of this pass (pass 0: written with the keys)
                FBBEV_SORT_DISPATCH(k_sort_hist, v, false, wgs, stream, kin, (const int*)counts, p * rb, rb, skip, matrix);
                FBBEV_CHECK_LAUNCH();
            }
            static const int swz = fbbev_env_int("FBBEV_RANK_XCD_SWIZZLE", 1);   // A/B knob, read once
            // pass 0 only: later passes size their grid for n but run on the P kept pairs -- a contiguous split would idle XCDs
            const bool sw = swz == 2 && p == 0;       // off by default: measured slower for the global sort (BL1 B = 1: 0.151 -> 0.156 ms)
            FBBEV_SORT_DISPATCH(k_sort_scatter, v, true, sw ? (wgs + 7) / 8 * 8 : wgs, stream, kin, vin, n, (const int*)matrix, p, rb, skip,
                                ko, vo, counts, sw ? wgs : 0);
            FBBEV_CHECK_LAUNCH();
            kin = ko; vin = vo;
        }
}
    const unsigned int* keys = reinterpret_cast<const unsigned int*>(ranks_bev);
    const unsigned int* vals = reinterpret_cast<const unsigned int*>(ranks_depth);
    const fbbev_fastdiv div_dhw = make_fastdiv((unsigned int)((long long)D * H * W)), div_hw = make_fastdiv((unsigned int)(H * W));
    switch (L.vi) {
        case 0:
            FBBEV_LAUNCH((k_interval_count<4, 4>), L.wgsi, 256, 0, stream, keys, (const int*)counts, skip, chunk_info);
            FBBEV_LAUNCH((k_interval_write<4, 4>), L.wgsi, 256, (size_t)2 * 4 * 256 * 4, stream, keys, vals, div_dhw, div_hw, (const int2*)chunk_info, skip,
                         ranks_feat, interval_starts, interval_lengths, interval_rank, counts);
            break;
        case 1:
            FBBEV_LAUNCH((k_interval_count<16, 4>), L.wgsi, 1024, 0, stream, keys, (const int*)counts, skip, chunk_info);
            FBBEV_LAUNCH((k_interval_write<16, 4>), L.wgsi, 1024, (size_t)2 * 4 * 1024 * 4, stream, keys, vals, div_dhw, div_hw, (const int2*)chunk_info, skip,
                         ranks_feat, interval_starts, interval_lengths, interval_rank, counts);
            break;
        default:
            FBBEV_LAUNCH((k_interval_count<16, 8>), L.wgsi, 1024, 0, stream, keys, (const int*)counts, skip, chunk_info);
            FBBEV_LAUNCH((k_interval_write<16, 8>), L.wgsi, 1024, (size_t)2 * 8 * 1024 * 4, stream, keys, vals, div_dhw, div_hw, (const int2*)chunk_info, skip,
                         ranks_feat, interval_starts, interval_lengths, interval_rank, counts);
            break;
    }
    FBBEV_CHECK_LAUNCH();
    return 0;
}

extern "C" int fbbev_rank_build(const float* coor, int B, int N, int D, int H, int W,
                                const float* lower3, const float* interval3,
                                const float* grid_size3, int32_t* ranks_bev, int32_t* ranks_depth,
                                int32_t* ranks_feat, int32_t* interval_starts,
                                int32_t* interval_lengths, int32_t* interval_rank, int32_t* counts,
                                void* workspace, size_t workspace_bytes, fbbev_stream_t stream_) {
    if (!coor) return FBBEV_E_BADARG;
    return rank_build_impl(coor, nullptr, nullptr, B, N, D, H, W, lower3, interval3, grid_size3, ranks_bev, ranks_depth,
                           ranks_feat, interval_starts, interval_lengths, interval_rank, counts, workspace,
                           workspace_bytes, (fbbev_rt_stream)stream_);
}

extern "C" int fbbev_rank_build_depth(const float* coor, const float* depth, float depth_threshold, int B, int N, int D,
                                      int H, int W, const float* lower3, const float* interval3,
                                      const float* grid_size3, int32_t* ranks_bev, int32_t* ranks_depth,
                                      int32_t* ranks_feat, int32_t* interval_starts, int32_t* interval_lengths,
                                      int32_t* interval_rank, int32_t* counts, void* workspace, size_t workspace_bytes,
                                      fbbev_stream_t stream_) {
    if (!coor || !depth) return FBBEV_E_BADARG;
    return rank_build_impl(coor, nullptr, nullptr, B, N, D, H, W, lower3, interval3, grid_size3, ranks_bev, ranks_depth,
                           ranks_feat, interval_starts, interval_lengths, interval_rank, counts, workspace,
                           workspace_bytes, (fbbev_rt_stream)stream_, depth, depth_threshold);
}

static int lift_rank_build_impl(const float* frustum, const float* xs, const float* ys, const float* ds,
                                const float* rots, const float* trans, const float* intrins, const float* post_rots,
                                const float* post_trans, const float* bda, int B, int N, int D, int H, int W,
                                const float* lower3, const float* interval3, const float* grid_size3,
                                int32_t* ranks_bev, int32_t* ranks_depth, int32_t* ranks_feat, int32_t* interval_starts,
                                int32_t* interval_lengths, int32_t* interval_rank, int32_t* counts, void* workspace,
                                size_t workspace_bytes, fbbev_rt_stream stream, uint32_t* cam_key, int32_t* cache_state) {
    if (!xs || !ys || !ds || !rots || !trans || !intrins || !post_rots || !post_trans || !bda) return FBBEV_E_BADARG;
    if (B <= 0 || N <= 0) return FBBEV_E_BADARG;
    fbbev_cam_ptrs g;
    g.xs = xs; g.ys = ys; g.ds = ds; g.rots = rots; g.trans = trans; g.intrins = intrins; g.post_rots = post_rots;
    g.post_trans = post_trans; g.bda = bda; g.N = N; g.D = D; g.H = H; g.W = W;
    const int* skip = nullptr;
    if (cam_key) {
        if (!cache_state) return FBBEV_E_BADARG;
        FBBEV_LAUNCH(k_cam_key, 1, 256, 0, stream, g, B, cam_key, cache_state);
        FBBEV_CHECK_LAUNCH();
        skip = cache_state;
    }
    return rank_build_impl(nullptr, &g, frustum, B, N, D, H, W, lower3, interval3, grid_size3, ranks_bev, ranks_depth,
                           ranks_feat, interval_starts, interval_lengths, interval_rank, counts, workspace,
                           workspace_bytes, stream, nullptr, 0.f, skip);
}

extern "C" int fbbev_lift_rank_build(const float* frustum, const float* xs, const float* ys, const float* ds,
                                     const float* rots,
                                     const float* trans, const float* intrins, const float* post_rots,
                                     const float* post_trans, const float* bda, int B, int N, int D, int H,
                                     int W, const float* lower3, const float* interval3,
                                     const float* grid_size3, int32_t* ranks_bev, int32_t* ranks_depth,
                                     int32_t* ranks_feat, int32_t* interval_starts, int32_t* interval_lengths,
                                     int32_t* interval_rank, int32_t* counts, void* workspace,
                                     size_t workspace_bytes, fbbev_stream_t stream_) {
    return lift_rank_build_impl(frustum, xs, ys, ds, rots, trans, intrins, post_rots, post_trans, bda, B, N, D, H, W, lower3,
                                interval3, grid_size3, ranks_bev, ranks_depth, ranks_feat, interval_starts,
                                interval_lengths, interval_rank, counts, workspace, workspace_bytes,
                                (fbbev_rt_stream)stream_, nullptr, nullptr);
}

extern "C" size_t fbbev_cam_key_words(int B, int N) {
    return (B <= 0 || N <= 0) ? 0 : (size_t)B * N * 33 + (size_t)B * 9;
}

extern "C" int fbbev_lift_rank_build_cached(const float* frustum, const float* xs, const float* ys, const float* ds,
                                            const float* rots, const float* trans, const float* intrins,
                                            const float* post_rots, const float* post_trans, const float* bda, int B,
                                            int N, int D, int H, int W, const float* lower3, const float* interval3,
                                            const float* grid_size3, int32_t* ranks_bev, int32_t* ranks_depth,
                                            int32_t* ranks_feat, int32_t* interval_starts, int32_t* interval_lengths,
                                            int32_t* interval_rank, int32_t* counts, void* workspace,
                                            size_t workspace_bytes, uint32_t* cam_key, int32_t* cache_state,
                                            fbbev_stream_t stream_) {
    if (!cam_key || !cache_state) return FBBEV_E_BADARG;
    return lift_rank_build_impl(frustum, xs, ys, ds, rots, trans, intrins, post_rots, post_trans, bda, B, N, D, H, W, lower3,
                                interval3, grid_size3, ranks_bev, ranks_depth, ranks_feat, interval_starts,
                                interval_lengths, interval_rank, counts, workspace, workspace_bytes,
                                (fbbev_rt_stream)stream_, cam_key, cache_state);
}

// ------------------------------------------------------------------------------ view-transformation pooling
// The lift-splat of the view transformation: the tile index over the ranked intervals, the dense forward that writes every voxel of
// the volume exactly once, the Z-mean, the store-floor diagnostic and the fused backward.  Every entry fills the small records
// below from its positional C arguments; everything under the entries works on those records.  Every entry strings its checks
// together itself: their ORDER is part of the ABI (tests/test_abi_symbols.py pins it), and what a flags word launches is pinned by
// tests/test_emu_pool_launch_record.py.
//   entry                               output layout                        kernels                                       flag bits and knobs that route it
//   fbbev_pool_tile_index[_cached]      tile table, (tiles + 1) x 2 ints     [k_tile_table_gate +] k_tile_lower_bound2     CHANNELS_LAST: flat tiles over B*Z*Y*X
//                                       first / last interval per tile       memset + k_tile_scatter                       CHANNELS_LAST with tiles of 8 / 16 / 32
//                                                                                                                          (_cached: UNSUPPORTED)
//   fbbev_bev_pool_v2_dense_fwd[_add]   planes (B, C, Z, Y, X), strided,     k_pool_fwd_dense2<TV, CPL, ST, NT, OT, T16,   store bits 0-1 and 17, CPL8, CSPLIT, WG,
//                                       fp32 / bf16 / fp16                   0, SPLIT, GU>                                 XCD_SWIZZLE + chunk, OUT_BF16 / OUT_F16,
//                                                                                                                          SPLIT_LONG, GATHER8 (not with SPLIT_LONG)
//                                       planes, fp32                         k_pool_fwd_dense_pipe<TV, CPL, 4, 256>        PIPE (fp32, 256 threads, `sc1 nt`, tiles
//                                                                                                                          64 .. 256, not SPLIT_LONG); FBBEV_POOL_PIPE_TPW
//                                       channels-last (B, Z, Y, X, C),       k_pool_fwd_dense_cl<TV, CPL, ST, 256>         CHANNELS_LAST (no addend, fp32); store bits,
//                                       dense, fp32                          tiles of 8 / 16 / 32: k_pool_fwd_cl_small<ST> CPL8, XCD_SWIZZLE + chunk
//   fbbev_bev_pool_v2_dense_fwd_rows    rows (B, Z*Y*X, C) of a strided      k_pool_fwd_dense_rows<TV, CPL, ST, 256, ET>   OUT_BF16 / OUT_F16 (then CPL 8, `sc1 nt`),
//                                       slot, fp32 / bf16 / fp16                                                           store bits, CPL8, XCD_SWIZZLE + chunk
//   fbbev_diag_pool_store_floor         planes, zeros                        k_pool_fwd_dense2<128, 8, 4, 256, OT, T16,    the one product route only; OUT_BF16,
//                                                                            MODE>                                         CSPLIT, XCD_SWIZZLE + chunk; `mode`
//   fbbev_lift_splat_fused              as fbbev_bev_pool_v2_dense_fwd       rank build, fbbev_nchw_to_nhwc, the tile      as the tile index and the dense forward
//                                                                            index and the dense forward's
//   fbbev_pool_zmean[_split|_rows]      (B, C, Y, X) or rows (B, Y*X, C)     k_pool_zmean<TV, CPL, 256>                    CPL8, CSPLIT; z_groups
//                                                                            [+ k_pool_zmean_reduce], or                   FBBEV_ZMEAN_COL=1 (planes, one group, Z <= 64)
//                                                                            k_pool_zmean_col<TV, CPL, 256>
//   fbbev_bev_pool_v2_dense_bwd[_z]     depth_grad, feat_grad                memset + k_point_row_table,                   none.  C > 128 with C % 8 != 0 is refused
//                                                                            k_tile_lower_bound2, k_pool_bwd_rows<128>,    (UNSUPPORTED) only AFTER the first three
//                                                                            k_pool_bwd_pixel<4 | 8>                       launches, where the pixel kernel is chosen
//   (behind the cross-attention family)
//   fbbev_pool_dense_workspace_bytes, fbbev_pool_dense_bwd_workspace_bytes, fbbev_lift_splat_fused_ws_bytes / _ws_offsets: host functions, no launch

static inline int pick_tile(int tile_voxels) {
    switch (tile_voxels) { case 64: case 128: case 256: case 512: case 1024: return tile_voxels; default: return 64; }
}
// channels-last small tiles: 8 / 16 / 32 voxels per workgroup (one 16-byte store per thread)
static inline int small_tile_shift(int tile_voxels) {
    switch (tile_voxels) { case 8: return 3; case 16: return 4; case 32: return 5; default: return 0; }
}

// The gather operands: depth (B, N, D, H, W), channels-last features and the ranked index arrays of the intervals
struct pool_gather {
    const float *depth, *feat;
    const int32_t *rd, *rf, *irank, *starts, *lengths;
};
static inline bool pool_gather_present(const pool_gather& g) { return g.depth && g.feat && g.rd && g.rf && g.irank && g.starts && g.lengths; }
#define FBBEV_POOL_GATHER(g) (g).depth, (g).feat, (g).rd, (g).rf, (g).irank, (g).starts, (g).lengths   /* as the kernels take them */

// The grid: yx = Y * X voxels of a plane, nvox = B * Z * Y * X of them in all -- saturated at 2^31, beyond which every entry only
// asks whether a flat voxel index still fits an int; both 0 unless every dimension is positive (an entry without channels says C = 1)
struct pool_grid {
    int B, C, Z, Y, X;
    long long yx, nvox;
};
static inline bool pool_grid_positive(const pool_grid& g) { return g.B > 0 && g.C > 0 && g.Z > 0 && g.Y > 0 && g.X > 0; }
static inline bool pool_grid_fits_int(const pool_grid& g) { return g.nvox < (1ll << 31); }
static inline pool_grid pool_grid_of(int B, int C, int Z, int Y, int X) {
    pool_grid g = {B, C, Z, Y, X, 0, 0};
    if (!pool_grid_positive(g)) return g;
    const long long lim = 1ll << 31;
    g.yx = (long long)Y * X;
    const long long zyx = g.yx < lim ? Z * g.yx : lim;
    g.nvox = zyx < lim ? B * zyx : lim;
    return g;
}

// The flags word of include/fbbev.h, decoded once.  What depends on the shape or on the kernel is a function of it.
struct pool_flags {
    int st_bits;                                            // store policy field: bits 0-1, bit 17 as bit 2
    bool bf16, f16;                                         // element type of the output (both: every entry that stores 16 bits refuses it)
    bool cpl8;                                              // the WISH for 8 channels per lane: cpl() grants it
    int csplit_field, wg, chunk_field;
    bool xcd_swizzle, channels_last, pipe, split_long;
    bool gather8;                                           // ignored when split_long is set
    // store cache policy: 0 plain, 1 nontemporal, anything else `sc1 nt` (4), the measured best
    int store() const { return st_bits == 0 ? 0 : st_bits == 1 ? 1 : 4; }
    int et() const { return bf16 ? 1 : f16 ? 2 : 0; }       // FBBEV_ELEM_*
    int threads() const { return wg == 1 ? 128 : 256; }
    // workgroups the channel range is split over: field 0xF means 20, what does not divide C into multiples of 4 means 1
    int csplit(int C) const {
        int n = csplit_field == 0xF ? 20 : csplit_field;
        if (n < 1 || C % (4 * n) != 0) n = 1;
        return n;
    }
    int cpl(int CC) const { return cpl8 && CC % 8 == 0 ? 8 : 4; }   // channels per lane for CC channels per workgroup
    // XCD order: 0 = off, else 1 + log2(tiles per chunk) with the kernel's own default for a chunk field of 0 (see the call sites)
    int swizzle(int default_chunk) const { return xcd_swizzle ? (chunk_field ? chunk_field : default_chunk) + 1 : 0; }
};
static inline pool_flags pool_flags_of(int flags) {
    pool_flags f;
    f.st_bits = (flags & FBBEV_POOL_STORE_MASK) | ((flags >> FBBEV_POOL_STORE_HI_SHIFT) & 1) << 2;
    f.bf16 = (flags & FBBEV_POOL_OUT_BF16) != 0;
    f.f16 = (flags & FBBEV_POOL_OUT_F16) != 0;
    f.cpl8 = (flags & FBBEV_POOL_CPL8) != 0;
    f.csplit_field = (flags >> FBBEV_POOL_CSPLIT_SHIFT) & 0xF;
    f.wg = (flags >> FBBEV_POOL_WG_SHIFT) & 0x3;
    f.chunk_field = (flags >> FBBEV_POOL_SWZ_CHUNK_SHIFT) & 0x1F;
    f.xcd_swizzle = (flags & FBBEV_POOL_XCD_SWIZZLE) != 0;
    f.channels_last = (flags & FBBEV_POOL_CHANNELS_LAST) != 0;
    f.pipe = (flags & FBBEV_POOL_PIPE) != 0;
    f.split_long = (flags & FBBEV_POOL_SPLIT_LONG) != 0;
    f.gather8 = (flags & FBBEV_POOL_GATHER8) != 0 && !f.split_long;
    return f;
}

// a swizzled grid is rounded up to whole groups of 8 chunks (the kernel skips what lies past n_blocks)
static inline long long pool_swizzled_grid(long long n_blocks, int swizzle) {
    if (!swizzle) return n_blocks;
    const long long g = 8ll << (swizzle - 1);
    return (n_blocks + g - 1) / g * g;
}
// the tile table: two ints per tile and one pair past the end
static inline size_t pool_tile_table_bytes(long long n_tiles) { return (size_t)(n_tiles + 1) * 8; }
// LDS of a tile's staged index (what the channels-last kernels use alone), and with the value tile of CC channels in fp32
// [CC][TV + 4] or in 16 bits [CC][TV + 8]
static inline size_t pool_index_lds_bytes(int TV) { return (3 * (size_t)TV + 2 * FBBEV_NP_STAGE) * sizeof(int); }
static inline size_t pool_planar_lds_bytes(int CC, int TV) { return (size_t)CC * (TV + 4) * sizeof(float) + pool_index_lds_bytes(TV); }
static inline size_t pool_planar_lds16_bytes(int CC, int TV) { return (size_t)CC * (TV + 8) * 2 + pool_index_lds_bytes(TV); }
// The strides of a (B, C, Z, Y, X) volume, forward output and backward gradient alike: 0 = contiguous; planes that would overlap
// or strides that are no multiple of 4 elements are FBBEV_E_BADARG
struct pool_strides { long long b, c; int err; };
static inline pool_strides pool_volume_strides(long long stride_b, long long stride_c, const pool_grid& g) {
    pool_strides s = {stride_b, stride_c, 0};
    if (s.c == 0) s.c = g.Z * g.yx;
    if (s.b == 0) s.b = g.C * s.c;
    if (s.c < g.Z * g.yx || s.b < g.C * s.c || s.c % 4 != 0 || s.b % 4 != 0) s.err = FBBEV_E_BADARG;
    return s;
}

// What every forward entry is given besides its output
struct pool_call {
    pool_gather in;
    pool_grid g;
    const void* tile_ws; size_t tile_ws_bytes; int tile_voxels;
    pool_flags f;
    fbbev_rt_stream stream;
};
// One launch of a dense kernel: n_blocks workgroups of work (the grid is pool_swizzled_grid of them)
struct pool_launch {
    pool_gather in; const int* tile_meta; fbbev_rt_stream stream;
    int C, Z, yx, zyx, nvox, tpp, csplit, swizzle;          // tpp: tiles per plane
    long long n_blocks; size_t lds;
    long long out_stride_b, out_stride_c, addend_stride;    // out_stride_c: planes; addend_stride: rows
    const float* addend;                                    // planes: (B, C, Y, X) added to every z; rows: (B, Y*X, C); may be null
    void* out;
};
static inline pool_launch pool_launch_of(const pool_call& c) {
    pool_launch a = {};
    a.in = c.in; a.tile_meta = static_cast<const int*>(c.tile_ws); a.stream = c.stream;
    a.C = c.g.C; a.Z = c.g.Z;
    return a;
}

// The family's template ladders: the statement(s) after the value, once per candidate, with `constexpr int NAME` set to the candidate
// the value equals (the last candidate where it equals none) -- a launch names its instantiation with it.  A `return` inside leaves
// the enclosing function.  Only the combinations a ladder spells out are instantiated, so a route built for fewer of them has its own.
#define FBBEV_POOL_WITH(NAME, v, V0, V1, ...) \
    do { if ((v) == (V0)) { constexpr int NAME = V0; __VA_ARGS__; } else { constexpr int NAME = V1; __VA_ARGS__; } } while (0)
#define FBBEV_POOL_WITH3(NAME, v, V0, V1, V2, ...)                                                                           \
    do { if ((v) == (V0)) { constexpr int NAME = V0; __VA_ARGS__; } else FBBEV_POOL_WITH(NAME, v, V1, V2, __VA_ARGS__); } while (0)
#define FBBEV_POOL_TILE3(tv, ...) FBBEV_POOL_WITH3(TV, tv, 64, 128, 256, __VA_ARGS__)
#define FBBEV_POOL_TILE(tv, ...)                                                                                             \
    do { if ((tv) == 64) { constexpr int TV = 64; __VA_ARGS__; } else if ((tv) == 128) { constexpr int TV = 128; __VA_ARGS__; } \
         else FBBEV_POOL_WITH3(TV, tv, 256, 512, 1024, __VA_ARGS__); } while (0)
#define FBBEV_POOL_CPL(cpl, ...) FBBEV_POOL_WITH(CPL, cpl, 8, 4, __VA_ARGS__)
#define FBBEV_POOL_ST(st, ...) FBBEV_POOL_WITH3(ST, st, 0, 1, 4, __VA_ARGS__)
#define FBBEV_POOL_NT(nt, ...) FBBEV_POOL_WITH(NT, nt, 128, 256, __VA_ARGS__)
#define FBBEV_POOL_ET16(et, ...) FBBEV_POOL_WITH(ET, et, 1, 2, __VA_ARGS__)

extern "C" size_t fbbev_pool_dense_workspace_bytes(int B, int Z, int Y, int X) {
    if (B <= 0 || Z <= 0 || Y <= 0 || X <= 0) return 256;
    const long long yx = (long long)Y * X;
    const long long tiles = ((long long)B * Z * yx + 7) / 8 + (long long)B * Z;   // smallest tile (8 voxels) = most tiles
    return align_up((size_t)(tiles + 2) * 8, 256);                // two ints per tile
}

// ---- the tile index
struct pool_index_args {
    const int32_t *irank, *starts, *counts; int n_max;
    pool_grid g;                                            // C = 1
    int tile_voxels; bool channels_last;
    void* tile_ws; size_t tile_ws_bytes;
    fbbev_rt_stream stream;
    const int32_t* skip;                                    // device flag: nonzero keeps the table as it is (the cached entry's gate); may be null
};
static int pool_tile_index(const pool_index_args& t) {
    const pool_grid& g = t.g;
    if (!pool_grid_positive(g) || t.n_max < 0) return FBBEV_E_BADARG;
    if (!t.irank || !t.starts || !t.counts || !t.tile_ws) return FBBEV_E_BADARG;
    if (!pool_grid_fits_int(g)) return FBBEV_E_UNSUPPORTED;
    if (t.channels_last && small_tile_shift(t.tile_voxels)) {
        // small tiles: scatter-built table (first/last interval per tile), -1 = empty
        const int sh = small_tile_shift(t.tile_voxels);
        const long long nt = (g.nvox + (1 << sh) - 1) >> sh;
        if (t.tile_ws_bytes < (size_t)nt * 8) return FBBEV_E_WORKSPACE;
        int* first = static_cast<int*>(t.tile_ws);
        int e = fbbev_rt_memset_async(first, 0xFF, (size_t)nt * 8, t.stream);
        if (e) return e;
        long long blocks = ((long long)t.n_max + 255) / 256;
        if (blocks > 4096) blocks = 4096;
        if (blocks < 1) blocks = 1;
        FBBEV_LAUNCH(k_tile_scatter, blocks, 256, 0, t.stream, t.irank, t.counts, t.n_max, sh, g.nvox, first, first + nt);
        FBBEV_CHECK_LAUNCH();
        return 0;
    }
    const int TV = pick_tile(t.tile_voxels);
    int tiles_per_plane = (int)((g.yx + TV - 1) / TV);
    long long n_tiles = (long long)g.B * g.Z * tiles_per_plane;
    long long plane = g.yx;
    if (t.channels_last) {   // flat tiling of the whole (B*Z*Y*X) rank space
        plane = g.nvox;
        n_tiles = (plane + TV - 1) / TV;
        tiles_per_plane = (int)n_tiles + 1;   // every tile index t (incl. t == n_tiles) stays in "plane" 0
    }
    if (t.tile_ws_bytes < pool_tile_table_bytes(n_tiles)) return FBBEV_E_WORKSPACE;
    FBBEV_LAUNCH(k_tile_lower_bound2, (n_tiles + 1 + 255) / 256, 256, 0, t.stream, (int)n_tiles, tiles_per_plane, (int)plane, TV,
                 t.irank, t.starts, t.counts, t.n_max, t.skip, static_cast<int*>(t.tile_ws));
    FBBEV_CHECK_LAUNCH();
    return 0;
}

extern "C" int fbbev_pool_tile_index(const int32_t* interval_rank, const int32_t* interval_starts,
                                     const int32_t* counts, int n_intervals_max, int B, int Z, int Y,
                                     int X, int tile_voxels, int flags, void* tile_ws, size_t tile_ws_bytes,
                                     fbbev_stream_t stream_) {
    return pool_tile_index({interval_rank, interval_starts, counts, n_intervals_max, pool_grid_of(B, 1, Z, Y, X), tile_voxels,
                            pool_flags_of(flags).channels_last, tile_ws, tile_ws_bytes, (fbbev_rt_stream)stream_, nullptr});
}

extern "C" int fbbev_pool_tile_index_cached(const int32_t* interval_rank, const int32_t* interval_starts,
                                            const int32_t* counts, int n_intervals_max, int B, int Z, int Y,
                                            int X, int tile_voxels, int flags, void* tile_ws, size_t tile_ws_bytes,
                                            const int32_t* cache_state, int32_t* table_gate,
                                            fbbev_stream_t stream_) {
    if (!cache_state || !table_gate) return FBBEV_E_BADARG;
    if (pool_flags_of(flags).channels_last && small_tile_shift(tile_voxels)) return FBBEV_E_UNSUPPORTED;
    // keep THIS table only if the index set is unchanged and the table was built for this very build; the gate is launched before
    // the shared argument checks run
    FBBEV_LAUNCH(k_tile_table_gate, 1, 1, 0, (fbbev_rt_stream)stream_, cache_state, table_gate);
    FBBEV_CHECK_LAUNCH();
    return pool_tile_index({interval_rank, interval_starts, counts, n_intervals_max, pool_grid_of(B, 1, Z, Y, X), tile_voxels,
                            pool_flags_of(flags).channels_last, tile_ws, tile_ws_bytes, (fbbev_rt_stream)stream_, table_gate + 1});
}

// ---- the dense forward on planes (and, with FBBEV_POOL_CHANNELS_LAST, on dense voxel rows)
// channels-last with tiles of 8 / 16 / 32 voxels (1 << sh): the scatter-built table, a lane per 4 channels of a voxel
static int pool_fwd_cl_small(const pool_call& c, float* out, int sh) {
    const long long nvox = c.g.nvox, nt = (nvox + (1 << sh) - 1) >> sh;
    if (c.tile_ws_bytes < (size_t)nt * 8) return FBBEV_E_WORKSPACE;
    int threads = (c.g.C / 4) << sh;
    if (threads > 1024) return FBBEV_E_UNSUPPORTED;
    threads = (threads + 63) / 64 * 64;
    // a chunk field of 0 means chunks of one tile, which is the plain round-robin: the sweep these tiles were measured with starts there
    // (profiles/r01_exp_pool_cl_small.jsonl, swz0 .. swz6)
    const int swz = c.f.swizzle(0);
    const long long grid = pool_swizzled_grid(nt, swz);
    const int* first = static_cast<const int*>(c.tile_ws);
    FBBEV_POOL_ST(c.f.store(), FBBEV_LAUNCH(k_pool_fwd_cl_small<ST>, grid, threads, 0, c.stream, c.g.C, sh, nvox, (int)nt, swz,
                                            FBBEV_POOL_GATHER(c.in), first, first + nt, out));
    return fbbev_rt_last_error();
}

// channels-last with flat tiles of tv voxels over the whole rank space: a linear store stream, no LDS value tile
static int pool_fwd_cl(const pool_call& c, float* out, int tv) {
    const int C = c.g.C, cpl = c.f.cpl(C), st = c.f.store();
    if (256 / (C / cpl) < 1) return FBBEV_E_UNSUPPORTED;
    const long long nvox = c.g.nvox, n_blocks = (nvox + tv - 1) / tv;
    if (c.tile_ws_bytes < pool_tile_table_bytes(n_blocks)) return FBBEV_E_WORKSPACE;
    const size_t lds = pool_index_lds_bytes(tv);
    // chunks of 16 tiles where the field is 0: the smaller of the two sizes the flat tiles were swept with (profiles/r01_exp_pool_cl.jsonl)
    const int swz = c.f.swizzle(4);
    const long long grid = pool_swizzled_grid(n_blocks, swz);
    const int* meta = static_cast<const int*>(c.tile_ws);
    FBBEV_POOL_TILE(tv, FBBEV_POOL_CPL(cpl, FBBEV_POOL_ST(st, FBBEV_LAUNCH((k_pool_fwd_dense_cl<TV, CPL, ST, 256>), grid, 256, lds, c.stream, C, (int)nvox,
                                                                           (int)n_blocks, swz, FBBEV_POOL_GATHER(c.in), meta, out))));
    return fbbev_rt_last_error();
}

// FBBEV_POOL_PIPE: a workgroup walks a run of tpw tiles, the next tile's index staged while the current one is summed
static int pool_fwd_pipe(pool_launch a, long long n_tiles, int tv, int cpl) {
    // tiles per workgroup: enough to amortise the pipeline's fill, few enough to keep >= ~8 workgroups per CU's worth of runs
    FBBEV_KNOB_ONCE(int, tpw_env, fbbev_env_int("FBBEV_POOL_PIPE_TPW", 0));   // tuning knob (the emulator tests switch the run length)
    int tpw = tpw_env > 0 ? (tpw_env > 64 ? 64 : tpw_env) : 4;
    if (tpw_env <= 0) while (tpw > 1 && (n_tiles / tpw) * a.csplit < 2048) tpw >>= 1;
    const long long groups = (n_tiles + tpw - 1) / tpw;
    a.n_blocks = groups * a.csplit;
    a.lds = pool_planar_lds_bytes(a.C / a.csplit, tv) + pool_index_lds_bytes(tv);   // a second staged index
    if (a.lds > 160 * 1024) return FBBEV_E_UNSUPPORTED;
    const long long grid = pool_swizzled_grid(a.n_blocks, a.swizzle);
    FBBEV_POOL_TILE3(tv, FBBEV_POOL_CPL(cpl, FBBEV_LAUNCH_DYN_LDS((k_pool_fwd_dense_pipe<TV, CPL, 4, 256>), grid, 256, a.lds, a.stream, a.C, a.Z,
                                                                  a.yx, a.tpp, a.csplit, (int)a.n_blocks, a.swizzle, tpw, (int)n_tiles,
                                                                  a.out_stride_b, a.out_stride_c, FBBEV_POOL_GATHER(a.in), a.tile_meta,
                                                                  a.addend, static_cast<float*>(a.out))));
    return fbbev_rt_last_error();
}

#define FBBEV_POOL_SPLIT_LEN 32      // points above which an interval is split over the lane groups in tolerance mode
template <int TV, int CPL, int ST, int NT, int OT, bool T16, int SPLIT, int GU>
static int pool_launch_dense2(const pool_launch& a) {
    FBBEV_LAUNCH_DYN_LDS((k_pool_fwd_dense2<TV, CPL, ST, NT, OT, T16, 0, SPLIT, GU>), pool_swizzled_grid(a.n_blocks, a.swizzle), NT, a.lds,
                         a.stream, a.C, a.Z, a.yx, a.tpp, a.csplit, (int)a.n_blocks, a.swizzle, a.out_stride_b, a.out_stride_c,
                         FBBEV_POOL_GATHER(a.in), a.tile_meta, a.addend, static_cast<float*>(a.out));
    return fbbev_rt_last_error();
}

// The plain route for one tile size and lane shape: `a` is complete but for the LDS of the routes that size their own.  (A template
// of its own, not one ladder per route: the instantiations of a tile size stay together, in this order, in the code object.)
template <int TV, int CPL>
static int pool_fwd_planar(pool_launch a, const pool_flags& f) {
    const int CC = a.C / a.csplit, nt = f.threads(), et = f.et();
    const int st = et != 0 ? 4 : f.store();                 // 16-bit output storage is built for the default store policy only
    if (f.split_long || f.gather8) {
        // tolerance mode (long intervals summed by the whole workgroup) and the eight-points-per-gather-batch experiment (same
        // bits): fp32 volume, default store policy, 256 threads, 64- / 128-voxel tiles
        if constexpr (TV == 64 || TV == 128) {
            if (st == 4 && et == 0 && nt == 256) {
                if (f.split_long) {
                    a.lds += ((size_t)TV + 4) * sizeof(int) + (size_t)FBBEV_POOL_SPLIT_GROUPS * CC * sizeof(float);   // long-interval list + partial sums
                    return pool_launch_dense2<TV, CPL, 4, 256, 0, false, FBBEV_POOL_SPLIT_LEN, 4>(a);
                }
                return pool_launch_dense2<TV, CPL, 4, 256, 0, false, 0, 8>(a);
            }
        }
        return FBBEV_E_UNSUPPORTED;
    }
    if (et != 0) {
        if (!a.addend && nt == 256) {                       // no epilogue add: the LDS tile itself is 16-bit (see the kernel)
            a.lds = pool_planar_lds16_bytes(CC, TV);
            FBBEV_POOL_ET16(et, return pool_launch_dense2<TV, CPL, 4, 256, ET, true, 0, 4>(a));
        }
        FBBEV_POOL_ET16(et, FBBEV_POOL_NT(nt, return pool_launch_dense2<TV, CPL, 4, NT, ET, false, 0, 4>(a)));
    }
    FBBEV_POOL_WITH3(ST, st, 4, 0, 1, FBBEV_POOL_NT(nt, return pool_launch_dense2<TV, CPL, ST, NT, 0, false, 0, 4>(a)));   // (the default policy first)
    return FBBEV_E_UNSUPPORTED;                             // (not reached: every ladder above returns)
}

// `strides`: as the caller passed them (0 = contiguous)
static int pool_dense_fwd(const pool_call& c, float* out, const pool_strides& strides, const float* addend) {
    const pool_grid& g = c.g;
    const pool_flags& f = c.f;
    if (!pool_grid_positive(g)) return FBBEV_E_BADARG;
    if (!pool_gather_present(c.in) || !out || !c.tile_ws) return FBBEV_E_BADARG;
    if (g.C % 4 != 0 || g.C > 256 || g.yx % 4 != 0 || !aligned16(out) || !aligned16(c.in.feat)) return FBBEV_E_UNSUPPORTED;
    if (!pool_grid_fits_int(g)) return FBBEV_E_UNSUPPORTED;
    const pool_strides s = pool_volume_strides(strides.b, strides.c, g);
    if (s.err) return s.err;
    const int tv = pick_tile(c.tile_voxels);
    const int tiles_per_plane = (int)((g.yx + tv - 1) / tv);
    const long long n_tiles = (long long)g.B * g.Z * tiles_per_plane;
    if (c.tile_ws_bytes < pool_tile_table_bytes(n_tiles)) return FBBEV_E_WORKSPACE;
    if (f.et() != 0) {   // 16-bit storage: 8 elements per 16-byte store
        if (f.bf16 && f.f16) return FBBEV_E_BADARG;
        if (f.channels_last) return FBBEV_E_UNSUPPORTED;
        if (g.yx % 8 != 0 || s.c % 8 != 0 || s.b % 8 != 0) return FBBEV_E_UNSUPPORTED;
    }
    if (addend && (f.channels_last || !aligned16(addend))) return FBBEV_E_UNSUPPORTED;
    if (f.channels_last) {
        // out is (B,Z,Y,X,C) contiguous
        if (s.b != (long long)g.C * g.Z * g.yx || s.c != g.Z * g.yx) return FBBEV_E_BADARG;
        if (const int sh = small_tile_shift(c.tile_voxels)) return pool_fwd_cl_small(c, out, sh);
        return pool_fwd_cl(c, out, tv);
    }
    pool_launch a = pool_launch_of(c);
    a.csplit = f.csplit(g.C);
    const int CC = g.C / a.csplit, cpl = f.cpl(CC), nt = f.threads();
    if (nt / (CC / cpl) < 1) return FBBEV_E_UNSUPPORTED;
    a.yx = (int)g.yx; a.tpp = tiles_per_plane;
    a.n_blocks = n_tiles * a.csplit;
    a.lds = pool_planar_lds_bytes(CC, tv);
    // chunks of 64 tiles where the field is 0: the planar kernel's first measurements with the swizzle name no chunk size
    // (profiles/r01_pool_variants_BL2_B16.jsonl, the `_swz` variants); the later sweeps and the Python side always say one
    a.swizzle = f.swizzle(6);
    if (a.n_blocks + 8 >= (1ll << 31) || a.lds > 160 * 1024) return FBBEV_E_UNSUPPORTED;
    a.out = out; a.out_stride_b = s.b; a.out_stride_c = s.c; a.addend = addend;
    if (f.pipe && f.et() == 0 && !f.split_long && nt == 256 && f.store() == 4 && (tv == 64 || tv == 128 || tv == 256))
        return pool_fwd_pipe(a, n_tiles, tv, cpl);
    FBBEV_POOL_TILE(tv, FBBEV_POOL_CPL(cpl, return pool_fwd_planar<TV, CPL>(a, f)));
    return FBBEV_E_UNSUPPORTED;                             // (not reached)
}

extern "C" int fbbev_bev_pool_v2_dense_fwd(const float* depth, const float* feat,
                                           const int32_t* ranks_depth, const int32_t* ranks_feat,
                                           const int32_t* interval_rank, const int32_t* interval_starts,
                                           const int32_t* interval_lengths, int B, int C, int Z, int Y,
                                           int X, float* out, long long out_stride_b, long long out_stride_c,
                                           const void* tile_ws, size_t tile_ws_bytes, int tile_voxels,
                                           int flags, fbbev_stream_t stream_) {
    const pool_call c = {{depth, feat, ranks_depth, ranks_feat, interval_rank, interval_starts, interval_lengths}, pool_grid_of(B, C, Z, Y, X),
                         tile_ws, tile_ws_bytes, tile_voxels, pool_flags_of(flags), (fbbev_rt_stream)stream_};
    return pool_dense_fwd(c, out, {out_stride_b, out_stride_c, 0}, nullptr);
}

// ... with a (B,C,Y,X) addend broadcast over z in the epilogue
extern "C" int fbbev_bev_pool_v2_dense_fwd_add(const float* depth, const float* feat,
                                               const int32_t* ranks_depth, const int32_t* ranks_feat,
                                               const int32_t* interval_rank, const int32_t* interval_starts,
                                               const int32_t* interval_lengths, int B, int C, int Z, int Y,
                                               int X, float* out, long long out_stride_b, long long out_stride_c,
                                               const void* tile_ws, size_t tile_ws_bytes, int tile_voxels,
                                               int flags, const float* addend, fbbev_stream_t stream_) {
    if (!addend) return FBBEV_E_BADARG;
    const pool_call c = {{depth, feat, ranks_depth, ranks_feat, interval_rank, interval_starts, interval_lengths}, pool_grid_of(B, C, Z, Y, X),
                         tile_ws, tile_ws_bytes, tile_voxels, pool_flags_of(flags), (fbbev_rt_stream)stream_};
    return pool_dense_fwd(c, out, {out_stride_b, out_stride_c, 0}, addend);
}

// ---- the dense forward as rows of a strided slot
template <int TV, int CPL, int ST, int ET>
static int pool_launch_rows(const pool_launch& a) {
    FBBEV_LAUNCH((k_pool_fwd_dense_rows<TV, CPL, ST, 256, ET>), pool_swizzled_grid(a.n_blocks, a.swizzle), 256, a.lds, a.stream, a.C, a.nvox, a.zyx,
                 a.yx, (int)a.n_blocks, a.swizzle, FBBEV_POOL_GATHER(a.in), a.tile_meta, a.addend, a.addend_stride, a.out, a.out_stride_b);
    return fbbev_rt_last_error();
}

// 16-bit rows: 8 channels per lane (one 16-byte store), built for the default `sc1 nt` store policy like the planar 16-bit kernels
template <int TV>
static int pool_fwd_rows(const pool_launch& a, int et, int cpl, int st) {
    if (et != 0) FBBEV_POOL_ET16(et, return pool_launch_rows<TV, 8, 4, ET>(a));
    FBBEV_POOL_CPL(cpl, FBBEV_POOL_ST(st, return pool_launch_rows<TV, CPL, ST, 0>(a)));
    return FBBEV_E_UNSUPPORTED;                             // (not reached)
}

extern "C" int fbbev_bev_pool_v2_dense_fwd_rows(const float* depth, const float* feat, const int32_t* ranks_depth,
                                                const int32_t* ranks_feat, const int32_t* interval_rank,
                                                const int32_t* interval_starts, const int32_t* interval_lengths, int B, int C,
                                                int Z, int Y, int X, void* out_rows, long long out_stride_b,
                                                const float* addend_rows, long long addend_row_stride, const void* tile_ws,
                                                size_t tile_ws_bytes, int tile_voxels, int flags, fbbev_stream_t stream_) {
    const pool_call c = {{depth, feat, ranks_depth, ranks_feat, interval_rank, interval_starts, interval_lengths}, pool_grid_of(B, C, Z, Y, X),
                         tile_ws, tile_ws_bytes, tile_voxels, pool_flags_of(flags), (fbbev_rt_stream)stream_};
    const pool_grid& g = c.g;
    const pool_flags& f = c.f;
    if (!pool_grid_positive(g)) return FBBEV_E_BADARG;
    if (!pool_gather_present(c.in) || !out_rows || !tile_ws) return FBBEV_E_BADARG;
    if (f.bf16 && f.f16) return FBBEV_E_BADARG;             // (here right after the pointers; the planar entries look at the table's bytes first)
    const int et = f.et();
    const int ve = et == 0 ? 4 : 8;                                     // elements of a 16-byte store
    if (!pool_grid_fits_int(g)) return FBBEV_E_UNSUPPORTED;             // flat voxel index: int
    const long long zyx = g.Z * g.yx;
    if (out_stride_b == 0) out_stride_b = zyx * C;                      // contiguous (B, Z*Y*X, C)
    if (addend_row_stride == 0) addend_row_stride = C;
    if (out_stride_b < zyx * C || addend_row_stride < C) return FBBEV_E_BADARG;
    if (C % ve != 0 || C > 256 || out_stride_b % ve != 0 || addend_row_stride % 4 != 0 || !aligned16(out_rows) || !aligned16(feat) ||
        !aligned16(addend_rows)) return FBBEV_E_UNSUPPORTED;
    if (small_tile_shift(tile_voxels)) return FBBEV_E_UNSUPPORTED;      // the small-tile kernel keeps its fp32, contiguous, no-addend form
    const int tv = pick_tile(tile_voxels);
    const int cpl = et != 0 ? 8 : f.cpl(C);
    if (256 / (C / cpl) < 1) return FBBEV_E_UNSUPPORTED;                // a voxel row takes more lanes than a workgroup has
    pool_launch a = pool_launch_of(c);
    a.n_blocks = (g.nvox + tv - 1) / tv;
    if (tile_ws_bytes < pool_tile_table_bytes(a.n_blocks)) return FBBEV_E_WORKSPACE;
    a.lds = pool_index_lds_bytes(tv);
    a.nvox = (int)g.nvox; a.zyx = (int)zyx; a.yx = (int)g.yx;
    a.swizzle = f.swizzle(4);                                           // the flat tiles' default: this kernel walks them as pool_fwd_cl's does
    a.addend = addend_rows; a.addend_stride = addend_row_stride; a.out = out_rows; a.out_stride_b = out_stride_b;
    FBBEV_POOL_TILE(tv, return pool_fwd_rows<TV>(a, et, cpl, f.store()));
    return FBBEV_E_UNSUPPORTED;                                         // (not reached)
}

// Measurement aid (bench.py `roofline.store_floor_ms` / `no_gather_ms`): the default fp32 instantiation of the dense kernel
// (128-voxel tiles, 8 channels per lane, 256 threads, `sc1 nt` stores) with its gathers compiled out -- same grid, tile
// walk and XCD order as the product launch with these flags.  mode 1: store pattern alone; mode 2: all but the depth /
// feature gathers.  Writes zeros to `out`.  With FBBEV_POOL_OUT_BF16: the 16-bit-tile instantiation of the bf16-storage leg.
extern "C" int fbbev_diag_pool_store_floor(const float* depth, const float* feat, const int32_t* ranks_depth,
                                           const int32_t* ranks_feat, const int32_t* interval_rank,
                                           const int32_t* interval_starts, const int32_t* interval_lengths, int B, int C,
                                           int Z, int Y, int X, float* out, const void* tile_ws, size_t tile_ws_bytes,
                                           int tile_voxels, int flags, int mode, fbbev_stream_t stream_) {
    const pool_call c = {{depth, feat, ranks_depth, ranks_feat, interval_rank, interval_starts, interval_lengths}, pool_grid_of(B, C, Z, Y, X),
                         tile_ws, tile_ws_bytes, tile_voxels, pool_flags_of(flags), (fbbev_rt_stream)stream_};
    const pool_grid& g = c.g;
    const pool_flags& f = c.f;
    if (!pool_grid_positive(g) || mode < 1 || mode > 3) return FBBEV_E_BADARG;
    if (!pool_gather_present(c.in) || !out || !tile_ws) return FBBEV_E_BADARG;
    if (tile_voxels != 128 || g.yx % (f.bf16 ? 8 : 4) != 0 || !aligned16(out) || f.channels_last || f.f16 || !pool_grid_fits_int(g))
        return FBBEV_E_UNSUPPORTED;
    pool_launch a = pool_launch_of(c);
    a.csplit = f.csplit(C);
    const int CC = C / a.csplit;
    if (f.cpl(CC) != 8 || f.store() != 4 || f.wg != 0 || 256 / (CC / 8) < 1) return FBBEV_E_UNSUPPORTED;
    a.yx = (int)g.yx; a.tpp = (int)((g.yx + 127) / 128);
    const long long n_tiles = (long long)B * Z * a.tpp;
    if (tile_ws_bytes < pool_tile_table_bytes(n_tiles)) return FBBEV_E_WORKSPACE;
    a.n_blocks = n_tiles * a.csplit;
    a.lds = f.bf16 ? pool_planar_lds16_bytes(CC, 128) : pool_planar_lds_bytes(CC, 128);
    a.swizzle = f.swizzle(6);                               // as the product launch (pool_dense_fwd)
    if (a.n_blocks + 8 >= (1ll << 31) || a.lds > 64 * 1024) return FBBEV_E_UNSUPPORTED;   // (64 KiB here; the product takes 160)
    a.out = out; a.out_stride_b = (long long)C * Z * g.yx; a.out_stride_c = Z * g.yx;
    const long long grid = pool_swizzled_grid(a.n_blocks, a.swizzle);
    FBBEV_POOL_WITH(OT, f.bf16 ? 1 : 0, 1, 0, FBBEV_POOL_WITH3(MODE, mode, 1, 2, 3, FBBEV_LAUNCH(
        (k_pool_fwd_dense2<128, 8, 4, 256, OT, OT == 1, MODE>), grid, 256, a.lds, a.stream, a.C, a.Z, a.yx, a.tpp, a.csplit, (int)a.n_blocks,
        a.swizzle, a.out_stride_b, a.out_stride_c, FBBEV_POOL_GATHER(a.in), a.tile_meta, a.addend, static_cast<float*>(a.out))));
    return fbbev_rt_last_error();
}

// ---- lift-splat in ONE entry
// Workspace layout of fbbev_lift_splat_fused (all blocks 256-byte aligned): the seven padded index tensors + counts the build
// writes, the NHWC feature rows, the tile table, the ranking workspace.
struct lift_dims { int B, N, D, H, W, C, Z, Y, X; };
static inline bool lift_dims_positive(const lift_dims& d) {
    return d.B > 0 && d.N > 0 && d.D > 0 && d.H > 0 && d.W > 0 && d.C > 0 && d.Z > 0 && d.Y > 0 && d.X > 0;
}
static inline long long lift_points(const lift_dims& d) { return (long long)d.B * d.N * d.D * d.H * d.W; }   // frustum points
struct lift_splat_layout {
    bool ok;                                                // positive dimensions and fewer than 2^31 frustum points
    size_t ranks_bev, ranks_depth, ranks_feat, interval_starts, interval_lengths, interval_rank, counts, feat, tile, rank, total;
    size_t tile_bytes, rank_bytes;
};
static lift_splat_layout lift_splat_plan(const lift_dims& d) {
    lift_splat_layout L = {};
    if (!lift_dims_positive(d)) return L;
    const long long n = lift_points(d);
    if (n >= (1ll << 31)) return L;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off = align_up(off + bytes, 256); return o; };
    L.ranks_bev = take((size_t)n * 4); L.ranks_depth = take((size_t)n * 4); L.ranks_feat = take((size_t)n * 4);
    L.interval_starts = take((size_t)n * 4); L.interval_lengths = take((size_t)n * 4); L.interval_rank = take((size_t)n * 4);
    L.counts = take(16);
    L.feat = take((size_t)d.B * d.N * d.H * d.W * d.C * 4);
    L.tile_bytes = fbbev_pool_dense_workspace_bytes(d.B, d.Z, d.Y, d.X);
    L.tile = take(L.tile_bytes);
    L.rank_bytes = fbbev_rank_workspace_bytes(n);
    L.rank = take(L.rank_bytes);
    L.total = off;
    L.ok = true;
    return L;
}

extern "C" size_t fbbev_lift_splat_fused_ws_bytes(int B, int N, int D, int H, int W, int C, int Z, int Y, int X) {
    return lift_splat_plan({B, N, D, H, W, C, Z, Y, X}).total;      // 0 without a plan
}

extern "C" int fbbev_lift_splat_fused_ws_offsets(int B, int N, int D, int H, int W, int C, int Z, int Y, int X, size_t* offsets8) {
    const lift_splat_layout L = lift_splat_plan({B, N, D, H, W, C, Z, Y, X});
    if (!offsets8 || !L.ok) return FBBEV_E_BADARG;
    offsets8[0] = L.ranks_bev; offsets8[1] = L.ranks_depth; offsets8[2] = L.ranks_feat; offsets8[3] = L.interval_starts;
    offsets8[4] = L.interval_lengths; offsets8[5] = L.interval_rank; offsets8[6] = L.counts; offsets8[7] = L.feat;
    return 0;
}

extern "C" int fbbev_lift_splat_fused(const float* frustum, const float* xs, const float* ys, const float* ds, const float* rots,
                                      const float* trans, const float* intrins, const float* post_rots, const float* post_trans,
                                      const float* bda, const float* depth, const float* context, int B, int N, int D, int H,
                                      int W, int C, const float* lower3, const float* interval3, const float* grid_size3, int Z,
                                      int Y, int X, void* out, long long out_stride_b, long long out_stride_c, int tile_voxels,
                                      int flags, void* workspace, size_t workspace_bytes, uint32_t* cam_key, int32_t* cache_state,
                                      fbbev_stream_t stream_) {
    const lift_dims d = {B, N, D, H, W, C, Z, Y, X};
    if (!depth || !context || !out || !workspace) return FBBEV_E_BADARG;      // (its four pointers before the plan)
    const lift_splat_layout L = lift_splat_plan(d);
    if (!L.ok) return FBBEV_E_BADARG;
    if ((cam_key == nullptr) != (cache_state == nullptr)) return FBBEV_E_BADARG;
    if (workspace_bytes < L.total) return FBBEV_E_WORKSPACE;
    if (!aligned16(workspace)) return FBBEV_E_UNSUPPORTED;
    char* ws = static_cast<char*>(workspace);
    auto i32 = [&](size_t o) { return reinterpret_cast<int32_t*>(ws + o); };
    const int n = (int)lift_points(d);
    // view_transformer.py:458-498 + :547-605: geometry + voxel ranking, device-side counts (cache_state[0] = 1 on a key hit)
    int rc = lift_rank_build_impl(frustum, xs, ys, ds, rots, trans, intrins, post_rots, post_trans, bda, B, N, D, H, W, lower3,
                                  interval3, grid_size3, i32(L.ranks_bev), i32(L.ranks_depth), i32(L.ranks_feat),
                                  i32(L.interval_starts), i32(L.interval_lengths), i32(L.interval_rank), i32(L.counts),
                                  ws + L.rank, L.rank_bytes, (fbbev_rt_stream)stream_, cam_key, cache_state);
    if (rc) return rc;
    // :536 / bev_pool.py:18: feat.permute(0,1,3,4,2).contiguous()
    float* feat = reinterpret_cast<float*>(ws + L.feat);
    rc = fbbev_nchw_to_nhwc(context, feat, B * N, C, H * W, stream_);
    if (rc) return rc;
    // bev_pool.py:24-35,88: new_zeros + kernel + permute().contiguous() as tile index + one dense pass
    if (cache_state)
        rc = fbbev_pool_tile_index_cached(i32(L.interval_rank), i32(L.interval_starts), i32(L.counts), n, B, Z, Y, X,
                                          tile_voxels, flags, ws + L.tile, L.tile_bytes, cache_state, cache_state + 2, stream_);
    else
        rc = fbbev_pool_tile_index(i32(L.interval_rank), i32(L.interval_starts), i32(L.counts), n, B, Z, Y, X, tile_voxels, flags,
                                   ws + L.tile, L.tile_bytes, stream_);
    if (rc) return rc;
    return fbbev_bev_pool_v2_dense_fwd(depth, feat, i32(L.ranks_depth), i32(L.ranks_feat), i32(L.interval_rank), i32(L.interval_starts),
                                       i32(L.interval_lengths), B, C, Z, Y, X, static_cast<float*>(out), out_stride_b, out_stride_c,
                                       ws + L.tile, L.tile_bytes, tile_voxels, flags, stream_);
}

// ---- the Z-mean: out = mean over z of the pooled volume, (B, C, Y, X) or as rows
struct pool_zmean_out {
    float* out;
    int z_groups; float* partial; size_t partial_bytes;     // z_groups > 1: the planes dealt to that many workgroups, summed by a second kernel
    int rows_out; const float* row_bias;                    // rows_out: out is (B, Y*X, C) = mean + row_bias (Y*X, C; may be null)
};
static int pool_zmean(const pool_call& c, const pool_zmean_out& o) {
    const pool_grid& g = c.g;
    const pool_flags& f = c.f;
    if (!pool_grid_positive(g)) return FBBEV_E_BADARG;
    if (o.rows_out && (o.z_groups != 1 || (o.row_bias && !aligned16(o.row_bias)))) return FBBEV_E_UNSUPPORTED;   // (before the pointers)
    if (!pool_gather_present(c.in) || !o.out || !c.tile_ws) return FBBEV_E_BADARG;
    if (g.C % 4 != 0 || g.C > 256 || g.yx % 4 != 0 || !aligned16(o.out) || !aligned16(c.in.feat)) return FBBEV_E_UNSUPPORTED;
    if (!pool_grid_fits_int(g) || f.channels_last) return FBBEV_E_UNSUPPORTED;
    const int tv = pick_tile(c.tile_voxels);
    if (tv > 256) return FBBEV_E_UNSUPPORTED;
    const int tiles_per_plane = (int)((g.yx + tv - 1) / tv);
    const long long n_tiles = (long long)g.B * g.Z * tiles_per_plane;
    if (c.tile_ws_bytes < pool_tile_table_bytes(n_tiles)) return FBBEV_E_WORKSPACE;
    const int csplit = f.csplit(g.C), CC = g.C / csplit, cpl = f.cpl(CC);
    if (256 / (CC / cpl) < 1) return FBBEV_E_UNSUPPORTED;
    const size_t lds = pool_planar_lds_bytes(CC, tv);
    if (lds > 64 * 1024) return FBBEV_E_UNSUPPORTED;
    const long long blocks = (long long)g.B * tiles_per_plane * csplit;
    const int z_groups = o.z_groups > g.Z ? g.Z : o.z_groups;
    const long long n_out = (long long)g.B * g.C * g.yx;
    if (z_groups > 1 && o.partial_bytes < (size_t)z_groups * n_out * sizeof(float)) return FBBEV_E_WORKSPACE;
    if (blocks * z_groups >= (1ll << 31)) return FBBEV_E_UNSUPPORTED;
    const int* meta = static_cast<const int*>(c.tile_ws);
    // round 5: the column form (every plane's metadata at once, a lane group per pixel; the same bits) when the column's slot table
    // fits -- OPT-IN (FBBEV_ZMEAN_COL=1): built to cut the Z dependent round-trip chains of the plane walk, measured SLOWER at the
    // BASELINE configs[2] grid, B = 4 (135.7 vs 103.9 us, S3 1.395 vs 1.360 ms: profiles/r05_exp_zmean_col.md -- 54 KB of LDS = 2
    // workgroups per CU instead of 5, and a lane group's pixels are a serial chain of their own)
    FBBEV_KNOB_ONCE(bool, col_on, fbbev_env_int("FBBEV_ZMEAN_COL", 0) != 0);
    const size_t lds_col = fbbev_zmean_col_lds_bytes(CC, tv, g.Z);
    if (col_on && !o.rows_out && z_groups == 1 && g.Z <= 64 && lds_col <= 64 * 1024) {
        FBBEV_POOL_TILE3(tv, FBBEV_POOL_CPL(cpl, FBBEV_LAUNCH((k_pool_zmean_col<TV, CPL, 256>), blocks, 256, lds_col, c.stream, g.C, g.Z, (int)g.yx,
                                                              tiles_per_plane, csplit, (int)blocks, FBBEV_POOL_GATHER(c.in), meta, o.out)));
        FBBEV_CHECK_LAUNCH();
        return 0;
    }
    FBBEV_POOL_TILE3(tv, FBBEV_POOL_CPL(cpl, FBBEV_LAUNCH((k_pool_zmean<TV, CPL, 256>), blocks * z_groups, 256, lds, c.stream, g.C, g.Z, (int)g.yx,
                                                          tiles_per_plane, csplit, (int)blocks, FBBEV_POOL_GATHER(c.in), meta, o.out, z_groups,
                                                          o.partial, o.rows_out, o.row_bias)));
    FBBEV_CHECK_LAUNCH();
    if (z_groups > 1) {
        FBBEV_LAUNCH(k_pool_zmean_reduce, (n_out / 4 + 255) / 256, 256, 0, c.stream, (const float*)o.partial, n_out, z_groups, (float)g.Z,
                     o.out);
        FBBEV_CHECK_LAUNCH();
    }
    return 0;
}

extern "C" int fbbev_pool_zmean(const float* depth, const float* feat, const int32_t* ranks_depth,
                                const int32_t* ranks_feat, const int32_t* interval_rank,
                                const int32_t* interval_starts, const int32_t* interval_lengths, int B, int C, int Z,
                                int Y, int X, float* out_mean, const void* tile_ws, size_t tile_ws_bytes,
                                int tile_voxels, int flags, fbbev_stream_t stream_) {
    const pool_call c = {{depth, feat, ranks_depth, ranks_feat, interval_rank, interval_starts, interval_lengths}, pool_grid_of(B, C, Z, Y, X),
                         tile_ws, tile_ws_bytes, tile_voxels, pool_flags_of(flags), (fbbev_rt_stream)stream_};
    return pool_zmean(c, {out_mean, 1, nullptr, 0, 0, nullptr});
}

// fbbev_pool_zmean with the Z planes of a tile dealt to z_groups workgroups (each walks ceil(Z / z_groups) planes) and a caller-owned
// partial buffer of z_groups * B*C*Y*X floats; a second small kernel adds the groups in order and divides by Z.  For grids with few
// tiles (the shipped 100x100x8 grid): the single pass is one Z-plane latency chain per workgroup.
extern "C" int fbbev_pool_zmean_split(const float* depth, const float* feat, const int32_t* ranks_depth,
                                      const int32_t* ranks_feat, const int32_t* interval_rank,
                                      const int32_t* interval_starts, const int32_t* interval_lengths, int B, int C, int Z,
                                      int Y, int X, float* out_mean, const void* tile_ws, size_t tile_ws_bytes,
                                      int tile_voxels, int flags, int z_groups, void* partial_ws, size_t partial_ws_bytes,
                                      fbbev_stream_t stream_) {
    if (z_groups < 1 || z_groups > 64) return FBBEV_E_BADARG;
    if (z_groups > 1 && (!partial_ws || !aligned16(partial_ws))) return FBBEV_E_BADARG;
    const pool_call c = {{depth, feat, ranks_depth, ranks_feat, interval_rank, interval_starts, interval_lengths}, pool_grid_of(B, C, Z, Y, X),
                         tile_ws, tile_ws_bytes, tile_voxels, pool_flags_of(flags), (fbbev_rt_stream)stream_};
    return pool_zmean(c, {out_mean, z_groups, static_cast<float*>(partial_ws), partial_ws_bytes, 0, nullptr});
}

// fbbev_pool_zmean with the result written as the backward projection's QUERY ROWS: out_rows (B, Y*X, C) = mean + row_bias (Y*X, C)
// (bev_embedding; may be null) -- backward_projection.py:96-99's flatten + permute + `+ bev_embedding` done by the Z-mean's store
// instead of a transposing pass over (B, C, Y, X).  Single pass only (no Z groups).
extern "C" int fbbev_pool_zmean_rows(const float* depth, const float* feat, const int32_t* ranks_depth, const int32_t* ranks_feat,
                                     const int32_t* interval_rank, const int32_t* interval_starts,
                                     const int32_t* interval_lengths, int B, int C, int Z, int Y, int X, const float* row_bias,
                                     float* out_rows, const void* tile_ws, size_t tile_ws_bytes, int tile_voxels, int flags,
                                     fbbev_stream_t stream_) {
    const pool_call c = {{depth, feat, ranks_depth, ranks_feat, interval_rank, interval_starts, interval_lengths}, pool_grid_of(B, C, Z, Y, X),
                         tile_ws, tile_ws_bytes, tile_voxels, pool_flags_of(flags), (fbbev_rt_stream)stream_};
    return pool_zmean(c, {out_rows, 1, nullptr, 0, 1, row_bias});
}

// ------------------------------------------------------------------------------ MSDeformAttn
extern "C" int fbbev_msda_fwd(const float* value, const int64_t* spatial_shapes,
                              const int64_t* level_start_index, const float* sampling_loc,
                              const float* attn_weight, int batch, int spatial_size, int num_heads,
                              int channels, int num_levels, int num_query, int num_point, float* out,
                              fbbev_stream_t stream_) {
    if (batch < 0 || spatial_size <= 0 || num_heads <= 0 || channels <= 0 || num_levels <= 0 ||
        num_query < 0 || num_point <= 0) return FBBEV_E_BADARG;
    const long long n = (long long)batch * num_query * num_heads * channels;
    if (n == 0) return 0;
    if (!value || !spatial_shapes || !level_start_index || !sampling_loc || !attn_weight || !out)
        return FBBEV_E_BADARG;
    fbbev_rt_stream stream = (fbbev_rt_stream)stream_;
    long long blocks = (n + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    FBBEV_LAUNCH(k_msda_fwd, blocks, 256, 0, stream, n, value, spatial_shapes, level_start_index,
                 sampling_loc, attn_weight, spatial_size, num_heads, channels, num_levels, num_query,
                 num_point, out);
    FBBEV_CHECK_LAUNCH();
    return 0;
}

extern "C" int fbbev_msda_fwd_fused(const float* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                                    const float* ref_points, const float* offsets, const float* attn_weight, int batch,
                                    int spatial_size, int num_heads, int channels, int num_levels, int num_query,
                                    int num_point, int head_stride, int offsets_head_minor, float* out,
                                    fbbev_stream_t stream_) {
    if (batch < 0 || spatial_size <= 0 || num_heads <= 0 || channels <= 0 || num_levels <= 0 || num_query < 0 ||
        num_point <= 0) return FBBEV_E_BADARG;
    const long long units = (long long)batch * num_query * num_heads;
    if (units == 0) return 0;
    if (!value || !spatial_shapes || !level_start_index || !ref_points || !offsets || !attn_weight || !out)
        return FBBEV_E_BADARG;
    const int HS = head_stride == 0 ? channels : head_stride;
    if (HS < channels) return FBBEV_E_BADARG;
    if ((((uintptr_t)offsets) & 7) != 0) return FBBEV_E_UNSUPPORTED;
    const bool wide = HS % 4 == 0 && HS >= (channels + 3) / 4 * 4 && aligned16(value);
    const bool qi = (offsets_head_minor & 4) != 0;                 // value rows stored [chunk][head][4 floats]
    if (qi && !wide) return FBBEV_E_UNSUPPORTED;
    if ((long long)batch * spatial_size * num_heads * HS * 4 >= (1ll << 32)) return FBBEV_E_UNSUPPORTED;   // 32-bit byte offsets
    long long ub = ((units + 255) / 256 + 7) / 8 * 8;             // XCD-contiguous order: a multiple of 8 workgroups
    if (ub > 65536) ub = 65536;
    // attention weights staged through LDS ([256][L*P+1] floats) when they fit beside 4 workgroups per CU
    const int LP = num_levels * num_point;
    const bool stage = LP % 4 == 0 && LP <= 36 && aligned16(attn_weight);
    const size_t lds = stage ? (size_t)256 * (LP + 1) * sizeof(float) : 0;
#define FBBEV_MSDA_UNIT_W(DH_, W_, Q_)                                                                               \
    FBBEV_LAUNCH((k_msda_fwd_unit<DH_, W_, Q_>), ub, 256, lds, (fbbev_rt_stream)stream_, units, value,                \
                 spatial_shapes, level_start_index, ref_points, offsets, attn_weight, spatial_size, num_heads,        \
                 num_levels, num_query, num_point, HS, (offsets_head_minor & 1) ? 1 : 0, stage ? 1 : 0, out)
#define FBBEV_MSDA_UNIT(DH_) do { if (qi) FBBEV_MSDA_UNIT_W(DH_, true, true); else if (wide) FBBEV_MSDA_UNIT_W(DH_, true, false); \
                                  else FBBEV_MSDA_UNIT_W(DH_, false, false); } while (0)
    if (channels == 10) FBBEV_MSDA_UNIT(10);
    else if (channels == 8) FBBEV_MSDA_UNIT(8);
    else if (channels == 16) FBBEV_MSDA_UNIT(16);
    else if (channels == 32) FBBEV_MSDA_UNIT(32);
    else if (channels == 4) FBBEV_MSDA_UNIT(4);
    else return FBBEV_E_UNSUPPORTED;
#undef FBBEV_MSDA_UNIT
#undef FBBEV_MSDA_UNIT_W
    FBBEV_CHECK_LAUNCH();
    return 0;
}

extern "C" int fbbev_msda_bwd(const float* value, const int64_t* spatial_shapes,
                              const int64_t* level_start_index, const float* sampling_loc,
                              const float* attn_weight, const float* grad_output, int batch,
                              int spatial_size, int num_heads, int channels, int num_levels,
                              int num_query, int num_point, float* grad_value,
                              float* grad_sampling_loc, float* grad_attn_weight,
                              fbbev_stream_t stream_) {
    if (batch < 0 || spatial_size <= 0 || num_heads <= 0 || channels <= 0 || num_levels <= 0 ||
        num_query < 0 || num_point <= 0) return FBBEV_E_BADARG;
    const long long n_units = (long long)batch * num_query * num_heads;
    if (n_units == 0) return 0;
    if (!value || !spatial_shapes || !level_start_index || !sampling_loc || !attn_weight ||
        !grad_output || !grad_value || !grad_sampling_loc || !grad_attn_weight) return FBBEV_E_BADARG;
    fbbev_rt_stream stream = (fbbev_rt_stream)stream_;
#define FBBEV_MSDA_BWD(GW)                                                                          \
    FBBEV_LAUNCH(k_msda_bwd<GW>, (n_units * GW + 255) / 256, 256, 0, stream, n_units, value,       \
                 spatial_shapes, level_start_index, sampling_loc, attn_weight, grad_output,         \
                 spatial_size, num_heads, channels, num_levels, num_query, num_point, grad_value,   \
                 grad_sampling_loc, grad_attn_weight)
    if (channels <= 16) FBBEV_MSDA_BWD(16);
    else if (channels <= 32) FBBEV_MSDA_BWD(32);
    else FBBEV_MSDA_BWD(64);
#undef FBBEV_MSDA_BWD
    FBBEV_CHECK_LAUNCH();
    return 0;
}

extern "C" size_t fbbev_msda_bwd_det_ws_bytes(int batch, int spatial_size, int num_heads, int channels) {
    if (batch <= 0 || spatial_size <= 0 || num_heads <= 0 || channels <= 0) return 0;
    return FBBEV_FIX_HDR + (size_t)batch * spatial_size * num_heads * channels * sizeof(unsigned long long);
}
// fbbev_msda_bwd with a flags word.  FBBEV_FLAG_DETERMINISTIC: the value gradient as 64-bit fixed point in det_ws (scale from
// max |grad_output| x max |attn_weight|, at most num_query * num_point adds per word), converted and ADDED to grad_value.
extern "C" int fbbev_msda_bwd_ex(const float* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                                 const float* sampling_loc, const float* attn_weight, const float* grad_output, int batch,
                                 int spatial_size, int num_heads, int channels, int num_levels, int num_query, int num_point,
                                 float* grad_value, float* grad_sampling_loc, float* grad_attn_weight, int flags, void* det_ws,
                                 size_t det_ws_bytes, fbbev_stream_t stream_) {
    if (!(flags & FBBEV_FLAG_DETERMINISTIC))
        return fbbev_msda_bwd(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, grad_output, batch, spatial_size,
                              num_heads, channels, num_levels, num_query, num_point, grad_value, grad_sampling_loc, grad_attn_weight,
                              stream_);
    if (batch < 0 || spatial_size <= 0 || num_heads <= 0 || channels <= 0 || num_levels <= 0 ||
        num_query < 0 || num_point <= 0) return FBBEV_E_BADARG;
    const long long n_units = (long long)batch * num_query * num_heads;
    if (n_units == 0) return 0;
    if (!value || !spatial_shapes || !level_start_index || !sampling_loc || !attn_weight ||
        !grad_output || !grad_value || !grad_sampling_loc || !grad_attn_weight || !det_ws) return FBBEV_E_BADARG;
    if (det_ws_bytes < fbbev_msda_bwd_det_ws_bytes(batch, spatial_size, num_heads, channels) || !aligned16(det_ws))
        return FBBEV_E_WORKSPACE;
    fbbev_rt_stream stream = (fbbev_rt_stream)stream_;
    const long long n_val = (long long)batch * spatial_size * num_heads * channels;
    const long long n_out = n_units * channels, n_attn = n_units * num_levels * num_point;
    unsigned int* hdr = static_cast<unsigned int*>(det_ws);
    int e = fbbev_rt_memset_async(det_ws, 0, fbbev_msda_bwd_det_ws_bytes(batch, spatial_size, num_heads, channels), stream);
    if (e) return e;
    auto grid = [](long long n) { long long g = (n + 255) / 256; return g > 1024 ? 1024 : (g < 1 ? 1 : g); };
    FBBEV_LAUNCH(k_da_taps_absmax, grid(n_out), 256, 0, stream, grad_output, n_out, hdr);
    FBBEV_LAUNCH(k_da_taps_absmax, grid(n_attn), 256, 0, stream, attn_weight, n_attn, hdr + 1);
    int kq = 0;
    while ((1ll << kq) < (long long)num_query * num_point) ++kq;
    FBBEV_LAUNCH(k_fix_scale, 1, 64, 0, stream, 2, kq, hdr);
    FBBEV_CHECK_LAUNCH();
    float* fix_ws = static_cast<float*>(det_ws);
#define FBBEV_MSDA_BWD_FIX(GW)                                                                                     \
    FBBEV_LAUNCH((k_msda_bwd<GW, true, true>), (n_units * GW + 255) / 256, 256, 0, stream, n_units, value,         \
                 spatial_shapes, level_start_index, sampling_loc, attn_weight, grad_output, spatial_size, num_heads, \
                 channels, num_levels, num_query, num_point, fix_ws, grad_sampling_loc, grad_attn_weight)
    if (channels <= 16) FBBEV_MSDA_BWD_FIX(16);
    else if (channels <= 32) FBBEV_MSDA_BWD_FIX(32);
    else FBBEV_MSDA_BWD_FIX(64);
#undef FBBEV_MSDA_BWD_FIX
    FBBEV_CHECK_LAUNCH();
    FBBEV_LAUNCH(k_fix_to_f32_add, grid(n_val) * 4, 256, 0, stream, (const unsigned int*)hdr, n_val, grad_value);
    FBBEV_CHECK_LAUNCH();
    return 0;
}

// Band-binned fixed-point backward (msda_bwd_kernels.h).  level_hw_host: HOST array of L (h, w) pairs -- the band count is a
// launch dimension.  Plan: tokens per LDS plane from the LDS budget (64 KB: two workgroups per CU; FBBEV_MSDA_BWD_LDS_KB,
// read once, tunes it), a band = whole rows of one level.
struct msda_bwd_plan { int budget, n_bands; size_t lds, ws_ranges, ws; };
static bool msda_bwd_plan_for(int B, int S, int M, int Dh, int L, int Q, int P, const int32_t* level_hw, msda_bwd_plan* pl) {
    if (!level_hw || !(Dh == 4 || Dh == 8 || Dh == 10 || Dh == 16 || Dh == 32) || Q <= 0) return false;
    // measured at BASELINE configs[2] (200 x 200 BEV, B = 4): scatter 2.24 / 0.80 / 0.45 ms with 32 / 64 / 128 KB planes -- the
    // halo of re-evaluated queries per band is what costs, so a band is as tall as LDS allows (one workgroup per CU) ...
    auto read_kb = [] { const int v = fbbev_env_int("FBBEV_MSDA_BWD_LDS_KB", 0); return v >= 1 && v <= 150 ? v : 144; };
    FBBEV_KNOB_ONCE(int, lds_kb, read_kb());      // read once: ws_bytes() and the launch must agree (the emulator tests switch budgets)
    int budget = (lds_kb * 1024) / (Dh * (int)sizeof(long long)) - 16;
    long long nb = 0, tokens = 0;
    int max_tok = 0, max_w = 1;
    for (int l = 0; l < L; ++l) max_w = level_hw[2 * l + 1] > max_w ? level_hw[2 * l + 1] : max_w;
    for (;;) {
        nb = 0; tokens = 0; max_tok = 0;
        for (int l = 0; l < L; ++l) {
            const int h = level_hw[2 * l], w = level_hw[2 * l + 1];
            if (h <= 0 || w <= 0 || h > 32767 || w > budget) return false;
            const int rpb = budget / w;
            nb += (h + rpb - 1) / rpb;
            tokens += (long long)h * w;
            const int t = (rpb < h ? rpb : h) * w;
            max_tok = t > max_tok ? t : max_tok;
        }
        // ... unless that leaves CUs idle: shrink the bands until there is a workgroup per CU (small grids / small batches)
        if ((long long)B * M * nb >= 256 || budget * 3 / 4 < 2 * max_w) break;
        budget = budget * 3 / 4;
    }
    if (tokens != S || nb > 65535 || (long long)B * M * nb >= (1ll << 31)) return false;
    pl->budget = budget;
    pl->n_bands = (int)nb;
    pl->lds = (size_t)FBBEV_DA_PLANE_WORDS(max_tok, Dh) * sizeof(long long);
    pl->ws_ranges = ((size_t)B * L * Q * sizeof(unsigned int) + 255) / 256 * 256;
    pl->ws = pl->ws_ranges + (size_t)B * nb * 2 * sizeof(int);
    return true;
}

extern "C" size_t fbbev_msda_bwd_ws_bytes(int batch, int spatial_size, int num_heads, int channels, int num_levels,
                                          int num_query, int num_point, const int32_t* level_hw_host) {
    msda_bwd_plan pl;
    if (batch <= 0 || spatial_size <= 0 || num_heads <= 0 || channels <= 0 || num_levels <= 0 || num_point <= 0 ||
        !msda_bwd_plan_for(batch, spatial_size, num_heads, channels, num_levels, num_query, num_point, level_hw_host, &pl))
        return 0;
    return pl.ws;
}

extern "C" int fbbev_msda_bwd_ws(const float* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                                 const float* sampling_loc, const float* attn_weight, const float* grad_output, int batch,
                                 int spatial_size, int num_heads, int channels, int num_levels, int num_query, int num_point,
                                 float* grad_value, float* grad_sampling_loc, float* grad_attn_weight,
                                 const int32_t* level_hw_host, void* ws, size_t ws_bytes, fbbev_stream_t stream_) {
    if (batch < 0 || spatial_size <= 0 || num_heads <= 0 || channels <= 0 || num_levels <= 0 || num_query < 0 ||
        num_point <= 0) return FBBEV_E_BADARG;
    msda_bwd_plan pl;
    if (batch == 0 || num_query == 0 || !ws ||
        !msda_bwd_plan_for(batch, spatial_size, num_heads, channels, num_levels, num_query, num_point, level_hw_host, &pl) ||
        ws_bytes < pl.ws)
        return fbbev_msda_bwd(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, grad_output, batch,
                              spatial_size, num_heads, channels, num_levels, num_query, num_point, grad_value,
                              grad_sampling_loc, grad_attn_weight, stream_);
    if (!value || !spatial_shapes || !level_start_index || !sampling_loc || !attn_weight || !grad_output || !grad_value ||
        !grad_sampling_loc || !grad_attn_weight) return FBBEV_E_BADARG;
    fbbev_rt_stream stream = (fbbev_rt_stream)stream_;
    const int B = batch, S = spatial_size, M = num_heads, Dh = channels, L = num_levels, Q = num_query, P = num_point;
    unsigned int* ranges = static_cast<unsigned int*>(ws);
    int* qrange = reinterpret_cast<int*>(static_cast<char*>(ws) + pl.ws_ranges);
    {
        const long long n = (long long)B * L * Q;
        long long blocks = (n + 255) / 256;
        if (blocks > 65536) blocks = 65536;
        FBBEV_LAUNCH(k_msda_row_ranges, blocks, 256, 0, stream, n, spatial_shapes, sampling_loc, M, L, Q, P, ranges);
        FBBEV_CHECK_LAUNCH();
        FBBEV_LAUNCH(k_msda_band_queries, (long long)B * pl.n_bands, 256, 0, stream, spatial_shapes, level_start_index,
                     (const unsigned int*)ranges, L, Q, pl.n_bands, pl.budget, qrange);
        FBBEV_CHECK_LAUNCH();
    }
    {
        // unit-owned gradients: one lane per unit with 8-byte corner loads when the rows allow it, else the atomic kernel's
        // lane groups without its atomics
        const long long n_units = (long long)B * Q * M;
        const bool lane_units = Dh % 2 == 0 && ((uintptr_t)value & 7) == 0 && ((uintptr_t)grad_output & 7) == 0 &&
                                ((uintptr_t)sampling_loc & 7) == 0 && ((uintptr_t)grad_sampling_loc & 7) == 0 &&      // 8-byte location / gradient pairs (round 6)
                                (n_units + 255) / 256 < (1ll << 31);
#define FBBEV_MSDA_BWD_UL(DH_)                                                                                        \
    FBBEV_LAUNCH((k_msda_bwd_unit<DH_>), (n_units + 255) / 256, 256, 0, stream, n_units, value, spatial_shapes,         \
                 level_start_index, sampling_loc, attn_weight, grad_output, S, M, L, Q, P, grad_sampling_loc, grad_attn_weight)
#define FBBEV_MSDA_BWD_U(GW)                                                                                          \
    FBBEV_LAUNCH((k_msda_bwd<GW, false>), (n_units * GW + 255) / 256, 256, 0, stream, n_units, value, spatial_shapes, \
                 level_start_index, sampling_loc, attn_weight, grad_output, S, M, Dh, L, Q, P, grad_value,             \
                 grad_sampling_loc, grad_attn_weight)
        if (lane_units && Dh == 10) FBBEV_MSDA_BWD_UL(10);
        else if (lane_units && Dh == 8) FBBEV_MSDA_BWD_UL(8);
        else if (lane_units && Dh == 4) FBBEV_MSDA_BWD_UL(4);
        else if (lane_units && Dh == 16) FBBEV_MSDA_BWD_UL(16);
        else if (Dh <= 16) FBBEV_MSDA_BWD_U(16);
        else FBBEV_MSDA_BWD_U(32);
#undef FBBEV_MSDA_BWD_U
#undef FBBEV_MSDA_BWD_UL
        FBBEV_CHECK_LAUNCH();
    }
    const long long wgs = (long long)B * M * pl.n_bands;
#define FBBEV_MSDA_BWD_SC(DH_)                                                                                             \
    FBBEV_LAUNCH_DYN_LDS((k_msda_bwd_scatter<512, DH_>), wgs, 512, pl.lds, stream, spatial_shapes, level_start_index,      \
                         sampling_loc, attn_weight, grad_output, (const unsigned int*)ranges, (const int*)qrange, S, M, L, \
                         Q, P, pl.n_bands, pl.budget, grad_value)
    if (Dh == 10) FBBEV_MSDA_BWD_SC(10);
    else if (Dh == 8) FBBEV_MSDA_BWD_SC(8);
    else if (Dh == 4) FBBEV_MSDA_BWD_SC(4);
    else if (Dh == 16) FBBEV_MSDA_BWD_SC(16);
    else FBBEV_MSDA_BWD_SC(32);
#undef FBBEV_MSDA_BWD_SC
    FBBEV_CHECK_LAUNCH();
    return 0;
}

// ------------------------------------------------------------------------------ fused DA cross-attention
// The depth-aware (DA) cross-attention family.  Every entry fills ONE da_args from its positional C arguments and everything
// below it works on that record.  Entry -> internal route:
//   forward
//     fbbev_da_cross_attn_fwd             da_fwd_rows: k_da_cross_attn_fwd_unit (a lane owns a (b, q, head) unit), else k_da_cross_attn_fwd
//     fbbev_da_cross_attn_fwd_e           fp32 rows: da_fwd_rows; 16-bit rows: its own checks, the same unit kernel (da_fwd_unit_launch)
//     fbbev_da_cross_attn_fwd_zt          k_da_cross_attn_fwd_pipe where da_pipe_shape_ok holds, else da_fwd_rows
//     fbbev_da_cross_attn_fused[_e|_ln]   da_fused: k_da_cross_attn_fused (query rows -> slots; _ln: -> output_proj + LayerNorm rows)
//     fbbev_da_cross_attn_fwd_planes      k_da_fwd_planes (the training forward on head planes)
//   backward
//     fbbev_da_cross_attn_bwd             da_bwd_atomic: k_da_cross_attn_bwd (global atomics)
//     fbbev_da_cross_attn_bwd_ex          flag off: da_bwd_atomic; deterministic: k_da_cross_attn_bwd<GW, true> + fbbev_da_depth_taps_det
//     fbbev_da_cross_attn_bwd_ws[_grid]   da_bwd_ws: da_bwd_owned_launch (output-owned planes), else the chunked scatter
//                                         (da_bwd_unit_launch + k_da_cross_attn_bwd_scatter + k_da_bwd_reduce), else da_bwd_atomic
//     fbbev_da_cross_attn_bwd_ws_grid_ex  flag off: da_bwd_ws; deterministic: da_bwd_det around da_bwd_ws (never da_bwd_atomic: -2)
//     fbbev_da_cross_attn_bwd_planes      da_bwd_planes: da_bwd_owned_launch on the forward's head planes
//     fbbev_da_cross_attn_bwd_planes_ex   flag off: da_bwd_planes; deterministic: da_bwd_det around da_bwd_planes
//   probes and sizes (host only)
//     fbbev_da_cross_attn_fwd_zt_fuses_softmax / _fused_supported / _fwd_planes_supported    the shape checks of their routes
//     fbbev_da_cross_attn_bwd_ws_bytes[_za] / _bwd_planes_supported                          da_own_plan_make, da_bwd_tile_plan
//     fbbev_da_cross_attn_bwd_det_ws_bytes / fbbev_da_bwd_det_ws_bytes / fbbev_da_depth_taps_det_ws_bytes    the deterministic workspaces
struct da_args {
    int B, Ncam, S, M, Dh, L, Q, P, Za, DC;
    float d0, dstep;
    int head_minor, HS, bev_w;                              // HS: floats per head in a value row (head_stride; 0 = Dh); bev_w 0 = no grid
    fbbev_rt_stream stream;
    const float* value;                                     // camera tokens as rows (fwd_e: 16-bit rows behind the same pointer) ...
    const float* planes;                                    // ... or as head planes: an entry takes one of the two
    const int64_t* spatial_shapes; const int64_t* level_start_index;
    const float* pred_depth; const float* ref_cam; const uint8_t* mask; const float* qdepth;
    const float* offsets; const float* attn;                // null in the fused entries (projected inside the kernel)
    float* slots;                                           // the forward's output
    const float* grad_slots;                                // the backward's input and outputs
    float* grad_value; float* grad_pred_depth; float* grad_offsets; float* grad_attn;
};
// An entry's record: the braces list its operands in the order above -- what it does not have is nullptr / 0, and trailing members may
// be left out (the probes and planners stop after bev_w: no operands) -- with head_stride in HS's place, resolved here.
static inline da_args da_record(da_args a) { if (a.HS == 0) a.HS = a.Dh; return a; }

// The checks the entries share.  Their ORDER inside an entry is part of the ABI (it decides the code where two defects coincide),
// so every entry strings them together itself.
// every dimension positive, except: Q >= q_min (0 admits the empty call) and bev_w >= w_min (0 admits "no grid")
static inline bool da_dims_ok(const da_args& a, int q_min, int w_min) {
    return a.B > 0 && a.Ncam > 0 && a.S > 0 && a.M > 0 && a.Dh > 0 && a.L > 0 && a.Q >= q_min && a.P > 0 && a.Za > 0 && a.DC > 0 &&
           a.bev_w >= w_min;
}
static inline bool da_anchors_ok(const da_args& a) { return a.Za <= FBBEV_DA_MAX_ZA && a.P % a.Za == 0; }
static inline bool da_geometry_present(const da_args& a) {
    return a.spatial_shapes && a.level_start_index && a.pred_depth && a.ref_cam && a.mask && a.qdepth;
}
static inline bool da_fwd_present(const da_args& a) {
    return (a.value || a.planes) && da_geometry_present(a) && a.offsets && a.attn && a.slots;
}
static inline bool da_bwd_present(const da_args& a) {
    return (a.value || a.planes) && da_geometry_present(a) && a.offsets && a.attn && a.grad_slots && a.grad_value &&
           a.grad_pred_depth && a.grad_offsets && a.grad_attn;
}
// 8-byte accesses to the (x, y) offset pairs and to channel pairs of the slots, in whichever direction the record has them
static inline bool da_pairs_aligned(const da_args& a) {
    return (((uintptr_t)a.offsets | (uintptr_t)a.slots | (uintptr_t)a.grad_offsets | (uintptr_t)a.grad_slots) & 7) == 0;
}
// the head-dimension ladders (they differ on purpose: the set of instantiations is each kernel's own)
#define FBBEV_DA_DH_FWD(DH, X) do { if ((DH) == 10) X(10); else if ((DH) == 8) X(8); else if ((DH) == 16) X(16); else X(32); } while (0)
#define FBBEV_DA_DH_BWD(DH, X) do { if ((DH) == 10) X(10); else if ((DH) == 8) X(8); else if ((DH) == 4) X(4); else X(16); } while (0)

// k_da_cross_attn_fwd_unit: a lane owns all Dh channels of a (b, q, head) unit.  wide / qi: the row layout of fp32 tokens; et: 16-bit
// tokens (1 bf16, 2 fp16: always chunk-major pieces)
static int da_fwd_unit_launch(const da_args& a, bool wide, bool qi, int et) {
    const long long units = (long long)a.B * a.Q * a.M;
    long long ub = ((units + 255) / 256 + 7) / 8 * 8;             // XCD-contiguous order: a multiple of 8 workgroups
    if (ub > 65536) ub = 65536;
    // attention weights in (B,Q,M,L,P) staged through LDS ([256][L*P+1] floats) when 4 workgroups per CU still fit
    const int LP = a.L * a.P;
    const bool stage = !(a.head_minor & 2) && LP % 4 == 0 && LP <= 36 && aligned16(a.attn);
    const size_t lds = stage ? (size_t)256 * (LP + 1) * sizeof(float) : 0;
#define FBBEV_DA_UNIT_W(DH_, W_, Q_, ET_)                                                                                  \
    FBBEV_LAUNCH((k_da_cross_attn_fwd_unit<DH_, W_, Q_, ET_>), ub, 256, lds, a.stream, units, a.value, a.spatial_shapes,    \
                 a.level_start_index, a.pred_depth, a.ref_cam, a.mask, a.qdepth, a.offsets, a.attn, a.B, a.Ncam, a.S, a.M, \
                 a.L, a.Q, a.P, a.Za, a.DC, a.d0, a.dstep, a.head_minor & 3, a.HS, stage ? 1 : 0, a.slots)
#define FBBEV_DA_UNIT(DH_)                                                                                       \
    do {                                                                                                         \
        if (et == 1) FBBEV_DA_UNIT_W(DH_, true, true, 1); else if (et == 2) FBBEV_DA_UNIT_W(DH_, true, true, 2); \
        else if (qi) FBBEV_DA_UNIT_W(DH_, true, true, 0); else if (wide) FBBEV_DA_UNIT_W(DH_, true, false, 0);   \
        else FBBEV_DA_UNIT_W(DH_, false, false, 0);                                                              \
    } while (0)
    FBBEV_DA_DH_FWD(a.Dh, FBBEV_DA_UNIT);
#undef FBBEV_DA_UNIT_W
#undef FBBEV_DA_UNIT
    FBBEV_CHECK_LAUNCH();
    return 0;
}

// token rows -> slots: the unit-per-lane kernel where the rows allow it, else the lane-per-channel kernel
static int da_fwd_rows(const da_args& a) {
    if (!da_dims_ok(a, 0, 0)) return FBBEV_E_BADARG;
    if (!da_anchors_ok(a)) return FBBEV_E_UNSUPPORTED;
    if (a.dstep == 0.f) return FBBEV_E_BADARG;
    const long long n = (long long)a.B * a.Q * a.M * a.Dh;
    if (n == 0) return 0;
    if (!da_fwd_present(a)) return FBBEV_E_BADARG;
    if (a.HS < a.Dh) return FBBEV_E_BADARG;
    const bool wide = a.HS % 4 == 0 && a.HS >= (a.Dh + 3) / 4 * 4 && aligned16(a.value);
    const bool qi = (a.head_minor & 4) != 0;                       // value rows stored [chunk][head][4 floats]
    if (qi && !wide) return FBBEV_E_UNSUPPORTED;
    const bool al8 = ((uintptr_t)a.value & 7) == 0 && da_pairs_aligned(a);
    const bool fits32 = (long long)a.B * a.Ncam * a.S * a.M * a.HS * 4 < (1ll << 32);   // unit kernels: 32-bit byte offsets into value
    if (qi && !fits32) return FBBEV_E_UNSUPPORTED;
    if (al8 && fits32 && a.HS % 2 == 0 && (a.Dh == 10 || a.Dh == 8 || a.Dh == 16 || a.Dh == 32)) return da_fwd_unit_launch(a, wide, qi, 0);
    long long blocks = (n + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    FBBEV_LAUNCH(k_da_cross_attn_fwd, blocks, 256, 0, a.stream, n, a.value, a.spatial_shapes, a.level_start_index, a.pred_depth,
                 a.ref_cam, a.mask, a.qdepth, a.offsets, a.attn, a.B, a.Ncam, a.S, a.M, a.Dh, a.L, a.Q, a.P, a.Za, a.DC, a.d0,
                 a.dstep, a.head_minor & 7, a.HS, a.slots);
    FBBEV_CHECK_LAUNCH();
    return 0;
}
extern "C" int fbbev_da_cross_attn_fwd(const float* value, const int64_t* spatial_shapes,
                                       const int64_t* level_start_index, const float* pred_depth,
                                       const float* ref_cam, const uint8_t* mask, const float* qdepth,
                                       const float* offsets, const float* attn, int B, int Ncam, int S, int M,
                                       int Dh, int L, int Q, int P, int Za, int DC, float d0, float dstep,
                                       int head_minor, int head_stride, float* slots, fbbev_stream_t stream_) {
    return da_fwd_rows(da_record({B, Ncam, S, M, Dh, L, Q, P, Za, DC, d0, dstep, head_minor, head_stride, 0, (fbbev_rt_stream)stream_,
                                  value, nullptr, spatial_shapes, level_start_index, pred_depth, ref_cam, mask, qdepth, offsets, attn,
                                  slots}));
}

// 16-bit token rows (value_elem_type 1 = bf16, 2 = f16): chunk-major rows of 8-element pieces, unit-per-lane kernel only
extern "C" int fbbev_da_cross_attn_fwd_e(const void* value, const int64_t* spatial_shapes,
                                         const int64_t* level_start_index, const float* pred_depth,
                                         const float* ref_cam, const uint8_t* mask, const float* qdepth,
                                         const float* offsets, const float* attn, int B, int Ncam, int S, int M,
                                         int Dh, int L, int Q, int P, int Za, int DC, float d0, float dstep,
                                         int head_minor, int head_stride, int value_elem_type, float* slots,
                                         fbbev_stream_t stream_) {
    da_args a = da_record({B, Ncam, S, M, Dh, L, Q, P, Za, DC, d0, dstep, head_minor, head_stride, 0, (fbbev_rt_stream)stream_,
                           static_cast<const float*>(value), nullptr, spatial_shapes, level_start_index, pred_depth, ref_cam, mask,
                           qdepth, offsets, attn, slots});
    if (value_elem_type == 0) return da_fwd_rows(a);
    if (value_elem_type != 1 && value_elem_type != 2) return FBBEV_E_BADARG;
    if (!da_dims_ok(a, 0, 0)) return FBBEV_E_BADARG;
    if (!da_anchors_ok(a)) return FBBEV_E_UNSUPPORTED;
    if (dstep == 0.f) return FBBEV_E_BADARG;
    if ((long long)B * Q * M == 0) return 0;
    if (!da_fwd_present(a)) return FBBEV_E_BADARG;
    a.HS = head_stride;                                            // 16-bit rows state their stride: 0 does not mean Dh here
    // chunk-major rows of 8-element pieces covering Dh; 32-bit byte offsets; 8-byte aligned offsets / slots
    if (!(head_minor & 4) || a.HS % 8 != 0 || a.HS < (Dh + 7) / 8 * 8 || !aligned16(value) || !da_pairs_aligned(a) ||
        (long long)B * Ncam * S * M * a.HS * 2 >= (1ll << 32) || !(Dh == 10 || Dh == 8 || Dh == 16 || Dh == 32))
        return FBBEV_E_UNSUPPORTED;
    return da_fwd_unit_launch(a, true, true, value_elem_type);
}

static bool da_pipe_disabled() {
    static const bool off = fbbev_env_int("FBBEV_DA_PIPE", 1) == 0;   // A/B timing knob, read once
    return off;
}
static bool da_pipe_shape_ok(const da_args& a) {
    const long long tokens = (long long)a.B * a.Ncam * a.S;
    const int LP = a.L * a.P;
    return (long long)a.B * a.Q * a.M > 0 && (a.head_minor & 7) == (1 | 4) &&        // head-minor offsets, (B,Q,M,L,P) attn, chunk-major rows
           a.Za == 4 && a.P % 4 == 0 && (a.Dh == 8 || a.Dh == 10) && a.HS == (a.Dh + 3) / 4 * 4 && LP % 4 == 0 && LP <= 36 &&
           (tokens + 1) * a.M * a.HS * 4 < (1ll << 32);                              // 32-bit byte offsets incl. the zero token
}
extern "C" int fbbev_da_cross_attn_fwd_zt_fuses_softmax(int B, int Ncam, int S, int M, int Dh, int L, int Q, int P, int Za,
                                                        int head_minor, int head_stride) {
    const da_args a = da_record({B, Ncam, S, M, Dh, L, Q, P, Za, 1, 0.f, 0.f, head_minor, head_stride, 0});
    if (!da_dims_ok(a, 1, 0)) return 0;
    return (!da_pipe_disabled() && da_pipe_shape_ok(a)) ? 1 : 0;
}

// Pipelined forward (k_da_cross_attn_fwd_pipe): the value buffer holds ONE MORE token than B*Ncam*S -- token index
// B*Ncam*S, M*HS floats, all +0.0f -- which padded corners and out-of-image samples read instead of branching around their
// loads.  Shapes outside the pipelined kernel's preconditions run da_fwd_rows on the same buffer.
extern "C" int fbbev_da_cross_attn_fwd_zt(const float* value, const int64_t* spatial_shapes,
                                          const int64_t* level_start_index, const float* pred_depth,
                                          const float* ref_cam, const uint8_t* mask, const float* qdepth,
                                          const float* offsets, const float* attn, int B, int Ncam, int S, int M,
                                          int Dh, int L, int Q, int P, int Za, int DC, float d0, float dstep,
                                          int head_minor, int head_stride, int bev_w, float* slots,
                                          fbbev_stream_t stream_) {
    const da_args a = da_record({B, Ncam, S, M, Dh, L, Q, P, Za, DC, d0, dstep, head_minor, head_stride, bev_w, (fbbev_rt_stream)stream_,
                                 value, nullptr, spatial_shapes, level_start_index, pred_depth, ref_cam, mask, qdepth, offsets, attn,
                                 slots});
    if (!da_dims_ok(a, 0, 0)) return FBBEV_E_BADARG;
    const int LP = L * P;
    const long long units = (long long)B * Q * M;
    const long long tokens = (long long)B * Ncam * S;
    const bool pipe = value && offsets && attn && slots && dstep != 0.f && da_pipe_shape_ok(a) && aligned16(attn) &&
                      aligned16(value) && da_pairs_aligned(a);
    if (!pipe || da_pipe_disabled()) {
        if (head_minor & FBBEV_DA_ATTN_LOGITS) return FBBEV_E_UNSUPPORTED;     // only the pipelined kernel fuses the softmax
        return da_fwd_rows(a);
    }
    if (!da_geometry_present(a)) return FBBEV_E_BADARG;
    // patch mapping (a workgroup = the 8 heads of an 8 x 4 patch of the BEV grid): needs the grid's row length
    static const bool patch_off = fbbev_env_int("FBBEV_DA_PATCH", 1) == 0;   // A/B timing knob, read once
    const int pw = (!patch_off && bev_w > 0 && M == 8 && Q % bev_w == 0) ? bev_w : 0;
    const long long wgs = pw ? (long long)B * ((pw + 7) / 8) * ((Q / pw + 3) / 4) : (units + 255) / 256;
    long long ub = (wgs + 7) / 8 * 8;                             // XCD-contiguous order: a multiple of 8 workgroups
    if (ub > 65536) ub = 65536;
    const size_t lds = (size_t)256 * (LP + 1) * sizeof(float);
    const unsigned zero_bytes = (unsigned)(tokens * M * a.HS * 4);
#define FBBEV_DA_PIPE(DH_, WPS_)                                                                                     \
    FBBEV_LAUNCH((k_da_cross_attn_fwd_pipe<DH_, 4, WPS_>), ub, 256, lds, a.stream, units, value, spatial_shapes,         \
                 level_start_index, pred_depth, ref_cam, mask, qdepth, offsets, attn, B, Ncam, S, M, L, Q, P, DC, d0,   \
                 dstep, a.HS, zero_bytes, (head_minor & FBBEV_DA_ATTN_LOGITS) ? 1 : 0, pw, slots)
    static const int wps = fbbev_env_int("FBBEV_DA_PIPE_WPS", 2);   // tuning knob, read once (3: 168 registers, spills outside the loop)
    if (Dh == 10) { if (wps == 2) FBBEV_DA_PIPE(10, 2); else FBBEV_DA_PIPE(10, 3); }
    else { if (wps == 2) FBBEV_DA_PIPE(8, 2); else FBBEV_DA_PIPE(8, 3); }
#undef FBBEV_DA_PIPE
    FBBEV_CHECK_LAUNCH();
    return 0;
}

// ---- fbbev_da_cross_attn_fused: query rows -> slots in one kernel (da_fused_kernels.h)
static bool da_fused_shape_ok(const da_args& a) {
    if (a.M != 8 || (a.Dh != 10 && a.Dh != 8) || a.P != FBBEV_DAF_P || a.Za != FBBEV_DAF_ZA || a.L < 1 || a.bev_w <= 0 ||
        a.Q % a.bev_w != 0 || a.Ncam > 32) return false;
    if (a.L > FBBEV_DAF_MAXL || fbbev_daf_lds_bytes(a.M * a.Dh, 8, a.Ncam) > 160 * 1024) return false;
    return (long long)a.S * a.Dh * 4 < (1ll << 31) && a.S < (1 << 24);               // 32-bit byte offsets inside a head plane, 24-bit token indices
}
extern "C" int fbbev_da_cross_attn_fused_supported(int B, int Ncam, int S, int M, int Dh, int L, int Q, int P, int Za, int bev_w) {
    const da_args a = da_record({B, Ncam, S, M, Dh, L, Q, P, Za, 1, 0.f, 0.f, 0, 0, bev_w});
    if (!da_dims_ok(a, 1, 0)) return 0;
    static const bool off = fbbev_env_int("FBBEV_DA_FUSED", 1) == 0;   // A/B timing knob, read once
    return (!off && da_fused_shape_ok(a)) ? 1 : 0;
}
// a: the planes, the geometry and the output (offsets and weights are projected in the kernel from the query rows' operands here)
static int da_fused(const da_args& a, const float* query, long long query_row_stride, const float* addend,
                    long long addend_row_stride, long long addend_period, const void* offsets_fragments, const float* offsets_bias,
                    const void* attn_fragments, const float* attn_bias, int min_level_width, fbbev_daf_outproj op, int elem_type) {
    if (!da_dims_ok(a, 0, 0) || elem_type < 0 || elem_type > 2) return FBBEV_E_BADARG;
    if (elem_type != 0 && op.w_frag) return FBBEV_E_UNSUPPORTED;          // 16-bit planes: the plain sampler only
    if (a.Q == 0) return 0;
    if (!a.planes || !da_geometry_present(a) || !query || !offsets_fragments || !offsets_bias || !attn_fragments || !attn_bias ||
        !a.slots || a.dstep == 0.f) return FBBEV_E_BADARG;
    const int E = a.M * a.Dh;
    if (query_row_stride == 0) query_row_stride = E;
    if (query_row_stride < E) return FBBEV_E_BADARG;
    if (addend) {
        if (addend_period <= 0) return FBBEV_E_BADARG;
        if (addend_row_stride == 0) addend_row_stride = E;
        if (addend_row_stride < E) return FBBEV_E_BADARG;
    } else { addend_row_stride = 0; addend_period = 1; }
    // min_level_width: the caller's host-side knowledge of the narrowest level (the x-corner runs are clamped into a row of at
    // least two tokens); the shapes themselves stay on the device
    if (!da_fused_shape_ok(a) || min_level_width < 2) return FBBEV_E_UNSUPPORTED;
    if (query_row_stride % 4 != 0 || addend_row_stride % 4 != 0 || !aligned16(query) || (addend && !aligned16(addend)) ||
        !aligned16(offsets_fragments) || !aligned16(attn_fragments) || !aligned16(offsets_bias) || ((uintptr_t)a.planes & 7) != 0 ||
        !da_pairs_aligned(a))
        return FBBEV_E_UNSUPPORTED;
    // heads per workgroup: 4 = two 256-thread workgroups per patch and per CU (one's prologue + projections under the other's
    // samples), 8 = one 512-thread workgroup per patch (FBBEV_DA_FUSED_HW, read once)
    FBBEV_KNOB_ONCE(int, hw_env, fbbev_env_int("FBBEV_DA_FUSED_HW", 4) == 8 ? 8 : 4);   // (the emulator tests run both forms)
    const int hw = op.w_frag ? 8 : (elem_type ? 4 : hw_env); // the output_proj + LayerNorm tail needs all 8 heads of a query in one workgroup
    const long long wgs = (long long)a.B * ((a.bev_w + 7) / 8) * ((a.Q / a.bev_w + 7) / 8) * (8 / hw);
    const long long grid = (wgs + 7) / 8 * 8;
    if (grid >= (1ll << 31)) return FBBEV_E_UNSUPPORTED;
    // round 5: floats of a wave's LDS staging region for coarse levels (the 8 x 22 level of BASELINE configs[2] at Dh = 10: 1 760);
    // a level that fits is sampled from LDS instead of through the vector L1.  FBBEV_DA_FUSED_STAGE=0 turns it off (A/B knob)
    auto read_stage = [] { const int v = fbbev_env_int("FBBEV_DA_FUSED_STAGE", 1760); return v < 0 ? 0 : (v > 8192 ? 8192 : v); };
    FBBEV_KNOB_ONCE(int, stage_floats, read_stage());
    // (fbbev_da_cross_attn_fused_supported budgets LDS WITHOUT the staging region -- a launch whose staged layout does not
    // fit (8 heads per workgroup with ~25+ cameras) runs unstaged instead of failing after the probe said yes)
    int stage_eff = stage_floats;
    if (fbbev_daf_lds_bytes(E, hw, a.Ncam, stage_eff) > 160 * 1024) stage_eff = 0;
    const size_t lds = fbbev_daf_lds_bytes(E, hw, a.Ncam, stage_eff);
    if (lds > 160 * 1024) return FBBEV_E_UNSUPPORTED;
    static const bool pre_off = fbbev_env_int("FBBEV_DA_FUSED_PRE", 1) == 0;   // A/B knob, read once
    static const int diag = [] {                                                         // timing diagnostics (wrong results), read once
        const int v = fbbev_env_int("FBBEV_DA_FUSED_DIAG", 0) & 63;
        if (v) fprintf(stderr, "libfbbev_hip: FBBEV_DA_FUSED_DIAG=%d -- fbbev_da_cross_attn_fused runs its timing-diagnostic build: RESULTS ARE WRONG BY DESIGN\n", v);
        return v;
    }();
    const int stage_arg = stage_eff | (pre_off ? 0x40000000 : 0) | (diag << 24);
#define FBBEV_DA_FUSED(DH_, NP_, HW_) FBBEV_DA_FUSED3(DH_, NP_, HW_, false, 0)
#define FBBEV_DA_FUSED2(DH_, NP_, HW_, OP_) FBBEV_DA_FUSED3(DH_, NP_, HW_, OP_, 0)
#define FBBEV_DA_FUSED3(DH_, NP_, HW_, OP_, ET_) FBBEV_DA_FUSED4(DH_, NP_, HW_, OP_, ET_, false)
#define FBBEV_DA_FUSED4(DH_, NP_, HW_, OP_, ET_, DIAG_)                                                                                    \
    FBBEV_LAUNCH_DYN_LDS((k_da_cross_attn_fused<DH_, 8, NP_, HW_, OP_, ET_, DIAG_>), grid, 64 * HW_, lds, a.stream, a.planes,              \
                         a.spatial_shapes, a.level_start_index, a.pred_depth, a.ref_cam, a.mask, a.qdepth, query, query_row_stride,        \
                         addend, addend_row_stride, addend_period, static_cast<const unsigned short*>(offsets_fragments), offsets_bias,    \
                         static_cast<const unsigned short*>(attn_fragments), attn_bias, a.B, a.Ncam, a.S, a.L, a.Q, a.bev_w, a.DC, a.d0,   \
                         a.dstep, a.slots, op, stage_arg)
    // (three samples in flight per lane -- FBBEV_DA_FUSED_NP=3 in round 4 -- measured no gain and, with the staged levels' second
    // sample loop, no longer fits the register file: the instantiations are gone, two in flight is the form)
    // (round 5, 16-bit planes: three / four samples in flight per lane -- 234 registers / 256 with 5 spills -- measured 401.3 / 405.1 us
    // against 402.1 us with two at BASELINE configs[2]: the sampler is not waiting for its gathers; profiles/r05_exp_da_fused_where.md)
    if (elem_type == 1) {              // round 5: camera tokens stored as bf16 / fp16 head planes (fp32 products and sums)
        if (a.Dh == 10) FBBEV_DA_FUSED3(10, 2, 4, false, 1); else FBBEV_DA_FUSED3(8, 2, 4, false, 1);
    } else if (elem_type == 2) {
        if (a.Dh == 10) FBBEV_DA_FUSED3(10, 2, 4, false, 2); else FBBEV_DA_FUSED3(8, 2, 4, false, 2);
    } else if (op.w_frag) {
        if (a.Dh == 10) FBBEV_DA_FUSED2(10, 2, 8, true); else FBBEV_DA_FUSED2(8, 2, 8, true);
    } else if (hw == 8) {
        if (a.Dh == 10) FBBEV_DA_FUSED(10, 2, 8); else FBBEV_DA_FUSED(8, 2, 8);
    } else if (diag && a.Dh == 10) {   // FBBEV_DA_FUSED_DIAG: the instantiation with the timing-diagnostic bits (wrong results by design)
        FBBEV_DA_FUSED4(10, 2, 4, false, 0, true);
    } else {
        if (a.Dh == 10) FBBEV_DA_FUSED(10, 2, 4); else FBBEV_DA_FUSED(8, 2, 4);
    }
#undef FBBEV_DA_FUSED
#undef FBBEV_DA_FUSED2
#undef FBBEV_DA_FUSED3
#undef FBBEV_DA_FUSED4
    FBBEV_CHECK_LAUNCH();
    return 0;
}

extern "C" int fbbev_da_cross_attn_fused(const float* planes, const int64_t* spatial_shapes, const int64_t* level_start_index,
                                         const float* pred_depth, const float* ref_cam, const uint8_t* mask, const float* qdepth,
                                         const float* query, long long query_row_stride, const float* addend,
                                         long long addend_row_stride, long long addend_period, const void* offsets_fragments,
                                         const float* offsets_bias, const void* attn_fragments, const float* attn_bias, int B,
                                         int Ncam, int S, int M, int Dh, int L, int Q, int P, int Za, int DC, float d0, float dstep,
                                         int bev_w, int min_level_width, float* slots, fbbev_stream_t stream_) {
    const da_args a = da_record({B, Ncam, S, M, Dh, L, Q, P, Za, DC, d0, dstep, 0, 0, bev_w, (fbbev_rt_stream)stream_, nullptr, planes,
                                 spatial_shapes, level_start_index, pred_depth, ref_cam, mask, qdepth, nullptr, nullptr, slots});
    return da_fused(a, query, query_row_stride, addend, addend_row_stride, addend_period, offsets_fragments, offsets_bias,
                    attn_fragments, attn_bias, min_level_width, fbbev_daf_outproj{nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0.f}, 0);
}
// The same kernel on 16-bit head planes (elem_type 1 bf16, 2 fp16; 0 = the entry above): the camera-token STORAGE option of the
// cross-attention (fbbev_rows_linear_x3_planes_e writes them); every product and sum stays fp32.
extern "C" int fbbev_da_cross_attn_fused_e(const void* planes, int elem_type, const int64_t* spatial_shapes, const int64_t* level_start_index,
                                         const float* pred_depth, const float* ref_cam, const uint8_t* mask, const float* qdepth,
                                         const float* query, long long query_row_stride, const float* addend,
                                         long long addend_row_stride, long long addend_period, const void* offsets_fragments,
                                         const float* offsets_bias, const void* attn_fragments, const float* attn_bias, int B,
                                         int Ncam, int S, int M, int Dh, int L, int Q, int P, int Za, int DC, float d0, float dstep,
                                         int bev_w, int min_level_width, float* slots, fbbev_stream_t stream_) {
    const da_args a = da_record({B, Ncam, S, M, Dh, L, Q, P, Za, DC, d0, dstep, 0, 0, bev_w, (fbbev_rt_stream)stream_, nullptr,
                                 static_cast<const float*>(planes), spatial_shapes, level_start_index, pred_depth, ref_cam, mask, qdepth,
                                 nullptr, nullptr, slots});
    return da_fused(a, query, query_row_stride, addend, addend_row_stride, addend_period, offsets_fragments, offsets_bias,
                    attn_fragments, attn_bias, min_level_width, fbbev_daf_outproj{nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0.f},
                    elem_type);
}
// ... followed, inside the same workgroups (8 heads per workgroup), by output_proj + residual + LayerNorm: out rows instead of slots
extern "C" int fbbev_da_cross_attn_fused_ln(const float* planes, const int64_t* spatial_shapes, const int64_t* level_start_index,
                                            const float* pred_depth, const float* ref_cam, const uint8_t* mask, const float* qdepth,
                                            const float* query, long long query_row_stride, const float* addend,
                                            long long addend_row_stride, long long addend_period, const void* offsets_fragments,
                                            const float* offsets_bias, const void* attn_fragments, const float* attn_bias,
                                            const void* out_fragments, const float* out_bias, const float* residual,
                                            long long residual_row_stride, const float* ln_weight, const float* ln_bias, float ln_eps,
                                            int B, int Ncam, int S, int M, int Dh, int L, int Q, int P, int Za, int DC, float d0,
                                            float dstep, int bev_w, int min_level_width, float* out, fbbev_stream_t stream_) {
    // (the tail's own checks come before the shared ones)
    if (!out_fragments || !out_bias || !ln_weight || !ln_bias || !(ln_eps >= 0.f) || M <= 0 || Dh <= 0) return FBBEV_E_BADARG;
    const int E = M * Dh;
    if (residual && residual_row_stride == 0) residual_row_stride = E;
    if (residual && residual_row_stride < E) return FBBEV_E_BADARG;
    if (E % 16 != 0 || !aligned16(out_fragments) || !aligned16(out_bias) || !aligned16(ln_weight) || !aligned16(ln_bias) ||
        !aligned16(out) || (residual && (!aligned16(residual) || residual_row_stride % 4 != 0))) return FBBEV_E_UNSUPPORTED;
    const da_args a = da_record({B, Ncam, S, M, Dh, L, Q, P, Za, DC, d0, dstep, 0, 0, bev_w, (fbbev_rt_stream)stream_, nullptr, planes,
                                 spatial_shapes, level_start_index, pred_depth, ref_cam, mask, qdepth, nullptr, nullptr, out});
    return da_fused(a, query, query_row_stride, addend, addend_row_stride, addend_period, offsets_fragments, offsets_bias,
                    attn_fragments, attn_bias, min_level_width,
                    fbbev_daf_outproj{static_cast<const unsigned short*>(out_fragments), out_bias, residual, residual_row_stride,
                                      ln_weight, ln_bias, ln_eps}, 0);
}

// ---- Z-mean / Z-sum of a materialised (B*C, Z, Y*X) volume (training path; k_volume_zreduce)
extern "C" int fbbev_volume_zreduce(const float* volume, long long n_bc, int Z, long long YX, float divisor, float* out,
                                    fbbev_stream_t stream_) {
    if (n_bc < 0 || Z <= 0 || YX <= 0 || divisor == 0.f) return FBBEV_E_BADARG;
    if (n_bc == 0) return 0;
    if (!volume || !out) return FBBEV_E_BADARG;
    if (YX % 4 != 0 || !aligned16(volume) || !aligned16(out)) return FBBEV_E_UNSUPPORTED;
    const long long items = n_bc * (YX / 4);
    if ((items + 255) / 256 >= (1ll << 31)) return FBBEV_E_UNSUPPORTED;
    FBBEV_LAUNCH(k_volume_zreduce, (items + 255) / 256, 256, 0, (fbbev_rt_stream)stream_, volume, n_bc, Z, YX, divisor, out);
    FBBEV_CHECK_LAUNCH();
    return 0;
}

extern "C" int fbbev_volume_zreduce_inner(const float* volume, long long n_pillars, int Z, float divisor, float* out,
                                          fbbev_stream_t stream_) {
    if (n_pillars < 0 || Z <= 0 || divisor == 0.f) return FBBEV_E_BADARG;
    if (n_pillars == 0) return 0;
    if (!volume || !out) return FBBEV_E_BADARG;
    if (Z % 4 != 0 || !aligned16(volume) || (n_pillars + 255) / 256 >= (1ll << 31)) return FBBEV_E_UNSUPPORTED;
    FBBEV_LAUNCH(k_volume_zreduce_inner, (n_pillars + 255) / 256, 256, 0, (fbbev_rt_stream)stream_, volume, n_pillars, Z, divisor, out);
    FBBEV_CHECK_LAUNCH();
    return 0;
}
extern "C" int fbbev_volume_z_to_front(const float* src, long long n_bc, int Z, long long YX, float* dst, fbbev_stream_t stream_) {
    if (n_bc < 0 || Z <= 0 || YX <= 0) return FBBEV_E_BADARG;
    if (n_bc == 0) return 0;
    if (!src || !dst || src == dst) return FBBEV_E_BADARG;
    if (Z % 4 != 0 || !aligned16(src) || (n_bc * YX + 255) / 256 >= (1ll << 31)) return FBBEV_E_UNSUPPORTED;
    FBBEV_LAUNCH(k_volume_z_to_front, (n_bc * YX + 255) / 256, 256, 0, (fbbev_rt_stream)stream_, src, n_bc, Z, YX, dst);
    FBBEV_CHECK_LAUNCH();
    return 0;
}

// ---- training forward on head planes (da_bwd_planes_kernels.h): offsets / softmaxed weights from memory, tokens as planes
extern "C" int fbbev_value_rows_to_head_planes(const float* value, long long n_tokens, int S, int M, int Dh, int head_stride,
                                               int interleaved, float* planes, fbbev_stream_t stream_) {
    if (n_tokens < 0 || S <= 0 || M <= 0 || Dh <= 0 || n_tokens % S != 0) return FBBEV_E_BADARG;
    if (n_tokens == 0) return 0;
    const int HS = head_stride == 0 ? Dh : head_stride;
    if (!value || !planes || HS < Dh || (interleaved && HS % 4 != 0)) return FBBEV_E_BADARG;
    const long long n_el = n_tokens * M * Dh;
    if ((n_el + 255) / 256 >= (1ll << 31)) return FBBEV_E_UNSUPPORTED;
    FBBEV_LAUNCH(k_value_rows_to_head_planes, (n_el + 255) / 256, 256, 0, (fbbev_rt_stream)stream_, value, n_tokens, S, M, Dh, HS,
                 interleaved ? 1 : 0, planes);
    FBBEV_CHECK_LAUNCH();
    return 0;
}
static bool da_fwd_planes_shape_ok(const da_args& a) {
    static const bool off = fbbev_env_int("FBBEV_DA_FWD_PLANES", 1) == 0;   // A/B timing knob, read once
    return !off && a.M == 8 && (a.Dh == 10 || a.Dh == 8) && a.P == FBBEV_DAF_P && a.Za == FBBEV_DAF_ZA &&
           (long long)a.S * a.Dh * 4 < (1ll << 31) && fbbev_dfp_lds_bytes(a.Ncam) <= 156 * 1024;
}
extern "C" int fbbev_da_cross_attn_fwd_planes_supported(int B, int Ncam, int S, int M, int Dh, int L, int Q, int P, int Za) {
    const da_args a = da_record({B, Ncam, S, M, Dh, L, Q, P, Za, 1});
    return (da_dims_ok(a, 1, 0) && da_fwd_planes_shape_ok(a)) ? 1 : 0;
}
extern "C" int fbbev_da_cross_attn_fwd_planes(const float* planes, const int64_t* spatial_shapes, const int64_t* level_start_index,
                                              const float* pred_depth, const float* ref_cam, const uint8_t* mask, const float* qdepth,
                                              const float* offsets, const float* attn, int B, int Ncam, int S, int M, int Dh, int L,
                                              int Q, int P, int Za, int DC, float d0, float dstep, int head_minor, int bev_w,
                                              int min_level_width, float* slots, fbbev_stream_t stream_) {
    const da_args a = da_record({B, Ncam, S, M, Dh, L, Q, P, Za, DC, d0, dstep, head_minor, 0, bev_w, (fbbev_rt_stream)stream_, nullptr,
                                 planes, spatial_shapes, level_start_index, pred_depth, ref_cam, mask, qdepth, offsets, attn, slots});
    if (!da_dims_ok(a, 0, 0)) return FBBEV_E_BADARG;
    if (Q == 0) return 0;                                          // (before dstep is looked at)
    if (!da_fwd_present(a) || dstep == 0.f) return FBBEV_E_BADARG;
    if (!da_fwd_planes_shape_ok(a) || min_level_width < 2 || ((uintptr_t)planes & 7) != 0 || !da_pairs_aligned(a) ||
        !aligned16(ref_cam) || !aligned16(qdepth) || ((uintptr_t)mask & 3) != 0) return FBBEV_E_UNSUPPORTED;
    const int gw = (bev_w > 0 && Q % bev_w == 0) ? bev_w : 0;
    const long long wgs = gw > 0 ? (long long)B * ((gw + 7) / 8) * ((Q / gw + 7) / 8) : (long long)B * ((Q + 63) / 64);
    const long long grid = (wgs + 7) / 8 * 8;
    if (grid >= (1ll << 31)) return FBBEV_E_UNSUPPORTED;
    const size_t lds = fbbev_dfp_lds_bytes(Ncam);
#define FBBEV_DA_FWD_PLANES(DH_)                                                                                            \
    FBBEV_LAUNCH_DYN_LDS((k_da_fwd_planes<DH_, 8>), grid, 512, lds, a.stream, planes, spatial_shapes,                       \
                         level_start_index, pred_depth, ref_cam, mask, qdepth, offsets, attn, B, Ncam, S, L, Q, gw, DC, d0, \
                         dstep, head_minor & 3, slots)
    if (Dh == 10) FBBEV_DA_FWD_PLANES(10); else FBBEV_DA_FWD_PLANES(8);
#undef FBBEV_DA_FWD_PLANES
    FBBEV_CHECK_LAUNCH();
    return 0;
}

// ---- fbbev_msda_self_fused: BEV self-attention, query rows -> attention output in one kernel (da_fused_kernels.h)
extern "C" int fbbev_msda_self_fused_supported(int B, int S, int M, int Dh, int L, int Q, int P, int bev_w) {
    if (B <= 0 || S <= 0 || M <= 0 || Dh <= 0 || L <= 0 || Q <= 0 || P <= 0) return 0;
    static const bool off = fbbev_env_int("FBBEV_MSDA_FUSED", 1) == 0;   // A/B timing knob, read once
    return (!off && M == 8 && (Dh == 10 || Dh == 8) && L == 1 && P == FBBEV_MSF_P && bev_w > 0 && Q % bev_w == 0 &&
            (long long)S * Dh * 4 < (1ll << 31)) ? 1 : 0;
}
static int msda_self_fused_impl(const float* planes, const float* reference_points, const float* query,
                                long long query_row_stride, const float* addend, long long addend_row_stride,
                                long long addend_period, const void* offsets_fragments, const float* offsets_bias,
                                const void* attn_fragments, const float* attn_bias, int B, int S, int M, int Dh, int L, int Q,
                                int P, int bev_w, int level_h, int level_w, float* out, fbbev_stream_t stream_,
                                fbbev_daf_outproj op) {
    if (B <= 0 || S <= 0 || M <= 0 || Dh <= 0 || L <= 0 || Q < 0 || P <= 0 || bev_w < 0 || level_h <= 0 || level_w <= 0)
        return FBBEV_E_BADARG;
    if (Q == 0) return 0;
    if (!planes || !reference_points || !query || !offsets_fragments || !offsets_bias || !attn_fragments || !attn_bias || !out)
        return FBBEV_E_BADARG;
    if ((long long)level_h * level_w != S) return FBBEV_E_BADARG;
    const int E = M * Dh;
    if (query_row_stride == 0) query_row_stride = E;
    if (query_row_stride < E) return FBBEV_E_BADARG;
    if (addend) {
        if (addend_period <= 0) return FBBEV_E_BADARG;
        if (addend_row_stride == 0) addend_row_stride = E;
        if (addend_row_stride < E) return FBBEV_E_BADARG;
    } else { addend_row_stride = 0; addend_period = 1; }
    if (!(M == 8 && (Dh == 10 || Dh == 8) && L == 1 && P == FBBEV_MSF_P && bev_w > 0 && Q % bev_w == 0) || level_w < 2 ||
        (long long)S * Dh * 4 >= (1ll << 31)) return FBBEV_E_UNSUPPORTED;
    if (query_row_stride % 4 != 0 || addend_row_stride % 4 != 0 || !aligned16(query) || (addend && !aligned16(addend)) ||
        !aligned16(offsets_fragments) || !aligned16(attn_fragments) || ((uintptr_t)planes & 7) != 0 || ((uintptr_t)out & 7) != 0 ||
        ((uintptr_t)reference_points & 7) != 0) return FBBEV_E_UNSUPPORTED;
    const long long wgs = (long long)B * ((bev_w + 7) / 8) * ((Q / bev_w + 7) / 8);
    const long long grid = (wgs + 7) / 8 * 8;
    if (grid >= (1ll << 31)) return FBBEV_E_UNSUPPORTED;
    const size_t lds = fbbev_msf_lds_bytes(E, M);
#define FBBEV_MSDA_SELF(DH_) do { if (op.w_frag) FBBEV_MSDA_SELF2(DH_, true); else FBBEV_MSDA_SELF2(DH_, false); } while (0)
#define FBBEV_MSDA_SELF2(DH_, OP_)                                                                                             \
    FBBEV_LAUNCH_DYN_LDS((k_msda_self_fused<DH_, 8, OP_>), grid, 512, lds, (fbbev_rt_stream)stream_, planes, reference_points, \
                         query, query_row_stride, addend, addend_row_stride, addend_period,                                    \
                         static_cast<const unsigned short*>(offsets_fragments), offsets_bias,                                  \
                         static_cast<const unsigned short*>(attn_fragments), attn_bias, B, Q, bev_w, S, level_h, level_w, out, op)
    if (Dh == 10) FBBEV_MSDA_SELF(10); else FBBEV_MSDA_SELF(8);
#undef FBBEV_MSDA_SELF
#undef FBBEV_MSDA_SELF2
    FBBEV_CHECK_LAUNCH();
    return 0;
}
extern "C" int fbbev_msda_self_fused(const float* planes, const float* reference_points, const float* query,
                                     long long query_row_stride, const float* addend, long long addend_row_stride,
                                     long long addend_period, const void* offsets_fragments, const float* offsets_bias,
                                     const void* attn_fragments, const float* attn_bias, int B, int S, int M, int Dh, int L, int Q,
                                     int P, int bev_w, int level_h, int level_w, float* out, fbbev_stream_t stream_) {
    return msda_self_fused_impl(planes, reference_points, query, query_row_stride, addend, addend_row_stride, addend_period,
                                offsets_fragments, offsets_bias, attn_fragments, attn_bias, B, S, M, Dh, L, Q, P, bev_w, level_h,
                                level_w, out, stream_, fbbev_daf_outproj{nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0.f});
}
// ... followed, inside the same workgroups, by output_proj + residual + LayerNorm: out = LN(W_o attention + b_o + residual)
extern "C" int fbbev_msda_self_fused_ln(const float* planes, const float* reference_points, const float* query,
                                        long long query_row_stride, const float* addend, long long addend_row_stride,
                                        long long addend_period, const void* offsets_fragments, const float* offsets_bias,
                                        const void* attn_fragments, const float* attn_bias, const void* out_fragments,
                                        const float* out_bias, const float* residual, long long residual_row_stride,
                                        const float* ln_weight, const float* ln_bias, float ln_eps, int B, int S, int M, int Dh,
                                        int L, int Q, int P, int bev_w, int level_h, int level_w, float* out,
                                        fbbev_stream_t stream_) {
    if (!out_fragments || !out_bias || !ln_weight || !ln_bias || !(ln_eps >= 0.f) || M <= 0 || Dh <= 0) return FBBEV_E_BADARG;
    const int E = M * Dh;
    if (residual && residual_row_stride == 0) residual_row_stride = E;
    if (residual && residual_row_stride < E) return FBBEV_E_BADARG;
    if (E % 16 != 0 || !aligned16(out_fragments) || !aligned16(out_bias) || !aligned16(ln_weight) || !aligned16(ln_bias) ||
        !aligned16(out) || (residual && (!aligned16(residual) || residual_row_stride % 4 != 0))) return FBBEV_E_UNSUPPORTED;
    return msda_self_fused_impl(planes, reference_points, query, query_row_stride, addend, addend_row_stride, addend_period,
                                offsets_fragments, offsets_bias, attn_fragments, attn_bias, B, S, M, Dh, L, Q, P, bev_w, level_h,
                                level_w, out, stream_,
                                fbbev_daf_outproj{static_cast<const unsigned short*>(out_fragments), out_bias, residual,
                                                  residual_row_stride, ln_weight, ln_bias, ln_eps});
}

extern "C" int fbbev_rows_to_head_planes(const float* rows, long long n_rows, int tokens_per_image, int M, int Dh, float* planes,
                                         fbbev_stream_t stream_) {
    if (n_rows < 0 || tokens_per_image <= 0 || M <= 0 || Dh <= 0) return FBBEV_E_BADARG;
    if (n_rows == 0) return 0;
    if (!rows || !planes || n_rows % tokens_per_image != 0) return FBBEV_E_BADARG;
    const long long n = n_rows * M * Dh;
    if ((n + 255) / 256 >= (1ll << 31)) return FBBEV_E_UNSUPPORTED;
    FBBEV_LAUNCH(k_rows_to_head_planes, (n + 255) / 256, 256, 0, (fbbev_rt_stream)stream_, rows, n_rows, tokens_per_image, M, Dh, planes);
    FBBEV_CHECK_LAUNCH();
    return 0;
}

// global atomics: the route every shape can take
static int da_bwd_atomic(const da_args& a) {
    if (!da_dims_ok(a, 0, 0)) return FBBEV_E_BADARG;
    if (!da_anchors_ok(a)) return FBBEV_E_UNSUPPORTED;
    if (a.dstep == 0.f) return FBBEV_E_BADARG;
    const long long units = (long long)a.B * a.Q * a.M;
    if (units == 0) return 0;
    if (!da_bwd_present(a)) return FBBEV_E_BADARG;
    if (a.Dh > 32) return FBBEV_E_UNSUPPORTED;
    if (a.HS < a.Dh) return FBBEV_E_BADARG;
    if ((a.head_minor & 4) && a.HS % 4 != 0) return FBBEV_E_UNSUPPORTED;
    if ((units * 32 + 255) / 256 >= (1ll << 31)) return FBBEV_E_UNSUPPORTED;
#define FBBEV_DA_BWD(GW_)                                                                                                \
    FBBEV_LAUNCH(k_da_cross_attn_bwd<GW_>, (units * GW_ + 255) / 256, 256, 0, a.stream, units, a.value, a.spatial_shapes, \
                 a.level_start_index, a.pred_depth, a.ref_cam, a.mask, a.qdepth, a.offsets, a.attn, a.grad_slots, a.B,   \
                 a.Ncam, a.S, a.M, a.Dh, a.L, a.Q, a.P, a.Za, a.DC, a.d0, a.dstep, a.head_minor & 7, a.HS, a.grad_value, \
                 a.grad_pred_depth, a.grad_offsets, a.grad_attn)
    if (a.Dh <= 16) FBBEV_DA_BWD(16);
    else FBBEV_DA_BWD(32);
#undef FBBEV_DA_BWD
    FBBEV_CHECK_LAUNCH();
    return 0;
}
extern "C" int fbbev_da_cross_attn_bwd(const float* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                                       const float* pred_depth, const float* ref_cam, const uint8_t* mask,
                                       const float* qdepth, const float* offsets, const float* attn,
                                       const float* grad_slots, int B, int Ncam, int S, int M, int Dh, int L, int Q,
                                       int P, int Za, int DC, float d0, float dstep, int head_minor, int head_stride,
                                       float* grad_value, float* grad_pred_depth, float* grad_offsets,
                                       float* grad_attn, fbbev_stream_t stream_) {
    return da_bwd_atomic(da_record({B, Ncam, S, M, Dh, L, Q, P, Za, DC, d0, dstep, head_minor, head_stride, 0, (fbbev_rt_stream)stream_,
                                    value, nullptr, spatial_shapes, level_start_index, pred_depth, ref_cam, mask, qdepth, offsets, attn,
                                    nullptr, grad_slots, grad_value, grad_pred_depth, grad_offsets, grad_attn}));
}

// ---- deterministic form of the global-atomic kernel (k_da_cross_attn_bwd<GW, true>): det_ws = [fixed-point value words]
// [per-head depth sums (Ncam, B, Q, M, Za)] [head-summed (Ncam, B, Q, Za)] [taps workspace]
static size_t da_taps_ws_bytes(int B, int Ncam, int DC, int H0, int W0);
static size_t da_glob_det_fix_bytes(int B, int Ncam, int S, int M, int HS) {
    return align_up(FBBEV_FIX_HDR + (size_t)B * Ncam * S * M * HS * sizeof(unsigned long long), 256);
}
extern "C" size_t fbbev_da_cross_attn_bwd_det_ws_bytes(int B, int Ncam, int S, int M, int HS, int Q, int Za, int DC, int H0, int W0) {
    if (B <= 0 || Ncam <= 0 || S <= 0 || M <= 0 || HS <= 0 || Q < 0 || Za <= 0 || DC <= 0 || H0 <= 0 || W0 <= 0) return 0;
    const size_t cbq = (size_t)Ncam * B * Q;
    return da_glob_det_fix_bytes(B, Ncam, S, M, HS) + align_up(cbq * M * Za * 4, 256) + align_up(cbq * Za * 4, 256) +
           da_taps_ws_bytes(B, Ncam, DC, H0, W0);
}
// fbbev_da_cross_attn_bwd with a flags word.  FBBEV_FLAG_DETERMINISTIC: the value gradient as 64-bit fixed point (scale from
// max |grad_slots| x max |attn| x max |pred_depth|, at most Q * P adds per word), the depth taps through fbbev_da_depth_taps_det;
// grad_value / grad_pred_depth accumulated into as by the plain entry.  H0, W0: level 0's shape on the host.
extern "C" int fbbev_da_cross_attn_bwd_ex(const float* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                                          const float* pred_depth, const float* ref_cam, const uint8_t* mask,
                                          const float* qdepth, const float* offsets, const float* attn,
                                          const float* grad_slots, int B, int Ncam, int S, int M, int Dh, int L, int Q,
                                          int P, int Za, int DC, float d0, float dstep, int head_minor, int head_stride,
                                          float* grad_value, float* grad_pred_depth, float* grad_offsets,
                                          float* grad_attn, int H0, int W0, int flags, void* det_ws, size_t det_ws_bytes,
                                          fbbev_stream_t stream_) {
    const da_args a = da_record({B, Ncam, S, M, Dh, L, Q, P, Za, DC, d0, dstep, head_minor, head_stride, 0, (fbbev_rt_stream)stream_,
                                 value, nullptr, spatial_shapes, level_start_index, pred_depth, ref_cam, mask, qdepth, offsets, attn,
                                 nullptr, grad_slots, grad_value, grad_pred_depth, grad_offsets, grad_attn});
    if (!(flags & FBBEV_FLAG_DETERMINISTIC)) return da_bwd_atomic(a);
    if (!da_dims_ok(a, 0, 0) || H0 <= 0 || W0 <= 0) return FBBEV_E_BADARG;
    if (!da_anchors_ok(a)) return FBBEV_E_UNSUPPORTED;
    if (dstep == 0.f) return FBBEV_E_BADARG;
    const long long units = (long long)B * Q * M;
    if (units == 0) return 0;
    if (!da_bwd_present(a) || !det_ws) return FBBEV_E_BADARG;
    if (Dh > 32) return FBBEV_E_UNSUPPORTED;
    const int HS = a.HS;
    if (HS < Dh) return FBBEV_E_BADARG;
    if ((head_minor & 4) && HS % 4 != 0) return FBBEV_E_UNSUPPORTED;
    if ((units * 32 + 255) / 256 >= (1ll << 31)) return FBBEV_E_UNSUPPORTED;
    if (det_ws_bytes < fbbev_da_cross_attn_bwd_det_ws_bytes(B, Ncam, S, M, HS, Q, Za, DC, H0, W0) || !aligned16(det_ws))
        return FBBEV_E_WORKSPACE;
    fbbev_rt_stream stream = a.stream;
    char* w = static_cast<char*>(det_ws);
    const size_t fix_b = da_glob_det_fix_bytes(B, Ncam, S, M, HS);
    const long long cbq = (long long)Ncam * B * Q;
    float* per_head = reinterpret_cast<float*>(w + fix_b);
    float* dsum = reinterpret_cast<float*>(w + fix_b + align_up((size_t)cbq * M * Za * 4, 256));
    char* taps = reinterpret_cast<char*>(dsum) + align_up((size_t)cbq * Za * 4, 256);
    int e = fbbev_rt_memset_async(w, 0, fix_b + align_up((size_t)cbq * M * Za * 4, 256), stream);
    if (e) return e;
    unsigned int* hdr = reinterpret_cast<unsigned int*>(w);
    auto grid = [](long long n) { long long g = (n + 255) / 256; return g > 1024 ? 1024 : (g < 1 ? 1 : g); };
    const long long n_g = units * Dh, n_a = units * L * P, n_d = (long long)B * Ncam * DC * H0 * W0;
    FBBEV_LAUNCH(k_da_taps_absmax, grid(n_g), 256, 0, stream, grad_slots, n_g, hdr);
    FBBEV_LAUNCH(k_da_taps_absmax, grid(n_a), 256, 0, stream, attn, n_a, hdr + 1);
    FBBEV_LAUNCH(k_da_taps_absmax, grid(n_d), 256, 0, stream, pred_depth, n_d, hdr + 2);
    int kq = 0;
    while ((1ll << kq) < (long long)Q * P) ++kq;
    FBBEV_LAUNCH(k_fix_scale, 1, 64, 0, stream, 3, kq, hdr);
    FBBEV_CHECK_LAUNCH();
    float* fix_ws = reinterpret_cast<float*>(w);
#define FBBEV_DA_BWD_FIX(GW_)                                                                                           \
    FBBEV_LAUNCH((k_da_cross_attn_bwd<GW_, true>), (units * GW_ + 255) / 256, 256, 0, stream, units, value,             \
                 spatial_shapes, level_start_index, pred_depth, ref_cam, mask, qdepth, offsets, attn, grad_slots, B,    \
                 Ncam, S, M, Dh, L, Q, P, Za, DC, d0, dstep, head_minor & 7, HS, fix_ws, per_head, grad_offsets, grad_attn)
    if (Dh <= 16) FBBEV_DA_BWD_FIX(16);
    else FBBEV_DA_BWD_FIX(32);
#undef FBBEV_DA_BWD_FIX
    FBBEV_CHECK_LAUNCH();
    const long long n_v = (long long)B * Ncam * S * M * HS;
    FBBEV_LAUNCH(k_fix_to_f32_add, grid(n_v) * 4, 256, 0, stream, (const unsigned int*)hdr, n_v, grad_value);
    FBBEV_LAUNCH(k_da_head_sum, grid(cbq * Za) * 4, 256, 0, stream, (const float*)per_head, cbq, M, Za, dsum);
    FBBEV_CHECK_LAUNCH();
    return fbbev_da_depth_taps_det(dsum, ref_cam, qdepth, B, Ncam, Q, Za, DC, H0, W0, d0, dstep, grad_pred_depth, taps,
                                   da_taps_ws_bytes(B, Ncam, DC, H0, W0), stream_);
}

// LDS-plane backward (needs a caller-owned partial buffer): k_da_cross_attn_bwd_unit (unit-owned gradients) +
// k_da_cross_attn_bwd_scatter per token region + k_da_bwd_reduce
struct da_region { int lvl0, lvl1, tok0, tok1; };
struct da_bwd_plan { int chunks, q_per_chunk, threads, n_regions, info_stride; size_t lds, ws, ws_part; da_region reg[32]; };

// token regions of at most `budget` tokens: whole consecutive levels, or bands of rows of a level larger than the budget
// (level_hw: HOST array of L (h, w) pairs; without it only the one-region case -- the whole pyramid fits -- is planned)
static int da_bwd_regions(int L, const int32_t* level_hw, int S, int budget, da_region* out, int cap) {
    if (!level_hw) {
        if (S > budget) return 0;
        out[0] = {0, L, 0, S};
        return 1;
    }
    int n = 0, start = 0;
    da_region cur = {0, 0, 0, 0};
    for (int l = 0; l < L; ++l) {
        const int h = level_hw[2 * l], w = level_hw[2 * l + 1];
        if (h <= 0 || w <= 0) return 0;
        const int cnt = h * w;
        if (cnt > budget) {
            if (cur.lvl1 > cur.lvl0) { if (n == cap) return 0; out[n++] = cur; }
            const int rows = budget / w;
            if (rows < 1) return 0;
            for (int r = 0; r < h; r += rows) {
                if (n == cap) return 0;
                out[n++] = {l, l + 1, start + r * w, start + (r + rows < h ? r + rows : h) * w};
            }
            cur = {l + 1, l + 1, start + cnt, start + cnt};
        } else if (cur.lvl1 > cur.lvl0 && (cur.tok1 - cur.tok0) + cnt > budget) {
            if (n == cap) return 0;
            out[n++] = cur;
            cur = {l, l + 1, start, start + cnt};
        } else {
            if (cur.lvl1 == cur.lvl0) cur = {l, l + 1, start, start + cnt};
            else { cur.lvl1 = l + 1; cur.tok1 = start + cnt; }
        }
        start += cnt;
    }
    if (cur.lvl1 > cur.lvl0) { if (n == cap) return 0; out[n++] = cur; }
    return start == S ? n : 0;
}

// Tuning / test overrides of the plan, read ONCE per process (function-local static: thread-safe) -- the Python forward
// derives the value-row layout from this planner and the backward launches from it, so a variable that changed between
// the two calls must not be able to make them disagree.  Unset = the measured defaults.
struct da_bwd_overrides { int tokens, chunks, threads, copies, lds_kb, prepass; };
static da_bwd_overrides da_bwd_read_env() {
    return da_bwd_overrides{fbbev_env_int("FBBEV_DA_BWD_TOKENS", 0), fbbev_env_int("FBBEV_DA_BWD_CHUNKS", 0),
                            fbbev_env_int("FBBEV_DA_BWD_THREADS", 0), fbbev_env_int("FBBEV_DA_BWD_COPIES", 0),
                            fbbev_env_int("FBBEV_DA_BWD_LDS_KB", 0), fbbev_env_int("FBBEV_DA_BWD_PREPASS", -1)};
}
// (the CPU emulator build re-reads them on every call: its tests switch plans inside one process)
static da_bwd_overrides da_bwd_env() { FBBEV_KNOB_ONCE(da_bwd_overrides, o, da_bwd_read_env()); return o; }

// LDS bytes of the fixed-point planes of one workgroup: 68 KB = two workgroups per CU (FBBEV_DA_BWD_LDS_KB tunes it)
static int da_bwd_plane_kb() { const int v = da_bwd_env().lds_kb; return v >= 8 && v <= 144 ? v : 68; }

static bool da_bwd_tile_plan(const da_args& a, const int32_t* level_hw, da_bwd_plan* pl) {
    if (a.Dh > 16 || a.HS % 4 != 0 || a.HS > 16 || a.Q <= 0) return false;
    if (a.P > FBBEV_DA_BWD_MAXP || !(a.Dh == 10 || a.Dh == 8 || a.Dh == 16 || a.Dh == 4)) return false;
    int budget = (da_bwd_plane_kb() * 1024) / (a.HS * (int)sizeof(long long)) - 8;   // tokens per LDS plane (64-bit words, skewed)
    { const int v = da_bwd_env().tokens; if (v > 0 && v < budget) budget = v; }   // tests: force bands
    pl->n_regions = da_bwd_regions(a.L, level_hw, a.S, budget, pl->reg, 32);
    if (pl->n_regions == 0) return false;
    int max_tok = 0;
    for (int r = 0; r < pl->n_regions; ++r) max_tok = pl->reg[r].tok1 - pl->reg[r].tok0 > max_tok ? pl->reg[r].tok1 - pl->reg[r].tok0 : max_tok;
    const size_t plane = (size_t)FBBEV_DA_PLANE_WORDS(max_tok, a.HS) * sizeof(long long);
    // two workgroups per CU in one round (512 of them)
    long long want = (512 + (long long)a.B * a.M - 1) / ((long long)a.B * a.M);
    { const int v = da_bwd_env().chunks; if (v > 0) want = v; }
    if (want < 1) want = 1;
    if (want > 256) want = 256;
    int qpc = (int)((a.Q + want - 1) / want);
    // one lane per query the camera sees: 512 threads (measured 0.177 vs 0.208 ms at the shipped shape) unless the chunk is short
    pl->threads = qpc >= 512 ? 512 : 256;
    { const int v = da_bwd_env().threads; if (v == 256 || v == 512) pl->threads = v; }
    const int ng = pl->threads;                                                   // queries per workgroup iteration
    qpc = (qpc + ng - 1) / ng * ng;
    if (qpc > 65535) return false;                                                // chunk-relative 16-bit query ids
    pl->q_per_chunk = qpc;
    pl->chunks = (a.Q + qpc - 1) / qpc;
    // + the camera's hit list, its counter, the block maximum
    pl->lds = plane + (size_t)((qpc + 1) & ~1) * 2 + (size_t)(1 + pl->threads / 64) * sizeof(int);
    if (pl->lds > (size_t)(da_bwd_plane_kb() + 12) * 1024) return false;
    pl->ws_part = ((size_t)a.B * a.M * pl->chunks * a.Ncam * a.S * a.HS * sizeof(float) + 255) / 256 * 256;
    // pre-pass (k_da_bwd_hitinfo; FBBEV_DA_BWD_PREPASS=0 turns it off): per (b, camera, query) the camera count and the Za depth
    // weights, behind the partials -- worth it when several region launches would each recompute them (configs[2] pyramid:
    // scatter 2.43 -> 2.22 ms, profiles/r03_exp_da_bwd_prepass.jsonl)
    pl->info_stride = 0;
    pl->ws = pl->ws_part;
    if (da_bwd_env().prepass != 0 && pl->n_regions > 1) {
        pl->info_stride = 8;                                        // 1 + Za <= 8 floats (Za is checked at the launch)
        pl->ws += (size_t)a.B * a.Ncam * a.Q * pl->info_stride * sizeof(float);
    }
    return true;
}

// ---- output-owned planes (k_da_bwd_scatter_owned; FBBEV_DA_BWD_OWNED=0 restores the chunked scatter above)
struct da_own_plan { fbbev_da_bwd_region_tab tab; int threads, info_stride, unit_planes; size_t lds, off_list, off_count, off_gmax, off_planes, ws; };
// FBBEV_DA_BWD_OWNED: 1 = whenever the shape is supported, 0 = never, unset = when the launch has at least one workgroup per CU
// (the shipped single-level shape at B = 4 has 192 (sample, camera, head) planes: the chunked scatter's 512 workgroups win there)
static int da_bwd_owned_mode() {
    auto read = [] { const char* e = fbbev_env_str("FBBEV_DA_BWD_OWNED"); return e ? (atoi(e) != 0 ? 1 : 0) : -1; };   // unset is a third state
    FBBEV_KNOB_ONCE(int, mode, read());
    return mode;
}
// LDS bytes of an owned plane: 136 KB = one 512-thread workgroup per CU; fewer, larger regions beat two workgroups per CU
// (configs[2] pyramid: 1.06 ms at 136 KB / 512 threads, 1.38 ms at 68 KB / 256, 2.18 ms at 68 KB / 512, 3.47 ms at 34 KB)
static int da_own_plane_kb() { const int v = da_bwd_env().lds_kb; return v >= 8 && v <= 144 ? v : 136; }
static bool da_own_plan_make(const da_args& a, const int32_t* level_hw, da_own_plan* pl) {
    const int mode = da_bwd_owned_mode();
    if (mode == 0) return false;
    if (a.Dh > 16 || a.HS % 4 != 0 || a.HS > 16 || a.Q <= 0 || a.P > FBBEV_DA_BWD_MAXP || !(a.Dh == 10 || a.Dh == 8 || a.Dh == 16 || a.Dh == 4)) return false;
    pl->info_stride = 0;
    if (a.Za > FBBEV_DA_HIT_ZA) return false;                             // a hit record holds 4 anchors
    const size_t budget_bytes = (size_t)da_own_plane_kb() * 1024;
    int budget = (int)(budget_bytes / (a.HS * sizeof(long long))) - 8;             // tokens per LDS plane (64-bit words, skewed)
    { const int v = da_bwd_env().tokens; if (v > 0 && v < budget) budget = v; }   // tests: force bands
    // one region per level (a level larger than the budget: bands of rows), so that every level gets the copies its size allows
    da_region reg[24];
    int n = 0;
    if (!level_hw) {
        if (a.S > budget) return false;
        reg[n++] = {0, a.L, 0, a.S};
    } else {
        int start = 0;
        for (int l = 0; l < a.L; ++l) {
            const int h = level_hw[2 * l], w = level_hw[2 * l + 1];
            if (h <= 0 || w <= 0) return false;
            const int cnt = h * w, rows = cnt > budget ? budget / w : h;
            if (rows < 1) return false;
            for (int r = 0; r < h; r += rows) {
                if (n == 24) return false;
                reg[n++] = {l, l + 1, start + r * w, start + (r + rows < h ? r + rows : h) * w};
            }
            start += cnt;
        }
        if (start != a.S) return false;
    }
    // small regions first in the launch order: their adds collide most, they run longest
    // (measured: 1 121-1 128 us small-first against 1 152-1 154 us large-first, tools/sessions_r04/gpu_r04_s39_region_order.sh)
    for (int i = 1; i < n; ++i)
        for (int j = i; j > 0 && reg[j].tok1 - reg[j].tok0 < reg[j - 1].tok1 - reg[j - 1].tok0; --j) { const da_region t = reg[j]; reg[j] = reg[j - 1]; reg[j - 1] = t; }
    size_t lds = 0;
    pl->tab.n = n;
    pl->tab.perm = 0u;
    for (int i = 0; i < n; ++i) {
        // lane -> hit permutation (spreads neighbouring queries over the waves) for whole levels only: in a BAND of rows it costs
        // more than it saves -- consecutive hits sample neighbouring rows, so whole waves skip the corners outside the band (-5 %)
        const bool band = level_hw && (reg[i].tok1 - reg[i].tok0) != level_hw[2 * reg[i].lvl0] * level_hw[2 * reg[i].lvl0 + 1];
        if (!band) pl->tab.perm |= 1u << i;
        const size_t one = (size_t)FBBEV_DA_PLANE_WORDS(reg[i].tok1 - reg[i].tok0, a.HS) * sizeof(long long);
        int copies = (int)(budget_bytes / one);
        copies = copies < 1 ? 1 : (copies > 16 ? 16 : copies);
        { const int v = da_bwd_env().copies; if (v >= 1 && v < copies) copies = v; }
        pl->tab.lvl0[i] = reg[i].lvl0; pl->tab.lvl1[i] = reg[i].lvl1; pl->tab.tok0[i] = reg[i].tok0; pl->tab.tok1[i] = reg[i].tok1;
        pl->tab.copies[i] = copies;
        lds = one * copies > lds ? one * copies : lds;
    }
    if (lds > budget_bytes + 12 * 1024) return false;
    pl->lds = lds;
    pl->threads = 512;
    { const int v = da_bwd_env().threads; if (v == 256 || v == 512) pl->threads = v; }
    if ((long long)n * a.B * a.Ncam * a.M >= (1ll << 31) || (long long)a.B * a.Ncam * a.Q >= (1ll << 31)) return false;
    if (mode < 0 && (long long)n * a.B * a.Ncam * a.M < 256) return false;              // too few planes to fill the chip: chunked scatter
    pl->off_list = 0;                                                  // hit records [B*Ncam][Q][16 floats] at the start of ws
    pl->off_count = align_up((size_t)a.B * a.Ncam * a.Q * FBBEV_DA_HIT_REC * sizeof(float), 256);
    pl->off_gmax = pl->off_count + align_up((size_t)a.B * a.Ncam * sizeof(int), 256);
    pl->ws = pl->off_gmax + align_up((size_t)a.B * sizeof(unsigned int), 256);          // one fixed-point scale per sample
    // unit gradients on head planes (k_da_bwd_unit_planes, da_bwd_planes_kernels.h; FBBEV_DA_BWD_UNIT_PLANES=0 keeps the row kernel):
    // M = 8, Dh in {8, 10}, 8 points, 4 anchors, every level at least 2 tokens wide; the planes sit behind the hit lists
    pl->unit_planes = 0;
    pl->off_planes = pl->ws;
    {
        FBBEV_KNOB_ONCE(bool, on, fbbev_env_int("FBBEV_DA_BWD_UNIT_PLANES", 1) != 0);
        bool wide = level_hw != nullptr;
        for (int l = 0; wide && l < a.L; ++l) wide = level_hw[2 * l + 1] >= 2;
        if (on && wide && a.M == 8 && (a.Dh == 10 || a.Dh == 8) && a.P == FBBEV_DAF_P && (long long)a.S * a.Dh * 4 < (1ll << 31) &&
            fbbev_dbp_lds_bytes(a.M, a.Ncam) <= 156 * 1024) {
            pl->unit_planes = 1;
            pl->ws += align_up((size_t)a.B * a.Ncam * a.M * a.S * a.Dh * sizeof(float), 256);
        }
    }
    return true;
}

extern "C" size_t fbbev_da_cross_attn_bwd_ws_bytes(int B, int Ncam, int S, int M, int Dh, int Q, int head_stride,
                                                   int num_levels, int num_points, const int32_t* level_hw_host) {
    const da_args a = da_record({B, Ncam, S, M, Dh, num_levels, Q, num_points, 1 /* anchor: see below */, 1, 0.f, 0.f, 0, head_stride});
    if (!da_dims_ok(a, 1, 0) || a.HS < Dh) return 0;
    // Za is not an argument here (the owned plan needs Za <= 4 and word-aligned records, which only the launch can check): the
    // size covers BOTH routes, so a launch whose owned plan fails still finds room for the chunked LDS planes instead of falling
    // back to global atomics
    da_own_plan op;
    da_bwd_plan pl;
    const size_t own = da_own_plan_make(a, level_hw_host, &op) ? op.ws : 0;
    const size_t tile = da_bwd_tile_plan(a, level_hw_host, &pl) ? pl.ws : 0;
    return own > tile ? own : tile;
}

// The same query with the number of Z anchors the launch will see: exactly the size of the route that launch takes (owned planes
// when their plan holds for this Za, the chunked planes otherwise) instead of the maximum over both.
extern "C" size_t fbbev_da_cross_attn_bwd_ws_bytes_za(int B, int Ncam, int S, int M, int Dh, int Q, int head_stride, int num_levels,
                                                      int num_points, int num_z_anchors, const int32_t* level_hw_host) {
    const da_args a = da_record({B, Ncam, S, M, Dh, num_levels, Q, num_points, num_z_anchors, 1, 0.f, 0.f, 0, head_stride});
    if (!da_dims_ok(a, 1, 0) || a.HS < Dh) return 0;
    da_own_plan op;
    if (num_points % num_z_anchors == 0 && da_own_plan_make(a, level_hw_host, &op)) return op.ws;
    da_bwd_plan pl;
    return da_bwd_tile_plan(a, level_hw_host, &pl) ? pl.ws : 0;
}

// (A) of both LDS-plane backward routes: unit-owned gradients (offsets / attention / depth distribution), the forward's launch shape
static int da_bwd_unit_launch(const da_args& a, unsigned int* gmax_bits, bool det) {
    const long long units = (long long)a.B * a.Q * a.M;
    long long ub = ((units + 255) / 256 + 7) / 8 * 8;
    if (ub > 65536) ub = 65536;
    const size_t lds_a = (size_t)256 * (4 * a.P + 1) * sizeof(float);
    const bool qi = (a.head_minor & 4) != 0;
#define FBBEV_DA_BWD_UNIT_K(DH_, QI_, DET_)                                                                              \
    FBBEV_LAUNCH((k_da_cross_attn_bwd_unit<DH_, QI_, DET_>), ub, 256, lds_a, a.stream, units, a.value, a.spatial_shapes, \
                 a.level_start_index, a.pred_depth, a.ref_cam, a.mask, a.qdepth, a.offsets, a.attn, a.grad_slots, a.B,   \
                 a.Ncam, a.S, a.M, a.L, a.Q, a.P, a.Za, a.DC, a.d0, a.dstep, a.head_minor & 3, a.HS, a.grad_pred_depth,  \
                 a.grad_offsets, a.grad_attn, gmax_bits)
#define FBBEV_DA_BWD_UNIT(DH_)                                                                                          \
    do {                                                                                                                \
    if (det) { if (qi) FBBEV_DA_BWD_UNIT_K(DH_, true, true); else FBBEV_DA_BWD_UNIT_K(DH_, false, true); }             \
    else if (qi) FBBEV_DA_BWD_UNIT_K(DH_, true, false);                                                                 \
    else FBBEV_DA_BWD_UNIT_K(DH_, false, false);                                                                        \
    } while (0)
    FBBEV_DA_DH_BWD(a.Dh, FBBEV_DA_BWD_UNIT);
#undef FBBEV_DA_BWD_UNIT
#undef FBBEV_DA_BWD_UNIT_K
    FBBEV_CHECK_LAUNCH();
    return 0;
}

// output-owned route: unit gradients, then init + hit lists + ONE scatter launch over every token region
static int da_bwd_owned_launch(const da_own_plan& op, const da_args& a, void* ws, bool det) {
    char* w = static_cast<char*>(ws);
    float* hit_rec = reinterpret_cast<float*>(w + op.off_list);
    int* hit_count = reinterpret_cast<int*>(w + op.off_count);
    unsigned int* gmax_bits = reinterpret_cast<unsigned int*>(w + op.off_gmax);
    FBBEV_LAUNCH(k_da_bwd_init, 1, 256, 0, a.stream, a.B * a.Ncam, hit_count, a.B, gmax_bits);
    FBBEV_CHECK_LAUNCH();
    int e = 0;
    // (the plane kernel reads a record's 4 mask bytes / 8 reference floats / 4 depths as whole words: alignment of the geometry inputs)
    if (op.unit_planes && a.Za == FBBEV_DAF_ZA && aligned16(a.ref_cam) && aligned16(a.qdepth) && ((uintptr_t)a.mask & 3) == 0) {
        // camera tokens as head planes, then the unit gradients with the forward's (head, patch) mapping
        const float* planes = a.planes;
        if (!planes) {                                                 // (round 6: the training forward's own head planes may be handed in)
            float* pl_w = reinterpret_cast<float*>(w + op.off_planes);
            const long long n_el = (long long)a.B * a.Ncam * a.S * a.M * a.Dh;
            FBBEV_LAUNCH(k_value_rows_to_head_planes, (n_el + 255) / 256, 256, 0, a.stream, a.value, (long long)a.B * a.Ncam * a.S, a.S,
                         a.M, a.Dh, a.HS, (a.head_minor & 4) ? 1 : 0, pl_w);
            FBBEV_CHECK_LAUNCH();
            planes = pl_w;
        }
        const int gw = (a.bev_w > 0 && a.Q % a.bev_w == 0) ? a.bev_w : 0;
        const long long wgs_u = gw > 0 ? (long long)a.B * ((gw + 7) / 8) * ((a.Q / gw + 7) / 8) : (long long)a.B * ((a.Q + 63) / 64);
        const long long grid_u = (wgs_u + 7) / 8 * 8;
        const size_t lds_u = fbbev_dbp_lds_bytes(a.M, a.Ncam);
        if (grid_u >= (1ll << 31)) return FBBEV_E_UNSUPPORTED;
#define FBBEV_DA_UNIT_PLANES(DH_, DET_)                                                                                        \
    FBBEV_LAUNCH_DYN_LDS((k_da_bwd_unit_planes<DH_, 8, DET_>), grid_u, 512, lds_u, a.stream, (const float*)planes,             \
                         a.spatial_shapes, a.level_start_index, a.pred_depth, a.ref_cam, a.mask, a.qdepth, a.offsets, a.attn,  \
                         a.grad_slots, a.B, a.Ncam, a.S, a.L, a.Q, gw, a.DC, a.d0, a.dstep, a.head_minor & 3, a.grad_pred_depth, \
                         a.grad_offsets, a.grad_attn, gmax_bits)
        if (det) { if (a.Dh == 10) FBBEV_DA_UNIT_PLANES(10, true); else FBBEV_DA_UNIT_PLANES(8, true); }
        else if (a.Dh == 10) FBBEV_DA_UNIT_PLANES(10, false); else FBBEV_DA_UNIT_PLANES(8, false);
#undef FBBEV_DA_UNIT_PLANES
        FBBEV_CHECK_LAUNCH();
    } else {
        e = da_bwd_unit_launch(a, gmax_bits, det);
        if (e) return e;
    }
    FBBEV_LAUNCH(k_da_bwd_hitlist, (long long)a.B * ((a.Q + 255) / 256), 256, 0, a.stream, a.spatial_shapes, a.pred_depth, a.ref_cam,
                 a.mask, a.qdepth, a.B, a.Ncam, a.Q, a.Za, a.DC, a.d0, a.dstep, hit_rec, hit_count);
    FBBEV_CHECK_LAUNCH();
    const fbbev_da_bwd_region_tab& tab = op.tab;
    const long long wgs = (long long)tab.n * a.B * a.Ncam * a.M;
#define FBBEV_DA_OWN(NT_, DH_)                                                                                                  \
    FBBEV_LAUNCH_DYN_LDS((k_da_bwd_scatter_owned<NT_, DH_>), wgs, NT_, op.lds, a.stream, a.spatial_shapes, a.level_start_index, \
                         a.ref_cam, a.offsets, a.attn, a.grad_slots, a.B, a.Ncam, a.S, a.M, a.L, a.Q, a.P, a.Za,                \
                         a.head_minor & 3, a.HS, tab, (const float*)hit_rec, (const int*)hit_count,                             \
                         (const unsigned int*)gmax_bits, (a.head_minor & 4) ? 1 : 0, a.grad_value)
#define FBBEV_DA_OWN_NT(DH_) do { if (op.threads == 512) FBBEV_DA_OWN(512, DH_); else FBBEV_DA_OWN(256, DH_); } while (0)   /* 1024 threads measured slower */
    FBBEV_DA_DH_BWD(a.Dh, FBBEV_DA_OWN_NT);
#undef FBBEV_DA_OWN_NT
#undef FBBEV_DA_OWN
    FBBEV_CHECK_LAUNCH();
    return 0;
}

// ---- deterministic depth taps (det_kernels.h): workspace = [per-(camera, sample, query, anchor) sums][max bits][fixed-point planes]
static size_t da_taps_ws_bytes(int B, int Ncam, int DC, int H0, int W0) {
    return 256 + align_up((size_t)B * Ncam * DC * H0 * W0 * sizeof(unsigned long long), 256);
}
static int da_taps_kq(int Q, int Za) {
    int kq = 0;
    while ((1ll << kq) < (long long)Q * Za) ++kq;
    return kq;
}
extern "C" size_t fbbev_da_depth_taps_det_ws_bytes(int B, int Ncam, int DC, int H0, int W0) {
    if (B <= 0 || Ncam <= 0 || DC <= 0 || H0 <= 0 || W0 <= 0) return 0;
    return da_taps_ws_bytes(B, Ncam, DC, H0, W0);
}
extern "C" int fbbev_da_depth_taps_det(const float* dsum, const float* ref_cam, const float* qdepth, int B, int Ncam, int Q, int Za, int DC,
                                       int H0, int W0, float d0, float dstep, float* grad_pred_depth, void* ws, size_t ws_bytes,
                                       fbbev_stream_t stream_) {
    if (B <= 0 || Ncam <= 0 || Q < 0 || Za <= 0 || DC <= 0 || H0 <= 0 || W0 <= 0 || dstep == 0.f) return FBBEV_E_BADARG;
    if (!dsum || !ref_cam || !qdepth || !grad_pred_depth || !ws) return FBBEV_E_BADARG;
    if (ws_bytes < da_taps_ws_bytes(B, Ncam, DC, H0, W0) || ((uintptr_t)ws & 7) != 0) return FBBEV_E_WORKSPACE;
    if ((long long)H0 * W0 >= (1ll << 31)) return FBBEV_E_UNSUPPORTED;
    if (Q == 0) return 0;
    fbbev_rt_stream stream = (fbbev_rt_stream)stream_;
    unsigned int* gmax = static_cast<unsigned int*>(ws);
    unsigned long long* acc = reinterpret_cast<unsigned long long*>(static_cast<char*>(ws) + 256);
    const long long n_sum = (long long)Ncam * B * Q * Za, n_out = (long long)B * Ncam * DC * H0 * W0;
    int e = fbbev_rt_memset_async(ws, 0, da_taps_ws_bytes(B, Ncam, DC, H0, W0), stream);
    if (e) return e;
    const int kq = da_taps_kq(Q, Za);
    long long gs = (n_sum + 255) / 256, go = (n_out + 255) / 256;
    gs = gs > 4096 ? 4096 : gs; go = go > 4096 ? 4096 : go;
    FBBEV_LAUNCH(k_da_taps_absmax, gs > 1024 ? 1024 : gs, 256, 0, stream, dsum, n_sum, gmax);
    FBBEV_CHECK_LAUNCH();
    FBBEV_LAUNCH(k_da_taps_i64, gs, 256, 0, stream, dsum, ref_cam, qdepth, B, Ncam, Q, Za, DC, H0, W0, d0, dstep, kq,
                 (const unsigned int*)gmax, acc);
    FBBEV_CHECK_LAUNCH();
    FBBEV_LAUNCH(k_i64_to_f32_add, go, 256, 0, stream, (const unsigned long long*)acc, n_out, kq, (const unsigned int*)gmax,
                 grad_pred_depth);
    FBBEV_CHECK_LAUNCH();
    return 0;
}
extern "C" size_t fbbev_da_bwd_det_ws_bytes(int B, int Ncam, int Q, int Za, int DC, int H0, int W0) {
    if (B <= 0 || Ncam <= 0 || Q <= 0 || Za <= 0 || DC <= 0 || H0 <= 0 || W0 <= 0) return 0;
    return align_up((size_t)Ncam * B * Q * Za * sizeof(float), 256) + da_taps_ws_bytes(B, Ncam, DC, H0, W0);
}
// The unit kernels' DET instantiations store the head-summed d / d depth weight into the front of det_ws (zeroed here first: a unit
// no camera sees stores nothing), `run` launches the route with that buffer as its grad_pred_depth, then the taps are added.
template <class Run>
static int da_bwd_det(const da_args& a, const int32_t* level_hw_host, void* det_ws, size_t det_ws_bytes, Run run) {
    if (!level_hw_host || !det_ws || !a.ref_cam || !a.qdepth || !a.grad_pred_depth) return FBBEV_E_BADARG;
    if (a.B <= 0 || a.Ncam <= 0 || a.Q <= 0 || a.Za <= 0 || a.DC <= 0 || a.dstep == 0.f) return FBBEV_E_BADARG;
    if (a.M > 64 || (a.M & (a.M - 1)) != 0) return FBBEV_E_UNSUPPORTED;            // the unit kernel's head reduction
    const int H0 = level_hw_host[0], W0 = level_hw_host[1];
    if (H0 <= 0 || W0 <= 0) return FBBEV_E_BADARG;
    if (det_ws_bytes < fbbev_da_bwd_det_ws_bytes(a.B, a.Ncam, a.Q, a.Za, a.DC, H0, W0) || !aligned16(det_ws)) return FBBEV_E_WORKSPACE;
    const size_t sum_bytes = align_up((size_t)a.Ncam * a.B * a.Q * a.Za * sizeof(float), 256);
    da_args d = a;
    d.grad_pred_depth = static_cast<float*>(det_ws);
    int e = fbbev_rt_memset_async(d.grad_pred_depth, 0, sum_bytes, a.stream);
    if (e) return e;
    e = run(d);
    if (e) return e;
    return fbbev_da_depth_taps_det(d.grad_pred_depth, a.ref_cam, a.qdepth, a.B, a.Ncam, a.Q, a.Za, a.DC, H0, W0, a.d0, a.dstep,
                                   a.grad_pred_depth, static_cast<char*>(det_ws) + sum_bytes, det_ws_bytes - sum_bytes,
                                   (fbbev_stream_t)a.stream);
}

// the LDS-plane routes on token rows: output-owned planes, else the chunked scatter, else (unless det) the global atomics
static int da_bwd_ws(const da_args& a, const int32_t* level_hw_host, void* ws, size_t ws_bytes, bool det) {
    if (!da_dims_ok(a, 0, 0)) return FBBEV_E_BADARG;
    {
        da_own_plan op;
        if (a.HS >= a.Dh && a.Q > 0 && ws && aligned16(ws) && aligned16(a.grad_value) && da_bwd_present(a) && a.dstep != 0.f &&
            a.P % a.Za == 0 && da_pairs_aligned(a) && da_own_plan_make(a, level_hw_host, &op) && ws_bytes >= op.ws)
            return da_bwd_owned_launch(op, a, ws, det);
    }
    da_bwd_plan pl;
    if (a.HS < a.Dh || a.Q == 0 || !ws || !aligned16(ws) || !aligned16(a.grad_value) || !aligned16(a.value) ||
        !da_bwd_tile_plan(a, level_hw_host, &pl) || ws_bytes < pl.ws || (long long)a.B * a.M * pl.chunks >= (1ll << 31) ||
        (long long)a.B * a.Ncam * a.S * a.M * a.HS * 4 >= (1ll << 32) || !da_pairs_aligned(a))
        return det ? FBBEV_E_UNSUPPORTED : da_bwd_atomic(a);
    if (!da_anchors_ok(a)) return FBBEV_E_UNSUPPORTED;
    if (a.dstep == 0.f) return FBBEV_E_BADARG;
    if (!da_bwd_present(a)) return FBBEV_E_BADARG;
    float* part = static_cast<float*>(ws);
    const long long wgs = (long long)a.B * a.M * pl.chunks;
    const float* info = nullptr;
    if (pl.info_stride > 0 && 1 + a.Za <= pl.info_stride) {
        float* info_w = reinterpret_cast<float*>(static_cast<char*>(ws) + pl.ws_part);
        FBBEV_LAUNCH(k_da_bwd_hitinfo, ((long long)a.B * a.Q + 255) / 256, 256, 0, a.stream, a.spatial_shapes, a.pred_depth, a.ref_cam,
                     a.mask, a.qdepth, a.B, a.Ncam, a.Q, a.Za, a.DC, a.d0, a.dstep, pl.info_stride, info_w);
        FBBEV_CHECK_LAUNCH();
        info = info_w;
    }
    if (const int e = da_bwd_unit_launch(a, nullptr, det)) return e;
    // (B) value gradient, one launch per token region
    for (int r = 0; r < pl.n_regions; ++r) {
        const da_region& rg = pl.reg[r];
        // small regions (coarse levels): up to 4 copies of the plane inside the LDS budget of the largest region
        const size_t one = (size_t)FBBEV_DA_PLANE_WORDS(rg.tok1 - rg.tok0, a.HS) * sizeof(long long);
        int copies = (int)((size_t)(da_bwd_plane_kb() * 1024) / one);
        copies = copies < 1 ? 1 : (copies > 4 ? 4 : copies);
        { const int v = da_bwd_env().copies; if (v >= 1 && v <= copies) copies = v; }
        const size_t lds_b = one * copies + (size_t)((pl.q_per_chunk + 1) & ~1) * 2 + (size_t)(1 + pl.threads / 64) * sizeof(int);
#define FBBEV_DA_BWD_SC(NT_, DH_)                                                                                              \
    FBBEV_LAUNCH((k_da_cross_attn_bwd_scatter<NT_, DH_>), wgs, NT_, lds_b, a.stream, a.spatial_shapes, a.level_start_index, \
                 a.pred_depth, a.ref_cam, a.mask, a.qdepth, a.offsets, a.attn, a.grad_slots, a.B, a.Ncam, a.S, a.M, a.L,    \
                 a.Q, a.P, a.Za, a.DC, a.d0, a.dstep, a.head_minor & 3, a.HS, pl.chunks, pl.q_per_chunk, rg.lvl0, rg.lvl1,  \
                 rg.tok0, rg.tok1, copies, part, info, pl.info_stride)
#define FBBEV_DA_BWD_SC_NT(DH_) do { if (pl.threads == 512) FBBEV_DA_BWD_SC(512, DH_); else FBBEV_DA_BWD_SC(256, DH_); } while (0)
        FBBEV_DA_DH_BWD(a.Dh, FBBEV_DA_BWD_SC_NT);
#undef FBBEV_DA_BWD_SC_NT
#undef FBBEV_DA_BWD_SC
        FBBEV_CHECK_LAUNCH();
    }
    const long long n = (long long)a.B * a.Ncam * a.S * a.M * a.HS;
    long long rb = (n + 255) / 256;
    if (rb > 65536) rb = 65536;
    FBBEV_LAUNCH(k_da_bwd_reduce, rb, 256, 0, a.stream, (const float*)part, a.B, a.Ncam, a.S, a.M, a.HS, pl.chunks,
                 (a.head_minor & 4) ? 1 : 0, a.grad_value);
    FBBEV_CHECK_LAUNCH();
    return 0;
}

extern "C" int fbbev_da_cross_attn_bwd_ws(const float* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                                          const float* pred_depth, const float* ref_cam, const uint8_t* mask,
                                          const float* qdepth, const float* offsets, const float* attn,
                                          const float* grad_slots, int B, int Ncam, int S, int M, int Dh, int L, int Q,
                                          int P, int Za, int DC, float d0, float dstep, int head_minor, int head_stride,
                                          float* grad_value, float* grad_pred_depth, float* grad_offsets,
                                          float* grad_attn, const int32_t* level_hw_host, void* ws, size_t ws_bytes,
                                          fbbev_stream_t stream_) {
    const da_args a = da_record({B, Ncam, S, M, Dh, L, Q, P, Za, DC, d0, dstep, head_minor, head_stride, 0, (fbbev_rt_stream)stream_,
                                 value, nullptr, spatial_shapes, level_start_index, pred_depth, ref_cam, mask, qdepth, offsets, attn,
                                 nullptr, grad_slots, grad_value, grad_pred_depth, grad_offsets, grad_attn});
    return da_bwd_ws(a, level_hw_host, ws, ws_bytes, false);
}
// ... with the BEV grid's width: the queries are a (Q / bev_w) x bev_w grid, so the unit gradients take 8 x 8 patches of it
// (k_da_bwd_unit_planes; bev_w = 0 or not a divisor of Q: runs of 64 consecutive queries)
extern "C" int fbbev_da_cross_attn_bwd_ws_grid(const float* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                                               const float* pred_depth, const float* ref_cam, const uint8_t* mask,
                                               const float* qdepth, const float* offsets, const float* attn,
                                               const float* grad_slots, int B, int Ncam, int S, int M, int Dh, int L, int Q,
                                               int P, int Za, int DC, float d0, float dstep, int head_minor, int head_stride,
                                               float* grad_value, float* grad_pred_depth, float* grad_offsets,
                                               float* grad_attn, const int32_t* level_hw_host, void* ws, size_t ws_bytes,
                                               int bev_w, fbbev_stream_t stream_) {
    const da_args a = da_record({B, Ncam, S, M, Dh, L, Q, P, Za, DC, d0, dstep, head_minor, head_stride, bev_w, (fbbev_rt_stream)stream_,
                                 value, nullptr, spatial_shapes, level_start_index, pred_depth, ref_cam, mask, qdepth, offsets, attn,
                                 nullptr, grad_slots, grad_value, grad_pred_depth, grad_offsets, grad_attn});
    return da_bwd_ws(a, level_hw_host, ws, ws_bytes, false);
}
// ... with a flags word (FBBEV_FLAG_DETERMINISTIC: the depth taps as 64-bit fixed point, no float atomics; det_ws of
// fbbev_da_bwd_det_ws_bytes; a shape neither LDS-plane route takes is FBBEV_E_UNSUPPORTED instead of the global-atomic kernel)
extern "C" int fbbev_da_cross_attn_bwd_ws_grid_ex(const float* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                                                  const float* pred_depth, const float* ref_cam, const uint8_t* mask,
                                                  const float* qdepth, const float* offsets, const float* attn,
                                                  const float* grad_slots, int B, int Ncam, int S, int M, int Dh, int L, int Q,
                                                  int P, int Za, int DC, float d0, float dstep, int head_minor, int head_stride,
                                                  float* grad_value, float* grad_pred_depth, float* grad_offsets,
                                                  float* grad_attn, const int32_t* level_hw_host, void* ws, size_t ws_bytes,
                                                  int bev_w, int flags, void* det_ws, size_t det_ws_bytes, fbbev_stream_t stream_) {
    const da_args a = da_record({B, Ncam, S, M, Dh, L, Q, P, Za, DC, d0, dstep, head_minor, head_stride, bev_w, (fbbev_rt_stream)stream_,
                                 value, nullptr, spatial_shapes, level_start_index, pred_depth, ref_cam, mask, qdepth, offsets, attn,
                                 nullptr, grad_slots, grad_value, grad_pred_depth, grad_offsets, grad_attn});
    if (!(flags & FBBEV_FLAG_DETERMINISTIC)) return da_bwd_ws(a, level_hw_host, ws, ws_bytes, false);
    return da_bwd_det(a, level_hw_host, det_ws, det_ws_bytes,
                      [&](const da_args& d) { return da_bwd_ws(d, level_hw_host, ws, ws_bytes, true); });
}

// Round 6: the backward of fbbev_da_cross_attn_fused for the training step that runs the one-kernel forward -- the camera tokens arrive as
// the HEAD PLANES the forward sampled (fbbev_rows_linear_x3_planes: no row copy of them exists), and on this route every output but
// grad_pred_depth is WRITTEN in full (grad_value by the plane owners incl. the padding channels, grad_offsets / grad_attn by the
// unit kernel for every query of the grid): the caller zeroes only grad_pred_depth.  Needs the output-owned plane route with the
// unit gradients on head planes (M = 8, Dh in {8, 10}, 8 points, 4 anchors, levels >= 2 wide, >= 256 planes) and queries on a
// bev_w-wide grid; FBBEV_E_UNSUPPORTED otherwise (the caller keeps fbbev_da_cross_attn_bwd_ws_grid on row tokens).
extern "C" int fbbev_da_cross_attn_bwd_planes_supported(int B, int Ncam, int S, int M, int Dh, int L, int Q, int P, int Za, int head_stride,
                                                        const int32_t* level_hw_host, int bev_w) {
    const da_args a = da_record({B, Ncam, S, M, Dh, L, Q, P, Za, 1, 0.f, 0.f, 0, head_stride, bev_w});
    if (!da_dims_ok(a, 1, 1) || Q % bev_w != 0) return 0;
    da_own_plan op;
    if (a.HS < Dh || P % Za != 0 || Za != FBBEV_DAF_ZA || !da_own_plan_make(a, level_hw_host, &op)) return 0;
    return op.unit_planes ? 1 : 0;
}
static int da_bwd_planes(const da_args& a, const int32_t* level_hw_host, void* ws, size_t ws_bytes, bool det) {
    if (!da_dims_ok(a, 1, 1)) return FBBEV_E_BADARG;
    if (!da_bwd_present(a) || !ws) return FBBEV_E_BADARG;
    if (a.dstep == 0.f) return FBBEV_E_BADARG;
    da_own_plan op;
    if (a.HS < a.Dh || a.P % a.Za != 0 || a.Za != FBBEV_DAF_ZA || a.Q % a.bev_w != 0 || !da_own_plan_make(a, level_hw_host, &op) ||
        !op.unit_planes) return FBBEV_E_UNSUPPORTED;
    if (!aligned16(ws) || !aligned16(a.grad_value) || !aligned16(a.ref_cam) || !aligned16(a.qdepth) || ((uintptr_t)a.mask & 3) != 0 ||
        ((uintptr_t)a.planes & 7) != 0 || !da_pairs_aligned(a)) return FBBEV_E_UNSUPPORTED;
    if (ws_bytes < op.ws) return FBBEV_E_WORKSPACE;
    return da_bwd_owned_launch(op, a, ws, det);
}
extern "C" int fbbev_da_cross_attn_bwd_planes(const float* planes, const int64_t* spatial_shapes, const int64_t* level_start_index,
                                              const float* pred_depth, const float* ref_cam, const uint8_t* mask,
                                              const float* qdepth, const float* offsets, const float* attn, const float* grad_slots,
                                              int B, int Ncam, int S, int M, int Dh, int L, int Q, int P, int Za, int DC, float d0,
                                              float dstep, int head_minor, int head_stride, float* grad_value, float* grad_pred_depth,
                                              float* grad_offsets, float* grad_attn, const int32_t* level_hw_host, void* ws,
                                              size_t ws_bytes, int bev_w, fbbev_stream_t stream_) {
    const da_args a = da_record({B, Ncam, S, M, Dh, L, Q, P, Za, DC, d0, dstep, head_minor, head_stride, bev_w, (fbbev_rt_stream)stream_,
                                 nullptr, planes, spatial_shapes, level_start_index, pred_depth, ref_cam, mask, qdepth, offsets, attn,
                                 nullptr, grad_slots, grad_value, grad_pred_depth, grad_offsets, grad_attn});
    return da_bwd_planes(a, level_hw_host, ws, ws_bytes, false);
}
// ... with a flags word (FBBEV_FLAG_DETERMINISTIC: the depth taps as 64-bit fixed point, det_ws of fbbev_da_bwd_det_ws_bytes)
extern "C" int fbbev_da_cross_attn_bwd_planes_ex(const float* planes, const int64_t* spatial_shapes, const int64_t* level_start_index,
                                                 const float* pred_depth, const float* ref_cam, const uint8_t* mask,
                                                 const float* qdepth, const float* offsets, const float* attn, const float* grad_slots,
                                                 int B, int Ncam, int S, int M, int Dh, int L, int Q, int P, int Za, int DC, float d0,
                                                 float dstep, int head_minor, int head_stride, float* grad_value, float* grad_pred_depth,
                                                 float* grad_offsets, float* grad_attn, const int32_t* level_hw_host, void* ws,
                                                 size_t ws_bytes, int bev_w, int flags, void* det_ws, size_t det_ws_bytes,
                                                 fbbev_stream_t stream_) {
    const da_args a = da_record({B, Ncam, S, M, Dh, L, Q, P, Za, DC, d0, dstep, head_minor, head_stride, bev_w, (fbbev_rt_stream)stream_,
                                 nullptr, planes, spatial_shapes, level_start_index, pred_depth, ref_cam, mask, qdepth, offsets, attn,
                                 nullptr, grad_slots, grad_value, grad_pred_depth, grad_offsets, grad_attn});
    if (!(flags & FBBEV_FLAG_DETERMINISTIC)) return da_bwd_planes(a, level_hw_host, ws, ws_bytes, false);
    return da_bwd_det(a, level_hw_host, det_ws, det_ws_bytes,
                      [&](const da_args& d) { return da_bwd_planes(d, level_hw_host, ws, ws_bytes, true); });
}

// ------------------------------------------------------------------------------ view-transformation pooling, continued: the fused backward
// (training).  On the records and helpers of the pooling block above; it stands here, behind the cross-attention family, because the
// compiler emits kernel instantiations in the order of their first use in this file, and the code objects are held byte-identical.
struct bwd_layout { size_t table, meta, rows, total; long long n_tiles; int tpp; long long max_rows; };

static bwd_layout pool_bwd_layout(const lift_dims& d) {
    bwd_layout l;
    const long long n = lift_points(d), yx = (long long)d.Y * d.X, nvox = (long long)d.B * d.Z * yx;
    l.tpp = (int)((yx + 127) / 128);
    l.n_tiles = (long long)d.B * d.Z * l.tpp;
    l.max_rows = n < nvox ? n : nvox;                 // I <= min(points, voxels)
    l.table = 0;
    l.meta = align_up((size_t)n * 4, 256);
    l.rows = l.meta + align_up(pool_tile_table_bytes(l.n_tiles), 256);
    l.total = l.rows + align_up((size_t)l.max_rows * d.C * 4, 256);
    return l;
}

extern "C" size_t fbbev_pool_dense_bwd_workspace_bytes(int B, int N, int D, int H, int W, int C, int Z, int Y, int X) {
    const lift_dims d = {B, N, D, H, W, C, Z, Y, X};
    return lift_dims_positive(d) ? pool_bwd_layout(d).total : 256;
}

struct pool_bwd_args {
    const float* out_grad; long long og_stride_b, og_stride_c;           // (B, C, Z, Y, X), strides as the caller passed them
    const float *depth, *feat;
    const int32_t *rd, *irank, *starts, *counts; int n_max;
    lift_dims d;
    float *depth_grad, *feat_grad;
    void* ws; size_t ws_bytes;
    fbbev_rt_stream stream;
    const float* zgrad; float zscale;                       // a second gradient (B, C, Y, X) every z plane receives, scaled; may be null
};
static int pool_dense_bwd(const pool_bwd_args& p) {
    const lift_dims& d = p.d;
    const int C = d.C;
    if (p.zgrad && !aligned16(p.zgrad)) return FBBEV_E_UNSUPPORTED;      // (before the dimensions)
    if (!lift_dims_positive(d) || p.n_max < 0) return FBBEV_E_BADARG;
    if (!p.out_grad || !p.depth || !p.feat || !p.rd || !p.irank || !p.starts || !p.counts || !p.depth_grad || !p.feat_grad || !p.ws)
        return FBBEV_E_BADARG;
    const pool_grid g = pool_grid_of(d.B, C, d.Z, d.Y, d.X);
    const long long n = lift_points(d);
    if (C % 4 != 0 || C > 256 || g.yx % 4 != 0 || !aligned16(p.out_grad) || !aligned16(p.feat) || !aligned16(p.feat_grad) ||
        !aligned16(p.ws)) return FBBEV_E_UNSUPPORTED;
    if (!pool_grid_fits_int(g) || n >= (1ll << 31)) return FBBEV_E_UNSUPPORTED;
    const pool_strides s = pool_volume_strides(p.og_stride_b, p.og_stride_c, g);
    if (s.err) return s.err;
    const bwd_layout l = pool_bwd_layout(d);
    if (p.ws_bytes < l.total) return FBBEV_E_WORKSPACE;
    const size_t lds = (size_t)C * (128 + 4) * 4;
    if (lds > 160 * 1024) return FBBEV_E_UNSUPPORTED;
    char* ws = static_cast<char*>(p.ws);
    int* table = reinterpret_cast<int*>(ws + l.table);
    int* meta = reinterpret_cast<int*>(ws + l.meta);
    float* rows = reinterpret_cast<float*>(ws + l.rows);
    int e = fbbev_rt_memset_async(table, 0xFF, (size_t)n * 4, p.stream);      // -1 = point dropped
    if (e) return e;
    {
        long long blocks = (n + 255) / 256;      // P <= n, grid-stride over the device-side P
        if (blocks > 8192) blocks = 8192;
        FBBEV_LAUNCH(k_point_row_table, blocks, 256, 0, p.stream, p.rd, p.starts, p.counts, p.n_max, table);
        FBBEV_CHECK_LAUNCH();
    }
    FBBEV_LAUNCH(k_tile_lower_bound2, (l.n_tiles + 1 + 255) / 256, 256, 0, p.stream, (int)l.n_tiles, l.tpp, (int)g.yx,
                 128, p.irank, p.starts, p.counts, p.n_max, (const int*)nullptr, meta);
    FBBEV_CHECK_LAUNCH();
    FBBEV_LAUNCH_DYN_LDS(k_pool_bwd_rows<128>, l.n_tiles, 256, lds, p.stream, C, d.Z, (int)g.yx, l.tpp, s.b, s.c,
                         p.out_grad, p.irank, meta, rows, p.zgrad, p.zscale);
    FBBEV_CHECK_LAUNCH();
    const long long n_pixels = (long long)d.B * d.N * d.H * d.W;
    const long long blocks = (n_pixels + 7) / 8;      // 8 half-waves per 256-thread workgroup
    if (C > 128 && C % 8 != 0) return FBBEV_E_UNSUPPORTED;               // (only here, behind three launches: see the table of entries)
    FBBEV_POOL_WITH(CPL, C <= 128 ? 4 : 8, 4, 8, FBBEV_LAUNCH(k_pool_bwd_pixel<CPL>, blocks, 256, 0, p.stream, C, d.D, d.H * d.W, n_pixels,
                                                              (long long)C, rows, p.depth, p.feat, table, p.depth_grad, p.feat_grad));
    FBBEV_CHECK_LAUNCH();
    return 0;
}

extern "C" int fbbev_bev_pool_v2_dense_bwd(const float* out_grad, long long og_stride_b, long long og_stride_c,
                                           const float* depth, const float* feat, const int32_t* ranks_depth,
                                           const int32_t* interval_rank, const int32_t* interval_starts,
                                           const int32_t* counts, int n_intervals_max, int B, int N, int D,
                                           int H, int W, int C, int Z, int Y, int X, float* depth_grad,
                                           float* feat_grad, void* workspace, size_t workspace_bytes,
                                           fbbev_stream_t stream_) {
    return pool_dense_bwd({out_grad, og_stride_b, og_stride_c, depth, feat, ranks_depth, interval_rank, interval_starts, counts,
                           n_intervals_max, {B, N, D, H, W, C, Z, Y, X}, depth_grad, feat_grad, workspace, workspace_bytes,
                           (fbbev_rt_stream)stream_, nullptr, 0.f});
}
// ... with a second gradient (B, C, Y, X) that every z plane receives, scaled by zscale: out_grad_eff = out_grad + zscale * zgrad[..., None]
extern "C" int fbbev_bev_pool_v2_dense_bwd_z(const float* out_grad, long long og_stride_b, long long og_stride_c,
                                             const float* zgrad, float zscale, const float* depth, const float* feat,
                                             const int32_t* ranks_depth, const int32_t* interval_rank,
                                             const int32_t* interval_starts, const int32_t* counts, int n_intervals_max, int B,
                                             int N, int D, int H, int W, int C, int Z, int Y, int X, float* depth_grad,
                                             float* feat_grad, void* workspace, size_t workspace_bytes, fbbev_stream_t stream_) {
    if (!zgrad) return FBBEV_E_BADARG;
    return pool_dense_bwd({out_grad, og_stride_b, og_stride_c, depth, feat, ranks_depth, interval_rank, interval_starts, counts,
                           n_intervals_max, {B, N, D, H, W, C, Z, Y, X}, depth_grad, feat_grad, workspace, workspace_bytes,
                           (fbbev_rt_stream)stream_, zgrad, zscale});
}

// ------------------------------------------------------------------------------ temporal history fusion
// The streaming detector's per-frame step: warp the ring of past frames into the current ego frame, store the current frame, run the
// two fused 1x1x1 convolutions over the T + 1 frames.  Every entry fills a history_ring per ring operand and one of the records
// below from its positional C arguments; everything under it works on those records.
//   entry                          ring layout               arithmetic        kernels                                        knobs that route it
//   fbbev_history_flow             -                         fp32              k_history_flow                                 -
//   fbbev_history_stream_prologue  -                         fp32              k_history_stream_prologue, k_history_flow      -
//   fbbev_history_warp[_e]         planes (B, CH, Z, Y, X)   fp32 taps         k_history_warp<ET> | k_history_warp_lds<ET>    FBBEV_HISTORY_WARP=lds
//   fbbev_history_warp_vm          voxel-major (B, T, N, C)  fp32 taps         k_history_warp_vm<ET, 2 (fp16: 4), 1>          FBBEV_HISTORY_VM_YB, _VM_TU, _WARP_LDS_PAD_KB
//   fbbev_history_warp_vm_src      voxel-major               fp32 taps         k_history_warp_vm_src<ET, 2 (fp16: 4), 1>      FBBEV_HISTORY_VM_YB
//   fbbev_history_frame_vm         planes -> one ring slot   -                 k_history_frame_vm<ET>                         -
//   fbbev_history_conv[_e]         planes (B, T1 * C, N)     fp32 MFMA         k_history_weight_fragments + k_history_conv_t  -
//                                                                              (C = Cout in {16, 80} and a workspace), else k_history_conv
//   fbbev_history_conv_vm          voxel-major               fp32 MFMA         k_history_weight_fragments + k_history_conv_t  -
//   fbbev_history_conv_bf16        either (voxel_major)      bf16 MFMA         k_history_weight_fragments_bf16 +              FBBEV_HISTORY_CONV_LDS_PAD_KB
//                                                                              k_history_conv_bf16
//   fbbev_history_fused_vm         voxel-major, 16-bit       bf16 MFMA         k_history_weight_fragments_bf16 +              -
//                                                                              k_history_fused_bf16 (warp + both convolutions)
//   fbbev_history_conv_bf16x3      voxel-major, 16-bit       split bf16 MFMA   k_history_weight_fragments_bf16x3 +            FBBEV_HX3_WAVES
//                                                                              k_history_conv_bf16x3
//   fbbev_history_fused_x3_vm      voxel-major, 16-bit       split bf16 MFMA   k_history_weight_fragments_bf16x3 +            -
//                                                                              k_history_fused_x3 (warp + both convolutions)
//   fbbev_history_step_x3_vm       voxel-major, 16-bit       split bf16 MFMA   warp_vm's and conv_bf16x3's kernels, band by   FBBEV_HISTORY_STEP_WAVES, _STEP_PRIORITY,
//                                                                              band on two streams                            and warp_vm's three

// A ring operand: B samples `stride` elements apart, each `frames` frames of N voxels x C channels -- voxel-major rows [N][C] or
// planes [C][N]; the rule below is the same for both.
struct history_ring {
    const void* p;
    long long stride;                                       // as the caller passed it (0 = dense) until history_ring_operand resolves it
    int frames, C;
    long long N;
    int et;                                                 // FBBEV_ELEM_*: 0 fp32, 1 bf16, 2 fp16
};
// The rule for a ring operand: a batch stride of 0 means dense (and becomes that), one below frames * frame is FBBEV_E_BADARG;
// rows read VE elements (16 bytes) at a time -- VE = 0: planes, no row accesses -- off a 16-byte boundary or a stride that is no
// multiple of VE are FBBEV_E_UNSUPPORTED; so is, where the kernels form 32-bit byte offsets inside a frame (limit32), a frame past
// them.  Two rings side by side go through row_worse: either one's BADARG comes first.
static inline int history_ring_operand(history_ring& r, int VE, bool limit32) {
    const long long frame = r.N * r.C;
    if (r.stride == 0) r.stride = r.frames * frame;
    if (r.stride < r.frames * frame) return FBBEV_E_BADARG;
    if (VE && (r.stride % VE != 0 || !aligned16(r.p))) return FBBEV_E_UNSUPPORTED;
    if (limit32 && frame * (r.et == 0 ? 4 : 2) >= (1ll << 32)) return FBBEV_E_UNSUPPORTED;
    return 0;
}
static inline bool history_et_ok(int et) { return et >= 0 && et <= 2; }

// The two convolutions over the frames of `feats`: out (B, Cout, N) = relu(bias2 + sum_t w2_t . relu(w1 . x_t + bias1_t))
struct history_conv_args {
    history_ring feats;                                     // frames = T1
    const float* w1; const float* bias1; const float* w2; const float* bias2;
    int B, Cout;
    float* out;
    void* ws; size_t ws_bytes;
    fbbev_rt_stream stream;
};
// A warp: the frames of `src` sampled at rt_flow's coordinates into `dst`
struct history_warp_args {
    history_ring src, dst;
    const float* rt_flow;
    int B, Z, Y, X;
    fbbev_rt_stream stream;
};
// A whole step: the warp of `history` into the slots 1.. of conv.feats (the next ring, whose slot 0 holds the current frame), then
// the convolutions over that ring
struct history_step_args {
    history_ring history;
    history_conv_args conv;
    const float* rt_flow;
    int Z, Y, X;
};

// The checks the entries share.  Their ORDER inside an entry is part of the ABI (it decides the code where two defects coincide),
// so every entry strings them together itself.
static inline bool history_conv_dims_ok(const history_conv_args& c) {
    return c.B >= 0 && c.feats.frames > 0 && c.feats.C > 0 && c.Cout > 0 && c.feats.N >= 0 && history_et_ok(c.feats.et);
}
static inline bool history_conv_empty(const history_conv_args& c) { return c.B == 0 || c.feats.N == 0; }
static inline bool history_conv_present(const history_conv_args& c) { return c.feats.p && c.w1 && c.bias1 && c.w2 && c.bias2 && c.out; }
// the MFMA kernels with register-resident weights are built for these two channel counts
static inline bool history_conv_square(const history_conv_args& c) { return c.feats.C == c.Cout && (c.Cout == 80 || c.Cout == 16); }
// (no element type here: the step entries make it a matter of FBBEV_E_UNSUPPORTED)
static inline bool history_step_dims_ok(const history_step_args& s) {
    return s.conv.B >= 0 && s.history.frames > 0 && s.history.C > 0 && s.conv.Cout > 0 && s.Z > 0 && s.Y > 0 && s.X > 0;
}
static inline bool history_step_present(const history_step_args& s) { return s.history.p && s.rt_flow && history_conv_present(s.conv); }
static inline bool history_step_16bit(const history_step_args& s) { return s.history.et == 1 || s.history.et == 2; }

// The region's template ladders: the statement(s) after the value, once per candidate, with `constexpr int NAME` set to the
// candidate the value equals (the last candidate where it equals none) -- a launch names its instantiation with it.  A `return`
// inside (FBBEV_LAUNCH_DYN_LDS has one) leaves the enclosing function.
#define FBBEV_HISTORY_WITH(NAME, v, A, B, ...)                                                                        \
    do { if ((v) == (A)) { constexpr int NAME = A; __VA_ARGS__; } else { constexpr int NAME = B; __VA_ARGS__; } } while (0)
// ET over the ring's element type: 16-bit rings only, or all three
#define FBBEV_HISTORY_ET16(et, ...) FBBEV_HISTORY_WITH(ET, et, 1, 2, __VA_ARGS__)
#define FBBEV_HISTORY_ET(et, ...) \
    do { if ((et) == 0) { constexpr int ET = 0; __VA_ARGS__; } else FBBEV_HISTORY_ET16(et, __VA_ARGS__); } while (0)

// Workgroups in XCD-contiguous order: the kernel maps workgroup w to block (w % 8) * per_xcd + w / 8 and skips what lies past
// `blocks`, so neighbouring blocks share an XCD's L2.  Callers bound `blocks` first (FBBEV_HISTORY_XCD_BLOCKS where nothing else does).
struct history_xcd_grid { int per_xcd; long long wgs; };
static inline history_xcd_grid history_xcd(long long blocks) {
    const int per_xcd = (int)((blocks + 7) / 8);
    return {per_xcd, (long long)per_xcd * 8};
}
static const long long FBBEV_HISTORY_XCD_BLOCKS = (1ll << 31) - 8;
// Bands of grid rows: YB rows of y (all z) make a slab of YB * Z workgroups per x chunk, 128 / Z rows unless the caller has another
// number; clamped to the grid
struct history_bands { int YB, nyb; };
static inline history_bands history_band_geometry(int YB, int Y) {
    if (YB < 1) YB = 1;
    if (YB > Y) YB = Y;
    return {YB, (Y + YB - 1) / YB};
}

extern "C" int fbbev_history_flow(const float* history_forward_augs, const float* curr_to_prev_ego_rt, const float* bda,
                                  const float* dx3, const float* lower3, int B, float* rt_flow, fbbev_stream_t stream_) {
    if (B < 0) return FBBEV_E_BADARG;
    if (B == 0) return 0;
    if (!history_forward_augs || !curr_to_prev_ego_rt || !bda || !dx3 || !lower3 || !rt_flow) return FBBEV_E_BADARG;
    if (!(dx3[0] > 0.f) || !(dx3[1] > 0.f) || !(dx3[2] > 0.f)) return FBBEV_E_BADARG;
    FBBEV_LAUNCH(k_history_flow, (B + 63) / 64, 64, 0, (fbbev_rt_stream)stream_, history_forward_augs, curr_to_prev_ego_rt,
                 bda, dx3[0], dx3[1], dx3[2], lower3[0], lower3[1], lower3[2], B, rt_flow);
    FBBEV_CHECK_LAUNCH();
    return 0;
}

// the device-state stream mode's per-frame prologue (history_kernels.h): k_history_stream_prologue, then k_history_flow on the
// augs it selected -- the kernel fbbev_history_flow launches, so rt_flow carries the default route's bits
extern "C" int fbbev_history_stream_prologue(const int32_t* flags, const float* curr_to_prev_ego_rt, const float* bda,
                                             const float* b1, const float* wt, const float* dx3, const float* lower3,
                                             float history_cam_sweep_freq, int B, int T, int C, float* history_forward_augs,
                                             float* sweep_time, float* flow_augs, float* rt_flow, float* bias1,
                                             fbbev_stream_t stream_) {
    if (B < 0 || T < 0 || C <= 0) return FBBEV_E_BADARG;
    if (B == 0) return 0;
    if (!flags || !curr_to_prev_ego_rt || !bda || !b1 || !wt || !dx3 || !lower3 || !history_forward_augs || !flow_augs || !rt_flow ||
        !bias1 || (T > 0 && !sweep_time)) return FBBEV_E_BADARG;
    if (!(dx3[0] > 0.f) || !(dx3[1] > 0.f) || !(dx3[2] > 0.f)) return FBBEV_E_BADARG;
    if (T > 8192) return FBBEV_E_UNSUPPORTED;                      // the new sweep times of a sample sit in LDS
    fbbev_rt_stream stream = (fbbev_rt_stream)stream_;
    FBBEV_LAUNCH(k_history_stream_prologue, B, 256, (size_t)(T + 1) * sizeof(float), stream, flags, bda, b1, wt,
                 history_cam_sweep_freq, T, C, history_forward_augs, sweep_time, flow_augs, bias1);
    FBBEV_CHECK_LAUNCH();
    FBBEV_LAUNCH(k_history_flow, (B + 63) / 64, 64, 0, stream, (const float*)flow_augs, curr_to_prev_ego_rt, bda, dx3[0], dx3[1],
                 dx3[2], lower3[0], lower3[1], lower3[2], B, rt_flow);
    FBBEV_CHECK_LAUNCH();
    return 0;
}

// ---- the warp on planes (the reference's layout): one "frame" of CH channel planes per sample
extern "C" int fbbev_history_warp_e(const void* history, long long history_stride_b, const float* rt_flow, int B, int CH,
                                    int Z, int Y, int X, void* out, long long out_stride_b, int elem_type,
                                    fbbev_stream_t stream_) {
    const long long zyx = (long long)Z * Y * X;
    history_warp_args a = {{history, history_stride_b, 1, CH, zyx, elem_type}, {out, out_stride_b, 1, CH, zyx, elem_type},
                           rt_flow, B, Z, Y, X, (fbbev_rt_stream)stream_};
    if (B < 0 || CH < 0 || Z < 2 || Y < 2 || X < 2) return FBBEV_E_BADARG;      // size-1 axes divide by zero in :208
    if (!history_et_ok(elem_type)) return FBBEV_E_BADARG;
    if (B == 0 || CH == 0) return 0;
    if (!history || !rt_flow || !out) return FBBEV_E_BADARG;
    if (zyx >= (1ll << 31)) return FBBEV_E_UNSUPPORTED;
    if (const int e = row_worse(history_ring_operand(a.src, 0, false), history_ring_operand(a.dst, 0, false))) return e;
    // FBBEV_HISTORY_WARP=lds selects the LDS-staged brick kernel (k_history_warp_lds: bit-identical, but as built --
    // one 1024-thread workgroup per CU, staging and taps of a channel serialised by two barriers -- 3x SLOWER than the
    // gather kernel on MI355X, profiles/r02_time_history_lds_vs_gather.jsonl; kept for the next iteration, not the default)
    const char* mode = fbbev_env_str("FBBEV_HISTORY_WARP");      // read on every call
    const bool lds = mode && mode[0] == 'l';
    if (lds && zyx >= 4096 && X >= 16) {
        int TX = 64;
        while (TX / 2 >= X) TX /= 2;
        const int BZ = Z < 8 ? Z : 8;
        int TY = 4096 / (BZ * TX);
        if (TY > Y) TY = Y;
        if (TY < 1) TY = 1;
        const int ntx = (X + TX - 1) / TX, nty = (Y + TY - 1) / TY, ntz = (Z + BZ - 1) / BZ;
        int cpb = 64;                                  // channels per workgroup: the brick's tap setup is amortised over them
        while (cpb > 8 && (long long)B * ntz * nty * ntx * ((CH + cpb - 1) / cpb) < 2048) cpb >>= 1;
        const int n_groups = (CH + cpb - 1) / cpb;
        const long long blocks = (long long)B * n_groups * ntz * nty * ntx;
        if (blocks >= (1ll << 31)) return FBBEV_E_UNSUPPORTED;
        FBBEV_HISTORY_ET(elem_type, FBBEV_LAUNCH(k_history_warp_lds<ET>, blocks, 1024, 0, a.stream, history, a.src.stride, rt_flow, CH,
                                                 Z, Y, X, BZ, TY, TX, ntz, nty, ntx, cpb, n_groups, out, a.dst.stride));
        FBBEV_CHECK_LAUNCH();
        return 0;
    }
    const int n_chunks = (int)((zyx + 255) / 256);
    // enough workgroups to fill 256 CUs several times over, at least 8 channels each to amortise the tap setup
    int cpb = 64;
    while (cpb > 8 && (long long)B * n_chunks * ((CH + cpb - 1) / cpb) < 4096) cpb >>= 1;
    const int n_groups = (CH + cpb - 1) / cpb;
    const long long blocks = (long long)B * n_groups * n_chunks;
    if (blocks >= (1ll << 31)) return FBBEV_E_UNSUPPORTED;       // (this kernel's own bound: eight more than the others take)
    const history_xcd_grid g = history_xcd(blocks);
    FBBEV_HISTORY_ET(elem_type, FBBEV_LAUNCH(k_history_warp<ET>, g.wgs, 256, 0, a.stream, history, a.src.stride, rt_flow, CH, Z, Y, X,
                                             cpb, n_groups, n_chunks, g.per_xcd, (int)blocks, out, a.dst.stride));
    FBBEV_CHECK_LAUNCH();
    return 0;
}

extern "C" int fbbev_history_warp(const float* history, long long history_stride_b, const float* rt_flow, int B, int CH,
                                  int Z, int Y, int X, float* out, long long out_stride_b, fbbev_stream_t stream_) {
    return fbbev_history_warp_e(history, history_stride_b, rt_flow, B, CH, Z, Y, X, out, out_stride_b, 0, stream_);
}

// ---- the warp on the voxel-major ring: frames [T][N][C] per sample (history_kernels.h)
struct fbbev_warp_vm_plan { int groups, n_xc, YB, nyb; };

// the checks of a voxel-major warp (0 also for the empty call: B == 0 or no frames) and its grid
static int history_warp_vm_plan(history_warp_args& a, fbbev_warp_vm_plan& pl) {
    const int T = a.src.frames, C = a.src.C, et = a.src.et;
    if (a.B < 0 || T < 0 || C <= 0 || a.Z < 2 || a.Y < 2 || a.X < 2) return FBBEV_E_BADARG;
    if (!history_et_ok(et)) return FBBEV_E_BADARG;
    if (a.B == 0 || T == 0) return 0;
    if (!a.src.p || !a.rt_flow || !a.dst.p) return FBBEV_E_BADARG;
    const int VE = et == 0 ? 4 : 8;
    if (a.src.N >= (1ll << 31)) return FBBEV_E_UNSUPPORTED;
    if (const int e = row_worse(history_ring_operand(a.src, VE, true), history_ring_operand(a.dst, VE, true))) return e;
    if (C % VE != 0) return FBBEV_E_UNSUPPORTED;
    pl.groups = C / VE;
    pl.n_xc = (a.X * pl.groups + 255) / 256;                      // workgroups per grid row
    // rows per band: a (z, y) slab of ~128 workgroups per x chunk; tuning knob, read on every call (profiles/r02_time_history_bf16_voxel_major.jsonl)
    const history_bands bands = history_band_geometry(fbbev_env_int("FBBEV_HISTORY_VM_YB", 128 / a.Z), a.Y);
    pl.YB = bands.YB;
    pl.nyb = bands.nyb;
    return 0;
}

// the bands yb0 .. yb0 + nyb_c - 1 of every sample (all of them: the whole warp)
static int history_warp_vm_bands(const history_warp_args& a, const fbbev_warp_vm_plan& pl, int yb0, int nyb_c) {
    const long long blocks = (long long)a.B * nyb_c * pl.n_xc * pl.YB * a.Z;
    if (blocks >= FBBEV_HISTORY_XCD_BLOCKS) return FBBEV_E_UNSUPPORTED;
    if (blocks == 0) return 0;
    const history_xcd_grid g = history_xcd(blocks);
    // occupancy experiment knob (round 3, profiles/r03_exp_history_occupancy.jsonl): dynamic LDS the kernel does not use, in KB
    static const size_t warp_pad = (size_t)fbbev_env_int("FBBEV_HISTORY_WARP_LDS_PAD_KB", 0) * 1024;
    // template arguments: frames in flight per thread, then ST = 1: non-temporal ring stores (A/B on one box: 4.0 vs 4.2 ms at
    // 400x400x16, 0.56 vs 0.61 ms at 100x100x8 B=4).  Two frames; an fp16 ring four (32 taps) -- the widening rides in the multiply
    // (v_fma_mix_f32), which left the registers for it (round 6: 3.45 -> 3.33 ms at 400x400x16); FBBEV_HISTORY_VM_TU=2 restores two
    static const int tu2 = fbbev_env_int("FBBEV_HISTORY_VM_TU", 0) == 2 ? 1 : 0;
    if (a.src.et == 2 && !tu2)
        FBBEV_LAUNCH_DYN_LDS((k_history_warp_vm<2, 4, 1>), g.wgs, 256, warp_pad, a.stream, a.src.p, a.src.stride, a.rt_flow, a.src.frames,
                             a.src.C, a.Z, a.Y, a.X, pl.groups, pl.n_xc, pl.YB, nyb_c, g.per_xcd, (int)blocks, const_cast<void*>(a.dst.p),
                             a.dst.stride, yb0);
    else
        FBBEV_HISTORY_ET(a.src.et, FBBEV_LAUNCH_DYN_LDS((k_history_warp_vm<ET, 2, 1>), g.wgs, 256, warp_pad, a.stream, a.src.p, a.src.stride,
                                                        a.rt_flow, a.src.frames, a.src.C, a.Z, a.Y, a.X, pl.groups, pl.n_xc, pl.YB, nyb_c,
                                                        g.per_xcd, (int)blocks, const_cast<void*>(a.dst.p), a.dst.stride, yb0));
    FBBEV_CHECK_LAUNCH();
    return 0;
}

extern "C" int fbbev_history_warp_vm(const void* history, long long history_stride_b, const float* rt_flow, int B, int T, int C,
                                     int Z, int Y, int X, void* out, long long out_stride_b, int elem_type,
                                     fbbev_stream_t stream_) {
    const long long zyx = (long long)Z * Y * X;
    history_warp_args a = {{history, history_stride_b, T, C, zyx, elem_type}, {out, out_stride_b, T, C, zyx, elem_type},
                           rt_flow, B, Z, Y, X, (fbbev_rt_stream)stream_};
    fbbev_warp_vm_plan pl{};
    const int e = history_warp_vm_plan(a, pl);
    if (e || B == 0 || T == 0) return e;
    return history_warp_vm_bands(a, pl, 0, pl.nyb);
}

// fbbev_history_warp_vm with a per-sample source: where flags[b] != 0 the T frames of sample b are sampled from curr[b] (the current
// frame's rows), the old ring of that sample is not read (k_history_warp_vm_src)
extern "C" int fbbev_history_warp_vm_src(const void* history, long long history_stride_b, const void* curr, long long curr_stride_b,
                                         const int32_t* flags, const float* rt_flow, int B, int T, int C, int Z, int Y, int X,
                                         void* out, long long out_stride_b, int elem_type, fbbev_stream_t stream_) {
    const long long zyx = (long long)Z * Y * X;
    history_warp_args a = {{history, history_stride_b, T, C, zyx, elem_type}, {out, out_stride_b, T, C, zyx, elem_type},
                           rt_flow, B, Z, Y, X, (fbbev_rt_stream)stream_};
    history_ring cur = {curr, curr_stride_b, 1, C, zyx, elem_type};
    fbbev_warp_vm_plan pl{};
    const int e = history_warp_vm_plan(a, pl);
    if (e || B == 0 || T == 0) return e;
    if (!curr || !flags) return FBBEV_E_BADARG;
    if (const int ec = history_ring_operand(cur, elem_type == 0 ? 4 : 8, false)) return ec;
    const long long blocks = (long long)B * pl.nyb * pl.n_xc * pl.YB * Z;
    if (blocks >= FBBEV_HISTORY_XCD_BLOCKS) return FBBEV_E_UNSUPPORTED;
    const history_xcd_grid g = history_xcd(blocks);
    // the instantiations fbbev_history_warp_vm launches by default: two frames in flight, four for an fp16 ring
    FBBEV_HISTORY_ET(elem_type, FBBEV_LAUNCH((k_history_warp_vm_src<ET, ET == 2 ? 4 : 2, 1>), g.wgs, 256, 0, a.stream, history, a.src.stride,
                                             curr, cur.stride, flags, rt_flow, T, C, Z, Y, X, pl.groups, pl.n_xc, pl.YB, pl.nyb, g.per_xcd,
                                             (int)blocks, out, a.dst.stride));
    FBBEV_CHECK_LAUNCH();
    return 0;
}

extern "C" int fbbev_history_frame_vm(const float* curr, int B, int C, int N, int inner, void* out, long long out_stride_b,
                                      int elem_type, fbbev_stream_t stream_) {
    history_ring slot = {out, out_stride_b, 1, C, N, elem_type};
    if (B < 0 || C <= 0 || N < 0 || !history_et_ok(elem_type)) return FBBEV_E_BADARG;
    if (inner < 1 || N % inner != 0) return FBBEV_E_BADARG;
    if (B == 0 || N == 0) return 0;
    if (!curr || !out) return FBBEV_E_BADARG;
    const int VE = elem_type == 0 ? 4 : 8;
    if (const int e = history_ring_operand(slot, VE, false)) return e;
    if (C % VE != 0 || C > 512) return FBBEV_E_UNSUPPORTED;
    const int tiles_per_b = (N + 63) / 64;
    const long long blocks = (long long)B * tiles_per_b;
    if (blocks >= (1ll << 31)) return FBBEV_E_UNSUPPORTED;
    const size_t lds = (size_t)C * 65 * sizeof(float);
    FBBEV_HISTORY_ET(elem_type, FBBEV_LAUNCH_DYN_LDS(k_history_frame_vm<ET>, blocks, 256, lds, (fbbev_rt_stream)stream_, curr, C, N, inner,
                                                     tiles_per_b, out, slot.stride));
    FBBEV_CHECK_LAUNCH();
    return 0;
}

// ---- the convolutions in fp32 (FP32 MFMA), planes or voxel-major (vm)
// Each weight-workspace layout below: where the pieces lie, how many bytes they take, and the one launch that fills them.
// fp32: fragment-ordered copies of the two weight matrices (tiny: (1 + T1) * C * C floats)
struct history_weights_f32 { const float* w1f; const float* w2f; size_t need; };
static int history_weights_f32_prepare(const history_conv_args& c, bool vm, history_weights_f32& w) {
    const int T1 = c.feats.frames, MT1 = c.feats.C / 16, MT2 = c.Cout / 16, KS = c.feats.C / 4;
    w.need = ((size_t)MT1 * KS + (size_t)T1 * MT2 * KS) * 64 * sizeof(float);
    if (c.ws_bytes < w.need) return FBBEV_E_WORKSPACE;
    float* w1f = static_cast<float*>(c.ws);
    w.w1f = w1f;
    w.w2f = w1f + (size_t)MT1 * KS * 64;
    const int nfrag = (MT1 * KS + T1 * MT2 * KS) * 64;
    FBBEV_LAUNCH(k_history_weight_fragments, (nfrag + 255) / 256, 256, 0, c.stream, c.w1, c.w2, MT1, MT2, KS, T1, vm ? 1 : 0, w1f);
    return 0;
}

static int history_conv_launch(const history_conv_args& c, bool vm) {
    const int T1 = c.feats.frames, C = c.feats.C, N = (int)c.feats.N;
    const int tiles_per_b = (N + 63) / 64;
    const long long blocks = (long long)c.B * tiles_per_b;
    if (blocks >= (1ll << 31)) return FBBEV_E_UNSUPPORTED;
    const size_t lds = (size_t)4 * C * 16 * sizeof(float);
    if (c.ws && history_conv_square(c)) {                          // the register-resident kernel
        history_weights_f32 w{};
        if (const int e = history_weights_f32_prepare(c, vm, w)) return e;
        FBBEV_HISTORY_WITH(VM, vm ? 1 : 0, 1, 0, FBBEV_HISTORY_WITH(MT, C / 16, 5, 1, FBBEV_HISTORY_ET(c.feats.et,
            FBBEV_LAUNCH((k_history_conv_t<MT, MT, ET, VM != 0>), blocks, 256, lds, c.stream, c.feats.p, c.feats.stride, w.w1f,
                         c.bias1, w.w2f, c.bias2, T1, N, tiles_per_b, c.out))));
    } else if (vm)
        return FBBEV_E_UNSUPPORTED;
    else
        FBBEV_HISTORY_ET(c.feats.et, FBBEV_LAUNCH(k_history_conv<ET>, blocks, 256, lds, c.stream, c.feats.p, c.feats.stride, c.w1, c.bias1,
                                                  c.w2, c.bias2, T1, C, c.Cout, N, tiles_per_b, c.out));
    FBBEV_CHECK_LAUNCH();
    return 0;
}

extern "C" int fbbev_history_conv_e(const void* feats, long long feats_stride_b, const float* w1, const float* bias1,
                                    const float* w2, const float* bias2, int B, int T1, int C, int Cout, int N,
                                    float* out, void* workspace, size_t workspace_bytes, int elem_type,
                                    fbbev_stream_t stream_) {
    history_conv_args c = {{feats, feats_stride_b, T1, C, N, elem_type}, w1, bias1, w2, bias2, B, Cout, out, workspace, workspace_bytes,
                           (fbbev_rt_stream)stream_};
    if (!history_conv_dims_ok(c)) return FBBEV_E_BADARG;
    if (history_conv_empty(c)) return 0;
    if (!history_conv_present(c)) return FBBEV_E_BADARG;
    if (C % 16 != 0 || Cout % 16 != 0 || C > 16 * FBBEV_HC_MAX_TILES || Cout > 16 * FBBEV_HC_MAX_TILES)
        return FBBEV_E_UNSUPPORTED;
    if (const int e = history_ring_operand(c.feats, 0, false)) return e;
    if (!aligned16(bias1)) return FBBEV_E_UNSUPPORTED;                                  // 16-byte bias loads
    return history_conv_launch(c, false);
}

extern "C" int fbbev_history_conv(const float* feats, long long feats_stride_b, const float* w1, const float* bias1,
                                  const float* w2, const float* bias2, int B, int T1, int C, int Cout, int N,
                                  float* out, void* workspace, size_t workspace_bytes, fbbev_stream_t stream_) {
    return fbbev_history_conv_e(feats, feats_stride_b, w1, bias1, w2, bias2, B, T1, C, Cout, N, out, workspace,
                                workspace_bytes, 0, stream_);
}

// the fp32-MFMA convolutions on a voxel-major ring (feats (B, T1, N, C)); C = Cout in {16, 80}, workspace required
extern "C" int fbbev_history_conv_vm(const void* feats, long long feats_stride_b, const float* w1, const float* bias1,
                                     const float* w2, const float* bias2, int B, int T1, int C, int Cout, int N,
                                     float* out, void* workspace, size_t workspace_bytes, int elem_type,
                                     fbbev_stream_t stream_) {
    history_conv_args c = {{feats, feats_stride_b, T1, C, N, elem_type}, w1, bias1, w2, bias2, B, Cout, out, workspace, workspace_bytes,
                           (fbbev_rt_stream)stream_};
    if (!history_conv_dims_ok(c)) return FBBEV_E_BADARG;
    if (history_conv_empty(c)) return 0;
    if (!history_conv_present(c)) return FBBEV_E_BADARG;
    if (!history_conv_square(c)) return FBBEV_E_UNSUPPORTED;
    if (!workspace) return FBBEV_E_WORKSPACE;
    if (const int e = history_ring_operand(c.feats, 8, true)) return e;                 // 8- / 16-byte row pieces
    if (!aligned16(bias1)) return FBBEV_E_UNSUPPORTED;
    return history_conv_launch(c, true);
}

// ---- the convolutions on the bf16 MFMAs (operands rounded to bf16, fp32 accumulate): C = Cout = 80 or 16
// bf16: the two weight matrices in fragment order, 8 elements per lane
struct history_weights_bf16 {
    const unsigned short* w1f; const unsigned short* w2f;
    int MT, KS;                                             // 16-row tiles of the output channels, 32-deep slices of the input channels
    size_t part1;                                           // elements of W1's fragments (= of one frame's W2)
    size_t a2s;                                             // ... padded to the 256 lanes that stage it
    size_t need;
};
static int history_weights_bf16_prepare(const history_conv_args& c, history_weights_bf16& w) {
    const int T1 = c.feats.frames, C = c.feats.C;
    w.MT = C / 16;
    w.KS = (C + 31) / 32;
    w.part1 = (size_t)w.MT * w.KS * 64 * 8;
    w.a2s = (size_t)((w.MT * w.KS * 64 + 255) / 256) * 256 * 8;
    w.need = (size_t)(1 + T1) * w.part1 * sizeof(unsigned short);
    if (!c.ws || !aligned16(c.ws) || c.ws_bytes < w.need) return FBBEV_E_WORKSPACE;
    unsigned short* w1f = static_cast<unsigned short*>(c.ws);
    w.w1f = w1f;
    w.w2f = w1f + w.part1;
    const int nfrag = (w.MT * w.KS + T1 * w.MT * w.KS) * 64;
    FBBEV_LAUNCH(k_history_weight_fragments_bf16, (nfrag + 255) / 256, 256, 0, c.stream, c.w1, c.w2, w.MT, w.MT, C, T1, w1f);
    return 0;
}

static int history_conv_bf16_launch(const history_conv_args& c, bool vm) {
    const int T1 = c.feats.frames, N = (int)c.feats.N;
    const int tiles_per_b = (N + 63) / 64;
    const long long blocks = (long long)c.B * tiles_per_b;
    if (blocks >= (1ll << 31)) return FBBEV_E_UNSUPPORTED;
    history_weights_bf16 w{};
    if (const int e = history_weights_bf16_prepare(c, w)) return e;
    size_t lds = (2 * w.a2s + (size_t)4 * 16 * (w.KS * 32 + 8)) * sizeof(unsigned short);           // W2_t x 2 + Y rows
    static const size_t conv_pad = (size_t)fbbev_env_int("FBBEV_HISTORY_CONV_LDS_PAD_KB", 0) * 1024;   // occupancy experiment knob
    if (conv_pad > lds) lds = conv_pad;
    if (c.feats.C == 80)
        FBBEV_HISTORY_WITH(VM, vm ? 1 : 0, 1, 0, FBBEV_HISTORY_ET(c.feats.et,
            FBBEV_LAUNCH_DYN_LDS((k_history_conv_bf16<5, 5, ET, VM != 0>), blocks, 256, lds, c.stream, c.feats.p, c.feats.stride, w.w1f,
                                 c.bias1, w.w2f, c.bias2, T1, N, tiles_per_b, c.out)));
    else
        FBBEV_HISTORY_WITH(VM, vm ? 1 : 0, 1, 0, FBBEV_HISTORY_ET(c.feats.et,
            FBBEV_LAUNCH((k_history_conv_bf16<1, 1, ET, VM != 0>), blocks, 256, lds, c.stream, c.feats.p, c.feats.stride, w.w1f, c.bias1,
                         w.w2f, c.bias2, T1, N, tiles_per_b, c.out)));
    FBBEV_CHECK_LAUNCH();
    return 0;
}

extern "C" int fbbev_history_conv_bf16(const void* feats, long long feats_stride_b, const float* w1, const float* bias1,
                                       const float* w2, const float* bias2, int B, int T1, int C, int Cout, int N,
                                       float* out, void* workspace, size_t workspace_bytes, int voxel_major, int elem_type,
                                       fbbev_stream_t stream_) {
    history_conv_args c = {{feats, feats_stride_b, T1, C, N, elem_type}, w1, bias1, w2, bias2, B, Cout, out, workspace, workspace_bytes,
                           (fbbev_rt_stream)stream_};
    if (!history_conv_dims_ok(c)) return FBBEV_E_BADARG;
    if (voxel_major != 0 && voxel_major != 1) return FBBEV_E_BADARG;
    if (history_conv_empty(c)) return 0;
    if (!history_conv_present(c)) return FBBEV_E_BADARG;
    if (!history_conv_square(c)) return FBBEV_E_UNSUPPORTED;
    if (const int e = history_ring_operand(c.feats, voxel_major ? 8 : 0, voxel_major != 0)) return e;   // 16-byte row pieces
    if (!aligned16(bias1)) return FBBEV_E_UNSUPPORTED;                                              // 16-byte bias loads
    return history_conv_bf16_launch(c, voxel_major != 0);
}

// Warp + new ring + both convolutions in ONE kernel (k_history_fused_bf16): history (B,T,N,C) -> next ring slots 1..T of
// `next` (B,T+1,N,C) (slot 0 = the current frame, stored by the caller with fbbev_history_frame_vm BEFORE this call) and
// out (B,Cout,N) = relu(bias2 + sum_t w2_t . relu(w1 . x_t + bias1_t)) over the T+1 frames of `next`, bf16 MFMA.
extern "C" int fbbev_history_fused_vm(const void* history, long long history_stride_b, void* next, long long next_stride_b,
                                      const float* rt_flow, const float* w1, const float* bias1, const float* w2,
                                      const float* bias2, int B, int T, int C, int Cout, int Z, int Y, int X, float* out,
                                      void* workspace, size_t workspace_bytes, int elem_type, fbbev_stream_t stream_) {
    const long long N = (long long)Z * Y * X;
    history_step_args s = {{history, history_stride_b, T, C, N, elem_type},
                           {{next, next_stride_b, T + 1, C, N, elem_type}, w1, bias1, w2, bias2, B, Cout, out, workspace, workspace_bytes,
                            (fbbev_rt_stream)stream_}, rt_flow, Z, Y, X};
    if (!history_step_dims_ok(s)) return FBBEV_E_BADARG;
    if (B == 0) return 0;
    if (!history_step_present(s)) return FBBEV_E_BADARG;
    if (C != 80 || Cout != 80 || !history_step_16bit(s) || Z < 2 || Y < 2 || X < 2) return FBBEV_E_UNSUPPORTED;
    if (const int e = row_worse(history_ring_operand(s.history, 8, true), history_ring_operand(s.conv.feats, 8, true))) return e;
    if (!aligned16(bias1) || N >= (1ll << 31)) return FBBEV_E_UNSUPPORTED;
    history_weights_bf16 w{};
    if (const int e = history_weights_bf16_prepare(s.conv, w)) return e;
    FBBEV_CHECK_LAUNCH();
    const int n_xc = (X + 63) / 64;                               // 64-voxel tiles per grid row
    // (z, y) slabs per x chunk, as the warp kernel orders its workgroups (its default: FBBEV_HISTORY_VM_YB is not read here)
    const history_bands bands = history_band_geometry(128 / Z, Y);
    const long long blocks = (long long)B * bands.nyb * n_xc * bands.YB * Z;
    if (blocks >= FBBEV_HISTORY_XCD_BLOCKS) return FBBEV_E_UNSUPPORTED;
    const history_xcd_grid g = history_xcd(blocks);
    // 4 W2 buffers + the W1 fragments + the Y rows + 4 operand tiles: 137 KB (one 1024-thread workgroup per CU)
    const size_t lds = ((size_t)4 * w.a2s + w.part1 + (size_t)4 * 16 * (w.KS * 32 + 8) + (size_t)4 * 64 * FBBEV_HF_XP) *
                       sizeof(unsigned short) + (size_t)4 * 80 * sizeof(float);
    FBBEV_HISTORY_ET16(elem_type, FBBEV_LAUNCH_DYN_LDS((k_history_fused_bf16<ET>), g.wgs, 1024, lds, s.conv.stream, history,
                                                       s.history.stride, next, s.conv.feats.stride, rt_flow, w.w1f, bias1, w.w2f, bias2,
                                                       T + 1, Z, Y, X, n_xc, bands.YB, bands.nyb, g.per_xcd, (int)blocks, out));
    FBBEV_CHECK_LAUNCH();
    return 0;
}

// ---- fp32-grade convolutions on the 16-bit MFMAs (split operands, history_conv_x3_kernels.h): voxel-major 16-bit ring
// split-operand: W1 (hi | lo) and every frame's W2 (hi | lo) in fragment order, then B * T1 * C biases scaled for the ring's type
struct history_weights_x3 { const unsigned short* w1x; const unsigned short* w2x; const float* biasx; size_t pieces, part1, need; };
static int history_weights_x3_prepare(const history_conv_args& c, history_weights_x3& w) {
    const int T1 = c.feats.frames, C = c.feats.C, MT = C / 16, KS = (C + 31) / 32;
    w.part1 = (size_t)MT * KS * 64 * 8;
    const size_t wbytes = (size_t)(1 + T1) * 2 * w.part1 * sizeof(unsigned short);
    w.need = wbytes + (size_t)c.B * T1 * C * sizeof(float);
    if (!c.ws || !aligned16(c.ws) || c.ws_bytes < w.need) return FBBEV_E_WORKSPACE;
    unsigned short* w1x = static_cast<unsigned short*>(c.ws);
    float* biasx = reinterpret_cast<float*>(static_cast<char*>(c.ws) + wbytes);
    w.w1x = w1x;
    w.w2x = w1x + 2 * w.part1;
    w.biasx = biasx;
    w.pieces = 2 * w.part1 / 8 + C / 4;                           // 16-byte pieces of a frame's W2 (hi | lo) and its bias row
    const long long nprep = (long long)(MT * KS + T1 * MT * KS) * 64 + (long long)c.B * T1 * C;
    if (nprep >= (1ll << 31)) return FBBEV_E_UNSUPPORTED;
    FBBEV_HISTORY_ET16(c.feats.et, FBBEV_LAUNCH(k_history_weight_fragments_bf16x3<ET>, (nprep + 255) / 256, 256, 0, c.stream, c.w1, c.w2,
                                                c.bias1, MT, MT, C, T1, c.B * T1, w1x, biasx));
    FBBEV_CHECK_LAUNCH();
    return 0;
}

// the checks of the split-operand convolutions (0 also for the empty call: B == 0 or N == 0), then their workspace
static int history_conv_x3_prepare(history_conv_args& c, history_weights_x3& w) {
    if (!history_conv_dims_ok(c)) return FBBEV_E_BADARG;
    if (history_conv_empty(c)) return 0;
    if (!history_conv_present(c)) return FBBEV_E_BADARG;
    if (!history_conv_square(c) || c.feats.et == 0) return FBBEV_E_UNSUPPORTED;
    if (const int e = history_ring_operand(c.feats, 8, true)) return e;
    if (!aligned16(c.bias1)) return FBBEV_E_UNSUPPORTED;
    return history_weights_x3_prepare(c, w);
}

// n segments of len voxels, stride apart from voxel seg0 on, in every sample (one segment of N voxels: the whole volume)
struct history_segments { int seg0, stride, len, n; };

// nw waves per workgroup -- 8: a workgroup fills a CU's registers; 4: half of them (the pipelined step)
static int history_conv_x3_segments(const history_conv_args& c, const history_weights_x3& w, history_segments sg, int nw,
                                    fbbev_rt_stream stream) {
    if (sg.len <= 0 || sg.n <= 0) return 0;
    const int T1 = c.feats.frames, N = (int)c.feats.N;
    const int nt = 64 * nw;
    const int tile_voxels = 16 * nw * FBBEV_HX3_NV;
    const int tiles_per_seg = (sg.len + tile_voxels - 1) / tile_voxels;
    const long long tiles_per_b = (long long)tiles_per_seg * sg.n;
    const long long blocks = (long long)c.B * tiles_per_b;
    if (blocks >= (1ll << 31)) return FBBEV_E_UNSUPPORTED;
    // one frame per workgroup barrier (FPB = 2, four W2 buffers: measured 2 % slower, profiles/r06_exp_history_step.md)
    const size_t lds = ((size_t)2 * ((w.pieces + nt - 1) / nt) * nt * 8 + 2 * w.part1) * sizeof(unsigned short);
    // template arguments after ET: two frames of X in flight (three spill: 256 registers at 2 waves / SIMD), the waves, one frame per barrier
    FBBEV_HISTORY_WITH(MT, c.feats.C / 16, 5, 1, FBBEV_HISTORY_WITH(NW, nw, 4, 8, FBBEV_HISTORY_ET16(c.feats.et,
        FBBEV_LAUNCH_DYN_LDS((k_history_conv_bf16x3<MT, MT, ET, 2, NW, 1>), blocks, 64 * NW, lds, stream, c.feats.p, c.feats.stride,
                             w.w1x, w.biasx, w.w2x, c.bias2, T1, N, (int)tiles_per_b, c.out, sg.seg0, sg.stride, sg.len, tiles_per_seg))));
    FBBEV_CHECK_LAUNCH();
    return 0;
}

extern "C" int fbbev_history_conv_bf16x3(const void* feats, long long feats_stride_b, const float* w1, const float* bias1,
                                         const float* w2, const float* bias2, int B, int T1, int C, int Cout, int N,
                                         float* out, void* workspace, size_t workspace_bytes, int elem_type,
                                         fbbev_stream_t stream_) {
    history_conv_args c = {{feats, feats_stride_b, T1, C, N, elem_type}, w1, bias1, w2, bias2, B, Cout, out, workspace, workspace_bytes,
                           (fbbev_rt_stream)stream_};
    history_weights_x3 w{};
    const int e = history_conv_x3_prepare(c, w);
    if (e || B <= 0 || N <= 0) return e;
    static const int nw = fbbev_env_int("FBBEV_HX3_WAVES", 8) == 4 ? 4 : 8;     // tuning: 256-thread workgroups
    return history_conv_x3_segments(c, w, {0, 0, N, 1}, nw, c.stream);
}

// One history step on a 16-bit voxel-major ring as ONE kernel (history_fused_x3_kernels.h): every MFMA wave warps its own operands.
// next[:, 0] must hold the current frame; writes next[:, 1:] (== fbbev_history_warp_vm) and out (== fbbev_history_conv_bf16x3).
extern "C" int fbbev_history_fused_x3_vm(const void* history, long long history_stride_b, void* next, long long next_stride_b,
                                         const float* rt_flow, const float* w1, const float* bias1, const float* w2,
                                         const float* bias2, int B, int T, int C, int Cout, int Z, int Y, int X, float* out,
                                         void* workspace, size_t workspace_bytes, int elem_type, fbbev_stream_t stream_) {
    const long long N = (long long)Z * Y * X;
    history_step_args s = {{history, history_stride_b, T, C, N, elem_type},
                           {{next, next_stride_b, T + 1, C, N, elem_type}, w1, bias1, w2, bias2, B, Cout, out, workspace, workspace_bytes,
                            (fbbev_rt_stream)stream_}, rt_flow, Z, Y, X};
    if (!history_step_dims_ok(s)) return FBBEV_E_BADARG;
    if (B == 0) return 0;
    if (!history_step_present(s)) return FBBEV_E_BADARG;
    if (C != 80 || Cout != 80 || !history_step_16bit(s) || Z < 2 || Y < 2 || X < 2) return FBBEV_E_UNSUPPORTED;
    if (const int e = row_worse(history_ring_operand(s.history, 8, true), history_ring_operand(s.conv.feats, 8, true))) return e;
    if (N >= (1ll << 31)) return FBBEV_E_UNSUPPORTED;
    if (workspace_bytes < 64) return FBBEV_E_WORKSPACE;
    s.conv.ws_bytes -= 64;                                                                      // the tail of the workspace: see `dump`
    history_weights_x3 w{};
    if (const int e = history_conv_x3_prepare(s.conv, w)) return e;
    void* dump = static_cast<char*>(workspace) + (s.conv.ws_bytes & ~(size_t)15);              // 16 bytes nobody reads
    const int n_xt = (X + 15) / 16, n_yt = (Y + 7) / 8;           // bricks of 16 x 8 voxels of one z plane, z fastest
    const long long blocks = (long long)B * n_yt * n_xt * Z;
    if (blocks >= FBBEV_HISTORY_XCD_BLOCKS) return FBBEV_E_UNSUPPORTED;
    const history_xcd_grid g = history_xcd(blocks);
    // two W2 / bias blocks + W1 (hi | lo) + two operand tiles [128 voxels][FBBEV_HFX_PITCH] + the voxel table [128][16 dwords]: 154 KB
    const size_t lds = ((size_t)2 * ((w.pieces + 511) / 512) * 512 * 8 + 2 * w.part1 + (size_t)2 * 128 * FBBEV_HFX_PITCH) * sizeof(unsigned short) +
                       (size_t)128 * 16 * sizeof(unsigned int);
    FBBEV_HISTORY_ET16(elem_type, FBBEV_LAUNCH_DYN_LDS((k_history_fused_x3<ET>), g.wgs, 512, lds, s.conv.stream, history, s.history.stride,
                                                       next, s.conv.feats.stride, rt_flow, w.w1x, w.biasx, w.w2x, bias2, T + 1, Z, Y, X,
                                                       n_xt, n_yt, g.per_xcd, (int)blocks, out, dump));
    FBBEV_CHECK_LAUNCH();
    return 0;
}

// One history step on a 16-bit voxel-major ring as a two-stream pipeline: the warp of a band of grid rows into next[:, 1:] on the
// caller's stream, the split-operand convolutions of the band before it on a second stream -- a bandwidth-bound gather kernel and
// an MFMA-bound one that leave each other's resource idle when they run back to back.  next[:, 0] must hold the current frame.
// The same kernels, operands and results as fbbev_history_warp_vm + fbbev_history_conv_bf16x3, bit for bit.
struct fbbev_side_stream { fbbev_rt_stream stream; fbbev_rt_event ev[2 + 64]; bool ok; };

static fbbev_side_stream* history_side_stream() {
    static fbbev_side_stream table[16];
    static bool made[16];
    const int d = fbbev_rt_device();
    if (d < 0 || d >= 16) return nullptr;
    static std::mutex mu;                                    // (first use from two host threads; the stream and its events are per DEVICE:
    std::lock_guard<std::mutex> lock(mu);                    //  callers serialise their calls per device, as with any stream-ordered workspace)
    if (!made[d]) {
        made[d] = true;
        // the convolutions' stream is created at the device's highest priority: built to let their workgroups in ahead of the thousands
        // of queued warp workgroups -- measured: no effect on the dispatch (profiles/r06_exp_history_step.md).
        // FBBEV_HISTORY_STEP_PRIORITY=0: equal priorities
        table[d].ok = fbbev_rt_stream_create(&table[d].stream, fbbev_env_int("FBBEV_HISTORY_STEP_PRIORITY", 1) == 0 ? 0 : 1) == 0;
        for (int i = 0; i < 2 + 64 && table[d].ok; ++i) table[d].ok = fbbev_rt_event_create(&table[d].ev[i]) == 0;
    }
    return table[d].ok ? &table[d] : nullptr;
}

extern "C" int fbbev_history_step_x3_vm(const void* history, long long history_stride_b, void* next, long long next_stride_b,
                                        const float* rt_flow, const float* w1, const float* bias1, const float* w2,
                                        const float* bias2, int B, int T, int C, int Cout, int Z, int Y, int X, float* out,
                                        void* workspace, size_t workspace_bytes, int elem_type, int chunks,
                                        fbbev_stream_t stream_) {
    const long long N = (long long)Z * Y * X;
    fbbev_rt_stream stream = (fbbev_rt_stream)stream_;
    history_step_args s = {{history, history_stride_b, T, C, N, elem_type},
                           {{next, next_stride_b, T + 1, C, N, elem_type}, w1, bias1, w2, bias2, B, Cout, out, workspace, workspace_bytes,
                            stream}, rt_flow, Z, Y, X};
    if (!history_step_dims_ok(s) || chunks < 0 || chunks > 64) return FBBEV_E_BADARG;
    if (B == 0) return 0;
    if (!history_step_present(s)) return FBBEV_E_BADARG;
    if (!history_step_16bit(s)) return FBBEV_E_UNSUPPORTED;
    if (N >= (1ll << 31)) return FBBEV_E_UNSUPPORTED;
    if (const int e = history_ring_operand(s.conv.feats, 0, false)) return e;                   // the history's stride: the warp's plan
    void* warped = static_cast<char*>(next) + N * C * 2;                                         // next[:, 1:]
    history_warp_args wa = {s.history, {warped, s.conv.feats.stride, T, C, N, elem_type}, rt_flow, B, Z, Y, X, stream};
    fbbev_warp_vm_plan wp{};
    int e = history_warp_vm_plan(wa, wp);
    if (e) return e;
    history_weights_x3 w{};
    e = history_conv_x3_prepare(s.conv, w);
    if (e) return e;
    if (chunks == 0) chunks = 10;
    // the convolutions of the pipeline in 256-thread workgroups: half a CU's registers, so that warp waves share the CU with them
    static const int step_nw = fbbev_env_int("FBBEV_HISTORY_STEP_WAVES", 4) == 8 ? 8 : 4;
    if (chunks > wp.nyb) chunks = wp.nyb;
    fbbev_side_stream* side = chunks > 1 ? history_side_stream() : nullptr;
    if (!side) {                                                                                  // one chunk: the two kernels back to back
        e = history_warp_vm_bands(wa, wp, 0, wp.nyb);
        if (e) return e;
        return history_conv_x3_segments(s.conv, w, {0, 0, (int)N, 1}, 8, stream);
    }
#define FBBEV_RT(x) do { const int e_ = (x); if (e_) return e_; } while (0)
    FBBEV_RT(fbbev_rt_event_record(side->ev[0], stream));
    FBBEV_RT(fbbev_rt_stream_wait(side->stream, side->ev[0]));
    for (int i = 0; i < chunks; ++i) {
        const int yb0 = (int)((long long)wp.nyb * i / chunks), yb1 = (int)((long long)wp.nyb * (i + 1) / chunks);
        e = history_warp_vm_bands(wa, wp, yb0, yb1 - yb0);
        if (e) return e;
        FBBEV_RT(fbbev_rt_event_record(side->ev[2 + i], stream));
        FBBEV_RT(fbbev_rt_stream_wait(side->stream, side->ev[2 + i]));
        const int y0 = yb0 * wp.YB, y1 = yb1 * wp.YB < Y ? yb1 * wp.YB : Y;
        e = history_conv_x3_segments(s.conv, w, {y0 * X, Y * X, (y1 - y0) * X, Z}, step_nw, side->stream);
        if (e) return e;
    }
    FBBEV_RT(fbbev_rt_event_record(side->ev[1], side->stream));
    FBBEV_RT(fbbev_rt_stream_wait(stream, side->ev[1]));
#undef FBBEV_RT
    return 0;
}

// ------------------------------------------------------------------------------ LayerNorm over short rows
extern "C" int fbbev_layernorm(const float* x, const float* residual, const float* weight, const float* bias, float eps,
                               long long rows, int C, float* out, fbbev_stream_t stream_) {
    if (rows < 0 || C <= 0 || !(eps >= 0.f)) return FBBEV_E_BADARG;
    if (rows == 0) return 0;
    if (!x || !weight || !bias || !out) return FBBEV_E_BADARG;
    if (C % 4 != 0 || C > 128 || !aligned16(x) || !aligned16(out) || !aligned16(weight) || !aligned16(bias) ||
        (residual && !aligned16(residual))) return FBBEV_E_UNSUPPORTED;
    const long long blocks = (rows + 7) / 8;          // 8 half-waves per 256-thread workgroup
    if (blocks >= (1ll << 31)) return FBBEV_E_UNSUPPORTED;
    FBBEV_LAUNCH(k_layernorm_rows, blocks, 256, 0, (fbbev_rt_stream)stream_, x, residual, weight, bias, eps, rows, C, out);
    FBBEV_CHECK_LAUNCH();
    return 0;
}

extern "C" int fbbev_layernorm_bwd_partials(long long rows) {
    // workgroups of fbbev_layernorm_bwd = rows of its `partial` output: enough to fill the chip, few enough that the
    // final sum over them stays small
    long long wgs = (rows + 7) / 8;
    if (wgs > 2048) wgs = 2048;
    return (int)(wgs < 1 ? 1 : wgs);
}

extern "C" int fbbev_layernorm_bwd(const float* x, const float* grad_out, const float* weight, float eps, long long rows,
                                   int C, float* grad_x, float* partial, fbbev_stream_t stream_) {
    if (rows < 0 || C <= 0 || !(eps >= 0.f)) return FBBEV_E_BADARG;
    if (!partial) return FBBEV_E_BADARG;
    if (rows > 0 && (!x || !grad_out || !weight || !grad_x)) return FBBEV_E_BADARG;
    if (C % 4 != 0 || C > 128 || !aligned16(x) || !aligned16(grad_out) || !aligned16(weight) || !aligned16(grad_x))
        return FBBEV_E_UNSUPPORTED;
    const int wgs = fbbev_layernorm_bwd_partials(rows);
    FBBEV_LAUNCH(k_layernorm_rows_bwd, wgs, 256, 0, (fbbev_rt_stream)stream_, x, grad_out, weight, eps, rows, C, grad_x, partial);
    FBBEV_CHECK_LAUNCH();
    return 0;
}

// ------------------------------------------------------------------------------ row-wise linear layers, split-operand bf16 MFMA
extern "C" size_t fbbev_rows_linear_x3_fragment_bytes(int in_features, int out_features) {
    if (in_features <= 0 || out_features <= 0) return 0;
    const size_t n_oc = (size_t)(out_features + 127) / 128, n_kc = (size_t)(in_features + 127) / 128;
    return n_oc * n_kc * 8 * FBBEV_RL_TILE_ELEMS * sizeof(unsigned short);
}

extern "C" int fbbev_rows_linear_x3_fragments(const float* weight, int in_features, int out_features, void* fragments,
                                              size_t fragment_bytes, fbbev_stream_t stream_) {
    if (in_features <= 0 || out_features <= 0 || !weight || !fragments) return FBBEV_E_BADARG;
    if (!aligned16(fragments) || fragment_bytes < fbbev_rows_linear_x3_fragment_bytes(in_features, out_features)) return FBBEV_E_WORKSPACE;
    const int n_oc = (out_features + 127) / 128, n_kc = (in_features + 127) / 128;
    const long long n = (long long)n_oc * n_kc * 8 * 4 * 64;
    FBBEV_LAUNCH(k_rows_linear_x3_fragments, (n + 255) / 256, 256, 0, (fbbev_rt_stream)stream_, weight, out_features, in_features,
                 n_oc, n_kc, static_cast<unsigned short*>(fragments));
    FBBEV_CHECK_LAUNCH();
    return 0;
}

// One row-GEMM call: out = epilogue((x [+ addend]) W^T + bias).  The nine fbbev_rows_linear_x3* / _f32* entries fill it -- the head
// every entry has in the order of their own operands, each optional operand BY NAME -- and every helper down to the launch takes it;
// an optional operand that is absent has a null pointer (the head planes: no tokens).
struct rows_ref { const float* p; long long stride; };             // rows `stride` floats apart (0: dense, see row_operand)
struct rows_gemm {
    rows_ref x;
    const void* weights; const float* bias;                        // weights: the fragment buffer (x3) or the weight matrix (out, in) (f32)
    float* out; long long out_stride;
    long long rows; int in_features, out_features, relu;
    fbbev_rt_stream stream;
    // (an entry names what follows; what it does not name is absent)
    struct { const float* p; long long stride, period; } addend;   // added to x: row r takes addend row r % period (none: period 1)
    rows_ref residual;                                             // added to the product (LayerNorm tail, training epilogue)
    struct { const float *weight, *bias; float eps; } ln;          // LayerNorm over a row of the outputs
    rows_ref mask;                                                 // training epilogue: the product is kept where mask > 0
    struct { int tokens_per_image, head_dim, elem_type; } planes;  // out as head planes (images, heads, tokens, head_dim) of FBBEV_ELEM_*
    bool train_epilogue;
};
// The head-plane epilogue takes the head width and the element type of the planes as ONE int, head_dim | elem_type << 16, and
// divides an output's index by head_dim through a 32-bit reciprocal, exact below 2^16: head_dim and out_features at most
// 0xffff, which also keeps the width clear of the type.  rows_planes_check is the only way into this family with planes set.
static inline int rows_plane_word(const rows_gemm& c) { return c.planes.head_dim | (c.planes.elem_type << 16); }
static int rows_planes_check(const rows_gemm& c) {
    const int head_dim = c.planes.head_dim, et = c.planes.elem_type;
    if (c.planes.tokens_per_image <= 0 || head_dim <= 0 || c.out_features <= 0 || et < 0 || et > 2) return FBBEV_E_BADARG;
    if (head_dim % 2 != 0 || c.out_features % head_dim != 0 || c.rows % c.planes.tokens_per_image != 0 || head_dim > 0xffff ||
        c.out_features > 0xffff) return FBBEV_E_UNSUPPORTED;
    return 0;
}

// What the split-bf16 (x3) and the exact-fp32 (f32) entries have in common: the checks of the addend and of the LayerNorm tail's
// operands, which the entries make before anything else is looked at, ...
static int rows_linear_addend_check(rows_gemm* c) {
    if (!c->addend.p || c->addend.period <= 0) return FBBEV_E_BADARG;
    return row_operand(c->addend.p, &c->addend.stride, c->in_features);
}
static int rows_linear_ln_check(rows_gemm* c) {
    if (!c->ln.weight || !c->ln.bias || c->out_features <= 0) return FBBEV_E_BADARG;
    if (c->out_features > 128) return FBBEV_E_UNSUPPORTED;
    if (c->residual.p) { if (const int e = row_operand(c->residual.p, &c->residual.stride, c->out_features)) return e; }
    if (!aligned16(c->ln.weight) || !aligned16(c->ln.bias)) return FBBEV_E_UNSUPPORTED;
    return 0;
}
// ... and the checks of x / weights / bias / out with the launch geometry.  A nonzero result, or rows == 0, ends the call.
struct rows_linear_geom { int n_oc, n_kc, nmt; long long tiles, RT, groups; };
static int rows_linear_prepare(rows_gemm* c, rows_linear_geom* g) {
    if (!c->addend.p) c->addend.period = 1;
    if (c->rows < 0 || c->in_features <= 0 || c->out_features <= 0) return FBBEV_E_BADARG;
    if (c->rows == 0) return 0;
    if (!c->x.p || !c->weights || !c->out) return FBBEV_E_BADARG;
    if (const int e = row_worse(row_operand(c->x.p, &c->x.stride, c->in_features), row_operand(c->out, &c->out_stride, c->out_features)))
        return e;
    if (c->in_features % 8 != 0 || c->out_features % 4 != 0 || !aligned16(c->weights) || (c->bias && !aligned16(c->bias)))
        return FBBEV_E_UNSUPPORTED;
    g->n_oc = (c->out_features + 127) / 128; g->n_kc = (c->in_features + 127) / 128;
    g->tiles = (c->rows + 127) / 128;
    if (g->tiles * g->n_oc >= (1ll << 31)) return FBBEV_E_UNSUPPORTED;
    g->nmt = c->out_features >= 128 ? 8 : (c->out_features + 15) / 16;
    // consecutive row tiles per workgroup (fragments / the weight staged once) as long as ~4 workgroups per CU remain; the chain of
    // an f32 element does not depend on it
    g->RT = g->n_kc == 1 ? g->tiles * g->n_oc / 1024 : 1;
    g->RT = g->RT < 1 ? 1 : (g->RT > 8 ? 8 : g->RT);
    const int rt_emu = FBBEV_KNOB_EMU_INT("FBBEV_ROWS_LINEAR_RT", 0);   // lets a small case walk several row tiles per workgroup
    if (g->n_kc == 1 && rt_emu >= 1 && rt_emu <= 8) g->RT = rt_emu;
    g->groups = (g->tiles + g->RT - 1) / g->RT;
    return 0;
}

// Which kernel takes a split-bf16 call.  Round 6: the persistent form (k_rows_linear_x3p: fragments staged once per workgroup, the
// next tile's rows in flight under the MFMAs, fragment reads under the MFMAs of the tile before) for one K chunk, no addend, no
// LayerNorm tail.  Same bits.  FBBEV_ROWS_LINEAR_P=0: off (A/B knob).  FBBEV_ROWS_LINEAR_NT=1: 16 rows per wave on the plain route.
enum rows_x3_route { ROWS_X3_PERSISTENT, ROWS_X3_TRAIN, ROWS_X3_LN, ROWS_X3_NT1, ROWS_X3_PLAIN };
static bool rows_linear_nt1() { static const bool v = fbbev_env_int("FBBEV_ROWS_LINEAR_NT", 0) == 1; return v; }   // tuning knob, read once
static rows_x3_route rows_x3_route_of(const rows_gemm& c, const rows_linear_geom& g) {
    FBBEV_KNOB_ONCE(bool, persist, fbbev_env_int("FBBEV_ROWS_LINEAR_P", 1) != 0);
    // (the training epilogue at 8 output tiles x 4 k-steps -- 96 < I <= 128 and O > 80: no layer of the model -- would spill: old kernel)
    if (persist && g.n_kc == 1 && !c.ln.weight && !c.addend.p && !(rows_linear_nt1() && !c.train_epilogue) &&
        !(c.train_epilogue && c.out_features > 80 && c.in_features > 96)) return ROWS_X3_PERSISTENT;
    if (c.train_epilogue) return ROWS_X3_TRAIN;
    if (c.ln.weight) return ROWS_X3_LN;
    return rows_linear_nt1() && g.n_kc == 1 ? ROWS_X3_NT1 : ROWS_X3_PLAIN;
}
// The kernel arguments every split-bf16 kernel starts with, and what k_rows_linear_x3 takes behind its geometry
#define FBBEV_ROWS_X3_HEAD(c) \
    c.x.p, c.x.stride, static_cast<const unsigned short*>(c.weights), c.bias, c.out, c.out_stride, c.rows, c.in_features, c.out_features, c.relu
#define FBBEV_ROWS_X3_TAIL(c)                                                                                                          \
    c.addend.p, c.addend.stride, c.addend.period, c.planes.tokens_per_image, rows_plane_word(c), c.residual.p, c.residual.stride, c.ln.weight, \
        c.ln.bias, c.ln.eps, c.mask.p, c.mask.stride
// The persistent kernel's ladders: NMTP output tiles x KSP k-steps; with the training epilogue all but <8, 4> (see the route)
#define FBBEV_ROWS_KSP(ksp, ...) FBBEV_POOL_WITH(KSP, ksp, 3, 4, __VA_ARGS__)
#define FBBEV_ROWS_TILES(nmtp, ksp, ...) FBBEV_POOL_WITH(NMTP, nmtp, 5, 8, FBBEV_ROWS_KSP(ksp, __VA_ARGS__))
#define FBBEV_ROWS_TILES_TRAIN(nmtp, ksp, ...) \
    do { if ((nmtp) == 5) { constexpr int NMTP = 5; FBBEV_ROWS_KSP(ksp, __VA_ARGS__); } else { constexpr int NMTP = 8, KSP = 3; __VA_ARGS__; } } while (0)

static int rows_linear_x3_dispatch(rows_gemm c) {
    rows_linear_geom g;
    int e = rows_linear_prepare(&c, &g);
    if (e || c.rows == 0) return e;
    const int n_oc = g.n_oc;
    const size_t lds = (size_t)g.nmt * FBBEV_RL_TILE_ELEMS * sizeof(unsigned short);
    // (kept ahead of the dispatch although most calls launch k_rows_linear_x3p: as the first use of these two kernels in the file it
    // also fixes their place in the code object, and device code is compared byte for byte across host-only changes)
    e = c.ln.weight ? fbbev_rt_allow_dyn_lds((const void*)k_rows_linear_x3<2, true>, lds) : fbbev_rt_allow_dyn_lds((const void*)k_rows_linear_x3<2, false>, lds);
    if (e) return e;
#define FBBEV_ROWS_X3(KERNEL, grid, rt) \
    FBBEV_LAUNCH_DYN_LDS(KERNEL, (grid) * n_oc, 256, lds, c.stream, FBBEV_ROWS_X3_HEAD(c), g.n_kc, n_oc, (int)(rt), FBBEV_ROWS_X3_TAIL(c))
    const rows_x3_route route = rows_x3_route_of(c, g);
    if (route == ROWS_X3_PERSISTENT) {
        const int nmtp = c.out_features <= 80 ? 5 : 8, ksp = c.in_features <= 96 ? 3 : 4;
        long long n_slots = 512 / n_oc;
        const int slots_emu = FBBEV_KNOB_EMU_INT("FBBEV_ROWS_LINEAR_SLOTS", 0);   // lets a small case walk several row tiles per workgroup
        if (slots_emu >= 1) n_slots = slots_emu;
        if (n_slots < 1) n_slots = 1;
        if (n_slots > g.tiles) n_slots = g.tiles;
        const size_t ldsp = (size_t)nmtp * FBBEV_RL_TILE_ELEMS * sizeof(unsigned short) + (size_t)16 * nmtp * sizeof(float);
#define FBBEV_ROWS_X3P(EPI_)                                                                                                       \
    FBBEV_LAUNCH_DYN_LDS((k_rows_linear_x3p<NMTP, KSP, EPI_>), n_slots * n_oc, 256, ldsp, c.stream, FBBEV_ROWS_X3_HEAD(c), n_oc,    \
                         (int)n_slots, c.planes.tokens_per_image, rows_plane_word(c), c.residual.p, c.residual.stride, c.mask.p, \
                         c.mask.stride)
        if (c.train_epilogue) FBBEV_ROWS_TILES_TRAIN(nmtp, ksp, FBBEV_ROWS_X3P(1));
        else FBBEV_ROWS_TILES(nmtp, ksp, FBBEV_ROWS_X3P(0));
#undef FBBEV_ROWS_X3P
    } else if (route == ROWS_X3_TRAIN) {
        FBBEV_ROWS_X3((k_rows_linear_x3<2, false, 1>), g.groups, g.RT);
    } else if (route == ROWS_X3_LN) {
        if (n_oc != 1) return FBBEV_E_UNSUPPORTED;
        FBBEV_ROWS_X3((k_rows_linear_x3<2, true>), g.groups, g.RT);
    } else if (route == ROWS_X3_NT1) {
        // 16 rows per wave (64 per workgroup): half the accumulators / row pieces in registers -> more waves per SIMD
        const long long tiles1 = (c.rows + 63) / 64;
        long long RT1 = tiles1 * n_oc / 2048;
        RT1 = RT1 < 1 ? 1 : (RT1 > 8 ? 8 : RT1);
        FBBEV_ROWS_X3((k_rows_linear_x3<1, false>), (tiles1 + RT1 - 1) / RT1, RT1);
    } else {
        FBBEV_ROWS_X3((k_rows_linear_x3<2, false>), g.groups, g.RT);
    }
#undef FBBEV_ROWS_X3
    FBBEV_CHECK_LAUNCH();
    return 0;
}

extern "C" int fbbev_rows_linear_x3(const float* x, long long x_row_stride, const void* fragments, const float* bias, long long rows,
                                    int in_features, int out_features, int relu, float* out, long long out_row_stride,
                                    fbbev_stream_t stream_) {
    rows_gemm c = {{x, x_row_stride}, fragments, bias, out, out_row_stride, rows, in_features, out_features, relu, (fbbev_rt_stream)stream_};
    return rows_linear_x3_dispatch(c);
}

extern "C" int fbbev_rows_linear_x3_add(const float* x, long long x_row_stride, const float* addend, long long addend_row_stride,
                                        long long addend_period, const void* fragments, const float* bias, long long rows,
                                        int in_features, int out_features, int relu, float* out, long long out_row_stride,
                                        fbbev_stream_t stream_) {
    rows_gemm c = {{x, x_row_stride}, fragments, bias, out, out_row_stride, rows, in_features, out_features, relu, (fbbev_rt_stream)stream_};
    c.addend = {addend, addend_row_stride, addend_period};
    if (const int e = rows_linear_addend_check(&c)) return e;
    return rows_linear_x3_dispatch(c);
}

// training epilogue (round 6): out = ((x W^T + b) [ReLU]) * [mask > 0] + residual -- the forward recomputations and dgrads of the
// encoder layer's backward with their neighbouring element-wise passes (residual adds, ReLU's threshold_backward, gradient sums)
extern "C" int fbbev_rows_linear_x3_train(const float* x, long long x_row_stride, const float* addend, long long addend_row_stride,
                                          long long addend_period, const void* fragments, const float* bias, long long rows,
                                          int in_features, int out_features, int relu, const float* residual, long long residual_row_stride,
                                          const float* mask, long long mask_row_stride, float* out, long long out_row_stride,
                                          fbbev_stream_t stream_) {
    rows_gemm c = {{x, x_row_stride}, fragments, bias, out, out_row_stride, rows, in_features, out_features, relu, (fbbev_rt_stream)stream_};
    c.addend = {addend, addend_row_stride, addend_period}; c.residual = {residual, residual_row_stride}; c.mask = {mask, mask_row_stride};
    c.train_epilogue = true;
    if (out_features <= 0 || in_features <= 0) return FBBEV_E_BADARG;
    if (addend) { if (const int e = rows_linear_addend_check(&c)) return e; }   // (none: its period is not looked at and becomes 1)
    if (residual) { if (const int e = row_operand(residual, &c.residual.stride, out_features)) return e; }
    if (mask) { if (const int e = row_operand(mask, &c.mask.stride, out_features)) return e; }
    return rows_linear_x3_dispatch(c);
}

// out = LayerNorm(x W^T + b [+ residual]) over the out_features outputs of a row, weight / bias / eps of torch.nn.LayerNorm: the
// `output_proj -> + residual -> norm` tail of the encoder layer's attention blocks and of its FFN (bevformer_encoder.py:250-377
// with operation_order (attn, norm, ...)) as ONE kernel -- the LayerNorm rides in the GEMM's store epilogue.  out_features <= 128
// (a workgroup must hold whole output rows).
extern "C" int fbbev_rows_linear_x3_ln(const float* x, long long x_row_stride, const void* fragments, const float* bias, long long rows,
                                       int in_features, int out_features, const float* residual, long long residual_row_stride,
                                       const float* ln_weight, const float* ln_bias, float ln_eps, float* out,
                                       long long out_row_stride, fbbev_stream_t stream_) {
    rows_gemm c = {{x, x_row_stride}, fragments, bias, out, out_row_stride, rows, in_features, out_features, 0, (fbbev_rt_stream)stream_};
    c.residual = {residual, residual_row_stride}; c.ln = {ln_weight, ln_bias, ln_eps};
    if (const int e = rows_linear_ln_check(&c)) return e;
    return rows_linear_x3_dispatch(c);
}

// ------------------------------------------------------------------------------ row-wise linear layers, exact fp32 (FP32 MFMA)
// fbbev_rows_linear_f32*: every output element is one fp32 fmaf chain in the order of fbbev_rows_linear_f32_k_order (the arithmetic
// contract in include/fbbev.h).  The weight is the nn.Linear parameter itself (row-major (out_features, in_features) fp32).
static int rows_linear_f32_dispatch(rows_gemm c) {
    rows_linear_geom g;
    const int e = rows_linear_prepare(&c, &g);
    if (e || c.rows == 0) return e;
    if (c.ln.weight && g.n_oc != 1) return FBBEV_E_UNSUPPORTED;
    const size_t lds = (size_t)g.nmt * FBBEV_RLF_TILE_FLOATS * sizeof(float);
#define FBBEV_RLF(LN_)                                                                                                            \
    FBBEV_LAUNCH_DYN_LDS((k_rows_linear_f32<LN_>), g.groups * g.n_oc, 256, lds, c.stream, c.x.p, c.x.stride, static_cast<const float*>(c.weights), \
                         c.bias, c.out, c.out_stride, c.rows, c.in_features, c.out_features, c.relu, g.n_kc, g.n_oc, (int)g.RT, c.addend.p, \
                         c.addend.stride, c.addend.period, c.residual.p, c.residual.stride, c.ln.weight, c.ln.bias, c.ln.eps)
    if (c.ln.weight) FBBEV_RLF(true); else FBBEV_RLF(false);
#undef FBBEV_RLF
    FBBEV_CHECK_LAUNCH();
    return 0;
}

extern "C" int fbbev_rows_linear_f32(const float* x, long long x_row_stride, const float* weight, const float* bias, long long rows,
                                     int in_features, int out_features, int relu, float* out, long long out_row_stride,
                                     fbbev_stream_t stream_) {
    rows_gemm c = {{x, x_row_stride}, weight, bias, out, out_row_stride, rows, in_features, out_features, relu, (fbbev_rt_stream)stream_};
    return rows_linear_f32_dispatch(c);
}

extern "C" int fbbev_rows_linear_f32_add(const float* x, long long x_row_stride, const float* addend, long long addend_row_stride,
                                         long long addend_period, const float* weight, const float* bias, long long rows,
                                         int in_features, int out_features, int relu, float* out, long long out_row_stride,
                                         fbbev_stream_t stream_) {
    rows_gemm c = {{x, x_row_stride}, weight, bias, out, out_row_stride, rows, in_features, out_features, relu, (fbbev_rt_stream)stream_};
    c.addend = {addend, addend_row_stride, addend_period};
    if (const int e = rows_linear_addend_check(&c)) return e;
    return rows_linear_f32_dispatch(c);
}

extern "C" int fbbev_rows_linear_f32_ln(const float* x, long long x_row_stride, const float* weight, const float* bias, long long rows,
                                        int in_features, int out_features, const float* residual, long long residual_row_stride,
                                        const float* ln_weight, const float* ln_bias, float ln_eps, float* out,
                                        long long out_row_stride, fbbev_stream_t stream_) {
    rows_gemm c = {{x, x_row_stride}, weight, bias, out, out_row_stride, rows, in_features, out_features, 0, (fbbev_rt_stream)stream_};
    c.residual = {residual, residual_row_stride}; c.ln = {ln_weight, ln_bias, ln_eps};
    if (const int e = rows_linear_ln_check(&c)) return e;
    return rows_linear_f32_dispatch(c);
}

extern "C" int fbbev_rows_linear_f32_k_order(int in_features, int* order) {
    if (in_features <= 0 || !order) return FBBEV_E_BADARG;
    fbbev_rows_linear_f32_order(in_features, order);
    return 0;
}

// y = x W^T + b written as HEAD PLANES: rows = (B*Ncam) x S tokens, out_features = M * head_dim (module order (head, channel));
// out (B*Ncam, M, S, head_dim) -- the camera-token layout of fbbev_da_cross_attn_fused (value_proj of the cross-attention).
extern "C" int fbbev_rows_linear_x3_planes(const float* x, long long x_row_stride, const void* fragments, const float* bias,
                                           long long rows, int in_features, int out_features, int tokens_per_image, int head_dim,
                                           float* out, fbbev_stream_t stream_) {
    rows_gemm c = {{x, x_row_stride}, fragments, bias, out, 0, rows, in_features, out_features, 0, (fbbev_rt_stream)stream_};
    c.planes = {tokens_per_image, head_dim, FBBEV_ELEM_F32};
    if (const int e = rows_planes_check(c)) return e;
    if (out && ((uintptr_t)out & 7) != 0) return FBBEV_E_UNSUPPORTED;
    return rows_linear_x3_dispatch(c);
}

// The same projection with the planes STORED in 16 bits (elem_type 1 bf16, 2 fp16; 0 = fbbev_rows_linear_x3_planes): the fp32 result
// rounded once -- the camera-token storage option of the cross-attention (DA_SpatialCrossAttention.value_dtype) on head planes.
extern "C" int fbbev_rows_linear_x3_planes_e(const float* x, long long x_row_stride, const void* fragments, const float* bias,
                                             long long rows, int in_features, int out_features, int tokens_per_image, int head_dim,
                                             int elem_type, void* out, fbbev_stream_t stream_) {
    rows_gemm c = {{x, x_row_stride}, fragments, bias, static_cast<float*>(out), 0, rows, in_features, out_features, 0, (fbbev_rt_stream)stream_};
    c.planes = {tokens_per_image, head_dim, elem_type};
    if (const int e = rows_planes_check(c)) return e;
    if (out && ((uintptr_t)out & (elem_type ? 3 : 7)) != 0) return FBBEV_E_UNSUPPORTED;
    if (out && !aligned16(out)) return FBBEV_E_UNSUPPORTED;
    return rows_linear_x3_dispatch(c);
}

// The FFN entries' row operands, checked side by side -- x (rows of in_features), out and the optional residual (rows of
// out_features) -- and their workgroups of 128 rows
struct rows_ffn_io { rows_ref x; float* out; long long out_stride; rows_ref residual; long long rows, wgs; };
static int rows_ffn_prepare(rows_ffn_io* io, int in_features, int out_features) {
    int e = row_worse(row_operand(io->x.p, &io->x.stride, in_features), row_operand(io->out, &io->out_stride, out_features));
    if (io->residual.p) e = row_worse(e, row_operand(io->residual.p, &io->residual.stride, out_features));
    if (e) return e;
    io->wgs = (io->rows + 127) / 128;
    return io->wgs >= (1ll << 31) ? FBBEV_E_UNSUPPORTED : 0;
}

// The FFN pair of the encoder layer in one kernel: out = [LayerNorm](W2 relu(W1 x + b1) + b2 [+ residual]) -- mmcv FFN
// (bevformer_encoder.py:250-377 with ffn_cfgs: Linear + ReLU, Linear, add_identity) and, when ln_weight is given, the layer's
// following LayerNorm.  w1_fragments / w2_fragments = fbbev_rows_linear_x3_fragments of W1 (hidden, in) / W2 (out, hidden).
// Supported: in_features <= 96, hidden % 64 == 0, out_features <= 80 (the FB-OCC shape 80 -> 320 -> 80); FBBEV_E_UNSUPPORTED otherwise.
extern "C" int fbbev_rows_ffn_x3(const float* x, long long x_row_stride, const void* w1_fragments, const float* b1,
                                 const void* w2_fragments, const float* b2, long long rows, int in_features, int hidden,
                                 int out_features, const float* residual, long long residual_row_stride, const float* ln_weight,
                                 const float* ln_bias, float ln_eps, float* out, long long out_row_stride, fbbev_stream_t stream_) {
    if (rows < 0 || in_features <= 0 || hidden <= 0 || out_features <= 0) return FBBEV_E_BADARG;
    if (rows == 0) return 0;
    if (!x || !w1_fragments || !b1 || !w2_fragments || !b2 || !out || (ln_weight && !ln_bias)) return FBBEV_E_BADARG;
    rows_ffn_io io = {{x, x_row_stride}, out, out_row_stride, {residual, residual_row_stride}, rows, 0};
    if (const int e = rows_ffn_prepare(&io, in_features, out_features)) return e;
    if (in_features > 96 || in_features % 8 != 0 || hidden % FBBEV_FFN_HC != 0 || out_features > 80 || out_features % 4 != 0 ||
        !aligned16(w1_fragments) || !aligned16(w2_fragments) || !aligned16(b1) || !aligned16(b2) ||
        (ln_weight && (!aligned16(ln_weight) || !aligned16(ln_bias)))) return FBBEV_E_UNSUPPORTED;
    // hidden units per chunk: 32 (three workgroups per CU) measured 1.480 vs 1.508 ms for 64 in the S3 scope (profiles/r04_time_fb_ffn_hc.jsonl)
    FBBEV_KNOB_ONCE(int, hc, fbbev_env_int("FBBEV_FFN_HC", 32));   // tuning knob (the emulator tests switch the chunk)
    const int n_kc2 = (hidden + 127) / 128;
#define FBBEV_FFN(LN_, HC_)                                                                                                              \
    do {                                                                                                                                 \
        const size_t lds = (size_t)fbbev_ffn_lds_bytes<3, 5, HC_>() + (size_t)hidden * 4; /* + b1 */                                     \
        FBBEV_LAUNCH_DYN_LDS((k_rows_ffn_x3<3, 5, LN_, HC_>), io.wgs, 256, lds, (fbbev_rt_stream)stream_, x, io.x.stride,                \
                             static_cast<const unsigned short*>(w1_fragments), b1, static_cast<const unsigned short*>(w2_fragments), b2, \
                             out, io.out_stride, rows, in_features, hidden, out_features, n_kc2, residual, io.residual.stride,           \
                             ln_weight, ln_bias, ln_eps, fbbev_ffn_pre{});                                                               \
    } while (0)
    if (hc == 64) { if (ln_weight) FBBEV_FFN(true, 64); else FBBEV_FFN(false, 64); }
    else { if (ln_weight) FBBEV_FFN(true, 32); else FBBEV_FFN(false, 32); }
#undef FBBEV_FFN
    FBBEV_CHECK_LAUNCH();
    return 0;
}

// The cross-attention block's tail AND the FFN block of the encoder layer in one kernel (round 5):
//   y1  = LayerNorm0(x W0^T + b0 + residual0)                 output_proj + residual + norm   (bevformer_encoder.py:250-377, ops 'cross_attn', 'norm')
//   out = LayerNorm1(y1 + W2 relu(W1 y1 + b1) + b2)           mmcv FFN (add_identity) + norm  (ops 'ffn', 'norm')
// x (rows, E) = the attention slots, residual0 (rows, E) = the block's input rows.  Supported: E in {16, 32, 48, 64, 80}, hidden % 64 == 0.
// `pre`: the tail's operands as the kernel takes them, filled by the entry.  tokens_per_image > 0: out as planes (rows / S, embed, S).
struct rows_tail_ffn {
    rows_ref x; fbbev_ffn_pre pre;
    const void *w1_fragments, *w2_fragments; const float *b1, *b2;
    long long rows; int embed, hidden;
    const float *ln1_weight, *ln1_bias; float ln1_eps;
    float* out; long long out_stride, tokens_per_image; fbbev_rt_stream stream;
};
static int rows_tail_ffn_x3_launch(rows_tail_ffn c) {
    const int embed = c.embed, hidden = c.hidden;
    if (c.rows < 0 || embed <= 0 || hidden <= 0 || c.tokens_per_image < 0) return FBBEV_E_BADARG;
    if (c.rows == 0) return 0;
    rows_ffn_io io = {c.x, c.out, c.out_stride, {c.pre.res0, c.pre.ld_res0}, c.rows, 0};
    if (c.tokens_per_image > 0) {
        if (c.rows % c.tokens_per_image != 0) return FBBEV_E_BADARG;
        if (c.rows >= (1ll << 31) || c.tokens_per_image >= (1ll << 31)) return FBBEV_E_UNSUPPORTED;   // 32-bit row arithmetic in the store
        io.out_stride = embed;                                 // (the planes have no row stride: dense rows pass the checks below)
    }
    if (!c.x.p || !c.pre.w0f || !c.pre.b0 || !c.pre.ln0_w || !c.pre.ln0_b || !c.w1_fragments || !c.b1 || !c.w2_fragments || !c.b2 ||
        !c.ln1_weight || !c.ln1_bias || !c.out) return FBBEV_E_BADARG;
    if (const int e = rows_ffn_prepare(&io, embed, embed)) return e;
    if (embed > 80 || embed % 16 != 0 || hidden % FBBEV_FFN_HC != 0 || !aligned16(c.pre.w0f) || !aligned16(c.w1_fragments) ||
        !aligned16(c.w2_fragments) || !aligned16(c.pre.b0) || !aligned16(c.b1) || !aligned16(c.b2) || !aligned16(c.pre.ln0_w) ||
        !aligned16(c.pre.ln0_b) || !aligned16(c.ln1_weight) || !aligned16(c.ln1_bias)) return FBBEV_E_UNSUPPORTED;
    const int n_kc2 = (hidden + 127) / 128;
    c.pre.ld_res0 = io.residual.stride;
    const long long ldo = c.tokens_per_image > 0 ? -c.tokens_per_image : io.out_stride;   // the kernel takes planes as a NEGATIVE row stride: -S
    // (hidden chunks of 64 -- FBBEV_TAIL_FFN_HC=64 until round 5 -- measured no gain: 1.392 vs 1.392 ms S3; gone)
    const size_t lds = (size_t)fbbev_ffn_pre_lds_bytes<3, 5, 32>() + (size_t)hidden * 4; /* + b1 */
    FBBEV_LAUNCH_DYN_LDS((k_rows_ffn_x3<3, 5, true, 32, true>), io.wgs, 256, lds, c.stream, c.x.p, io.x.stride,
                         static_cast<const unsigned short*>(c.w1_fragments), c.b1, static_cast<const unsigned short*>(c.w2_fragments), c.b2,
                         c.out, ldo, c.rows, embed, hidden, embed, n_kc2, (const float*)nullptr, (long long)0, c.ln1_weight, c.ln1_bias,
                         c.ln1_eps, c.pre);
    FBBEV_CHECK_LAUNCH();
    return 0;
}

extern "C" int fbbev_rows_tail_ffn_x3(const float* x, long long x_row_stride, const void* w0_fragments, const float* b0,
                                      const float* residual0, long long residual0_row_stride, const float* ln0_weight,
                                      const float* ln0_bias, float ln0_eps, const void* w1_fragments, const float* b1,
                                      const void* w2_fragments, const float* b2, long long rows, int embed, int hidden,
                                      const float* ln1_weight, const float* ln1_bias, float ln1_eps, float* out,
                                      long long out_row_stride, fbbev_stream_t stream_) {
    const fbbev_ffn_pre pre = {static_cast<const unsigned short*>(w0_fragments), b0, residual0, residual0_row_stride, ln0_weight, ln0_bias, ln0_eps};
    return rows_tail_ffn_x3_launch({{x, x_row_stride}, pre, w1_fragments, w2_fragments, b1, b2, rows, embed, hidden, ln1_weight, ln1_bias,
                                    ln1_eps, out, out_row_stride, 0, (fbbev_rt_stream)stream_});
}

// The same with the result written as planes: out (rows / tokens_per_image, embed, tokens_per_image) -- the (B, C, Y, X) refined BEV
// the final pooling re-adds (backward_projection.py:129: permute + view + contiguous), without the transposing pass behind the layer.
extern "C" int fbbev_rows_tail_ffn_x3_planes(const float* x, long long x_row_stride, const void* w0_fragments, const float* b0,
                                             const float* residual0, long long residual0_row_stride, const float* ln0_weight,
                                             const float* ln0_bias, float ln0_eps, const void* w1_fragments, const float* b1,
                                             const void* w2_fragments, const float* b2, long long rows, int embed, int hidden,
                                             const float* ln1_weight, const float* ln1_bias, float ln1_eps,
                                             long long tokens_per_image, float* out, fbbev_stream_t stream_) {
    if (tokens_per_image <= 0) return FBBEV_E_BADARG;
    const fbbev_ffn_pre pre = {static_cast<const unsigned short*>(w0_fragments), b0, residual0, residual0_row_stride, ln0_weight, ln0_bias, ln0_eps};
    return rows_tail_ffn_x3_launch({{x, x_row_stride}, pre, w1_fragments, w2_fragments, b1, b2, rows, embed, hidden, ln1_weight, ln1_bias,
                                    ln1_eps, out, 0, tokens_per_image, (fbbev_rt_stream)stream_});
}

// ------------------------------------------------------------------------------ convolutions, channels-last (NDHWC)
// The shape of a convolution call: B samples, the input and the output volume.  An image is a volume of one plane.
struct conv_volume { int D, H, W, C; };
struct conv_window {
    int ksize, stride, pad;
    // stride 1 / 2, padding 0 / 1, kernel size 1 / 3 -- and 2 where `with_k2`: the fp32 3-D kernels have it, the bf16 and 2-D routes do not
    bool supported(bool with_k2) const { return (ksize == 1 || ksize == 3 || (with_k2 && ksize == 2)) && (stride == 1 || stride == 2) && pad >= 0 && pad <= 1; }
};
struct conv_dims {
    int B; conv_volume in, out;
    bool positive() const { return B >= 0 && in.D > 0 && in.H > 0 && in.W > 0 && in.C > 0 && out.D > 0 && out.H > 0 && out.W > 0 && out.C > 0; }
    static bool axis_ok(int in, int out, conv_window w) { return out == (in + 2 * w.pad - w.ksize) / w.stride + 1; }
    bool geometry_ok_planar(conv_window w) const { return axis_ok(in.H, out.H, w) && axis_ok(in.W, out.W, w); }   // the depth axis is the caller's
    bool geometry_ok(conv_window w) const { return axis_ok(in.D, out.D, w) && geometry_ok_planar(w); }
    bool same_volume() const { return out.D == in.D && out.H == in.H && out.W == in.W; }   // (the transposed route: 2x2x2 outputs per voxel)
    long long out_voxels() const { return (long long)B * out.D * out.H * out.W; }
    conv_dims swapped() const { return conv_dims{B, out, in}; }
};
// How the MFMA kernels tile a launch: mt_total 16-channel output tiles, MT of them per workgroup (4, 2 or 1: what divides mt_total),
// gy = mt_total / MT workgroups per block of output; `gx` blocks (256 voxels, or one LDS tile), `per_block` workgroup groups for each
// (8: the parities of the transposed route); pstride: weight fragment elements per tap (`cin_granule` input channels per fragment)
struct conv_tile_plan { int mt_total, MT, gy; long long gx, grid, pstride; };
static conv_tile_plan conv_tile_plan_of(const conv_dims& d, int cin_granule, long long gx, int per_block) {
    const int mt_total = (d.out.C + 15) / 16, MT = mt_total % 4 == 0 ? 4 : (mt_total % 2 == 0 ? 2 : 1), gy = mt_total / MT;
    return conv_tile_plan{mt_total, MT, gy, gx, gx * gy * per_block, (long long)(d.in.C / cin_granule) * mt_total * (16 * cin_granule)};
}
#define FBBEV_CONV_MT(mt, ...) FBBEV_POOL_WITH3(MT, mt, 4, 2, 1, __VA_ARGS__)

// One forward-kernel call (the dgrad is one too: the gather form over dy).  mode: 0 convolution, 1 transposed 2x2x2, 2 dgrad
struct conv_call {
    const float* x; const void* weights; const float *bias, *residual; float* out;
    conv_dims d; conv_window w;
    int relu, mode; bool planar, bf16;
    fbbev_rt_stream stream;
};
// what every forward entry asks of its operands once the shape is accepted and B > 0
static int conv_operands_check(const conv_call& c, int cin_granule) {
    if (!c.x || !c.weights || !c.bias || !c.out) return FBBEV_E_BADARG;
    if (c.d.in.C % cin_granule != 0 || !aligned16(c.x) || !aligned16(c.weights) || !aligned16(c.bias) || !aligned16(c.out) ||
        (c.residual && !aligned16(c.residual))) return FBBEV_E_UNSUPPORTED;
    return 0;
}
#define FBBEV_CONV_DIMS(d) (d).B, (d).in.D, (d).in.H, (d).in.W, (d).in.C, (d).out.D, (d).out.H, (d).out.W, (d).out.C   /* as the kernels take them */

// What the entries ask of a shape before anything else: positive dimensions (BADARG); the transposed route (mode 1) wants the same
// volume in and out, has no planar form and sets its own window; otherwise the window must be one the kernels have (UNSUPPORTED)
// and the geometry hold (BADARG) -- planar: one plane in, one plane out stands in for the depth axis's
static int conv_shape_check(const conv_dims& d, conv_window* w, int mode, bool planar, bool with_k2) {
    if (!d.positive()) return FBBEV_E_BADARG;
    if (mode == 1) {
        if (!d.same_volume() || planar) return FBBEV_E_BADARG;
        *w = {1, 1, 0};
        return 0;
    }
    if (!w->supported(with_k2)) return FBBEV_E_UNSUPPORTED;
    return (planar ? d.in.D == 1 && d.out.D == 1 && d.geometry_ok_planar(*w) : d.geometry_ok(*w)) ? 0 : FBBEV_E_BADARG;
}

// the per-voxel kernels, fp32 (16 input channels per weight fragment) and bf16 (32), over blocks of 256 output voxels
static int conv3d_launch(const conv_call& c) {
    if (c.d.B == 0) return 0;
    const int cin_granule = c.bf16 ? 32 : 16;
    if (const int e = conv_operands_check(c, cin_granule)) return e;
    const conv_tile_plan p = conv_tile_plan_of(c.d, cin_granule, (c.d.out_voxels() + 255) / 256, c.mode == 1 ? 8 : 1);
    if (p.grid >= (1ll << 31)) return FBBEV_E_UNSUPPORTED;
#define FBBEV_CONV3D(KERNEL, WT, KD_, KS_)                                                                                        \
    FBBEV_CONV_MT(p.MT, FBBEV_LAUNCH((KERNEL<KD_, KS_, MT>), p.grid, 256, 0, c.stream, c.x, static_cast<const WT*>(c.weights), c.bias, \
                                     c.residual, c.out, FBBEV_CONV_DIMS(c.d), p.mt_total, c.w.stride, c.w.pad, c.relu ? 1 : 0, c.mode,   \
                                     p.pstride, (int)p.gx, p.gy))
    const int k = c.w.ksize;
    if (!c.bf16) {
        if (k == 3 && c.planar) FBBEV_CONV3D(k_conv3d_ndhwc, float, 1, 3); else if (k == 3) FBBEV_CONV3D(k_conv3d_ndhwc, float, 3, 3);
        else if (k == 2) FBBEV_CONV3D(k_conv3d_ndhwc, float, 2, 2); else FBBEV_CONV3D(k_conv3d_ndhwc, float, 1, 1);
    } else {
        if (k == 3 && c.planar) FBBEV_CONV3D(k_conv3d_ndhwc_bf16, unsigned short, 1, 3); else if (k == 3) FBBEV_CONV3D(k_conv3d_ndhwc_bf16, unsigned short, 3, 3);
        else FBBEV_CONV3D(k_conv3d_ndhwc_bf16, unsigned short, 1, 1);
    }
#undef FBBEV_CONV3D
    FBBEV_CHECK_LAUNCH();
    return 0;
}

extern "C" int fbbev_conv3d_ndhwc(const float* x, const float* weight_fragments, const float* bias, const float* residual,
                                  int B, int Di, int Hi, int Wi, int Cin, int Do, int Ho, int Wo, int Cout, int ksize,
                                  int stride, int pad, int relu, int transposed, float* out, fbbev_stream_t stream_) {
    conv_call c = {x, weight_fragments, bias, residual, out, {B, {Di, Hi, Wi, Cin}, {Do, Ho, Wo, Cout}}, {ksize, stride, pad}, relu,
                   transposed ? 1 : 0, false, false, (fbbev_rt_stream)stream_};
    if (const int e = conv_shape_check(c.d, &c.w, c.mode, c.planar, true)) return e;
    return conv3d_launch(c);
}

extern "C" int fbbev_conv2d_nhwc(const float* x, const float* weight_fragments, const float* bias, const float* residual,
                                 int B, int Hi, int Wi, int Cin, int Ho, int Wo, int Cout, int ksize, int stride, int pad,
                                 int relu, float* out, fbbev_stream_t stream_) {
    // an NHWC image is an NDHWC volume with one plane; the planar instantiation has a single tap along that axis
    conv_call c = {x, weight_fragments, bias, residual, out, {B, {1, Hi, Wi, Cin}, {1, Ho, Wo, Cout}}, {ksize, stride, pad}, relu, 0, true,
                   false, (fbbev_rt_stream)stream_};
    if (const int e = conv_shape_check(c.d, &c.w, c.mode, c.planar, false)) return e;
    return conv3d_launch(c);
}

extern "C" int fbbev_conv3d_ndhwc_bf16(const float* x, const void* weight_fragments_bf16, const float* bias,
                                       const float* residual, int B, int Di, int Hi, int Wi, int Cin, int Do, int Ho, int Wo,
                                       int Cout, int ksize, int stride, int pad, int relu, int transposed, int planar,
                                       float* out, fbbev_stream_t stream_) {
    conv_call c = {x, weight_fragments_bf16, bias, residual, out, {B, {Di, Hi, Wi, Cin}, {Do, Ho, Wo, Cout}}, {ksize, stride, pad}, relu,
                   transposed ? 1 : 0, planar != 0, true, (fbbev_rt_stream)stream_};
    if (const int e = conv_shape_check(c.d, &c.w, c.mode, c.planar, false)) return e;
    return conv3d_launch(c);
}

extern "C" int fbbev_conv3d_k3s1_tiled_bf16(const float* x, const void* weight_fragments_bf16, const float* bias,
                                            const float* residual, int B, int D, int H, int W, int Cin, int Cout, int relu,
                                            float* out, fbbev_stream_t stream_) {
    const conv_call c = {x, weight_fragments_bf16, bias, residual, out, {B, {D, H, W, Cin}, {D, H, W, Cout}}};
    if (!c.d.positive()) return FBBEV_E_BADARG;
    if (B == 0) return 0;
    if (const int e = conv_operands_check(c, 32)) return e;
    const int tiles_d = (D + 3) / 4, tiles_h = (H + 7) / 8, tiles_w = (W + 7) / 8;
    const long long n_tiles = (long long)B * tiles_d * tiles_h * tiles_w;
    const conv_tile_plan p = conv_tile_plan_of(c.d, 32, (n_tiles + 7) / 8 * 8, 1);   // whole groups of 8 tiles (one per XCD), see the kernel
    if (p.grid >= (1ll << 31)) return FBBEV_E_UNSUPPORTED;
    const size_t lds = (size_t)2 * 600 * 32 * sizeof(unsigned short);
    FBBEV_CONV_MT(p.MT, FBBEV_LAUNCH_DYN_LDS((k_conv3d_k3_tile_bf16<MT>), p.grid, 512, lds, (fbbev_rt_stream)stream_, x,
                                             static_cast<const unsigned short*>(weight_fragments_bf16), bias, residual, out, B, D, H, W,
                                             Cin, Cout, p.mt_total, relu ? 1 : 0, tiles_d, tiles_h, tiles_w, p.gy));
    FBBEV_CHECK_LAUNCH();
    return 0;
}

extern "C" int fbbev_conv3d_dgrad_ndhwc(const float* dy, const float* weight_fragments_t, const float* zero_bias, int B,
                                        int Do, int Ho, int Wo, int Cout, int Di, int Hi, int Wi, int Cin, int ksize,
                                        int stride, int pad, float* dx, fbbev_stream_t stream_) {
    conv_call c = {dy, weight_fragments_t, zero_bias, nullptr, dx, {B, {Di, Hi, Wi, Cin}, {Do, Ho, Wo, Cout}}, {ksize, stride, pad}, 0, 2,
                   false, false, (fbbev_rt_stream)stream_};           // (the forward's shape, for the checks)
    if (const int e = conv_shape_check(c.d, &c.w, c.mode, c.planar, true)) return e;
    // gather form: the kernel's "input" is dy (Cout channels), its "output" voxels are those of dx (Cin channels)
    c.d = c.d.swapped();
    return conv3d_launch(c);
}

// voxel chunk per wave: enough chunks to fill the chip a few times over, at least 256 voxels (16 loop iterations)
static long long conv3d_wgrad_chunk(long long nvox) {
    long long chunk = nvox / 64;
    if (chunk < 256) chunk = 256;
    if (chunk > 4096) chunk = 4096;
    return (chunk + 15) / 16 * 16;
}
// dw += the weight gradient; `part`: the deterministic route's per-chunk partial sums (then added to dw in chunk order), null: atomics
struct conv_wgrad_call { const float *x, *dy; float *dw, *part; conv_dims d; conv_window w; fbbev_rt_stream stream; };
static int conv3d_wgrad_impl(conv_wgrad_call c) {
    const conv_dims& d = c.d;
    if (const int e = conv_shape_check(d, &c.w, 0, false, true)) return e;
    if (d.B == 0) return 0;
    if (!c.x || !c.dy || !c.dw) return FBBEV_E_BADARG;
    if (d.in.C % 4 != 0 || d.out.C % 4 != 0 || !aligned16(c.x) || !aligned16(c.dy)) return FBBEV_E_UNSUPPORTED;
    const long long nvox = d.out_voxels();
    const int cout_blocks = (d.out.C + 63) / 64, cin_blocks = (d.in.C + 63) / 64, T = c.w.ksize * c.w.ksize * c.w.ksize;
    const long long chunk = conv3d_wgrad_chunk(nvox);
    const long long n_chunks = (nvox + chunk - 1) / chunk;
    const long long tasks = n_chunks * cout_blocks * cin_blocks * T;
    const long long blocks = (tasks + 3) / 4;
    if (blocks >= (1ll << 31)) return FBBEV_E_UNSUPPORTED;
#define FBBEV_WGRAD(KS_, DET_, OUT_)                                                                                      \
    FBBEV_LAUNCH((k_conv3d_wgrad_ndhwc<KS_, DET_>), blocks, 256, 0, c.stream, c.x, c.dy, OUT_, FBBEV_CONV_DIMS(d), c.w.stride, \
                 c.w.pad, (int)chunk, (int)n_chunks, cout_blocks, cin_blocks)
    if (c.part) {
        if (c.w.ksize == 3) FBBEV_WGRAD(3, true, c.part); else if (c.w.ksize == 2) FBBEV_WGRAD(2, true, c.part); else FBBEV_WGRAD(1, true, c.part);
        FBBEV_CHECK_LAUNCH();
        const long long n = (long long)T * d.out.C * d.in.C;
        long long g = (n + 255) / 256;
        g = g > 4096 ? 4096 : g;
        FBBEV_LAUNCH(k_sum_chunks_add, g, 256, 0, c.stream, (const float*)c.part, (int)n_chunks, n, c.dw);
    } else {
        if (c.w.ksize == 3) FBBEV_WGRAD(3, false, c.dw); else if (c.w.ksize == 2) FBBEV_WGRAD(2, false, c.dw); else FBBEV_WGRAD(1, false, c.dw);
    }
#undef FBBEV_WGRAD
    FBBEV_CHECK_LAUNCH();
    return 0;
}

extern "C" int fbbev_conv3d_wgrad_ndhwc(const float* x, const float* dy, int B, int Di, int Hi, int Wi, int Cin, int Do,
                                        int Ho, int Wo, int Cout, int ksize, int stride, int pad, float* dw,
                                        fbbev_stream_t stream_) {
    return conv3d_wgrad_impl({x, dy, dw, nullptr, {B, {Di, Hi, Wi, Cin}, {Do, Ho, Wo, Cout}}, {ksize, stride, pad}, (fbbev_rt_stream)stream_});
}
extern "C" size_t fbbev_conv3d_wgrad_ws_bytes(int B, int Do, int Ho, int Wo, int Cin, int Cout, int ksize, int flags) {
    if (!(flags & FBBEV_FLAG_DETERMINISTIC) || B <= 0 || Do <= 0 || Ho <= 0 || Wo <= 0 || Cin <= 0 || Cout <= 0 || ksize <= 0) return 0;
    const long long nvox = (long long)B * Do * Ho * Wo, chunk = conv3d_wgrad_chunk(nvox);
    return (size_t)((nvox + chunk - 1) / chunk) * ksize * ksize * ksize * Cout * Cin * sizeof(float);
}
extern "C" int fbbev_conv3d_wgrad_ndhwc_ex(const float* x, const float* dy, int B, int Di, int Hi, int Wi, int Cin, int Do, int Ho,
                                           int Wo, int Cout, int ksize, int stride, int pad, float* dw, int flags, void* ws,
                                           size_t ws_bytes, fbbev_stream_t stream_) {
    conv_wgrad_call c = {x, dy, dw, nullptr, {B, {Di, Hi, Wi, Cin}, {Do, Ho, Wo, Cout}}, {ksize, stride, pad}, (fbbev_rt_stream)stream_};
    if (!(flags & FBBEV_FLAG_DETERMINISTIC)) return conv3d_wgrad_impl(c);
    if (B == 0) return 0;
    if (!ws) return FBBEV_E_BADARG;
    if (ws_bytes < fbbev_conv3d_wgrad_ws_bytes(B, Do, Ho, Wo, Cin, Cout, ksize, flags)) return FBBEV_E_WORKSPACE;
    c.part = static_cast<float*>(ws);
    return conv3d_wgrad_impl(c);
}

extern "C" int fbbev_blend_levels_ndhwc(const float* level0, const float* const* coarse, const int* coarse_dims,
                                        int n_coarse, const float* wsoft, int K, int B, int D, int H, int W, int C,
                                        float* out, fbbev_stream_t stream_) {
    if (B < 0 || D <= 0 || H <= 0 || W <= 0 || C <= 0 || n_coarse < 0 || n_coarse > 3 || K < n_coarse + 1) return FBBEV_E_BADARG;
    if (B == 0) return 0;
    if (!level0 || !wsoft || !out || (n_coarse > 0 && (!coarse || !coarse_dims))) return FBBEV_E_BADARG;
    if (C % 4 != 0 || !aligned16(level0) || !aligned16(out)) return FBBEV_E_UNSUPPORTED;
    fbbev_blend_level lv[3] = {{nullptr, 1, 1, 1}, {nullptr, 1, 1, 1}, {nullptr, 1, 1, 1}};
    for (int k = 0; k < n_coarse; ++k) {
        if (!coarse[k] || coarse_dims[3 * k] <= 0 || coarse_dims[3 * k + 1] <= 0 || coarse_dims[3 * k + 2] <= 0) return FBBEV_E_BADARG;
        if (!aligned16(coarse[k])) return FBBEV_E_UNSUPPORTED;
        lv[k] = fbbev_blend_level{coarse[k], coarse_dims[3 * k], coarse_dims[3 * k + 1], coarse_dims[3 * k + 2]};
    }
    const long long total = (long long)B * D * H * W * (C / 4);
    long long blocks = (total + 255) / 256;
    if (blocks > 262144) blocks = 262144;
    FBBEV_LAUNCH(k_blend_levels_ndhwc, blocks, 256, 0, (fbbev_rt_stream)stream_, level0, lv[0], lv[1], lv[2], n_coarse, wsoft, K,
                 B, D, H, W, C, out);
    FBBEV_CHECK_LAUNCH();
    return 0;
}

// ------------------------------------------------------------------------------ occupancy classes + mIoU confusion matrix
extern "C" int fbbev_occ_classes(const float* logits, long long stride_b, long long stride_c, long long stride_h, long long stride_w,
                                 long long stride_d, int B, int C, int c0, int H, int W, int D, uint8_t* classes, const uint8_t* gt,
                                 const uint8_t* mask, const uint8_t* column_mask, int32_t* hist, fbbev_stream_t stream_) {
    if (!logits || !classes || B < 0 || C <= 0 || H <= 0 || W <= 0 || D <= 0 || c0 < 0) return FBBEV_E_BADARG;
    if (!gt && (mask || column_mask || hist)) return FBBEV_E_BADARG;
    if (B == 0) return 0;
    const int n = C - c0;
    if (n < 2 || n > 32 || (long long)B * H * W * D >= (1ll << 31)) return FBBEV_E_UNSUPPORTED;
    // tile: TD depth cells (the whole depth up to 64) x T x T columns, <= FBBEV_OCC_TILE_VOXELS voxels
    const int TD = D < 64 ? D : 64, T = TD >= 16 ? 8 : 16;
    const int nth = (H + T - 1) / T, ntw = (W + T - 1) / T, ntd = (D + TD - 1) / TD;
    const long long ntiles = (long long)B * nth * ntw * ntd;
    // channels-last (a voxel's logits contiguous, voxels C apart along d) goes through LDS while 256 rows fit in 40 KiB
    const int staged = (stride_c == 1 && stride_d == C && C <= 40) ? 1 : 0;
    const int row_runs = (staged && TD == D && stride_w == (long long)D * C) ? 1 : 0;
    auto aligned4 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; };
    const int vec4 = (D % 4 == 0 && aligned4(classes) && aligned4(gt) && aligned4(mask)) ? 1 : 0;
    const size_t lds = (staged ? (size_t)FBBEV_OCC_THREADS * C * 4 : 0) + (size_t)n * n * 4 + FBBEV_OCC_TILE_VOXELS;
    const long long blocks = ntiles < 1536 ? ntiles : 1536;          // six workgroups per CU resident: one wave of workgroups
#define FBBEV_OCC_LAUNCH(S, V)                                                                                                          \
    FBBEV_LAUNCH((k_occ_classes<S, V>), blocks, FBBEV_OCC_THREADS, lds, (fbbev_rt_stream)stream_, logits, stride_b, stride_c, stride_h, \
                 stride_w, stride_d, C, c0, H, W, D, T, TD, nth, ntw, ntd, (int)ntiles, row_runs, classes, gt, mask, column_mask, hist)
    if (staged && vec4) FBBEV_OCC_LAUNCH(true, true);
    else if (staged) FBBEV_OCC_LAUNCH(true, false);
    else if (vec4) FBBEV_OCC_LAUNCH(false, true);
    else FBBEV_OCC_LAUNCH(false, false);
#undef FBBEV_OCC_LAUNCH
    FBBEV_CHECK_LAUNCH();
    return 0;
}

// ------------------------------------------------------------------------------ occupancy F-score: the four counts of a frame
extern "C" int fbbev_occ_fscore_counts(const uint8_t* classes, const uint8_t* gt, const uint8_t* mask, const uint32_t* void_bits,
                                       const double* sq_x, const double* sq_y, const double* sq_z, const int32_t* offsets, int n_off,
                                       int R, double T_acc, double T_cmpl, int B, int X, int Y, int Z, int32_t* counts,
                                       fbbev_stream_t stream_) {
    if (!classes || !gt || !void_bits || !sq_x || !sq_y || !sq_z || !offsets || !counts) return FBBEV_E_BADARG;
    if (B < 0 || X <= 0 || Y <= 0 || Z <= 0 || R < 0 || n_off <= 0) return FBBEV_E_BADARG;
    if (B == 0) return 0;
    if (Z > FBBEV_OCCF_MAX_Z || R > FBBEV_OCCF_MAX_R || X > (1 << 30) || Y > (1 << 30)) return FBBEV_E_UNSUPPORTED;
    long long nvox = B;                                  // factor by factor: each is below 2^31, so no product leaves 64 bits
    for (const int f : {X, Y, Z}) {
        nvox *= f;
        if (nvox >= (1ll << 31)) return FBBEV_E_UNSUPPORTED;
    }
    fbbev_occf_void vb;
    for (int i = 0; i < 8; ++i) vb.w[i] = void_bits[i];
    const int ntx = (X + FBBEV_OCCF_TILE - 1) / FBBEV_OCCF_TILE, nty = (Y + FBBEV_OCCF_TILE - 1) / FBBEV_OCCF_TILE;
    const long long blocks = (long long)B * ntx * nty;
    auto aligned4 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; };
    const int vec4 = (Z % 4 == 0 && aligned4(classes) && aligned4(gt) && aligned4(mask)) ? 1 : 0;
    const size_t lds = fbbev_occf_lds_bytes(R, Z);
#define FBBEV_OCCF_LAUNCH(V)                                                                                                          \
    FBBEV_LAUNCH((k_occ_fscore<V>), blocks, FBBEV_OCCF_THREADS, lds, (fbbev_rt_stream)stream_, classes, gt, mask, vb, sq_x, sq_y, sq_z, \
                 offsets, n_off, R, T_acc, T_cmpl, X, Y, Z, ntx, nty, counts)
    if (vec4) FBBEV_OCCF_LAUNCH(true);
    else FBBEV_OCCF_LAUNCH(false);
#undef FBBEV_OCCF_LAUNCH
    FBBEV_CHECK_LAUNCH();
    return 0;
}

// ------------------------------------------------------------------------------ occupancy voxel losses: statistics + gradient
namespace {
struct occl_plan {
    int T, TD, nth, ntw, ntd, staged, row_runs;
    long long ntiles, blocks;
};
// the tile walk of fbbev_occ_classes; the grid is a function of the shape alone (the workgroup records are added in grid order)
occl_plan occl_plan_of(long long stride_c, long long stride_w, long long stride_d, int B, int C, int H, int W, int D) {
    occl_plan p;
    p.TD = D < 64 ? D : 64;
    p.T = p.TD >= 16 ? 8 : 16;
    p.nth = (H + p.T - 1) / p.T; p.ntw = (W + p.T - 1) / p.T; p.ntd = (D + p.TD - 1) / p.TD;
    p.ntiles = (long long)B * p.nth * p.ntw * p.ntd;
    p.blocks = p.ntiles < FBBEV_OCCL_MAX_BLOCKS ? p.ntiles : FBBEV_OCCL_MAX_BLOCKS;
    p.staged = (stride_c == 1 && stride_d == C) ? 1 : 0;
    p.row_runs = (p.staged && p.TD == D && stride_w == (long long)D * C) ? 1 : 0;
    return p;
}
// the checks both entries share; 1 = nothing to do (B == 0)
int occl_check(const void* logits, int B, int C, int H, int W, int D, const void* labels, const void* plane_weight, int empty_idx,
               int flags, const void* a, const void* b) {
    if (!logits || !labels || !a || !b || B < 0 || C <= 0 || H <= 0 || W <= 0 || D <= 0) return FBBEV_E_BADARG;
    if (empty_idx < 0 || empty_idx >= C || ((flags & FBBEV_OCC_LOSS_FOCAL) && !plane_weight)) return FBBEV_E_BADARG;
    if (B == 0) return 1;
    if (C < 2 || C > 32) return FBBEV_E_UNSUPPORTED;
    long long nvox = B;                                  // factor by factor: each is below 2^31, so no product leaves 64 bits
    for (const int f : {H, W, D}) {
        nvox *= f;
        if (nvox >= (1ll << 31)) return FBBEV_E_UNSUPPORTED;
    }
    return 0;
}
}  // namespace

extern "C" size_t fbbev_occ_loss_ws_bytes(int B, int C, int H, int W, int D) {
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || D <= 0) return 0;
    const occl_plan p = occl_plan_of(0, 0, 0, B, C, H, W, D);
    return align_up((size_t)p.blocks * (3 * C + 4) * sizeof(float), 16) + align_up((size_t)p.blocks * (C + 1) * sizeof(int32_t), 16);
}

extern "C" int fbbev_occ_loss_stats(const float* logits, long long stride_b, long long stride_c, long long stride_h, long long stride_w,
                                    long long stride_d, int B, int C, int H, int W, int D, const uint8_t* labels,
                                    const float* class_weight, const float* plane_weight, int empty_idx, int flags, float gamma,
                                    float alpha, float* stats_f, int32_t* stats_i, void* ws, size_t ws_bytes, fbbev_stream_t stream_) {
    if (B > 0 && !ws) return FBBEV_E_BADARG;
    const int chk = occl_check(logits, B, C, H, W, D, labels, plane_weight, empty_idx, flags, stats_f, stats_i);
    if (chk < 0) return chk;
    if (chk == 1) {
        int e = fbbev_rt_memset_async(stats_f, 0, (size_t)(3 * C + 4) * sizeof(float), (fbbev_rt_stream)stream_);
        if (!e) e = fbbev_rt_memset_async(stats_i, 0, (size_t)(C + 1) * sizeof(int32_t), (fbbev_rt_stream)stream_);
        return e;
    }
    if (ws_bytes < fbbev_occ_loss_ws_bytes(B, C, H, W, D) || !aligned16(ws)) return FBBEV_E_WORKSPACE;
    const occl_plan p = occl_plan_of(stride_c, stride_w, stride_d, B, C, H, W, D);
    float* part_f = static_cast<float*>(ws);
    int* part_i = reinterpret_cast<int*>(static_cast<char*>(ws) + align_up((size_t)p.blocks * (3 * C + 4) * sizeof(float), 16));
    const size_t lds = ((size_t)FBBEV_OCCL_THREADS * C + 2 * FBBEV_OCCL_THREADS + C) * 4;
    const int focal = flags & FBBEV_OCC_LOSS_FOCAL;
#define FBBEV_OCCL_LAUNCH(S)                                                                                                              \
    FBBEV_LAUNCH((k_occ_loss_stats<S>), p.blocks, FBBEV_OCCL_THREADS, lds, (fbbev_rt_stream)stream_, logits, stride_b, stride_c, stride_h, \
                 stride_w, stride_d, C, H, W, D, p.T, p.TD, p.nth, p.ntw, p.ntd, (int)p.ntiles, p.row_runs, labels, class_weight,         \
                 plane_weight, empty_idx, focal, gamma, alpha, part_f, part_i)
    if (p.staged) FBBEV_OCCL_LAUNCH(true);
    else FBBEV_OCCL_LAUNCH(false);
#undef FBBEV_OCCL_LAUNCH
    FBBEV_CHECK_LAUNCH();
    const size_t lds_reduce = (size_t)FBBEV_OCCL_REDUCE_CHUNK * (4 * C + 5) * 4;          // a chunk of float and int records
    FBBEV_LAUNCH(k_occ_loss_reduce, 1, FBBEV_OCCL_THREADS, lds_reduce, (fbbev_rt_stream)stream_, part_f, part_i, (int)p.blocks, C,
                 stats_f, stats_i);
    FBBEV_CHECK_LAUNCH();
    return 0;
}

extern "C" int fbbev_occ_loss_grad(const float* logits, long long stride_b, long long stride_c, long long stride_h, long long stride_w,
                                   long long stride_d, int B, int C, int H, int W, int D, const uint8_t* labels,
                                   const float* class_weight, const float* plane_weight, int empty_idx, int flags, float gamma,
                                   float alpha, const float* grad_stats, float* grad_logits, fbbev_stream_t stream_) {
    const int chk = occl_check(logits, B, C, H, W, D, labels, plane_weight, empty_idx, flags, grad_stats, grad_logits);
    if (chk < 0) return chk;
    if (chk == 1) return 0;
    const occl_plan p = occl_plan_of(stride_c, stride_w, stride_d, B, C, H, W, D);
    const size_t lds = ((size_t)FBBEV_OCCL_THREADS * C + 4 * C + 4) * 4;
    const int focal = flags & FBBEV_OCC_LOSS_FOCAL;
    const long long blocks = p.ntiles < 2048 ? p.ntiles : 2048;     // nothing is added across workgroups here: any grid gives the same bits
#define FBBEV_OCCL_LAUNCH(S)                                                                                                           \
    FBBEV_LAUNCH((k_occ_loss_grad<S>), blocks, FBBEV_OCCL_THREADS, lds, (fbbev_rt_stream)stream_, logits, stride_b, stride_c, stride_h, \
                 stride_w, stride_d, C, H, W, D, p.T, p.TD, p.nth, p.ntw, p.ntd, (int)p.ntiles, p.row_runs, labels, class_weight,      \
                 plane_weight, empty_idx, focal, gamma, alpha, grad_stats, grad_logits)
    if (p.staged) FBBEV_OCCL_LAUNCH(true);
    else FBBEV_OCCL_LAUNCH(false);
#undef FBBEV_OCCL_LAUNCH
    FBBEV_CHECK_LAUNCH();
    return 0;
}

// the training-path entries live in their own translation unit (capi_train.hip: a header-only edit there recompiles in seconds); the
// CPU emulator build (tests/emu) is ONE translation unit and takes them from here
#ifdef FBBEV_TEST_OVERRIDES
#include "capi_train.hip"
#endif
