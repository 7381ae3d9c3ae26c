// capi_train.hip -- extern "C" entry points of the training path added in round 6 (include/fbbev.h): their own translation unit of
// libfbbev_hip.so, so that an edit of these kernels recompiles in seconds; the CPU emulator build includes this file from capi.hip.
#include <stdio.h>
#include <stdlib.h>
#include "rt.h"
#include "capi_common.h"
#include "wgrad_kernels.h"
#include "rows_wgrad_f32_kernels.h"
#include "occ_lovasz_kernels.h"
#include "depth_loss_kernels.h"
#include "points_depth_kernels.h"
#include "image_prep_kernels.h"
#include "../../include/fbbev.h"

// ------------------------------------------------------------------------------ weight / bias gradient of a row-wise linear layer
struct wgrad_plan { int nti, n_oc, n_ic, ksteps, kps, n_split, amt; size_t part_w, part_b, total; };

static bool wgrad_plan_make(long long rows, int I, int O, wgrad_plan* p) {
    if (rows <= 0 || I <= 0 || O <= 0 || I % 4 != 0 || O % 4 != 0) return false;
    const long long ks = (rows + 31) / 32;
    if (ks >= (1ll << 30)) return false;
    p->nti = I <= 80 ? 5 : 8;
    p->n_oc = (O + 127) / 128;
    p->n_ic = (I + 16 * p->nti - 1) / (16 * p->nti);
    p->ksteps = (int)ks;
    // enough workgroups to fill the chip twice, few enough partial results that the fixed-order reduction stays small
    p->amt = O >= 128 ? 8 : (O + 15) / 16;
    // (768 workgroups for the narrow layers -- three per CU at their 41 KB of LDS -- measured slower than 256: 48.8 -> 54.8 us at 80 x 80)
    long long want = 512 / ((long long)p->n_oc * p->n_ic);
    // tuning knob (FBBEV_KNOB_ONCE: the emulator's tests switch it inside one process)
    FBBEV_KNOB_ONCE(int, env_split, fbbev_env_int("FBBEV_WGRAD_SPLITS", 0));
    if (env_split > 0) want = env_split;
    if (want < 8) want = 8;
    if (want > 256) want = 256;
    if (want > ks) want = ks;
    p->kps = (int)((ks + want - 1) / want);
    p->n_split = (int)((ks + p->kps - 1) / p->kps);
    p->part_w = 0;
    p->part_b = align_up((size_t)p->n_split * O * I * sizeof(float), 256);
    p->total = p->part_b + align_up((size_t)p->n_split * O * sizeof(float), 256);
    return true;
}

extern "C" size_t fbbev_rows_wgrad_x3_ws_bytes(long long rows, int in_features, int out_features) {
    wgrad_plan p;
    return wgrad_plan_make(rows, in_features, out_features, &p) ? p.total : 0;
}

extern "C" int fbbev_rows_wgrad_x3(const float* grad_out, long long ld_grad, const float* x, long long ldx, const float* x_addend,
                                   long long addend_row_stride, long long addend_period, long long rows, int in_features,
                                   int out_features, float* grad_weight, float* grad_bias, void* workspace, size_t workspace_bytes,
                                   fbbev_stream_t stream_) {
    const int I = in_features, O = out_features;
    if (rows < 0 || I <= 0 || O <= 0) return FBBEV_E_BADARG;
    if (!grad_weight) return FBBEV_E_BADARG;
    fbbev_rt_stream stream = (fbbev_rt_stream)stream_;
    if (rows == 0) {
        int e = fbbev_rt_memset_async(grad_weight, 0, (size_t)O * I * sizeof(float), stream);
        if (!e && grad_bias) e = fbbev_rt_memset_async(grad_bias, 0, (size_t)O * sizeof(float), stream);
        return e;
    }
    if (!grad_out || !x) return FBBEV_E_BADARG;
    const int e_rows = row_worse(row_operand(grad_out, &ld_grad, O), row_operand(x, &ldx, I));
    if (e_rows == FBBEV_E_BADARG) return e_rows;
    if (x_addend) {
        if (addend_period <= 0 || addend_period >= (1ll << 31)) return FBBEV_E_BADARG;
        if (const int e = row_operand(x_addend, &addend_row_stride, I)) return e;
    } else {
        addend_period = 1;
    }
    wgrad_plan p;
    if (!wgrad_plan_make(rows, I, O, &p) || e_rows) return FBBEV_E_UNSUPPORTED;   // (the addend's checks come before these two operands' alignment)
    if (!workspace || !aligned16(workspace) || workspace_bytes < p.total) return FBBEV_E_WORKSPACE;
    float* part_w = reinterpret_cast<float*>(static_cast<char*>(workspace) + p.part_w);
    float* part_b = grad_bias ? reinterpret_cast<float*>(static_cast<char*>(workspace) + p.part_b) : nullptr;
    const long long wgs = (long long)p.n_split * p.n_oc * p.n_ic;
    if (wgs >= (1ll << 31)) return FBBEV_E_UNSUPPORTED;
    const size_t lds = (size_t)2 * (p.amt + p.nti) * FBBEV_WG_TILE_DW * 4;
#define FBBEV_WGRAD_LAUNCH(NTI_, ADD_)                                                                                                 \
    FBBEV_LAUNCH_DYN_LDS((k_rows_wgrad_x3<NTI_, ADD_>), wgs, 256, lds, stream, grad_out, ld_grad, x, ldx, x_addend, addend_row_stride, \
                         (int)addend_period, rows, O, I, p.n_oc, p.n_ic, p.ksteps, p.kps, p.amt, part_w, part_b)
    if (p.nti == 5) { if (x_addend) FBBEV_WGRAD_LAUNCH(5, true); else FBBEV_WGRAD_LAUNCH(5, false); }
    else { if (x_addend) FBBEV_WGRAD_LAUNCH(8, true); else FBBEV_WGRAD_LAUNCH(8, false); }
#undef FBBEV_WGRAD_LAUNCH
    FBBEV_CHECK_LAUNCH();
    const long long OI = (long long)O * I, total = OI + (grad_bias ? O : 0);
    FBBEV_LAUNCH(k_rows_wgrad_reduce<8>, (total + 31) / 32, 256, 0, stream, (const float*)part_w, (const float*)part_b, p.n_split, OI,
                 O, grad_weight, grad_bias);
    FBBEV_CHECK_LAUNCH();
    return 0;
}

// ------------------------------------------------------------------------------ the same gradients in exact fp32 (FP32 MFMA)
struct wgf_plan { int L, S, n_oc, n_ic; long long items; size_t part_b, total; };

static bool wgf_plan_make(long long rows, int I, int O, wgf_plan* p) {
    if (rows <= 0 || I <= 0 || O <= 0 || I % 8 != 0 || O % 8 != 0) return false;
    const long long L = fbbev_rows_wgrad_f32_slice(rows, I, O), S = (rows + L - 1) / L;
    p->n_oc = (O + 16 * FBBEV_WGF_TO - 1) / (16 * FBBEV_WGF_TO);
    p->n_ic = (I + 16 * FBBEV_WGF_TI - 1) / (16 * FBBEV_WGF_TI);
    p->items = S * p->n_oc * p->n_ic;
    if (S >= (1ll << 31) || p->items + 3 >= (1ll << 32)) return false;                    // (the kernel decodes the item in 32 bits)
    p->L = (int)L;
    p->S = (int)S;
    p->part_b = align_up((size_t)S * O * I * sizeof(float), 256);
    p->total = p->part_b + align_up((size_t)S * O * sizeof(float), 256);
    return true;
}

extern "C" long long fbbev_rows_wgrad_f32_slice_rows(long long rows, int in_features, int out_features) {
    if (rows < 0 || in_features <= 0 || out_features <= 0) return FBBEV_E_BADARG;
    if (in_features % 8 != 0 || out_features % 8 != 0) return FBBEV_E_UNSUPPORTED;
    return fbbev_rows_wgrad_f32_slice(rows, in_features, out_features);
}

extern "C" size_t fbbev_rows_wgrad_f32_ws_bytes(long long rows, int in_features, int out_features) {
    wgf_plan p;
    return wgf_plan_make(rows, in_features, out_features, &p) ? p.total : 0;
}

extern "C" int fbbev_rows_wgrad_f32(const float* grad_out, long long ld_grad, const float* x, long long ldx, long long rows,
                                    int in_features, int out_features, float* grad_weight, float* grad_bias, void* workspace,
                                    size_t workspace_bytes, fbbev_stream_t stream_) {
    const int I = in_features, O = out_features;
    if (rows < 0 || I <= 0 || O <= 0 || ld_grad < 0 || ldx < 0) return FBBEV_E_BADARG;
    if (!grad_weight || (rows > 0 && (!grad_out || !x))) return FBBEV_E_BADARG;
    int e_rows = 0;
    if (rows > 0) {
        e_rows = row_worse(row_operand(grad_out, &ld_grad, O), row_operand(x, &ldx, I));
        if (e_rows == FBBEV_E_BADARG) return e_rows;
    }
    if (I % 8 != 0 || O % 8 != 0 || e_rows || !aligned16(grad_weight) || (grad_bias && !aligned16(grad_bias))) return FBBEV_E_UNSUPPORTED;
    fbbev_rt_stream stream = (fbbev_rt_stream)stream_;
    if (rows == 0) {
        int e = fbbev_rt_memset_async(grad_weight, 0, (size_t)O * I * sizeof(float), stream);
        if (!e && grad_bias) e = fbbev_rt_memset_async(grad_bias, 0, (size_t)O * sizeof(float), stream);
        return e;
    }
    wgf_plan p;
    if (!wgf_plan_make(rows, I, O, &p)) return FBBEV_E_UNSUPPORTED;
    if (!workspace || !aligned16(workspace) || workspace_bytes < p.total) return FBBEV_E_WORKSPACE;
    float* part_w = reinterpret_cast<float*>(workspace);
    float* part_b = grad_bias ? reinterpret_cast<float*>(static_cast<char*>(workspace) + p.part_b) : nullptr;
    FBBEV_LAUNCH(k_rows_wgrad_f32<FBBEV_WGF_DEPTH>, (p.items + 3) / 4, 256, 0, stream, grad_out, ld_grad, x, ldx, rows, O, I, p.L, p.n_oc,
                 p.n_ic, (unsigned int)p.items, part_w, part_b);
    FBBEV_CHECK_LAUNCH();
    const long long OI = (long long)O * I, total = OI + (grad_bias ? O : 0);
    FBBEV_LAUNCH(k_rows_wgrad_f32_reduce<8>, (total + 255) / 256, 256, 0, stream, (const float*)part_w, (const float*)part_b, p.S, OI, O,
                 grad_weight, grad_bias);
    FBBEV_CHECK_LAUNCH();
    return 0;
}

// out (N) = sum over the leading dimension of x (B, N) [+ x2 (B, N)], ascending b
extern "C" int fbbev_sum_leading(const float* x, const float* x2, int B, long long N, float* out, fbbev_stream_t stream_) {
    if (B <= 0 || N < 0) return FBBEV_E_BADARG;
    if (N == 0) return 0;
    if (!x || !out) return FBBEV_E_BADARG;
    if (N % 4 != 0 || !aligned16(x) || !aligned16(out) || (x2 && !aligned16(x2))) return FBBEV_E_UNSUPPORTED;
    const long long n4 = N / 4;
    if ((n4 + 255) / 256 >= (1ll << 31)) return FBBEV_E_UNSUPPORTED;
    FBBEV_LAUNCH(k_sum_leading<0>, (n4 + 255) / 256, 256, 0, (fbbev_rt_stream)stream_, x, x2, B, n4, reinterpret_cast<fbbev_v4f*>(out));
    FBBEV_CHECK_LAUNCH();
    return 0;
}

// out (len) = sum over the n rows of part (n, len), fixed association (32 lanes each adding every 32nd row in ascending order, lane sums
// added in lane order): the per-workgroup partial parameter gradients of fbbev_layernorm_bwd -- ATen's reduction over the leading
// dimension of a (2048, 160) tensor is one latency chain per column (79 us per LayerNorm at 160 000 rows)
extern "C" int fbbev_sum_partials(const float* part, int n, long long len, float* out, fbbev_stream_t stream_) {
    if (n <= 0 || len < 0) return FBBEV_E_BADARG;
    if (len == 0) return 0;
    if (!part || !out) return FBBEV_E_BADARG;
    FBBEV_LAUNCH(k_rows_wgrad_reduce<32>, (len + 31) / 32, 1024, 0, (fbbev_rt_stream)stream_, part, (const float*)nullptr, n, len, 0, out,
                 (float*)nullptr);
    FBBEV_CHECK_LAUNCH();
    return 0;
}

// diagnostics (tools/dbg_store_policy.py): fill n floats with 16-byte stores of cache policy `policy` (fbbev_store4: 0 plain, 1 nt, 2 sc1,
// 3 sc0 sc1, 4 sc1 nt, 5 sc0 nt, 6 sc0 sc1 nt, 7 sc0) -- what a kernel's stores leave behind for the NEXT kernel's store stream
template <int ST>
__global__ void __launch_bounds__(256)
k_diag_fill(float* __restrict__ p, long long n4, float v) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256)
        fbbev_store4<ST>(p + 4 * i, fbbev_v4f{v, v, v, v});
}
extern "C" int fbbev_diag_fill(float* p, long long n, int policy, fbbev_stream_t stream_) {
    if (!p || n < 0 || n % 4 != 0 || policy < 0 || policy > 7 || !aligned16(p)) return FBBEV_E_BADARG;
    if (n == 0) return 0;
    const long long n4 = n / 4;
    long long blocks = (n4 + 255) / 256;
    if (blocks > 256 * 32) blocks = 256 * 32;
    fbbev_rt_stream stream = (fbbev_rt_stream)stream_;
    switch (policy) {
    case 0: FBBEV_LAUNCH(k_diag_fill<0>, blocks, 256, 0, stream, p, n4, 1.f); break;
    case 1: FBBEV_LAUNCH(k_diag_fill<1>, blocks, 256, 0, stream, p, n4, 1.f); break;
    case 2: FBBEV_LAUNCH(k_diag_fill<2>, blocks, 256, 0, stream, p, n4, 1.f); break;
    case 3: FBBEV_LAUNCH(k_diag_fill<3>, blocks, 256, 0, stream, p, n4, 1.f); break;
    case 4: FBBEV_LAUNCH(k_diag_fill<4>, blocks, 256, 0, stream, p, n4, 1.f); break;
    case 5: FBBEV_LAUNCH(k_diag_fill<5>, blocks, 256, 0, stream, p, n4, 1.f); break;
    case 6: FBBEV_LAUNCH(k_diag_fill<6>, blocks, 256, 0, stream, p, n4, 1.f); break;
    default: FBBEV_LAUNCH(k_diag_fill<7>, blocks, 256, 0, stream, p, n4, 1.f); break;
    }
    FBBEV_CHECK_LAUNCH();
    return 0;
}

// ------------------------------------------------------------------------------ read-ahead of a kernel's gather sources
// The dense pooling kernel at the END of the forward-backward step gathers through index tensors, depth and feature rows that were
// written ~1 ms and ~0.7 GB of intermediate traffic earlier: they have left the 256 MB memory-side cache, and the kernel's dependent
// gather chains run at HBM latency (tools/dbg_pool_in_step.py: 260 us cold, 176 us with the ~30 MB of sources read once right before).
// fbbev_touch reads up to 8 spans with 16-byte loads and discards them: the lines are back in the memory-side cache (and the L2s) when
// the gathers start.
struct fbbev_touch_spans { const char* p[8]; unsigned long long n16[8]; };
template <int UNUSED>
__global__ void __launch_bounds__(256)
k_touch(fbbev_touch_spans sp, int n) {
    fbbev_v4u acc = {0u, 0u, 0u, 0u};
    for (int k = 0; k < n; ++k) {
        const fbbev_v4u* q = reinterpret_cast<const fbbev_v4u*>(sp.p[k]);
        for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < sp.n16[k]; i += (unsigned long long)gridDim.x * 256) {
            const fbbev_v4u v = q[i];
            acc[0] |= v[0]; acc[1] |= v[1]; acc[2] |= v[2]; acc[3] |= v[3];
        }
    }
    fbbev_opaque_u32(acc[0] | acc[1] | acc[2] | acc[3]);                                 // the loads are used; nothing is stored
}
extern "C" int fbbev_touch(const void* const* spans, const size_t* bytes, int n, fbbev_stream_t stream_) {
    if (n < 0 || n > 8 || (n > 0 && (!spans || !bytes))) return FBBEV_E_BADARG;
    fbbev_touch_spans sp;
    unsigned long long total = 0;
    int m = 0;
    for (int k = 0; k < n; ++k) {
        if (!spans[k] || bytes[k] < 16) continue;
        const uintptr_t a = (reinterpret_cast<uintptr_t>(spans[k]) + 15u) & ~(uintptr_t)15u;      // whole 16-byte pieces inside the span
        const size_t skip = a - reinterpret_cast<uintptr_t>(spans[k]);
        sp.p[m] = reinterpret_cast<const char*>(a);
        sp.n16[m] = (bytes[k] - skip) / 16;
        total += sp.n16[m];
        ++m;
    }
    if (m == 0 || total == 0) return 0;
    unsigned long long blocks = (total + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    FBBEV_LAUNCH(k_touch<0>, blocks, 256, 0, (fbbev_rt_stream)stream_, sp, m);
    FBBEV_CHECK_LAUNCH();
    return 0;
}

// softmax over groups of `group` consecutive floats and its backward (the attention weights of the deformable attentions, training)
template <bool BWD>
static int softmax_groups_launch(const float* a, const float* b, long long n_groups, int group, float* out, fbbev_stream_t stream_) {
    if (n_groups < 0 || group <= 0) return FBBEV_E_BADARG;
    if (n_groups == 0) return 0;
    if (!a || !out || (BWD && !b)) return FBBEV_E_BADARG;
    if (!(group == 4 || group == 8 || group == 16 || group == 32) || !aligned16(a) || !aligned16(out) || (b && !aligned16(b)))
        return FBBEV_E_UNSUPPORTED;
    const long long n4 = n_groups * (group / 4), blocks = (n4 + 255) / 256;
    if (blocks >= (1ll << 31)) return FBBEV_E_UNSUPPORTED;
    fbbev_rt_stream stream = (fbbev_rt_stream)stream_;
    switch (group) {
    case 4: FBBEV_LAUNCH((k_softmax_groups<4, BWD>), blocks, 256, 0, stream, a, b, n4, out); break;
    case 8: FBBEV_LAUNCH((k_softmax_groups<8, BWD>), blocks, 256, 0, stream, a, b, n4, out); break;
    case 16: FBBEV_LAUNCH((k_softmax_groups<16, BWD>), blocks, 256, 0, stream, a, b, n4, out); break;
    default: FBBEV_LAUNCH((k_softmax_groups<32, BWD>), blocks, 256, 0, stream, a, b, n4, out); break;
    }
    FBBEV_CHECK_LAUNCH();
    return 0;
}
extern "C" int fbbev_softmax_groups(const float* x, long long n_groups, int group, float* y, fbbev_stream_t stream_) {
    return softmax_groups_launch<false>(x, nullptr, n_groups, group, y, stream_);
}
extern "C" int fbbev_softmax_groups_bwd(const float* y, const float* grad_y, long long n_groups, int group, float* grad_x,
                                        fbbev_stream_t stream_) {
    return softmax_groups_launch<true>(y, grad_y, n_groups, group, grad_x, stream_);
}

// ------------------------------------------------------------------------------ Lovasz-softmax occupancy loss: segmented sort + scan
namespace {
struct occlv_plan {
    int T, TD, nth, ntw, ntd, staged, row_runs;          // the tile walk of fbbev_occ_loss_stats
    long long ntiles, blocks;
    int nvox, cps, group;                                // voxels, sort chunks per class, classes sorted together
    size_t off_b, off_matrix, off_tot, off_cstat, off_sfg, off_part, total;
};
// 1 = nothing to do (B == 0)
int occlv_check(const void* logits, int B, int C, int H, int W, int D, const void* labels) {
    if (!logits || !labels || B < 0 || C <= 0 || H <= 0 || W <= 0 || D <= 0) return FBBEV_E_BADARG;
    if (B == 0) return 1;
    if (C < 2 || C > 32) return FBBEV_E_UNSUPPORTED;
    long long nvox = B;                                  // factor by factor: each is below 2^31, so no product leaves 64 bits
    for (const int f : {H, W, D}) {
        nvox *= f;
        if (nvox >= (1ll << 26)) return FBBEV_E_UNSUPPORTED;
    }
    return 0;
}
// B H W D < 2^26 has been checked
occlv_plan occlv_plan_of(long long stride_c, long long stride_w, long long stride_d, int B, int C, int H, int W, int D) {
    occlv_plan p;
    p.TD = D < 64 ? D : 64;
    p.T = p.TD >= 16 ? 8 : 16;
    p.nth = (H + p.T - 1) / p.T; p.ntw = (W + p.T - 1) / p.T; p.ntd = (D + p.TD - 1) / p.TD;
    p.ntiles = (long long)B * p.nth * p.ntw * p.ntd;
    p.blocks = p.ntiles < FBBEV_OCCLV_MAX_BLOCKS ? p.ntiles : FBBEV_OCCLV_MAX_BLOCKS;
    p.staged = (stride_c == 1 && stride_d == C) ? 1 : 0;
    p.row_runs = (p.staged && p.TD == D && stride_w == (long long)D * C) ? 1 : 0;
    p.nvox = B * H * W * D;
    p.cps = (p.nvox + FBBEV_OCCLV_TILE - 1) / FBBEV_OCCLV_TILE;
    // classes per group: two pair buffers of 8 bytes per (class, voxel) stay below 2 x 128 MiB (all 19 classes at once at the shipped
    // shape with B = 1, six at a time at B = 4, one at a time from B = 14); the emulator's tests shrink it to walk several groups at
    // their sizes
    long long pairs = FBBEV_KNOB_EMU_INT("FBBEV_OCC_LOVASZ_GROUP_PAIRS", 1 << 24);
    if (pairs < 1) pairs = 1;
    long long group = pairs / p.nvox;
    p.group = (int)(group < 1 ? 1 : (group > C ? C : group));
    const size_t g = (size_t)p.group, seg = align_up(g * p.nvox * sizeof(uint2), 16);
    p.off_b = seg;
    p.off_matrix = 2 * seg;
    p.off_tot = p.off_matrix + align_up(g * p.cps * FBBEV_OCCLV_MAX_NB * sizeof(int), 16);
    p.off_cstat = p.off_tot + align_up(g * FBBEV_OCCLV_MAX_NB * sizeof(int), 16);
    p.off_sfg = p.off_cstat + align_up(g * p.cps * sizeof(int2), 16);
    p.off_part = p.off_sfg + align_up(g * p.cps * sizeof(int), 16);
    p.total = p.off_part + align_up(g * p.cps * sizeof(double), 16);
    return p;
}
}  // namespace

extern "C" size_t fbbev_occ_lovasz_ws_bytes(int B, int C, int H, int W, int D) {
    int dummy = 0;
    if (occlv_check(&dummy, B, C, H, W, D, &dummy) != 0) return 0;
    return occlv_plan_of(0, 0, 0, B, C, H, W, D).total;
}

extern "C" int fbbev_occ_lovasz_fwd(const float* logits, long long stride_b, long long stride_c, long long stride_h, long long stride_w,
                                    long long stride_d, int B, int C, int H, int W, int D, const uint8_t* labels, float* loss_c,
                                    int32_t* fg_count, float* coef, float* errors_out, void* ws, size_t ws_bytes,
                                    fbbev_stream_t stream_) {
    if (!loss_c || !fg_count || (B > 0 && (!coef || !ws))) return FBBEV_E_BADARG;
    const int chk = occlv_check(logits, B, C, H, W, D, labels);
    if (chk < 0) return chk;
    fbbev_rt_stream stream = (fbbev_rt_stream)stream_;
    if (chk == 1) {
        int e = fbbev_rt_memset_async(loss_c, 0, (size_t)C * sizeof(float), stream);
        if (!e) e = fbbev_rt_memset_async(fg_count, 0, (size_t)(C + 1) * sizeof(int32_t), stream);
        return e;
    }
    const occlv_plan p = occlv_plan_of(stride_c, stride_w, stride_d, B, C, H, W, D);
    if (ws_bytes < p.total || !aligned16(ws)) return FBBEV_E_WORKSPACE;
    // digit width of the radix passes: 10 bits = 3 passes, 8 bits = 4 passes over the 30 key bits (DESIGN 3.9 has the measurement)
    FBBEV_KNOB_ONCE(int, env_rb, fbbev_env_int("FBBEV_OCC_LOVASZ_DIGIT_BITS", 10));
    const int rb = env_rb == 8 ? 8 : 10, nb = 1 << rb, passes = rb == 8 ? 4 : 3;
    char* w8 = static_cast<char*>(ws);
    uint2* buf_a = reinterpret_cast<uint2*>(w8);
    uint2* buf_b = reinterpret_cast<uint2*>(w8 + p.off_b);
    unsigned int* keys0 = reinterpret_cast<unsigned int*>(buf_b);        // read by the first pass only, which writes buf_a
    int* matrix = reinterpret_cast<int*>(w8 + p.off_matrix);
    int* tot = reinterpret_cast<int*>(w8 + p.off_tot);
    int2* cstat = reinterpret_cast<int2*>(w8 + p.off_cstat);
    int* sfg = reinterpret_cast<int*>(w8 + p.off_sfg);
    double* part = reinterpret_cast<double*>(w8 + p.off_part);
    const size_t lds = (size_t)FBBEV_OCCL_THREADS * C * 4;
    for (int c0 = 0; c0 < C; c0 += p.group) {
        const int g = C - c0 < p.group ? C - c0 : p.group;
#define FBBEV_OCCLV_KEYS(S)                                                                                                             \
    FBBEV_LAUNCH((k_occ_lovasz_keys<S>), p.blocks, FBBEV_OCCL_THREADS, lds, stream, logits, stride_b, stride_c, stride_h, stride_w,    \
                 stride_d, C, H, W, D, p.T, p.TD, p.nth, p.ntw, p.ntd, (int)p.ntiles, p.row_runs, labels, c0, g, p.nvox, keys0, coef,  \
                 errors_out)
        if (p.staged) FBBEV_OCCLV_KEYS(true);
        else FBBEV_OCCLV_KEYS(false);
#undef FBBEV_OCCLV_KEYS
        FBBEV_CHECK_LAUNCH();
        const long long chunks = (long long)g * p.cps;
        const uint2* src = nullptr;
        uint2* dst = buf_a;
        for (int pass = 0; pass < passes; ++pass) {
            if (pass == 0) {
                FBBEV_LAUNCH(k_occ_lovasz_hist<true>, chunks, FBBEV_OCCLV_NT, 0, stream, (const unsigned int*)keys0, src, pass, rb, p.nvox,
                             p.cps, C, c0, (const int*)fg_count, matrix, cstat);
                FBBEV_CHECK_LAUNCH();
                FBBEV_LAUNCH(k_occ_lovasz_colscan<true>, g * (nb >> 8), 256, 0, stream, rb, p.cps, C, c0, fg_count, matrix, tot,
                             (const int2*)cstat);
                FBBEV_CHECK_LAUNCH();
                FBBEV_LAUNCH(k_occ_lovasz_scatter<true>, chunks, FBBEV_OCCLV_NT, 0, stream, (const unsigned int*)keys0, src, pass, rb,
                             p.nvox, p.cps, C, c0, (const int*)fg_count, (const int*)matrix, (const int*)tot, dst);
                FBBEV_CHECK_LAUNCH();
            } else {
                FBBEV_LAUNCH(k_occ_lovasz_hist<false>, chunks, FBBEV_OCCLV_NT, 0, stream, (const unsigned int*)nullptr, src, pass, rb,
                             p.nvox, p.cps, C, c0, (const int*)fg_count, matrix, cstat);
                FBBEV_CHECK_LAUNCH();
                FBBEV_LAUNCH(k_occ_lovasz_colscan<false>, g * (nb >> 8), 256, 0, stream, rb, p.cps, C, c0, fg_count, matrix, tot,
                             (const int2*)cstat);
                FBBEV_CHECK_LAUNCH();
                FBBEV_LAUNCH(k_occ_lovasz_scatter<false>, chunks, FBBEV_OCCLV_NT, 0, stream, (const unsigned int*)nullptr, src, pass, rb,
                             p.nvox, p.cps, C, c0, (const int*)fg_count, (const int*)matrix, (const int*)tot, dst);
                FBBEV_CHECK_LAUNCH();
            }
            src = dst;
            dst = dst == buf_a ? buf_b : buf_a;
        }
        FBBEV_LAUNCH(k_occ_lovasz_fgsum, chunks, FBBEV_OCCLV_NT, 0, stream, src, p.nvox, p.cps, C, c0, (const int*)fg_count, sfg);
        FBBEV_CHECK_LAUNCH();
        FBBEV_LAUNCH(k_occ_lovasz_coef, chunks, FBBEV_OCCLV_NT, 0, stream, src, p.nvox, p.cps, C, c0, (const int*)fg_count,
                     (const int*)sfg, coef, part);
        FBBEV_CHECK_LAUNCH();
        FBBEV_LAUNCH(k_occ_lovasz_loss, g, FBBEV_OCCLV_NT, 0, stream, p.cps, C, c0, (const int*)fg_count, (const double*)part, loss_c);
        FBBEV_CHECK_LAUNCH();
    }
    return 0;
}

extern "C" int fbbev_occ_lovasz_grad(const float* logits, long long stride_b, long long stride_c, long long stride_h, long long stride_w,
                                     long long stride_d, int B, int C, int H, int W, int D, const uint8_t* labels, const float* coef,
                                     const float* scale, float* grad_logits, fbbev_stream_t stream_) {
    if (!scale || !grad_logits || (B > 0 && !coef)) return FBBEV_E_BADARG;
    const int chk = occlv_check(logits, B, C, H, W, D, labels);
    if (chk < 0) return chk;
    if (chk == 1) return 0;
    const occlv_plan p = occlv_plan_of(stride_c, stride_w, stride_d, B, C, H, W, D);
    const size_t lds = (size_t)2 * FBBEV_OCCL_THREADS * C * 4;            // <= 64 KiB at C = 32
#define FBBEV_OCCLV_GRAD(S)                                                                                                             \
    FBBEV_LAUNCH((k_occ_lovasz_grad<S>), p.blocks, FBBEV_OCCL_THREADS, lds, (fbbev_rt_stream)stream_, logits, stride_b, stride_c,       \
                 stride_h, stride_w, stride_d, C, H, W, D, p.T, p.TD, p.nth, p.ntw, p.ntd, (int)p.ntiles, p.row_runs, labels, coef,    \
                 p.nvox, scale, grad_logits)
    if (p.staged) FBBEV_OCCLV_GRAD(true);
    else FBBEV_OCCLV_GRAD(false);
#undef FBBEV_OCCLV_GRAD
    FBBEV_CHECK_LAUNCH();
    return 0;
}

// ------------------------------------------------------------------------------ depth supervision loss: labels + BCE, and its backward
namespace {
struct dl_plan { int h, w, cc, vec; long long nrec; size_t off_i, total; };
// the counts the kernels index with 32 bits: cells and elements below 2^31 (factor by factor: no product leaves 64 bits)
bool dl_counts_fit(int BN, int D, int h, int w) {
    long long cells = BN;
    for (const int f : {h, w}) {
        cells *= f;
        if (cells >= (1ll << 31)) return false;
    }
    return cells * D < (1ll << 31);
}
dl_plan dl_plan_of(const void* gt, int BN, int W, int ds, int h, int w) {
    dl_plan p;
    p.h = h; p.w = w;
    p.cc = FBBEV_DL_COLS / ds;                                             // ds <= FBBEV_DL_COLS has been checked
    if (p.cc >= 4) p.cc &= ~3;                                             // a chunk starts on a column that is a multiple of 4
    p.vec = (W % 4 == 0 && aligned16(gt) && ((long long)p.cc * ds) % 4 == 0) ? 1 : 0;
    p.nrec = (long long)BN * h;
    p.off_i = align_up((size_t)p.nrec * sizeof(float), 16);
    p.total = p.off_i + align_up((size_t)p.nrec * sizeof(int32_t), 16);
    return p;
}
}  // namespace

extern "C" size_t fbbev_depth_loss_ws_bytes(int BN, int h, int w, int D) {
    if (BN <= 0 || h <= 0 || w <= 0 || D <= 0 || !dl_counts_fit(BN, D, h, w)) return 0;
    return dl_plan_of(nullptr, BN, 4, 1, h, w).total;
}

extern "C" int fbbev_depth_loss_fwd(const float* gt, int BN, int H, int W, int ds, const float* probs, int D, float bin0, float step,
                                    int32_t* labels, float* out_f, int32_t* out_i, void* ws, size_t ws_bytes, fbbev_stream_t stream_) {
    if (!gt || !labels || !out_f || !out_i || (BN > 0 && !ws)) return FBBEV_E_BADARG;
    if (BN < 0 || H <= 0 || W <= 0 || ds <= 0 || D <= 0 || H % ds != 0 || W % ds != 0) return FBBEV_E_BADARG;
    if (!(step > 0.f) || !(step <= 3.402823466e38f) || !(bin0 >= -3.402823466e38f && bin0 <= 3.402823466e38f)) return FBBEV_E_BADARG;
    fbbev_rt_stream stream = (fbbev_rt_stream)stream_;
    if (BN == 0) {
        int e = fbbev_rt_memset_async(out_f, 0, 2 * sizeof(float), stream);
        if (!e) e = fbbev_rt_memset_async(out_i, 0, sizeof(int32_t), stream);
        return e;
    }
    const int h = H / ds, w = W / ds;
    if (D > FBBEV_DL_MAX_D || ds > FBBEV_DL_COLS || !dl_counts_fit(BN, D, h, w)) return FBBEV_E_UNSUPPORTED;
    const dl_plan p = dl_plan_of(gt, BN, W, ds, h, w);
    if (ws_bytes < p.total || !aligned16(ws)) return FBBEV_E_WORKSPACE;
    float* part_f = static_cast<float*>(ws);
    int* part_i = reinterpret_cast<int*>(static_cast<char*>(ws) + p.off_i);
    const size_t lds = ((size_t)2 * FBBEV_DL_COLS + FBBEV_DL_THREADS) * 4;
#define FBBEV_DL_LAUNCH(V)                                                                                                        \
    FBBEV_LAUNCH((k_depth_loss_fwd<V>), p.nrec, FBBEV_DL_THREADS, lds, stream, gt, H, W, ds, h, w, p.cc, probs, D, bin0, step, labels, \
                 part_f, part_i)
    if (p.vec) FBBEV_DL_LAUNCH(true);
    else FBBEV_DL_LAUNCH(false);
#undef FBBEV_DL_LAUNCH
    FBBEV_CHECK_LAUNCH();
    FBBEV_LAUNCH(k_depth_loss_reduce, 1, FBBEV_DL_THREADS, (size_t)FBBEV_DL_THREADS * 12, stream, (const float*)part_f,
                 (const int*)part_i, (int)p.nrec, out_f, out_i);
    FBBEV_CHECK_LAUNCH();
    return 0;
}

extern "C" int fbbev_depth_loss_grad(const float* probs, const int32_t* labels, const int32_t* out_i, const float* grad_loss, int BN,
                                     int D, int h, int w, float* grad_probs, fbbev_stream_t stream_) {
    if (!probs || !labels || !out_i || !grad_loss || !grad_probs || BN < 0 || D <= 0 || h <= 0 || w <= 0) return FBBEV_E_BADARG;
    if (BN == 0) return 0;
    if (D > FBBEV_DL_MAX_D || !dl_counts_fit(BN, D, h, w)) return FBBEV_E_UNSUPPORTED;
    const unsigned int hw = (unsigned int)h * w, total = (unsigned int)BN * D * hw;
    FBBEV_LAUNCH(k_depth_loss_grad, (total + FBBEV_DL_THREADS - 1) / FBBEV_DL_THREADS, FBBEV_DL_THREADS, 0, (fbbev_rt_stream)stream_, probs,
                 labels, out_i, grad_loss, (unsigned int)D, hw, total, grad_probs);
    FBBEV_CHECK_LAUNCH();
    return 0;
}

// ------------------------------------------------------------------------------ LiDAR points -> multi-view depth maps
extern "C" int fbbev_points_to_depth(const float* points, int point_stride, const int32_t* offsets, int max_points, int B, int N,
                                     const float* lidar2img, const float* post_rots, const float* post_trans, int H, int W,
                                     int downsample, float depth_lo, float depth_hi, float* out, fbbev_stream_t stream_) {
    if (!points || !offsets || !lidar2img || !post_rots || !post_trans || !out) return FBBEV_E_BADARG;
    if (point_stride < 3 || downsample < 1 || max_points < 0 || B < 0 || N < 0 || H < 0 || W < 0) return FBBEV_E_BADARG;
    if (!(depth_lo > 0.f) || depth_hi != depth_hi) return FBBEV_E_BADARG;          // a kept depth must be positive (and lo no NaN)
    const int h = H / downsample, w = W / downsample;
    if (h == 0 || w == 0 || B == 0 || N == 0) return 0;                            // nothing to write
    if (depth_hi >= 100.f) return FBBEV_E_DEPTH_RANGE;
    if ((long long)h * w >= (1ll << 24)) return FBBEV_E_MAP_SIZE;
    const long long BN = (long long)B * N;
    if (BN >= (1ll << 24)) return FBBEV_E_UNSUPPORTED;                             // BN * chunks < 2^31; BN * h * w < 2^48
    fbbev_rt_stream stream = (fbbev_rt_stream)stream_;
    const long long n = BN * h * w;
    unsigned int* plane = reinterpret_cast<unsigned int*>(out);
    const int e = fbbev_rt_memset_async(plane, 0, (size_t)n * sizeof(float), stream);
    if (e) return e;
    if (max_points == 0) return 0;                                                 // zeros are the resolved plane already
    long long chunks = ((long long)max_points + FBBEV_PD_THREADS - 1) / FBBEV_PD_THREADS;
    if (chunks > FBBEV_PD_MAX_CHUNKS) chunks = FBBEV_PD_MAX_CHUNKS;
    FBBEV_LAUNCH(k_points_depth_splat, BN * chunks, FBBEV_PD_THREADS, 0, stream, points, point_stride, (const int*)offsets, N, (int)chunks,
                 lidar2img, post_rots, post_trans, (float)downsample, h, w, depth_lo, depth_hi, plane);
    FBBEV_CHECK_LAUNCH();
    long long head = (long long)((16 - (reinterpret_cast<uintptr_t>(out) & 15u)) & 15u) / 4;   // out is 4-byte aligned
    if (head > n) head = n;
    const long long nv = (n - head) / 4;
    long long blocks = (nv + FBBEV_PD_THREADS - 1) / FBBEV_PD_THREADS;
    if (blocks < 1) blocks = 1;
    if (blocks > FBBEV_PD_RESOLVE_BLOCKS) blocks = FBBEV_PD_RESOLVE_BLOCKS;
    FBBEV_LAUNCH(k_points_depth_resolve, blocks, FBBEV_PD_THREADS, 0, stream, plane, n, (int)head, nv);
    FBBEV_CHECK_LAUNCH();
    return 0;
}

// ------------------------------------------------------------------------------ camera frames -> network input
extern "C" int fbbev_image_prep_limits(int* tile_w, int* tile_h, int* max_taps, int* max_box_w, int* max_box_h, int* max_src_rows,
                                       int* max_src_cols) {
    if (!tile_w || !tile_h || !max_taps || !max_box_w || !max_box_h || !max_src_rows || !max_src_cols) return FBBEV_E_BADARG;
    *tile_w = FBBEV_IP_TILE_W;
    *tile_h = FBBEV_IP_TILE_H;
    *max_taps = FBBEV_IP_MAX_TAPS;
    *max_box_w = FBBEV_IP_BOX_W;
    *max_box_h = FBBEV_IP_BOX_H;
    *max_src_rows = FBBEV_IP_SRC_ROWS;
    *max_src_cols = FBBEV_IP_SRC_COLS;
    return 0;
}

extern "C" int fbbev_image_prep(const uint8_t* frames, long long image_stride, int n_img, int Hs, int Ws, int fH, int fW,
                                const int32_t* plan, const int32_t* host_need, const float* mean3, const float* inv_std3, int flags,
                                float* out, uint8_t* canvas, fbbev_stream_t stream_) {
    if (!frames || !plan || !host_need || !mean3 || !inv_std3 || !out) return FBBEV_E_BADARG;
    if (n_img < 0 || Hs <= 0 || Ws <= 0 || fH <= 0 || fW <= 0 || (flags & ~(FBBEV_IP_SWAP | FBBEV_IP_CHANNELS_LAST))) return FBBEV_E_BADARG;
    if (image_stride < (long long)Hs * Ws * 3) return FBBEV_E_BADARG;
    for (int i = 0; i < 5; ++i)
        if (host_need[i] < 0) return FBBEV_E_BADARG;
    if (n_img == 0) return 0;
    if (host_need[0] > FBBEV_IP_MAX_TAPS || host_need[1] > FBBEV_IP_BOX_W || host_need[2] > FBBEV_IP_BOX_H ||
        host_need[3] > FBBEV_IP_SRC_ROWS || host_need[4] > FBBEV_IP_SRC_COLS)
        return FBBEV_E_UNSUPPORTED;
    if (!aligned16(out) || (reinterpret_cast<uintptr_t>(frames) & 3u) || (reinterpret_cast<uintptr_t>(plan) & 3u)) return FBBEV_E_UNSUPPORTED;
    if (fH >= 16384 || fW >= 16384 || Hs >= (1 << 24) || Ws >= (1 << 24)) return FBBEV_E_UNSUPPORTED;   // the 16.16 walk; row * Ws in 48 bits
    const long long tiles_x = (fW + FBBEV_IP_TILE_W - 1) / FBBEV_IP_TILE_W, tiles_y = (fH + FBBEV_IP_TILE_H - 1) / FBBEV_IP_TILE_H;
    const long long grid = tiles_x * tiles_y * n_img;
    if (grid >= (1ll << 31)) return FBBEV_E_UNSUPPORTED;
    const long long frames_end = (long long)(n_img - 1) * image_stride + (long long)Hs * Ws * 3;
    FBBEV_LAUNCH(k_image_prep, grid, FBBEV_IP_THREADS, 0, (fbbev_rt_stream)stream_, (const unsigned char*)frames, image_stride, frames_end,
                 Hs, Ws, fH, fW, (int)tiles_x, (int)tiles_y, (const int*)plan, mean3[0], mean3[1], mean3[2], inv_std3[0], inv_std3[1],
                 inv_std3[2], (flags & FBBEV_IP_SWAP) ? 1 : 0, (flags & FBBEV_IP_CHANNELS_LAST) ? 1 : 0, out, (unsigned char*)canvas);
    FBBEV_CHECK_LAUNCH();
    return 0;
}
