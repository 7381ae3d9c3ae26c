// image_prep_kernels.h -- camera frames to network input in one kernel.
// Replaces PrepareImageInputs' image side (mmdet3d/datasets/pipelines/loading.py:1044-1051 img_transform_core and :972-983
// mmlabNormalize of the reference), a CPU pipeline step: PIL's resize (bicubic, two 8-bit passes with 22-bit fixed-point
// coefficients), crop (zero padding), horizontal flip and rotate (nearest, 16.16 fixed-point affine walk, black fill), then
// (float(v) - mean) * inv_std after a channel swap.  Every pixel is integer arithmetic on tables the host builds in float64
// (fb_bev_amd/image_prep.py), so the uint8 result equals PIL's bit for bit.
//
// Plan (int32, device): n_img records of FBBEV_IP_REC words, then tables.  Record: [0] newW [1] newH (not read here) [2] flip
// [3] 0 [4..9] a0..a5 [10] word offset of the horizontal table [11] of the vertical table [12] tap stride of the horizontal table
// [13] of the vertical one.  A table over n outputs of the crop window (n = fW or fH) with tap stride ks: first[n], count[n],
// taps[n * ks]; output i reads source samples first[i] .. first[i] + count[i] - 1; count 0 = outside the resized image (PIL's zero
// padding: (2^21) >> 22 = 0 falls out of the same formula); first and first + count never decrease along a table.
//
// A workgroup owns one FBBEV_IP_TILE_W x FBBEV_IP_TILE_H output tile of one image:
//   box      the four tile corners through (xin, yin) = ((a2 + y a1 + x a0) >> 16, (a5 + y a4 + x a3) >> 16) -- each is monotone in
//            x and in y, so the corners bound the tile -- clipped to the fW x fH frame; the flip turns box columns into window columns;
//            the tables' first / count at the box's ends give the source columns c0..c1 and rows r0..r1 it needs.
//   H pass   FBBEV_IP_CHUNK source rows at a time: thread t requests dword t of each row's segment (4-byte aligned addresses, all
//            requests before the first use), stores them to LDS, and the rows' box columns x 3 channels are filtered from LDS bytes
//            into s_h (uint8): v = clamp((2^21 + sum_k tap_k p_k) >> 22, 0, 255).
//   V pass   s_h -> s_v (uint8), the resized pixels of the box, same arithmetic.
//   gather   an output pixel computes (xin, yin) in closed form (PIL's running sums are exact integers: the same numbers), undoes the
//            flip, reads s_v or takes 0 outside the frame, writes canvas (uint8 RGB) and out[c] = (float(v[swap ? 2 - c : c]) - mean[c])
//            * inv_std[c]: one correctly rounded subtraction, one multiplication.
// Intermediates never leave LDS; no atomics.  A plan whose footprint exceeds the LDS plan is declined on the host
// (fbbev_image_prep's host_need); the kernel still holds every index against its buffers and writes zeros for such a tile.
#pragma once
#include "rt.h"

#define FBBEV_IP_THREADS 256
#define FBBEV_IP_TILE_W 64
#define FBBEV_IP_TILE_H 16
#define FBBEV_IP_MAX_TAPS 20                                     // resize 0.25: support 8, at most 17 taps
#define FBBEV_IP_BOX_W 72                                        // a 64 x 16 tile turned by 10 degrees: 68 x 29
#define FBBEV_IP_BOX_H 32
#define FBBEV_IP_SRC_ROWS 152                                    // 32 box rows at downscale 4 and twice the support: 145
#define FBBEV_IP_SRC_COLS 336                                    // 3 * 336 + 3 bytes of misalignment <= 1024: one dword per thread
#define FBBEV_IP_CHUNK 8
#define FBBEV_IP_REC 16
#define FBBEV_IP_HSTRIDE (FBBEV_IP_BOX_W * 3)

__device__ __forceinline__ int ip_mn(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int ip_mx(int a, int b) { return a > b ? a : b; }
__device__ __forceinline__ int ip_min4(int a, int b, int c, int d) { return ip_mn(ip_mn(a, b), ip_mn(c, d)); }
__device__ __forceinline__ int ip_max4(int a, int b, int c, int d) { return ip_mx(ip_mx(a, b), ip_mx(c, d)); }
__device__ __forceinline__ int ip_walk(int base, int ay, int ax, int y, int x) {
    return (int)(((long long)base + (long long)y * ay + (long long)x * ax) >> 16);
}
__device__ __forceinline__ int ip_clip8(int ss) { return ip_mn(ip_mx(ss >> 22, 0), 255); }

__global__ void __launch_bounds__(FBBEV_IP_THREADS)
k_image_prep(const unsigned char* __restrict__ frames, long long image_stride, long long frames_end, int Hs, int Ws, int fH, int fW,
             int tiles_x, int tiles_y, const int* __restrict__ plan, float m0, float m1, float m2, float s0, float s1, float s2, int swap,
             int channels_last, float* __restrict__ out, unsigned char* __restrict__ canvas) {
    __shared__ unsigned int s_stage[FBBEV_IP_CHUNK * FBBEV_IP_THREADS];
    __shared__ unsigned char s_h[FBBEV_IP_SRC_ROWS * FBBEV_IP_HSTRIDE];
    __shared__ unsigned char s_v[FBBEV_IP_BOX_H * FBBEV_IP_HSTRIDE];
    const int t = threadIdx.x;
    const unsigned int tiles = (unsigned int)tiles_x * tiles_y;
    const unsigned int img = blockIdx.x / tiles, rem_t = blockIdx.x - img * tiles;
    const int ty = rem_t / (unsigned int)tiles_x, tx = rem_t - ty * (unsigned int)tiles_x;
    const int* rec = plan + (size_t)img * FBBEV_IP_REC;
    const int flip = rec[2], a0 = rec[4], a1 = rec[5], a2 = rec[6], a3 = rec[7], a4 = rec[8], a5 = rec[9];
    const int* ht = plan + rec[10];
    const int* vt = plan + rec[11];
    const int hks = rec[12], vks = rec[13];
    const int x0 = tx * FBBEV_IP_TILE_W, y0 = ty * FBBEV_IP_TILE_H;
    const int x1 = ip_mn(x0 + FBBEV_IP_TILE_W, fW) - 1, y1 = ip_mn(y0 + FBBEV_IP_TILE_H, fH) - 1;
    // the box of the tile in the flipped, cropped, resized image
    const int xa = ip_walk(a2, a1, a0, y0, x0), xb = ip_walk(a2, a1, a0, y0, x1), xc = ip_walk(a2, a1, a0, y1, x0), xd = ip_walk(a2, a1, a0, y1, x1);
    const int ya = ip_walk(a5, a4, a3, y0, x0), yb = ip_walk(a5, a4, a3, y0, x1), yc = ip_walk(a5, a4, a3, y1, x0), yd = ip_walk(a5, a4, a3, y1, x1);
    const int bx0 = ip_mx(ip_min4(xa, xb, xc, xd), 0), bx1 = ip_mn(ip_max4(xa, xb, xc, xd), fW - 1);
    const int by0 = ip_mx(ip_min4(ya, yb, yc, yd), 0), by1 = ip_mn(ip_max4(ya, yb, yc, yd), fH - 1);
    int bw = bx1 - bx0 + 1, bh = by1 - by0 + 1;
    int wc0 = 0, wr0 = 0, c0 = 0, c1 = 0, r0 = 0, r1 = 0;
    if (bw > 0 && bh > 0 && bw <= FBBEV_IP_BOX_W && bh <= FBBEV_IP_BOX_H) {
        wc0 = flip ? fW - 1 - bx1 : bx0;
        wr0 = by0;
        c0 = ht[wc0];
        c1 = ht[wc0 + bw - 1] + ht[fW + wc0 + bw - 1];
        r0 = vt[wr0];
        r1 = vt[wr0 + bh - 1] + vt[fH + wr0 + bh - 1];
    } else {
        bw = 0;
        bh = 0;
    }
    // what the host checked, held again: a footprint outside the buffers or the source leaves the tile black
    if (c0 < 0 || c1 > Ws || c1 < c0 || c1 - c0 > FBBEV_IP_SRC_COLS || r0 < 0 || r1 > Hs || r1 < r0 || r1 - r0 > FBBEV_IP_SRC_ROWS ||
        hks < 0 || vks < 0) {
        bw = 0;
        bh = 0;
    }
    const int nrows = bh > 0 ? r1 - r0 : 0, ncols = c1 - c0, bw3 = bw * 3;
    const long long img_base = (long long)img * image_stride;

    // ---------------------------------------------------------------- horizontal pass, a chunk of source rows at a time
    for (int rb = 0; rb < nrows; rb += FBBEV_IP_CHUNK) {
        const int nr = ip_mn(FBBEV_IP_CHUNK, nrows - rb);
        unsigned int w[FBBEV_IP_CHUNK];
#pragma unroll
        for (int k = 0; k < FBBEV_IP_CHUNK; ++k) {
            w[k] = 0u;
            const long long off = img_base + ((long long)(r0 + rb + k) * Ws + c0) * 3;        // the segment's first byte
            const long long a = (off & ~3ll) + 4ll * t;
            if (k < nr && a < off + 3ll * ncols) {
                if (a + 4 <= frames_end) {
                    w[k] = *reinterpret_cast<const unsigned int*>(frames + a);
                } else {                                             // the last bytes of the last frame: no dword beyond them
                    for (int q = 0; q < 4; ++q)
                        if (a + q < frames_end) w[k] |= (unsigned int)frames[a + q] << (8 * q);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < FBBEV_IP_CHUNK; ++k) s_stage[k * FBBEV_IP_THREADS + t] = w[k];
        __syncthreads();
        for (int idx = t; idx < nr * bw3; idx += FBBEV_IP_THREADS) {
            const int row = idx / bw3, rem = idx - row * bw3, j = rem / 3, ch = rem - 3 * j;
            const int wc = wc0 + j, first = ht[wc];
            int cnt = ht[fW + wc];
            if (first < c0 || first + cnt > c1 || cnt > hks) cnt = 0;
            const int* taps = ht + 2 * fW + (size_t)wc * hks;
            const int shift = (int)((img_base + ((long long)(r0 + rb + row) * Ws + c0) * 3) & 3);
            const unsigned char* src = reinterpret_cast<const unsigned char*>(s_stage + row * FBBEV_IP_THREADS) + shift + (first - c0) * 3 + ch;
            int ss = 1 << 21;
            for (int k = 0; k < cnt; ++k) ss += (int)src[3 * k] * taps[k];
            s_h[(rb + row) * FBBEV_IP_HSTRIDE + rem] = (unsigned char)ip_clip8(ss);
        }
        __syncthreads();
    }

    // ---------------------------------------------------------------- vertical pass
    for (int idx = t; idx < bh * bw3; idx += FBBEV_IP_THREADS) {
        const int i = idx / bw3, rem = idx - i * bw3;
        const int wr = wr0 + i, first = vt[wr];
        int cnt = vt[fH + wr];
        if (first < r0 || first + cnt > r1 || cnt > vks) cnt = 0;
        const int* taps = vt + 2 * fH + (size_t)wr * vks;
        const unsigned char* src = s_h + (first - r0) * FBBEV_IP_HSTRIDE + rem;
        int ss = 1 << 21;
        for (int k = 0; k < cnt; ++k) ss += (int)src[k * FBBEV_IP_HSTRIDE] * taps[k];
        s_v[i * FBBEV_IP_HSTRIDE + rem] = (unsigned char)ip_clip8(ss);
    }
    __syncthreads();

    // ---------------------------------------------------------------- gather, normalise, store
    const int x = x0 + (t & (FBBEV_IP_TILE_W - 1));
#pragma unroll
    for (int k = 0; k < FBBEV_IP_TILE_H / (FBBEV_IP_THREADS / FBBEV_IP_TILE_W); ++k) {
        const int y = y0 + (t / FBBEV_IP_TILE_W) + k * (FBBEV_IP_THREADS / FBBEV_IP_TILE_W);
        if (x >= fW || y >= fH) continue;
        const int xin = ip_walk(a2, a1, a0, y, x), yin = ip_walk(a5, a4, a3, y, x);
        int v0 = 0, v1 = 0, v2 = 0;
        if (xin >= 0 && xin < fW && yin >= 0 && yin < fH) {
            const int j = (flip ? fW - 1 - xin : xin) - wc0, i = yin - wr0;
            if (j >= 0 && j < bw && i >= 0 && i < bh) {
                const unsigned char* p = s_v + i * FBBEV_IP_HSTRIDE + j * 3;
                v0 = p[0];
                v1 = p[1];
                v2 = p[2];
            }
        }
        const size_t pix = ((size_t)img * fH + y) * fW + x;
        if (canvas) {
            canvas[pix * 3 + 0] = (unsigned char)v0;
            canvas[pix * 3 + 1] = (unsigned char)v1;
            canvas[pix * 3 + 2] = (unsigned char)v2;
        }
        const float f0 = fbbev_mul(fbbev_sub((float)(swap ? v2 : v0), m0), s0);
        const float f1 = fbbev_mul(fbbev_sub((float)v1, m1), s1);
        const float f2 = fbbev_mul(fbbev_sub((float)(swap ? v0 : v2), m2), s2);
        if (channels_last) {
            out[pix * 3 + 0] = f0;
            out[pix * 3 + 1] = f1;
            out[pix * 3 + 2] = f2;
        } else {
            const size_t plane = (size_t)fH * fW, o = (size_t)img * 3 * plane + (size_t)y * fW + x;
            out[o] = f0;
            out[o + plane] = f1;
            out[o + 2 * plane] = f2;
        }
    }
}
