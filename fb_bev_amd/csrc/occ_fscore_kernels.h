// occ_fscore_kernels.h -- the four integer counts of the occupancy F-score (mmdet3d/datasets/occ_metrics.py:182-282 Metric_FScore)
// without a KD-tree.  The reference turns the occupied voxels of the prediction (P) and of the labels (G) into the centres of a regular
// grid and asks, per point, whether its nearest neighbour in the other set is closer than a threshold.  On a grid that is a bounded
// stencil over two occupancy bitmaps.
//
// Everything that rounds is built by the host in float64 (fb_bev_amd/occ_metrics.py):
//   sq_a[i][o + R] = (c_a[i] - c_a[i + o])^2 for o in -R..R per axis a, inf where i + o leaves the grid;
//   T = the largest float64 d2 with sqrt(d2) < threshold, so `sqrt(d2) < threshold` <=> `d2 <= T` and no root is taken here;
//   the list of offsets (ox, oy, oz) that can pass the larger T anywhere in the grid.
// The device forms (sq_x[qx][ox] + sq_y[qy][oy]) + sq_z[qz][oz] with two float64 ADDS in that order (nothing to contract: there is no
// multiply) and compares with T.  The same source under the CPU emulator gives the same bits.
//
// With Z <= 32 a column's occupancy is one 32-bit word per set.  A workgroup of 256 threads owns a tile of 16 x 16 columns:
//   stage: the bit columns of both sets for the tile plus an R-wide halo (zero outside the grid) are built in LDS from the three byte
//          maps, four bytes per load where Z % 4 == 0 and the maps are 4-byte aligned; the tile's rows of sq_x / sq_y and all of sq_z
//          go to LDS beside them (inf for the rows of a partial tile that lie outside the grid).
//   walk:  one lane per column walks the offset list.  For (ox, oy) it forms the xy sum once per offset; for oz it turns the Z
//          comparisons into a bit mask per threshold and combines it with the query word and the shifted target column.  A column
//          with no occupied voxel, a neighbour column with no target, and a column whose voxels have all been hit skip the arithmetic.
//   count: popcount of the four words, a shuffle reduction per wave, four LDS words per wave, and four integer atomics per workgroup
//          (zeros are not sent).  Integer adds only: exact and identical run to run.
// An offset outside -R..R is skipped, so no LDS index depends on the contents of device memory.
#pragma once
#include "rt.h"

#define FBBEV_OCCF_THREADS 256
#define FBBEV_OCCF_TILE 16
#define FBBEV_OCCF_MAX_R 4
#define FBBEV_OCCF_MAX_Z 32

struct fbbev_occf_void { unsigned int w[8]; };      // bit id set: class id `id` is void (not occupied)

// dynamic LDS of k_occ_fscore for a halo of R and a depth of Z, in bytes
static inline size_t fbbev_occf_lds_bytes(int R, int Z) {
    const int Wd = 2 * R + 1, HW = FBBEV_OCCF_TILE + 2 * R;
    return (size_t)(Z + 2 * FBBEV_OCCF_TILE) * Wd * sizeof(double) + (size_t)2 * HW * HW * 4 + 8 * 4 + 16 * 4;
}

__device__ __forceinline__ unsigned int occf_occupied(const unsigned int* vbits, unsigned int id) {
    return ((vbits[id >> 5] >> (id & 31u)) & 1u) ^ 1u;
}

// counts[b] = (n_gt, n_pred, n_cmpl, n_acc), ADDED to
template <bool VEC4>
__global__ void __launch_bounds__(FBBEV_OCCF_THREADS)
k_occ_fscore(const unsigned char* __restrict__ classes, const unsigned char* __restrict__ gt, const unsigned char* __restrict__ mask,
             fbbev_occf_void vb, const double* __restrict__ sqx, const double* __restrict__ sqy, const double* __restrict__ sqz,
             const int* __restrict__ offsets, int n_off, int R, double t_acc, double t_cmpl, int X, int Y, int Z, int ntx, int nty,
             int* __restrict__ counts) {
    constexpr int TILE = FBBEV_OCCF_TILE;
    const int Wd = 2 * R + 1, HW = TILE + 2 * R;
    double* sz = reinterpret_cast<double*>(fbbev_dyn_lds_f32());         // [Z][Wd]
    double* sx = sz + Z * Wd;                                            // [TILE][Wd]
    double* sy = sx + TILE * Wd;                                         // [TILE][Wd]
    unsigned int* pw = reinterpret_cast<unsigned int*>(sy + TILE * Wd);  // [HW][HW] prediction bit columns
    unsigned int* gw = pw + HW * HW;                                     // [HW][HW] label bit columns
    unsigned int* vbits = gw + HW * HW;                                  // [8]
    int* red = reinterpret_cast<int*>(vbits + 8);                        // [4 waves][4]
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;

    unsigned int r = blockIdx.x;
    const int iy = (int)(r % (unsigned int)nty); r /= (unsigned int)nty;
    const int ix = (int)(r % (unsigned int)ntx);
    const int b = (int)(r / (unsigned int)ntx);
    const int x0 = ix * TILE, y0 = iy * TILE;

    if (t == 0) {
#pragma unroll
        for (int i = 0; i < 8; ++i) vbits[i] = vb.w[i];
    }
    const double inf = (double)__builtin_inff();
    for (int i = t; i < Z * Wd; i += FBBEV_OCCF_THREADS) sz[i] = sqz[i];
    for (int i = t; i < TILE * Wd; i += FBBEV_OCCF_THREADS) {
        const int row = i / Wd, o = i - row * Wd;
        sx[i] = x0 + row < X ? sqx[(long long)(x0 + row) * Wd + o] : inf;
        sy[i] = y0 + row < Y ? sqy[(long long)(y0 + row) * Wd + o] : inf;
    }
    __syncthreads();

    // ---- stage: bit columns of the tile and its halo
    for (int c = t; c < HW * HW; c += FBBEV_OCCF_THREADS) {
        const int hx = c / HW, hy = c - hx * HW;
        const int gx = x0 - R + hx, gy = y0 - R + hy;
        unsigned int p = 0, g = 0;
        if (gx >= 0 && gx < X && gy >= 0 && gy < Y) {
            const long long o = (((long long)b * X + gx) * Y + gy) * Z;
            if (VEC4) {
                for (int k = 0; k < Z; k += 4) {
                    const unsigned int c4 = *reinterpret_cast<const unsigned int*>(classes + o + k);
                    const unsigned int g4 = *reinterpret_cast<const unsigned int*>(gt + o + k);
                    const unsigned int m4 = mask ? *reinterpret_cast<const unsigned int*>(mask + o + k) : 0x01010101u;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const bool seen = ((m4 >> (8 * e)) & 0xffu) != 0;
                        p |= occf_occupied(vbits, seen ? (c4 >> (8 * e)) & 0xffu : 255u) << (k + e);
                        g |= occf_occupied(vbits, seen ? (g4 >> (8 * e)) & 0xffu : 255u) << (k + e);
                    }
                }
            } else {
                for (int k = 0; k < Z; ++k) {
                    const bool seen = mask ? mask[o + k] != 0 : true;
                    p |= occf_occupied(vbits, seen ? classes[o + k] : 255u) << k;
                    g |= occf_occupied(vbits, seen ? gt[o + k] : 255u) << k;
                }
            }
        }
        pw[c] = p;
        gw[c] = g;
    }
    __syncthreads();

    // ---- walk: one lane per column (lanes run along y)
    const int tx = t / TILE, ty = t - tx * TILE;
    const unsigned int P = pw[(tx + R) * HW + ty + R], G = gw[(tx + R) * HW + ty + R];   // zero for a column outside the grid
    unsigned int hit_p = 0, hit_g = 0;                  // voxels of P that hit G within t_acc; of G that hit P within t_cmpl
    if (P | G) {
        for (int i = 0; i < n_off; ++i) {
            const int ox = offsets[3 * i], oy = offsets[3 * i + 1], oz = offsets[3 * i + 2];
            if (ox < -R || ox > R || oy < -R || oy > R || oz < -R || oz > R) continue;
            const int nb = (tx + R + ox) * HW + ty + R + oy;
            const unsigned int Tg = P ? gw[nb] : 0u, Tp = G ? pw[nb] : 0u;
            if (!(Tg | Tp)) continue;
            const double xy = sx[tx * Wd + ox + R] + sy[ty * Wd + oy + R];
            unsigned int za = 0, zc = 0;
            for (int k = 0; k < Z; ++k) {
                const double s = xy + sz[k * Wd + oz + R];
                za |= (s <= t_acc ? 1u : 0u) << k;
                zc |= (s <= t_cmpl ? 1u : 0u) << k;
            }
            // bit k of the shifted word = the target at depth k + oz
            const unsigned int sg = oz >= 0 ? Tg >> oz : Tg << (-oz), sp = oz >= 0 ? Tp >> oz : Tp << (-oz);
            hit_p |= P & za & sg;
            hit_g |= G & zc & sp;
            if (hit_p == P && hit_g == G) break;
        }
    }

    // ---- count
    int v[4] = {(int)__popcll((unsigned long long)G), (int)__popcll((unsigned long long)P), (int)__popcll((unsigned long long)hit_g),
                (int)__popcll((unsigned long long)hit_p)};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) v[j] += __shfl_xor(v[j], m, 64);
    }
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) red[wave * 4 + j] = v[j];
    }
    __syncthreads();
    if (t < 4) {
        const int sum = red[t] + red[4 + t] + red[8 + t] + red[12 + t];
        if (sum) atomicAdd(&counts[b * 4 + t], sum);
    }
}
