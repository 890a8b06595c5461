// k_pdist.h -- pairwise distances between the rows of a dense row-major float64[n_rows][row_len]
// matrix, the arithmetic of
//   get_pairwise_dists / sliding_window_dist / euclidian_dist   (tombo_stats.py:158-196)   mode W
//   order_reads' pdist metric np.nanmean(np.sqrt((u - v)**2))   (tombo_stats.py:142-156)   mode N
//
// The pairs are cut into tiles of PDIST_TILE x PDIST_TILE; a workgroup of PDIST_TILE^2 threads owns
// one tile of the triangle that holds values and every thread owns one pair.  Only these tiles are
// launched (block b of the grid is tile (ta, tb), tb <= ta, row-major over the triangle).  The
// workgroup copies the two sets of PDIST_TILE rows into LDS first (coalesced: the rows of a set are
// consecutive in memory).  The LDS row stride is row_len | 1: the sixteen rows that the lanes of a
// 32-lane group read at one column then lie on distinct pairs of banks; the other set is read at
// two addresses per group, which broadcast.  Rows longer than PDIST_LDS_ROW_MAX do not fit twice
// sixteen times into 64 KB of LDS: the same threads then read them from global memory (use_lds 0),
// where the caches hold the 32 rows of a tile.
//
// Every sum is np_sum_by over exactly the terms numpy adds, in numpy's order; nothing is shared
// between the windows of a pair (running or diagonal sums would round differently).  sqrt is the
// correctly rounded one, -ffp-contract=off keeps d * d and the additions apart.
#pragma once
#include "tba_common.h"

#define PDIST_TILE 16              // rows per set and tile; PDIST_TILE^2 = 256 threads
#define PDIST_LDS_ROW_MAX 255      // longest row staged in LDS: 2 x 16 rows x 255 doubles = 65280 bytes
#define PDIST_MAX_ROWS 16384       // n_rows of one call (mode W's output: 2 GiB)
#define PDIST_MAX_ELEMS ((i64)1 << 28)   // n_rows * row_len of one call (2 GiB of input)

// block b -> tile (ta, tb), tb <= ta: b = ta (ta + 1) / 2 + tb
__device__ __forceinline__ void pd_tile_of(u32 b, int &ta, int &tb)
{
    int t = (int)((sqrt(8.0 * (double)b + 1.0) - 1.0) * 0.5);
    while ((i64)t * (t + 1) / 2 > (i64)b) t--;
    while ((i64)(t + 1) * (t + 2) / 2 <= (i64)b) t++;
    ta = t;
    tb = (int)((i64)b - (i64)t * (t + 1) / 2);
}

// rows ta * PDIST_TILE .. into lds[0 .. PDIST_TILE), rows tb * PDIST_TILE .. into the PDIST_TILE
// after them, row stride `stride`; rows past n_rows are left alone (no pair reads them).  Called by
// the whole workgroup.
__device__ __forceinline__ void pd_stage(const double *rows, i64 n_rows, int row_len, int stride, int ta, int tb,
                                         double *lds)
{
    for (int set = 0; set < 2; set++) {
        const i64 r0 = (i64)(set ? tb : ta) * PDIST_TILE;
        const int nr = n_rows - r0 < PDIST_TILE ? (int)(n_rows - r0) : PDIST_TILE;
        const double *src = rows + r0 * row_len;
        for (int e = threadIdx.x; e < nr * row_len; e += PDIST_TILE * PDIST_TILE) {
            const int r = e / row_len;
            lds[(set * PDIST_TILE + r) * stride + (e - r * row_len)] = src[e];
        }
    }
    __syncthreads();
}

// Mode W.  out[i][j], j <= i: sqrt of the minimum over the window starts i1, i2 in [0, 2 span] (i1
// outer) of sum((a_i[i1 : i1 + nb] - a_j[i2 : i2 + nb])^2), nb = row_len - 2 span; Python's min():
// the first value stays unless a later one is smaller, so a NaN stays only when it comes first.
// out[i][j] = 0 for j > i: inside a diagonal tile by the pair's own thread, else by the thread of
// the mirrored pair.
__global__ void __launch_bounds__(PDIST_TILE * PDIST_TILE) k_pdist_window(i64 n_rows, i64 row_len, i64 span,
    int use_lds, const double *rows, double *out)
{
    extern __shared__ double pd_lds[];
    int ta, tb;
    pd_tile_of(blockIdx.x, ta, tb);
    const int ly = threadIdx.x / PDIST_TILE, lx = threadIdx.x % PDIST_TILE;
    const int stride = (int)row_len | 1;
    if (use_lds) pd_stage(rows, n_rows, (int)row_len, stride, ta, tb, pd_lds);
    const i64 i = (i64)ta * PDIST_TILE + ly, j = (i64)tb * PDIST_TILE + lx;
    if (i >= n_rows || j >= n_rows) return;
    if (j > i) { out[i * n_rows + j] = 0.0; return; }
    const double *a = use_lds ? pd_lds + ly * stride : rows + i * row_len;
    const double *b = use_lds ? pd_lds + (PDIST_TILE + lx) * stride : rows + j * row_len;
    const i64 nb = row_len - 2 * span;
    double best = 0.0;
    for (i64 i1 = 0; i1 <= 2 * span; i1++)
        for (i64 i2 = 0; i2 <= 2 * span; i2++) {
            const double *wa = a + i1, *wb = b + i2;
            const double s = np_sum_by([wa, wb](i64 k) { const double d = wa[k] - wb[k]; return d * d; }, nb);
            if ((i1 == 0 && i2 == 0) || s < best) best = s;
        }
    out[i * n_rows + j] = sqrt(best);
    if (ta != tb) out[j * n_rows + i] = 0.0;
}

// Mode N.  condensed[k(i, j)], i < j, scipy's pdist order k = n i - i (i + 1) / 2 + j - i - 1:
// the sum over all row_len terms sqrt(d * d), d = u_i - u_j, a NaN term counted as 0, divided by the
// number of terms that are not NaN (0 / 0 = NaN without one).  sqrt(d * d) is NaN exactly when d is.
// The j of a tile come from set 0 and vary fastest over the lanes: the stores of a lane row are
// consecutive.
__global__ void __launch_bounds__(PDIST_TILE * PDIST_TILE) k_pdist_nanmean(i64 n_rows, i64 row_len, int use_lds,
    const double *rows, double *condensed)
{
    extern __shared__ double pd_lds[];
    int ta, tb;
    pd_tile_of(blockIdx.x, ta, tb);
    const int ly = threadIdx.x / PDIST_TILE, lx = threadIdx.x % PDIST_TILE;
    const int stride = (int)row_len | 1;
    if (use_lds) pd_stage(rows, n_rows, (int)row_len, stride, ta, tb, pd_lds);
    const i64 j = (i64)ta * PDIST_TILE + lx, i = (i64)tb * PDIST_TILE + ly;
    if (j >= n_rows || i >= j) return;
    const double *u = use_lds ? pd_lds + (PDIST_TILE + ly) * stride : rows + i * row_len;
    const double *v = use_lds ? pd_lds + lx * stride : rows + j * row_len;
    i64 cnt = 0;
    for (i64 k = 0; k < row_len; k++) { const double d = u[k] - v[k]; cnt += d == d; }
    const double tot = np_sum_by([u, v](i64 k) {
        const double d = u[k] - v[k];
        const double t = sqrt(d * d);
        return t == t ? t : 0.0;
    }, row_len);
    condensed[n_rows * i - i * (i + 1) / 2 + (j - i - 1)] = tot / (double)cnt;
}
