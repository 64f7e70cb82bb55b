// 2-D correlation / convolution of fp32 arrays: np_correlate2d (include/np_hip.h).
//
// The definition is scipy.signal.correlate2d / convolve2d (the loop of the reference's signal.c:152-207 is the same
// computation; the reference refuses GPU arrays, signal.c:219-221).  Everything is reduced to ONE form,
//
//     out[m][n] = sum over the footprint (j, k), 0 <= j < wh, 0 <= k < ww, of  W(j, k) * P(m + r0 + j, n + c0 + k)
//
// where P is the image extended by the boundary rule (fill / wrap / symm), r0 / c0 place the footprint for the mode, and
// W(j, k) is the window read as it lies over the image: w[j][k] for a correlation, w[wh-1-j][ww-1-k] for a convolution (the
// flip is an index, never a copy).  (j, k) are FOOTPRINT coordinates, so convolve2d(a, b) and correlate2d(a, b reversed
// along both axes) run the same multiplications in the same order.
//
// One kernel template, two paths (the dispatch looks at the window alone):
//   staged   wh <= 15 and ww <= 15: a workgroup of 256 lanes owns a 64 x 64 output tile and stages the tile plus the
//            whole halo, (64 + wh - 1) x (64 + ww - 1) cells, into LDS ONCE.  Every cell is resolved against the boundary
//            rule when it is staged — once per cell, not once per tap.
//   chunked  anything larger, 255 x 255 or 1000 x 3 alike: the footprint is cut into chunks of 16 x 16 taps; per chunk the
//            matching (64 + 15) x (64 + 15) cells are staged and the accumulators stay in registers across chunks, so LDS
//            never limits the window.
// Lane l of a wave owns COLUMN l of the tile and a register block of 16 outputs down that column (wave w: tile rows 16 w ...
// 16 w + 15).  Per footprint column k it reads the 16 + rows - 1 cells below its first output into registers once and uses
// each for up to 16 outputs: (16 + wh - 1) / (16 wh) LDS reads per FMA, 0.38 for 3 x 3, 0.13 for 15 x 15.  Lanes read consecutive
// LDS words, so no read conflicts at any pitch; output rows are stored as full 256-byte lines.  The pitch of 80 words
// places the four rows a wave writes in the second staging pass (columns 64 ... 78) on disjoint banks.
// The window's coefficients are never staged: their index is uniform across the wave, they arrive through scalar loads.
//
// Summation order, fixed for every output element whatever its place in a tile: acc = +0.0f, then acc = fmaf(W, P, acc)
// chunk by chunk in row-major chunk order (the staged path has one chunk), inside a chunk footprint column by footprint
// column, each column top to bottom.  Every tap is multiplied and added — no skipping of zero coefficients or fill cells.
#include "np_internal.h"

#include <limits.h>

namespace {

constexpr int kTileW = 64;        // output columns per workgroup = lanes of a wave
constexpr int kRegRows = 16;      // outputs per lane, down its column
constexpr int kTileH = 64;        // output rows per workgroup = 4 waves x kRegRows
constexpr int kSmallMax = 15;     // the staged path takes windows up to kSmallMax x kSmallMax
constexpr int kChunk = 16;        // the chunked path stages kChunk x kChunk taps at a time
constexpr int kPitch = 80;        // LDS words per staged row: >= kTileW + kChunk - 1, and 16 mod 32 (see above)
static_assert(kPitch >= kTileW + kChunk - 1 && kPitch % 32 == 16, "kPitch");
static_assert(kSmallMax < kChunk + 1, "the staged path's halo must fit the staged rows");

constexpr size_t kMaxTiles = ((size_t)1 << 24) - 1;   // a launch stays under 2^32 lanes: about 2^36 outputs, more than a device holds
int g_conv2d_last_path = 0;       // np_debug_conv2d_last_path
int g_conv2d_chunked_only = 0;    // np_debug_conv2d_staged_path(0)

struct Conv2dArgs {
    const float *a;       // image, ah x aw
    const float *w;       // window, wh x ww
    float *out;           // oh x ow
    int ah, aw, wh, ww, oh, ow;
    int r0, c0;           // image row / column under footprint (0, 0) of output (0, 0)
    int boundary;         // NP_CONV_FILL / SYMM / WRAP
    int flip;             // the window is read reversed along both axes
    int reverse;          // the result is stored reversed along both axes ('valid' correlation with swapped operands)
    float fill;
};

// signal.c:84-101 (scipy's _sigtoolsmodule): the index an out-of-range j stands for, any number of periods away
__device__ __forceinline__ int wrap_index(long long j, long long m) {
    return (int)(j >= 0 ? j % m : (j % m + m) % m);
}
__device__ __forceinline__ int symm_index(long long j, long long m) {
    const long long k = (j >= 0 ? j : -(j + 1)) % (2 * m);
    return (int)(k >= m ? 2 * m - k - 1 : k);
}

// the value of the extended image at (r, c): resolved once per staged cell
__device__ __forceinline__ float cell(const Conv2dArgs &p, long long r, long long c) {
    const bool in = r >= 0 && r < p.ah && c >= 0 && c < p.aw;
    if (!in) {
        if (p.boundary == NP_CONV_FILL) return p.fill;
        if (p.boundary == NP_CONV_WRAP) {
            r = wrap_index(r, p.ah);
            c = wrap_index(c, p.aw);
        } else {
            r = symm_index(r, p.ah);
            c = symm_index(c, p.aw);
        }
    }
    return p.a[(size_t)r * (size_t)p.aw + (size_t)c];
}

// CH: footprint rows per chunk (compile time: the register strip holds kRegRows + CH - 1 cells).  CHUNKED: loop over chunks of
// CH x kChunk taps; otherwise the whole window (wh <= CH, ww <= kSmallMax) is the one chunk.
template <int CH, bool CHUNKED>
__global__ __launch_bounds__(256) void conv2d_kernel(const Conv2dArgs p) {
    __shared__ float tile[(kTileH + CH - 1) * kPitch];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned tiles_x = ((unsigned)p.ow + kTileW - 1) / kTileW;   // a flat grid: neither extent is held to 65535 tiles
    const long long y0 = (long long)(blockIdx.x / tiles_x) * kTileH, x0 = (long long)(blockIdx.x % tiles_x) * kTileW;
    float acc[kRegRows];
#pragma unroll
    for (int r = 0; r < kRegRows; ++r) acc[r] = 0.0f;

    // W(j, k) = wbase[j wsj + k wsk]: the window as it lies over the image, read backwards for a convolution
    const float *wbase = p.flip ? p.w + ((size_t)p.wh * (size_t)p.ww - 1) : p.w;
    const long long wsj = p.flip ? -(long long)p.ww : (long long)p.ww, wsk = p.flip ? -1 : 1;
    const int chunk_rows = CHUNKED ? (p.wh + CH - 1) / CH : 1;
    const int chunk_cols = CHUNKED ? (p.ww + kChunk - 1) / kChunk : 1;
    for (int cj = 0; cj < chunk_rows; ++cj) {
        const int j0 = cj * CH;
        const int nj = CHUNKED ? min(CH, p.wh - j0) : p.wh;            // footprint rows of this chunk
        for (int ck = 0; ck < chunk_cols; ++ck) {
            const int k0 = ck * kChunk;
            const int nk = CHUNKED ? min(kChunk, p.ww - k0) : p.ww;    // footprint columns of this chunk
            const int rows = kTileH + nj - 1, extra = nk - 1;          // staged cells: rows x (kTileW + extra)
            const long long gr0 = y0 + p.r0 + j0, gc0 = x0 + p.c0 + k0;
            if (CHUNKED && (cj | ck)) __syncthreads();                 // the previous chunk's reads are over
            // pass 1: columns 0 .. 63 of every staged row, a wave per row: one 256-byte line each
            // pass 2: the `extra` columns right of them, 16 lanes per row, four rows per wave instruction
            const int sub = lane & 15, row2 = wave * 4 + (lane >> 4);
            if (gr0 >= 0 && gr0 + rows <= p.ah && gc0 >= 0 && gc0 + kTileW + extra <= p.aw) {
                // every staged cell lies inside the image (all tiles but the border's): nothing to resolve, and every load of
                // the wave is issued before the first is stored to LDS
                constexpr int kLoads1 = (kTileH + CH - 1 + 3) / 4, kLoads2 = (kTileH + CH - 1 + 15) / 16;
                const float *src = p.a + (size_t)gr0 * (size_t)p.aw + (size_t)gc0;
                float t1[kLoads1], t2[kLoads2];
#pragma unroll
                for (int i = 0; i < kLoads1; ++i)
                    if (wave + 4 * i < rows) t1[i] = src[(size_t)(wave + 4 * i) * (size_t)p.aw + lane];
#pragma unroll
                for (int i = 0; i < kLoads2; ++i)
                    if (row2 + 16 * i < rows && sub < extra) t2[i] = src[(size_t)(row2 + 16 * i) * (size_t)p.aw + kTileW + sub];
#pragma unroll
                for (int i = 0; i < kLoads1; ++i)
                    if (wave + 4 * i < rows) tile[(wave + 4 * i) * kPitch + lane] = t1[i];
#pragma unroll
                for (int i = 0; i < kLoads2; ++i)
                    if (row2 + 16 * i < rows && sub < extra) tile[(row2 + 16 * i) * kPitch + kTileW + sub] = t2[i];
            } else {
                for (int row = wave; row < rows; row += 4) tile[row * kPitch + lane] = cell(p, gr0 + row, gc0 + lane);
                for (int row = row2; row < rows; row += 16)
                    if (sub < extra) tile[row * kPitch + kTileW + sub] = cell(p, gr0 + row, gc0 + kTileW + sub);
            }
            __syncthreads();
            const float *col = tile + wave * kRegRows * kPitch + lane;
            for (int k = 0; k < nk; ++k) {
                float v[kRegRows + CH - 1];
#pragma unroll
                for (int i = 0; i < kRegRows + CH - 1; ++i) v[i] = col[i * kPitch + k];   // rows past the chunk's: inside the array, never used
#pragma unroll
                for (int j = 0; j < CH; ++j) {
                    if (j < nj) {      // uniform: a tap that does not exist is not added (0 * Inf would be NaN)
                        const float c = wbase[(long long)(j0 + j) * wsj + (long long)(k0 + k) * wsk];
#pragma unroll
                        for (int r = 0; r < kRegRows; ++r) acc[r] = fmaf(c, v[r + j], acc[r]);
                    }
                }
            }
        }
    }
    const long long n = x0 + lane;
    if (n >= p.ow) return;
#pragma unroll
    for (int r = 0; r < kRegRows; ++r) {
        const long long m = y0 + wave * kRegRows + r;
        if (m < p.oh) {
            const size_t at = p.reverse ? (size_t)(p.oh - 1 - m) * (size_t)p.ow + (size_t)(p.ow - 1 - n) : (size_t)m * (size_t)p.ow + (size_t)n;
            p.out[at] = acc[r];
        }
    }
}

bool covers(size_t ah, size_t aw, size_t bh, size_t bw) { return ah >= bh && aw >= bw; }

int check_extents(const char *who, size_t ah, size_t aw, size_t bh, size_t bw, int mode) {
    if (mode != NP_CONV_VALID && mode != NP_CONV_SAME && mode != NP_CONV_FULL) return np::fail(NP_ERR_INVALID, "%s: unknown mode %d", who, mode);
    if (ah < 1 || aw < 1 || bh < 1 || bw < 1) return np::fail(NP_ERR_INVALID, "%s: every extent must be at least 1", who);
    const size_t lim = (size_t)INT_MAX;
    if (ah > lim || aw > lim || bh > lim || bw > lim || (mode == NP_CONV_FULL && (ah + bh - 1 > lim || aw + bw - 1 > lim)))
        return np::fail(NP_ERR_INVALID, "%s: an extent does not fit the int shape of an NDArray", who);
    if (mode == NP_CONV_VALID && !covers(ah, aw, bh, bw) && !covers(bh, bw, ah, aw))
        return np::fail(NP_ERR_INVALID, "For 'valid' mode, one input must be at least as large as the other in every dimension");
    return NP_OK;
}

}  // namespace

extern "C" {

int np_correlate2d_shape(size_t ah, size_t aw, size_t bh, size_t bw, int mode, size_t *oh, size_t *ow) {
    if (!oh || !ow) return np::fail(NP_ERR_INVALID, "np_correlate2d_shape: null pointer");
    if (int rc = check_extents("np_correlate2d_shape", ah, aw, bh, bw, mode)) return rc;
    if (mode == NP_CONV_FULL) {
        *oh = ah + bh - 1;
        *ow = aw + bw - 1;
    } else if (mode == NP_CONV_SAME) {
        *oh = ah;
        *ow = aw;
    } else if (covers(ah, aw, bh, bw)) {
        *oh = ah - bh + 1;
        *ow = aw - bw + 1;
    } else {
        *oh = bh - ah + 1;
        *ow = bw - aw + 1;
    }
    return NP_OK;
}

int np_correlate2d(const float *a, size_t ah, size_t aw, const float *b, size_t bh, size_t bw, int mode, int boundary,
                   float fill_value, int flip, float *out) {
    // the argument checks need no device and come first: a refused call has touched nothing
    if (!a || !b || !out) return np::fail(NP_ERR_INVALID, "np_correlate2d: null pointer");
    if (boundary != NP_CONV_FILL && boundary != NP_CONV_SYMM && boundary != NP_CONV_WRAP)
        return np::fail(NP_ERR_INVALID, "np_correlate2d: unknown boundary %d", boundary);
    size_t oh = 0, ow = 0;
    if (int rc = np_correlate2d_shape(ah, aw, bh, bw, mode, &oh, &ow)) return rc;
    if (int rc = np::ensure_init()) return rc;
    // scipy's _inputs_swap_needed: in 'valid' mode the operand that does not cover the other becomes the window; a
    // correlation computed that way comes out reversed along both axes
    const bool swap = mode == NP_CONV_VALID && !covers(ah, aw, bh, bw);
    Conv2dArgs p = {};
    p.a = swap ? b : a;
    p.w = swap ? a : b;
    p.out = out;
    p.ah = (int)(swap ? bh : ah);
    p.aw = (int)(swap ? bw : aw);
    p.wh = (int)(swap ? ah : bh);
    p.ww = (int)(swap ? aw : bw);
    p.oh = (int)oh;
    p.ow = (int)ow;
    p.boundary = boundary;
    p.flip = flip ? 1 : 0;
    p.reverse = swap && !flip ? 1 : 0;
    p.fill = fill_value;
    // signal.c:155-157 / 164-166 in footprint coordinates: a convolution's first footprint row lies wh - 1 rows above the
    // reference's new_m
    if (mode == NP_CONV_FULL) {
        p.r0 = -(p.wh - 1);
        p.c0 = -(p.ww - 1);
    } else if (mode == NP_CONV_SAME) {
        p.r0 = flip ? -(p.wh / 2) : -((p.wh - 1) / 2);
        p.c0 = flip ? -(p.ww / 2) : -((p.ww - 1) / 2);
    }
    const size_t gx = (ow + kTileW - 1) / kTileW, gy = (oh + kTileH - 1) / kTileH;
    if (gx * gy > kMaxTiles) return np::fail(NP_ERR_INVALID, "np_correlate2d: a result of %zu x %zu is more than %zu tiles", oh, ow, kMaxTiles);
    const dim3 grid((unsigned)(gx * gy)), block(256);
    const bool staged = p.wh <= kSmallMax && p.ww <= kSmallMax && !g_conv2d_chunked_only;
    if (!staged) {
        conv2d_kernel<kChunk, true><<<grid, block, 0, np::stream()>>>(p);
    } else if (p.wh <= 3) {
        conv2d_kernel<3, false><<<grid, block, 0, np::stream()>>>(p);
    } else if (p.wh <= 7) {
        conv2d_kernel<7, false><<<grid, block, 0, np::stream()>>>(p);
    } else {
        conv2d_kernel<kSmallMax, false><<<grid, block, 0, np::stream()>>>(p);
    }
    NP_LAUNCH_CHECK("conv2d_kernel");
    g_conv2d_last_path = staged ? 1 : 2;
    return NP_OK;
}

int np_debug_conv2d_last_path(int *host_path) {
    if (!host_path) return np::fail(NP_ERR_INVALID, "np_debug_conv2d_last_path: null pointer");
    *host_path = g_conv2d_last_path;
    return NP_OK;
}

int np_debug_conv2d_staged_path(int on) {
    g_conv2d_chunked_only = on ? 0 : 1;
    return NP_OK;
}

}  // extern "C"
