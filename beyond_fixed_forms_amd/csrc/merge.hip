// The merge stage (include/bff_hip.h: a9-a12): row statistics, tile masks, the two tile-pair filters and the tile
// pass that finds the connected components of the merge graph with a union-find forest and no adjacency matrix;
// merge_adjacency_kernel, the adjacency-matrix form, is kept as an independent cross-check.
#include <hip/hip_ext.h>

#include <cstdlib>

#include "rows.h"

static thread_local hipEvent_t g_merge_start = nullptr, g_merge_stop = nullptr;   // bff_profile_next_merge

namespace bff {

// ---- row statistics for the block-sparse Gram -------------------------------------------------
// Per row: popcount, occupancy mask over chunks of kCW words, and the mean word position of its set
// bits (sort key that brings rows covering the same region of the -- spatially sorted -- cloud together).
constexpr int kBins = 64;     // histogram bins per row (each ceil(nw/64) words wide)

// 30-bit sort key of a row from its heavy-bin ballot: the first five heavy bins (ascending), 6 bits each, most
// significant first; unused slots = 63.  Rows of one object share the key whatever the view.
__device__ __forceinline__ int64_t heavy_signature(uint64_t heavy)
{
    uint32_t key = 0;
#pragma unroll
    for (int s = 0; s < 5; ++s) {
        int b = 63;
        if (heavy) { b = __ffsll((unsigned long long)heavy) - 1; heavy &= heavy - 1; }
        key = (key << 6) | (uint32_t)b;
    }
    return (int64_t)key;
}

__global__ __launch_bounds__(256) void row_stats_kernel(const uint64_t *__restrict__ rows, int64_t nw, int mw,
                                                         int bin_words, int32_t *__restrict__ area,
                                                         int32_t *__restrict__ mean_word,
                                                         uint64_t *__restrict__ cmask, uint32_t *__restrict__ hist,
                                                         int64_t *__restrict__ signature, uint16_t *__restrict__ cpop)
{
    extern __shared__ uint64_t s_cm[];                 // mw words
    __shared__ int part[4];
    __shared__ unsigned long long psum[4];
    __shared__ uint32_t s_hist[kBins];
    const int r = blockIdx.x, tid = threadIdx.x;
    const uint64_t *row = rows + (int64_t)r * nw;
    for (int i = tid; i < mw; i += 256) s_cm[i] = 0;
    if (tid < kBins) s_hist[tid] = 0;
    __syncthreads();
    int s = 0;
    unsigned long long ws = 0;
    for (int64_t w = tid; w < nw; w += 256) {
        const uint64_t v = row[w];
        if (v) {
            const int c = (int)(w / kCW);
            atomicOr((unsigned long long *)&s_cm[c >> 6], 1ull << (c & 63));
            const int pc = popc64(v);
            atomicAdd(&s_hist[(int)(w / bin_words)], (uint32_t)pc);
            s += pc;
            ws += (unsigned long long)pc * (unsigned long long)w;
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { s += __shfl_down(s, d); ws += __shfl_down(ws, d); }
    if (lane_id() == 0) { part[tid >> 6] = s; psum[tid >> 6] = ws; }
    __syncthreads();
    for (int i = tid; i < mw; i += 256) cmask[(int64_t)r * mw + i] = s_cm[i];
    if (cpop) {                                    // points per 512-point chunk (second-level bound of the tile pass)
        const int n_chunks = (int)((nw + kCW - 1) / kCW);
        for (int c = tid; c < mw * 64; c += 256) {
            int pc = 0;
            if (c < n_chunks)
#pragma unroll
                for (int k = 0; k < kCW; ++k) { const int64_t w = (int64_t)c * kCW + k; if (w < nw) pc += popc64(row[w]); }
            cpop[(int64_t)r * mw * 64 + c] = (uint16_t)pc;
        }
    }
    const int a_all = part[0] + part[1] + part[2] + part[3];
    if (tid < kBins) {
        hist[(int64_t)r * kBins + tid] = s_hist[tid];
        // bins holding >= 15 % of the row: rows of one object share this signature whatever the view, and
        // stray "bleed" points never enter it.
        const uint64_t heavy = __ballot((uint64_t)s_hist[tid] * 100 >= (uint64_t)a_all * 15 && a_all > 0);
        if (tid == 0) signature[r] = heavy_signature(a_all ? heavy : 0);
    }
    if (tid == 0) {
        const int a = part[0] + part[1] + part[2] + part[3];
        const unsigned long long t = psum[0] + psum[1] + psum[2] + psum[3];
        area[r] = a;
        mean_word[r] = a ? (int32_t)(t / (unsigned long long)a) : 0x7fffffff;   // empty rows sort last
    }
}

// The same statistics when the rows' chunk masks are already known (the sweep flags the chunks it stores
// into): one wave per row, lane l takes the flagged chunks l, l+64, ... and reads only those 64 bytes.
__global__ __launch_bounds__(256) void row_stats_sparse_kernel(const uint64_t *__restrict__ rows, int n_rows, int64_t nw,
                                                                int mw, int bin_words, int32_t *__restrict__ area,
                                                                int32_t *__restrict__ mean_word,
                                                                const uint64_t *__restrict__ cmask,
                                                                uint32_t *__restrict__ hist, int64_t *__restrict__ signature,
                                                                uint16_t *__restrict__ cpop)
{
    __shared__ uint32_t s_hist[4][kBins];
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const int r = blockIdx.x * 4 + wave;
    if (r >= n_rows) return;                                   // wave-uniform; no block barrier below
    const uint64_t *row = rows + (int64_t)r * nw;
    uint32_t *hs = s_hist[wave];
    hs[lane] = 0;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    int s = 0;
    unsigned long long ws = 0;
    for (int i = 0; i < mw; ++i) {
        const uint64_t m = cmask[(int64_t)r * mw + i];
        if ((m >> lane) & 1) {
            const int64_t w0 = ((int64_t)i * 64 + lane) * kCW;
            int in_chunk = 0;
#pragma unroll
            for (int k = 0; k < kCW; ++k) {
                const int64_t w = w0 + k;
                const uint64_t v = w < nw ? row[w] : 0;
                if (v) {
                    const int pc = popc64(v);
                    atomicAdd(&hs[(int)(w / bin_words)], (uint32_t)pc);
                    s += pc;
                    in_chunk += pc;
                    ws += (unsigned long long)pc * (unsigned long long)w;
                }
            }
            if (cpop) cpop[(int64_t)r * mw * 64 + i * 64 + lane] = (uint16_t)in_chunk;     // unflagged chunks: zeroed by the caller
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { s += __shfl_xor(s, d); ws += __shfl_xor(ws, d); }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    const uint32_t hv = hs[lane];
    hist[(int64_t)r * kBins + lane] = hv;
    const uint64_t heavy = __ballot((uint64_t)hv * 100 >= (uint64_t)s * 15 && s > 0);
    if (lane == 0) {
        signature[r] = heavy_signature(s ? heavy : 0);
        area[r] = s;
        mean_word[r] = s ? (int32_t)(ws / (unsigned long long)s) : 0x7fffffff;
    }
}

// Per tile t (rows order[64t .. 64t+63]): tmask[t] = OR of the rows' chunk masks; optionally the sorted,
// packed histogram copy hist_sorted[bin pair][position] (two 16-bit bins per word: coalesced tile loads, one
// v_pk_min_u16 + v_dot2_u32_u16 per two bins), the bin-wise maxima and the smallest non-empty area of the tile.
// 256 threads: thread (k = tid & 63, q = tid >> 6) works on row k of the tile.
__global__ __launch_bounds__(256) void tile_masks_kernel(const uint64_t *__restrict__ cmask,
                                                          const int32_t *__restrict__ order, int n, int mw,
                                                          uint64_t *__restrict__ tmask, const uint32_t *__restrict__ hist,
                                                          uint32_t *__restrict__ hist_sorted, int n_pos,
                                                          const int32_t *__restrict__ area,
                                                          uint32_t *__restrict__ tile_hmax, int32_t *__restrict__ tile_amin,
                                                          const int32_t *__restrict__ label_id,
                                                          int32_t *__restrict__ row_sorted, int32_t *__restrict__ area_sorted,
                                                          int32_t *__restrict__ label_sorted, int32_t *__restrict__ parent_init)
{
    __shared__ uint32_t s_hmax[kBins];
    __shared__ int s_amin;
    const int t = blockIdx.x, tid = threadIdx.x, k = tid & 63, q = tid >> 6;
    const int pos = t * kT + k;
    const int row = pos < n ? (order ? order[pos] : pos) : -1;
    if (parent_init && q == 0 && row >= 0) parent_init[row] = row;     // disjoint-set forest: every row its own root
    // chunk-mask OR: lanes = rows, each wave takes every 4th mask word and OR-reduces it across the wave
    for (int i = q; i < mw; i += 4) {
        uint64_t v = row >= 0 ? cmask[(int64_t)row * mw + i] : 0;
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) v |= __shfl_xor(v, d);
        if (k == 0) tmask[(int64_t)t * mw + i] = v;
    }
    if (!hist_sorted) return;
    if (tid < kBins) s_hmax[tid] = 0;
    if (tid == 0) s_amin = 0x7fffffff;
    __syncthreads();
    // wave q handles bin pairs q, q+4, ...: row k's two bins -> packed word, tile maxima via LDS atomics
    for (int b = q; b < kBins / 2; b += 4) {
        const uint32_t lo = row >= 0 ? hist[(int64_t)row * kBins + 2 * b] : 0;
        const uint32_t hi = row >= 0 ? hist[(int64_t)row * kBins + 2 * b + 1] : 0;
        hist_sorted[(int64_t)b * n_pos + pos] = lo | (hi << 16);
        uint32_t mlo = lo, mhi = hi;
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) { mlo = max(mlo, (uint32_t)__shfl_xor(mlo, d)); mhi = max(mhi, (uint32_t)__shfl_xor(mhi, d)); }
        if (k == 0) { s_hmax[2 * b] = mlo; s_hmax[2 * b + 1] = mhi; }
    }
    if (q == 0) {
        int a = row >= 0 ? area[row] : 0;
        if (row_sorted) {                          // position-indexed copies: the tile pass loads them coalesced
            row_sorted[pos] = row;
            area_sorted[pos] = a;
            label_sorted[pos] = row >= 0 ? label_id[row] : -1;
        }
        a = a > 0 ? a : 0x7fffffff;
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) a = min(a, __shfl_xor(a, d));
        if (k == 0) s_amin = a;
    }
    __syncthreads();
    if (tid < kBins) tile_hmax[(int64_t)t * kBins + tid] = s_hmax[tid];
    if (tid == 0) tile_amin[t] = s_amin;
}

// Upper-triangular tile pairs of the symmetric Gram matrix.  Tile (bi, bj) covers rows
// order[64 bi ..] x order[64 bj ..]; with tile chunk masks it visits only the chunks of kCW words
// that both tiles occupy (four chunks = 32 words per LDS stage), otherwise every word.  The epilogue
// applies the reference's float32 IoU test and emits adjacency words for the tile and its mirror
// image, indexed by position in `order`.
constexpr int kMaxChunks = 4096;     // chunk list capacity (LDS): N <= 4096*512 = 2.1 M points per call
constexpr int kSplitStages = 12;     // split mode: LDS stages per part (a part = ~50 us of tile pass)
constexpr int kMaxParts = 8;         // parts per tile pair
constexpr int kMaxSlots = 512;       // tile pairs that can be split in one call (16 KiB of partial counts each)

__global__ __launch_bounds__(256) void merge_adjacency_kernel(const uint64_t *__restrict__ rows, int n, int64_t nw,
                                                               const int32_t *__restrict__ order,
                                                               const uint64_t *__restrict__ tmask, int mw,
                                                               const uint32_t *__restrict__ hist,
                                                               const int32_t *__restrict__ area,
                                                               const int32_t *__restrict__ label_id, float thr,
                                                               uint64_t *__restrict__ adj, int aw,
                                                               int32_t *__restrict__ inter, int n_tiles)
{
    __shared__ uint64_t sa[kKW][kPitch], sb[kKW][kPitch];
    __shared__ uint8_t flag[kT][kT + 4];
    __shared__ uint16_t clist[kMaxChunks];
    __shared__ int s_cnt;
    // linear upper-triangular index -> (bi <= bj)
    int t = blockIdx.x, bi = 0;
    while (t >= n_tiles - bi) { t -= n_tiles - bi; ++bi; }
    const int bj = bi + t;
    const int i0 = bi * kT, j0 = bj * kT;
    const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;
    const int n_chunks = (int)((nw + kCW - 1) / kCW);

    // ---- can any pair of this tile be adjacent at all?  I(i,j) <= UB = sum over 64 bins of
    // min(hist_i, hist_j); the float32 IoU expression below is monotone non-decreasing in I (a_i + a_j
    // fixed, correctly rounded ops), so "label equal and iou(min(UB, a_i, a_j)) > thr" is a sound
    // superset of the adjacent pairs.  A tile without candidates skips its word loop (all bits 0).
    bool any_candidate = true;
    if (hist) {
        uint32_t (*ha)[kBins] = reinterpret_cast<uint32_t (*)[kBins]>(&sa[0][0]);    // [bin][row], 16 KB each
        uint32_t (*hb)[kBins] = reinterpret_cast<uint32_t (*)[kBins]>(&sb[0][0]);
        {
            const int lane = tid & 63, wv = tid >> 6;
            const int ra = i0 + lane, rb = j0 + lane;
            const uint32_t *ga = ra < n ? hist + (int64_t)(order ? order[ra] : ra) * kBins : nullptr;
            const uint32_t *gb = rb < n ? hist + (int64_t)(order ? order[rb] : rb) * kBins : nullptr;
#pragma unroll
            for (int q = 0; q < kBins / 4; ++q) {
                const int b = wv * (kBins / 4) + q;
                ha[b][lane] = ga ? ga[b] : 0;
                hb[b][lane] = gb ? gb[b] : 0;
            }
        }
        __syncthreads();
        uint32_t ub[4][4];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) ub[r][c] = 0;
#pragma unroll 4
        for (int b = 0; b < kBins; ++b) {
            uint32_t av[4], bv[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) { av[r] = ha[b][ti * 4 + r]; bv[r] = hb[b][tj * 4 + r]; }
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) ub[r][c] += min(av[r], bv[c]);
        }
        bool cand = false;
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int si = i0 + ti * 4 + r, sj = j0 + tj * 4 + c;
                if (si < n && sj < n) {
                    const int i = order ? order[si] : si, j = order ? order[sj] : sj;
                    const int ai = area[i], aj = area[j];
                    const float fi = (float)min((int)ub[r][c], min(ai, aj));
                    const float iou = __fdiv_rn(fi, (float)ai + (float)aj - fi);
                    cand |= (label_id[i] == label_id[j]) && (iou > thr);
                }
            }
        any_candidate = __syncthreads_or(cand);
    }

    // ---- chunks to visit
    if (tid < kWave) {
        int base = 0;
        for (int m = 0; m < (n_chunks + 63) / 64; ++m) {
            const uint64_t bits = tmask ? (tmask[(int64_t)bi * mw + m] & tmask[(int64_t)bj * mw + m]) : ~0ull;
            const int c = m * 64 + tid;
            const bool on = ((bits >> tid) & 1) && c < n_chunks;
            const uint64_t bal = __ballot(on);
            if (on) clist[base + __popcll(bal & ((1ull << tid) - 1))] = (uint16_t)c;
            base += __popcll(bal);
        }
        if (tid == 0) s_cnt = base;
    }
    __syncthreads();
    const int cnt = any_candidate ? s_cnt : 0;

    int acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = 0;
    if (cnt) {
        const int lk = tid & (kKW - 1), lr = tid >> 5;      // loader: staged word lk of rows lr, lr+8, ...
        const int slot = lk / kCW, cw = lk % kCW;
        const uint64_t *pa[8];
        const uint64_t *pb[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int ra = i0 + lr + 8 * q, rb = j0 + lr + 8 * q;
            pa[q] = ra < n ? rows + (int64_t)(order ? order[ra] : ra) * nw : nullptr;
            pb[q] = rb < n ? rows + (int64_t)(order ? order[rb] : rb) * nw : nullptr;
        }
        for (int g = 0; g < cnt; g += kKW / kCW) {
            const int64_t w = (g + slot < cnt) ? (int64_t)clist[g + slot] * kCW + cw : nw;
            const bool kin = w < nw;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                sa[lk][lr + 8 * q] = (kin && pa[q]) ? pa[q][w] : 0;
                sb[lk][lr + 8 * q] = (kin && pb[q]) ? pb[q][w] : 0;
            }
            __syncthreads();
#pragma unroll 8
            for (int kk = 0; kk < kKW; ++kk) {
                uint64_t av[4], bv[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) { av[r] = sa[kk][ti * 4 + r]; bv[r] = sb[kk][tj * 4 + r]; }
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int c = 0; c < 4; ++c) acc[r][c] += popc64(av[r] & bv[c]);
            }
            __syncthreads();
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int si = i0 + ti * 4 + r, sj = j0 + tj * 4 + c;
            bool ok = false;
            if (si < n && sj < n) {
                const int i = order ? order[si] : si, j = order ? order[sj] : sj;
                const float fi = (float)acc[r][c];
                const float uni = (float)area[i] + (float)area[j] - fi;
                const float iou = __fdiv_rn(fi, uni);           // 0/0 -> NaN -> compares false
                ok = (label_id[i] == label_id[j]) && (iou > thr);
                if (inter) {
                    inter[(int64_t)i * n + j] = acc[r][c];
                    inter[(int64_t)j * n + i] = acc[r][c];
                }
            }
            flag[ti * 4 + r][tj * 4 + c] = ok ? 1 : 0;
        }
    __syncthreads();
    if (tid < kT) {
        const int i = i0 + tid;
        if (i < n) {
            uint64_t w = 0;
            for (int c = 0; c < kT; ++c) w |= (uint64_t)flag[tid][c] << c;
            adj[(int64_t)i * aw + bj] = w;
        }
    } else if (tid < 2 * kT && bi != bj) {
        const int c = tid - kT, j = j0 + c;
        if (j < n) {
            uint64_t w = 0;
            for (int r = 0; r < kT; ++r) w |= (uint64_t)flag[r][c] << r;
            adj[(int64_t)j * aw + bi] = w;
        }
    }
}

// ---- components without an adjacency matrix: union-find in the tile epilogue -----------------------
// The forest, uf_find and uf_union: rows.h.
__global__ void uf_init_kernel(int32_t *parent, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) parent[i] = i;
}

__global__ void uf_flatten_kernel(int32_t *parent, int n, int32_t *comp)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) comp[i] = uf_find(parent, i);                      // = smallest row index of the component
}

// Tile pairs are enumerated diagonal-first (|bi - bj| = 0, 1, 2, ...): with rows clustered by signature
// the first tiles discover the large components, and later tiles find most of their possible edges
// already inside one component and skip their word loop.  index t -> (bi, d = bj - bi).
__device__ __forceinline__ void tile_pair_of(int t, int n_tiles, int &bi, int &d)
{
    // offset of diagonal d: d * n_tiles - d (d - 1) / 2; invert with a float estimate and fix up
    const double a = 2.0 * n_tiles + 1.0;
    int dd = (int)((a - sqrt(a * a - 8.0 * (double)t)) * 0.5);
    dd = max(0, min(dd, n_tiles - 1));
    auto off = [&](int q) { return (int64_t)q * n_tiles - (int64_t)q * (q - 1) / 2; };
    while (dd > 0 && off(dd) > t) --dd;
    while (dd + 1 < n_tiles && off(dd + 1) <= t) ++dd;
    d = dd;
    bi = (int)(t - off(dd));
}

// Tile-level quick reject for every tile pair, ahead of the tile pass: the pairs that can hold an edge are
// appended to `list` (wave-aggregated, so the list keeps the diagonal-first order up to wave granularity).
// Every pair of rows of tiles (A, B) has I <= u = sum_b min(maxA[b], maxB[b]) and a_i + a_j >= aminA + aminB,
// hence IoU = I / (a_i + a_j - I) <= u / (aminA + aminB - u) whenever that denominator is positive (float32
// evaluation is monotone in both arguments); otherwise no conclusion.
__global__ __launch_bounds__(256) void tile_pair_filter_kernel(const uint32_t *__restrict__ tile_hmax,
                                                                const int32_t *__restrict__ tile_amin, int n_tiles,
                                                                int total, float thr, int32_t *__restrict__ list,
                                                                int32_t *__restrict__ count)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    bool possible = false;
    if (t < total) {
        int bi, d;
        tile_pair_of(t, n_tiles, bi, d);
        const int bj = bi + d;
        const int amin_a = tile_amin[bi], amin_b = tile_amin[bj];
        // a tile of empty rows has no edges at all -- unless the threshold is negative: an empty row then links to
        // every non-empty row of its label (IoU 0 > thr, P:149-166), and the bound below holds with amin = INT_MAX
        // too (quotient >= 0 > thr)
        if (0.0f > thr || (amin_a != 0x7fffffff && amin_b != 0x7fffffff)) {
            const uint4 *ha = reinterpret_cast<const uint4 *>(tile_hmax + (int64_t)bi * kBins);
            const uint4 *hb = reinterpret_cast<const uint4 *>(tile_hmax + (int64_t)bj * kBins);
            uint32_t u = 0;
#pragma unroll 4
            for (int q = 0; q < kBins / 4; ++q) {
                const uint4 x = ha[q], y = hb[q];
                u += min(x.x, y.x) + min(x.y, y.y) + min(x.z, y.z) + min(x.w, y.w);
            }
            const float fi = (float)u;
            const float den = (float)amin_a + (float)amin_b - fi;
            possible = !(den > 0.0f) || (__fdiv_rn(fi, den) > thr);
        }
    }
    const uint64_t bal = __ballot(possible);
    if (!bal) return;
    const int lane = lane_id();
    int base = 0;
    if (lane == 0) base = atomicAdd(count, __popcll(bal));
    base = __shfl(base, 0);
    if (possible) list[base + __popcll(bal & ((1ull << lane) - 1))] = t;
}

// Row-level bound for the tile pairs that survived the tile-level one: one wave per listed pair, lane k = row k of
// tile A (then of tile B).  Row i of A against the bin-wise maxima of tile B: I(i, j) <= u_i = sum_b min(h_i[b],
// maxB[b]) for every j of B and a_j >= aminB, so IoU(i, j) <= min(u_i, a_i) / (a_i + aminB - min(u_i, a_i)) whenever the
// denominator is positive (same monotone float32 expression as the exact test).  Rows that fail cannot have an edge
// into the other tile.  Pairs in which some row of A and some row of B pass are appended to list2 together with
// the two 64-bit pass masks; most pairs end here, at the cost of one wave instead of a 256-thread block.
__global__ __launch_bounds__(256) void tile_pair_rows_kernel(const uint32_t *__restrict__ hist, int n_pos,
                                                              const int32_t *__restrict__ area_sorted,
                                                              const uint32_t *__restrict__ tile_hmax,
                                                              const int32_t *__restrict__ tile_amin, int n_tiles, float thr,
                                                              const int32_t *__restrict__ list1,
                                                              const int32_t *__restrict__ count1,
                                                              int32_t *__restrict__ list2, uint64_t *__restrict__ pass2,
                                                              int32_t *__restrict__ count2,
                                                              const uint64_t *__restrict__ tmask, int mw,
                                                              int32_t *__restrict__ part2, int32_t *__restrict__ n_slots,
                                                              int list_cap)
{
    const int lane = lane_id();
    const int e = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (e >= *count1) return;                                      // wave-uniform
    const int t = list1[e];
    int bi, d;
    tile_pair_of(t, n_tiles, bi, d);
    const int bj = bi + d;
    constexpr int kBP = kBins / 2;
    // lane b holds bin b of both tiles' maxima; read back per bin pair with a wave broadcast
    const uint32_t hmA = tile_hmax[(int64_t)bi * kBins + lane], hmB = tile_hmax[(int64_t)bj * kBins + lane];
    const int aA = area_sorted[bi * kT + lane], aB = area_sorted[bj * kT + lane];
    const int aminA = tile_amin[bi], aminB = tile_amin[bj];
    uint32_t uA = 0, uB = 0;
#pragma unroll                                    // fully: the broadcasts below become v_readlane with constant lanes
    for (int b = 0; b < kBP; ++b) {
        const uint32_t wa = hist[(int64_t)b * n_pos + bi * kT + lane];
        const uint32_t wb = hist[(int64_t)b * n_pos + bj * kT + lane];
        const uint32_t mB0 = __shfl(hmB, 2 * b), mB1 = __shfl(hmB, 2 * b + 1);
        const uint32_t mA0 = __shfl(hmA, 2 * b), mA1 = __shfl(hmA, 2 * b + 1);
        uA += min(wa & 0xffffu, mB0) + min(wa >> 16, mB1);
        uB += min(wb & 0xffffu, mA0) + min(wb >> 16, mA1);
    }
    // padding positions carry area 0 and an all-zero histogram: with thr >= 0 they fail (0/x or NaN), with thr < 0
    // the tile pass ignores them by their row index (-1)
    auto passes = [&](uint32_t u, int a_self, int a_other) {
        const float fi = (float)min((int)u, a_self);
        const float den = (float)a_self + (float)a_other - fi;
        return !(den > 0.0f) || (__fdiv_rn(fi, den) > thr);
    };
    const uint64_t pa = __ballot(passes(uA, aA, aminB));
    const uint64_t pb = __ballot(passes(uB, aB, aminA));
    if (!pa || !pb) return;
    // Tile pairs that share many chunks are the longest blocks of the tile pass (up to the whole cloud: 100 LDS
    // stages); their chunk list is dealt to several blocks (kSplitStages stages each, at most kMaxParts) whose
    // partial intersections meet in a scratch slot (merge_tile_pair, split mode).
    int shared = 0;
    if (tmask && lane < mw) shared = __popcll(tmask[(int64_t)bi * mw + lane] & tmask[(int64_t)bj * mw + lane]);
#pragma unroll
    for (int dd = 32; dd > 0; dd >>= 1) shared += __shfl_xor(shared, dd);
    if (lane == 0) {
        int n_parts = 1, slot = 0;
        if (part2 && shared >= 2 * kSplitStages * (kKW / kCW)) {
            n_parts = min(kMaxParts, shared / (kSplitStages * (kKW / kCW)));
            slot = atomicAdd(n_slots, 1);
            if (slot >= kMaxSlots) n_parts = 1;                    // out of slots: one block, as before
        }
        const int at = atomicAdd(count2, n_parts);
        if (at + n_parts > list_cap) return;                       // cannot happen with the caps chosen by the host
        for (int p = 0; p < n_parts; ++p) {
            list2[at + p] = t;
            pass2[2 * (at + p)] = pa;
            pass2[2 * (at + p) + 1] = pb;
            if (part2) part2[at + p] = n_parts > 1 ? ((slot << 8) | (n_parts << 4) | p) : 0;
        }
    }
}

// diagnostics only: thread 0 adds the cycles since *t0 to diag[slot] (>> 6 to stay inside int32) and restarts the clock
__device__ __forceinline__ void diag_lap(int32_t *diag, int slot, long long *t0)
{
    if (diag && threadIdx.x == 0) {
        const long long now = (long long)__builtin_readcyclecounter();
        atomicAdd(diag + slot, (int)((now - *t0) >> 6));
        *t0 = now;
    }
}

// Disjoint sets over the 128 rows of ONE tile pair, in LDS (ids 0..63 = rows of A, 64..127 = rows of B; links go
// to the smaller id).  They start from the global forest (rows that share a global root share a local set) and
// absorb every edge the block proves, so that (a) a pair whose rows have meanwhile become connected inside the
// tile is dropped without finishing its intersection and (b) only the edges that merge two local sets -- at most
// 127 per tile pair -- are pushed into the global forest with compare-and-swap.
__device__ __forceinline__ int local_find(volatile int *lid, int x)
{
    int p = lid[x];
    while (p != x) { x = p; p = lid[x]; }
    return x;
}

__device__ __forceinline__ bool local_union(int *lid, int a, int b)
{
    for (;;) {
        a = local_find(lid, a);
        b = local_find(lid, b);
        if (a == b) return false;
        if (a < b) { const int t = a; a = b; b = t; }              // a > b: hang a under b
        if (atomicCAS(&lid[a], a, b) == a) return true;
    }
}

__shared__ int g_block_info[2];        // [0] candidate pairs | shared chunks << 16, [1] LDS stages executed (diagnostics)

template <bool kDiag>
__device__ __forceinline__ void merge_tile_pair(int t, uint64_t pass_a, uint64_t pass_b,
                                                const uint64_t *__restrict__ rows, int n, int64_t nw,
                                                const uint64_t *__restrict__ tmask, int mw,
                                                const uint32_t *__restrict__ hist, int n_pos,
                                                const int32_t *__restrict__ row_sorted,
                                                const int32_t *__restrict__ area_sorted,
                                                const int32_t *__restrict__ label_sorted, float thr,
                                                int32_t *__restrict__ parent, int n_tiles,
                                                int32_t *__restrict__ diag, const uint16_t *__restrict__ cpop,
                                                int part_info, int32_t *__restrict__ partial, int32_t *__restrict__ arrive)
{
    // split mode (part_info != 0): this block is part `part` of `n_parts` of the tile pair and counts only every
    // n_parts-th LDS stage of the chunk list.  All parts must agree on the candidate pairs, so those come from the
    // static bounds alone (not from the forest, which changes while the parts run), nothing is settled early, and the
    // partial counts are added into the pair's scratch slot; the part that arrives last reads the sums and decides.
    const bool split = part_info != 0;
    const int part = part_info & 15, n_parts = split ? (part_info >> 4) & 15 : 1, pslot = part_info >> 8;
    __shared__ uint64_t sa[kKW][kPitch], sb[kKW][kPitch];
    __shared__ uint16_t clist[kMaxChunks];
    __shared__ int s_cnt;
    __shared__ int rowA[kT], rowB[kT], rootA[kT], rootB[kT];
    __shared__ int areaA[kT], areaB[kT], labA[kT], labB[kT];       // fetched once per tile pair
    __shared__ int lid[2 * kT];                                    // local disjoint sets, see above
    int bi, d;
    tile_pair_of(t, n_tiles, bi, d);
    const int bj = bi + d;
    const int i0 = bi * kT, j0 = bj * kT;
    const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;
    const int n_chunks = (int)((nw + kCW - 1) / kCW);
    long long t_lap = kDiag ? (long long)__builtin_readcyclecounter() : 0;     // kDiag: counters + phase clocks

    // one round trip: position-indexed row / area / label of the 128 rows, then the roots of the rows that can
    // still have an edge into the other tile (the others never enter a candidate pair)
    if (tid < kT) {
        const int row = row_sorted[i0 + tid];
        const bool live = row >= 0 && ((pass_a >> tid) & 1);
        rowA[tid] = row;
        areaA[tid] = area_sorted[i0 + tid];
        labA[tid] = label_sorted[i0 + tid];
        rootA[tid] = live ? (split ? row : uf_find(parent, row)) : -1;
    } else if (tid < 2 * kT) {
        const int k = tid - kT;
        const int row = row_sorted[j0 + k];
        const bool live = row >= 0 && ((pass_b >> k) & 1);
        rowB[k] = row;
        areaB[k] = area_sorted[j0 + k];
        labB[k] = label_sorted[j0 + k];
        rootB[k] = live ? (split ? row : uf_find(parent, row)) : -2;
    }
    // histogram bound (see merge_adjacency_kernel): possible edges only.  hist holds two 16-bit bins per
    // word, so one v_pk_min_u16 + one v_dot2_u32_u16 accumulates two bins of sum_b min(hist_i, hist_j).
    constexpr int kBP = kBins / 2;
    uint32_t (*ha)[kT] = reinterpret_cast<uint32_t (*)[kT]>(&sa[0][0]);      // [bin pair][row], 8 KB each
    uint32_t (*hb)[kT] = reinterpret_cast<uint32_t (*)[kT]>(&sb[0][0]);
    {
        const int lane = tid & 63, wv = tid >> 6;          // 256-B coalesced rows of the sorted histogram
#pragma unroll
        for (int q = 0; q < kBP / 4; ++q) {
            const int b = wv * (kBP / 4) + q;
            ha[b][lane] = hist[(int64_t)b * n_pos + i0 + lane];
            hb[b][lane] = hist[(int64_t)b * n_pos + j0 + lane];
        }
    }
    __syncthreads();
    if (kDiag) diag_lap(diag, 4, &t_lap);                                     // rows, roots, histogram staging
    // local sets start from the global forest: a live row joins the first live row of the tile pair with its root
    if (tid < 2 * kT) {                            // waves 0 and 1; loops without early exit: the LDS reads pipeline
        const int mine = tid < kT ? rootA[tid] : rootB[tid - kT];
        int first = tid;
#pragma unroll 16
        for (int q = 0; q < kT; ++q)
            if (rootA[q] == mine && q < first) first = q;
        if (tid >= kT) {
#pragma unroll 16
            for (int q = 0; q < kT; ++q)
                if (rootB[q] == mine && kT + q < first) first = kT + q;
        }
        lid[tid] = mine >= 0 ? first : tid;        // roots of rows that cannot have an edge are -1 / -2: sets of their own
    }
    typedef unsigned short us2 __attribute__((ext_vector_type(2)));
    uint32_t ub[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) ub[r][c] = 0;
    const us2 ones = {1, 1};
    const uint32_t mine_a = (uint32_t)(pass_a >> (ti * 4)) & 0xFu;          // 4 flags each
    const uint32_t mine_b = (uint32_t)(pass_b >> (tj * 4)) & 0xFu;
    if (mine_a && mine_b)
#pragma unroll 4
    for (int b = 0; b < kBP; ++b) {
        uint32_t av[4], bv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) { av[r] = ha[b][ti * 4 + r]; bv[r] = hb[b][tj * 4 + r]; }
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const us2 m = __builtin_elementwise_min(__builtin_bit_cast(us2, av[r]), __builtin_bit_cast(us2, bv[c]));
                ub[r][c] = __builtin_amdgcn_udot2(m, ones, ub[r][c], false);
            }
    }
    unsigned cand = 0;                                             // bit 4r+c: pair still needs the exact test
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int i = rowA[ti * 4 + r], j = rowB[tj * 4 + c];
            if (((mine_a >> r) & 1) && ((mine_b >> c) & 1) && i >= 0 && j >= 0 && i != j &&
                rootA[ti * 4 + r] != rootB[tj * 4 + c] && (d > 0 || ti * 4 + r < tj * 4 + c)) {
                const int ai = areaA[ti * 4 + r], aj = areaB[tj * 4 + c];
                const float fi = (float)min((int)ub[r][c], min(ai, aj));
                const float iou = __fdiv_rn(fi, (float)ai + (float)aj - fi);
                if ((labA[ti * 4 + r] == labB[tj * 4 + c]) && (iou > thr)) cand |= 1u << (4 * r + c);
            }
        }
    int any_candidate = __syncthreads_or(cand != 0);
    if (kDiag) diag_lap(diag, 5, &t_lap);                                     // per-pair histogram bound
    if (!any_candidate) return;                                    // block-uniform

    __shared__ uint16_t plist[kT * kT];
    __shared__ int wbase[4];
    const int lane = tid & 63, wv = tid >> 6;
    if (tid < kWave) {                                             // chunks both tiles occupy
        int base = 0;
        for (int m = 0; m < (n_chunks + 63) / 64; ++m) {
            const uint64_t bits = tmask ? (tmask[(int64_t)bi * mw + m] & tmask[(int64_t)bj * mw + m]) : ~0ull;
            const int c = m * 64 + tid;
            const bool on = ((bits >> tid) & 1) && c < n_chunks;
            const uint64_t bal = __ballot(on);
            if (on) clist[base + __popcll(bal & ((1ull << tid) - 1))] = (uint16_t)c;
            base += __popcll(bal);
        }
        if (tid == 0) s_cnt = base;
    }
    __syncthreads();
    // ---- second-level bound, same expression with the 512-point chunks both tiles occupy as the bins:
    // I(i, j) <= sum over shared chunks of min(points of i in the chunk, points of j in the chunk).  A bin of the
    // first bound spans several thousand points; objects that are neighbours in space (or two groups of views of one
    // object) share bins but far fewer points per chunk -- most surviving non-edges are decided here, for 2 bytes
    // per (row, chunk) instead of the chunk's 64 bytes.
    if (cpop && tmask) {
        uint32_t (*pa2)[kT] = reinterpret_cast<uint32_t (*)[kT]>(&sa[0][0]);      // [chunk pair][row]: two chunks per word
        uint32_t (*pb2)[kT] = reinterpret_cast<uint32_t (*)[kT]>(&sb[0][0]);
        constexpr int kPairsPerStep = 64;                          // 128 chunks per step (16 KB per side)
        const int cnt2 = s_cnt;
        const int64_t cstride = (int64_t)mw * 64;
        uint32_t ub2[4][4];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) ub2[r][c] = 0;
        for (int c0 = 0; c0 < cnt2; c0 += 2 * kPairsPerStep) {
            const int n_here = min(2 * kPairsPerStep, cnt2 - c0), np_here = (n_here + 1) / 2;
            // thread (row k of A or B, strided over chunk pairs): 2-byte gathers along the row's chunk table
            for (int q = tid; q < np_here * 2 * kT; q += 256) {
                const int kp = q / (2 * kT), rr = q % (2 * kT);
                const int row = rr < kT ? rowA[rr] : rowB[rr - kT];
                uint32_t v = 0;
                if (row >= 0) {
                    const uint16_t *t = cpop + (int64_t)row * cstride;
                    const int s0 = c0 + 2 * kp;
                    v = t[clist[s0]];
                    if (s0 + 1 < cnt2) v |= (uint32_t)t[clist[s0 + 1]] << 16;
                }
                if (rr < kT) pa2[kp][rr] = v; else pb2[kp][rr - kT] = v;
            }
            __syncthreads();
            if (cand)
                for (int kp = 0; kp < np_here; ++kp) {
                    uint32_t av[4], bv[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) { av[r] = pa2[kp][ti * 4 + r]; bv[r] = pb2[kp][tj * 4 + r]; }
#pragma unroll
                    for (int r = 0; r < 4; ++r)
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            const us2 m = __builtin_elementwise_min(__builtin_bit_cast(us2, av[r]), __builtin_bit_cast(us2, bv[c]));
                            ub2[r][c] = __builtin_amdgcn_udot2(m, ones, ub2[r][c], false);
                        }
                }
            __syncthreads();
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (cand & (1u << (4 * r + c))) {
                    const int ai = areaA[ti * 4 + r], aj = areaB[tj * 4 + c];
                    const float fi = (float)min((int)ub2[r][c], min(ai, aj));
                    const float iou = __fdiv_rn(fi, (float)ai + (float)aj - fi);
                    if (!(iou > thr)) cand &= ~(1u << (4 * r + c));
                }
        any_candidate = __syncthreads_or(cand != 0);
        if (kDiag) diag_lap(diag, 11, &t_lap);                                // chunk-level bound
        if (!any_candidate) return;                                // block-uniform
    }

    // ---- compact the candidate pairs of the tile: (row index in A) << 8 | (row index in B)
    const int mine_n = __popc(cand);
    int incl = mine_n;
#pragma unroll
    for (int q = 1; q < 64; q <<= 1) { const int up = __shfl_up(incl, q); if (lane >= q) incl += up; }
    if (lane == 63) wbase[wv] = incl;
    __shared__ unsigned long long s_live[2];                       // rows that still take part in a candidate pair
    if (tid < 2) s_live[tid] = 0;
    __syncthreads();
    int pos = incl - mine_n;
    for (int q = 0; q < wv; ++q) pos += wbase[q];
    const int n_pairs = wbase[0] + wbase[1] + wbase[2] + wbase[3];
    if (tid == 0) g_block_info[0] = n_pairs | (s_cnt << 16);      // timeline diagnostics (mode 2) read this
    // only the words of rows in a candidate pair are fetched below (the others stage as zeros)
    {
        unsigned cc = cand;
        unsigned ra4 = 0, rb4 = 0;                                 // which of this thread's 4 + 4 rows appear
        while (cc) {
            const int q = __ffs(cc) - 1;
            cc &= cc - 1;
            ra4 |= 1u << (q >> 2);
            rb4 |= 1u << (q & 3);
            plist[pos++] = (uint16_t)(((ti * 4 + (q >> 2)) << 8) | (tj * 4 + (q & 3)));
        }
        if (ra4) atomicOr(&s_live[0], (unsigned long long)ra4 << (ti * 4));
        if (rb4) atomicOr(&s_live[1], (unsigned long long)rb4 << (tj * 4));
    }
    __syncthreads();
    const uint64_t live_a = s_live[0], live_b = s_live[1];
    const int cnt = s_cnt;
    if (kDiag) {                                                   // diagnostics only
        if (tid == 0) { atomicAdd(diag + 0, 1); atomicAdd(diag + 1, cnt); atomicAdd(diag + 2, n_pairs); }
    }
    const int lk = tid & (kKW - 1), lr = tid >> 5;
    const int slot = lk / kCW, cw = lk % kCW;
    const uint64_t *pa[8];
    const uint64_t *pb[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int ra = rowA[lr + 8 * q], rb = rowB[lr + 8 * q];
        pa[q] = (ra >= 0 && ((live_a >> (lr + 8 * q)) & 1)) ? rows + (int64_t)ra * nw : nullptr;
        pb[q] = (rb >= 0 && ((live_b >> (lr + 8 * q)) & 1)) ? rows + (int64_t)rb * nw : nullptr;
    }
    // Staging is software pipelined: the words of stage g+1 are fetched into registers while stage g is
    // combined out of LDS, so a stage costs max(load latency, compute) instead of their sum.
    uint64_t ra[8], rb[8];
    auto fetch = [&](int g) {
        const int64_t w = (g + slot < cnt) ? (int64_t)clist[g + slot] * kCW + cw : nw;
        const bool kin = w < nw;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            ra[q] = (kin && pa[q]) ? pa[q][w] : 0;
            rb[q] = (kin && pb[q]) ? pb[q][w] : 0;
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int q = 0; q < 8; ++q) { sa[lk][lr + 8 * q] = ra[q]; sb[lk][lr + 8 * q] = rb[q]; }
    };
    // One pair against the intersection counted SO FAR (final = the chunk loop has ended): returns true when the
    // pair is settled.  Already in one local set: nothing to learn.  iou(partial) > thr: the final intersection is
    // at least the partial one and the float32 expression is monotone in it, so the edge exists (P:149-166) --
    // record it now (the edges that merge two local sets are queued for the global forest, see flush).
    // Otherwise keep counting; after the last chunk the count is exact and decides.
    __shared__ int edge_cnt;
    __shared__ uint8_t edge_a[2 * kT], edge_b[2 * kT];             // at most 127 local unions can succeed
    if (tid == 0) edge_cnt = 0;                                    // ordered before its first use by the barriers below
    auto settle = [&](int ia, int jb, int inter, bool final) -> bool {
        if (local_find(lid, ia) == local_find(lid, kT + jb)) return true;
        const float fi = (float)inter;
        const float iou = __fdiv_rn(fi, (float)areaA[ia] + (float)areaB[jb] - fi);
        if (iou > thr) {                                                         // labels already equal
            if (local_union(lid, ia, kT + jb)) {
                const int k = atomicAdd(&edge_cnt, 1);
                edge_a[k] = (uint8_t)ia;
                edge_b[k] = (uint8_t)jb;
            }
            return true;
        }
        return final;
    };
    int flushed = 0;
    auto flush = [&]() {                                           // call after a barrier that follows the settle phase
        const int n_edges = edge_cnt;
        const int k = flushed + tid;
        if (k < n_edges) {
            uf_union(parent, rowA[edge_a[k]], rowB[edge_b[k]]);
            if (kDiag) atomicAdd(diag + 3, 1);
        }
        flushed = n_edges;
    };
    constexpr int kStep = kKW / kCW;                               // chunks per stage
    // pair-list path: at most 7 pairs per thread (1792 of the 4096).  3 was the first choice; interleaved A/B at config 2
    // (library variants side by side, BFF_HIP_LIB): tile pass alone 0.34 ms with 3, 0.30 with 6, 0.283-0.291 with 7, 0.31-0.33
    // with 10 (a pair-list stage costs ~4 us at 3 pairs per thread and grows with them, a 4x4-block stage ~11 us);
    // 8 and more need __launch_bounds__(256, 3) to stay at three blocks per CU.  Staging tile B permuted so that the 4x4
    // pass reads 16 consecutive words instead of 16 words 32 B apart was measured too: 0.34 ms (slower).
    constexpr int kSparse = 7;
    // settle pairs every `check_every` stages: 2 at first; a settle phase that closes no pair doubles the interval
    // (tiles between two groups of one object never settle early: their phases would cost as much as the counting)
    int check_every = 2, next_check = 2;
    if (kDiag) diag_lap(diag, 6, &t_lap);                                     // pair / chunk lists
    const int g_first = part * kStep, g_step = n_parts * kStep;    // split mode: every n_parts-th stage is this block's
    __shared__ int s_last;
    // split mode, after the chunk loop: add this part's counts to the slot; the last part to arrive takes the sums.
    // Only read-modify-write atomics touch the slot (they are coherent across the chip's L2s); every thread's adds
    // are complete (agent-scope fence) before thread 0 takes the ticket.
    auto arrive_last = [&]() -> bool {
        __threadfence();
        __syncthreads();
        if (tid == 0) s_last = atomicAdd(arrive + pslot, 1) == n_parts - 1;
        __syncthreads();
        return s_last != 0;                                        // block-uniform
    };
    int32_t *my_partial = split ? partial + (int64_t)pslot * (kT * kT) : nullptr;
    if (g_first < cnt) fetch(g_first);
    if (n_pairs <= kSparse * 256) {
        // few candidates: accumulate only those pairs (2 LDS reads per pair word)
        int pi[kSparse], pj[kSparse], accs[kSparse];
        unsigned open = 0;                                         // bit q: pair q of this thread is undecided
#pragma unroll
        for (int q = 0; q < kSparse; ++q) {
            const int p = tid + q * 256;
            const int code = p < n_pairs ? plist[p] : 0;
            pi[q] = code >> 8; pj[q] = code & 255; accs[q] = 0;
            if (p < n_pairs) open |= 1u << q;
        }
        int stages_done = 0;
        for (int g = g_first; g < cnt; g += g_step) {
            stage();
            if (tid == 0) g_block_info[1] += 1;
            __syncthreads();
            if (g + g_step < cnt) fetch(g + g_step);
#pragma unroll
            for (int q = 0; q < kSparse; ++q)
                if ((open >> q) & 1) {
                    int a2 = 0;
#pragma unroll 8
                    for (int kk = 0; kk < kKW; ++kk) a2 += popc64(sa[kk][pi[q]] & sb[kk][pj[q]]);
                    accs[q] += a2;
                }
            const bool last = g + g_step >= cnt;
            if (split) {
                __syncthreads();
            } else if (++stages_done == next_check || last) {
                const unsigned before_open = open;
#pragma unroll
                for (int q = 0; q < kSparse; ++q)
                    if (((open >> q) & 1) && settle(pi[q], pj[q], accs[q], last)) open &= ~(1u << q);
                const int any_open = __syncthreads_or(open != 0);
                const int progress = __syncthreads_or(open != before_open);
                flush();
                if (!any_open) break;                              // every pair settled: the rest of the chunks is moot
                if (!progress) check_every *= 2;
                next_check = stages_done + check_every;
            } else {
                __syncthreads();
            }
        }
        if (split) {
#pragma unroll
            for (int q = 0; q < kSparse; ++q)
                if (((open >> q) & 1) && accs[q]) atomicAdd(my_partial + pi[q] * kT + pj[q], accs[q]);
            if (arrive_last()) {
#pragma unroll
                for (int q = 0; q < kSparse; ++q)
                    if ((open >> q) & 1) settle(pi[q], pj[q], atomicAdd(my_partial + pi[q] * kT + pj[q], 0), true);
                __syncthreads();
                flush();
            }
        }
        if (kDiag) diag_lap(diag, 7, &t_lap);                                 // pair-list pass (incl. its unions)
        if (kDiag && tid == 0) atomicAdd(diag + 9, 1);
        return;
    }
    // many candidates: full 4x4 register blocks.  For a settle phase the 64 x 64 partial counts go through LDS (the
    // staging image `sa` is free between two stages) and the candidate list is walked pair by pair, thread p
    // taking pairs p, p + 256, ...: evenly spread whatever the shape of the candidate set, and a rolled loop.
    int acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = 0;
    int (*cnts)[kT + 1] = reinterpret_cast<int (*)[kT + 1]>(&sa[0][0]);       // 64 x 65 int32 = 16 640 B <= sizeof(sa)
    static_assert(sizeof(int) * kT * (kT + 1) <= sizeof(sa), "partial-count image must fit the staging buffer");
    const int n_mine = min(kT * kT / 256, max(0, (n_pairs - tid + 255) / 256));
    unsigned open = (1u << n_mine) - 1;                            // bit q: pair tid + 256 q of plist is undecided
    int stages_done = 0;
    for (int g = g_first; g < cnt; g += g_step) {
        stage();
        if (tid == 0) g_block_info[1] += 0x10000;                 // dense stages count in the upper half
        __syncthreads();
        if (g + g_step < cnt) fetch(g + g_step);
#pragma unroll 8
        for (int kk = 0; kk < kKW; ++kk) {
            uint64_t av[4], bv[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) { av[r] = sa[kk][ti * 4 + r]; bv[r] = sb[kk][tj * 4 + r]; }
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[r][c] += popc64(av[r] & bv[c]);
        }
        __syncthreads();
        const bool last = g + g_step >= cnt;
        if (!split && (++stages_done == next_check || last)) {
            const unsigned before_open = open;
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) cnts[ti * 4 + r][tj * 4 + c] = acc[r][c];
            __syncthreads();
#pragma unroll 1
            for (int q = 0; q < kT * kT / 256; ++q) {
                const int p = tid + q * 256;
                if (p >= n_pairs) break;
                if (!((open >> q) & 1)) continue;
                const int code = plist[p];
                if (settle(code >> 8, code & 255, cnts[code >> 8][code & 255], last)) open &= ~(1u << q);
            }
            const int any_open = __syncthreads_or(open != 0);
            const int progress = __syncthreads_or(open != before_open);
            flush();
            if (!any_open) break;
            if (!progress) check_every *= 2;
            next_check = stages_done + check_every;
        }
    }
    if (split) {
        // this part's counts go through the LDS image (as in a settle phase) and are added pair by pair: a rolled loop
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) cnts[ti * 4 + r][tj * 4 + c] = acc[r][c];
        __syncthreads();
#pragma unroll 1
        for (int q = 0; q < kT * kT / 256; ++q) {
            const int p = tid + q * 256;
            if (p >= n_pairs) break;
            const int code = plist[p];
            const int v = cnts[code >> 8][code & 255];
            if (v) atomicAdd(my_partial + (code >> 8) * kT + (code & 255), v);
        }
        if (arrive_last()) {
#pragma unroll 1
            for (int q = 0; q < kT * kT / 256; ++q) {
                const int p = tid + q * 256;
                if (p >= n_pairs) break;
                const int code = plist[p];
                settle(code >> 8, code & 255, atomicAdd(my_partial + (code >> 8) * kT + (code & 255), 0), true);
            }
            __syncthreads();
            flush();
        }
    }
    if (kDiag) diag_lap(diag, 8, &t_lap);                                     // dense pass (incl. its unions)
    if (kDiag && tid == 0) atomicAdd(diag + 10, 1);
}

// Tile pass over the filtered list: block b takes entry b; blocks beyond the list (its length is only known on
// the device) leave at once.  (A grid-stride or work-queue loop around the tile pair costs 60-80 registers and a
// third of the occupancy: measured slower.)  kMode: 0 production; 1 counters + phase clocks (costs registers: one
// block less per CU); 2 block timeline only -- start / end of every block at production occupancy.
template <int kMode>
__global__ __launch_bounds__(256) void merge_components_kernel(const uint64_t *__restrict__ rows, int n, int64_t nw,
                                                                const uint64_t *__restrict__ tmask, int mw,
                                                                const uint32_t *__restrict__ hist, int n_pos,
                                                                const int32_t *__restrict__ row_sorted,
                                                                const int32_t *__restrict__ area_sorted,
                                                                const int32_t *__restrict__ label_sorted, float thr,
                                                                int32_t *__restrict__ parent, int n_tiles,
                                                                int32_t *__restrict__ diag,
                                                                const int32_t *__restrict__ list,
                                                                const uint64_t *__restrict__ pass,
                                                                const int32_t *__restrict__ count,
                                                                const uint16_t *__restrict__ cpop,
                                                                const int32_t *__restrict__ part2,
                                                                int32_t *__restrict__ partial, int32_t *__restrict__ arrive)
{
    if ((int)blockIdx.x >= *count) return;                         // block-uniform
    long long t_start = 0;
    if (kMode) t_start = (long long)__builtin_amdgcn_s_memrealtime();    // 100 MHz, one clock for the whole chip
    if (threadIdx.x == 0) { g_block_info[0] = 0; g_block_info[1] = 0; }
    merge_tile_pair<kMode == 1>(list[blockIdx.x], pass[2 * blockIdx.x], pass[2 * blockIdx.x + 1], rows, n, nw, tmask, mw, hist,
                                n_pos, row_sorted, area_sorted, label_sorted, thr, parent, n_tiles, kMode == 1 ? diag : nullptr, cpop,
                                part2 ? part2[blockIdx.x] : 0, partial, arrive);
    if (kMode && threadIdx.x == 0 && diag[15] > 0 && (int)blockIdx.x < diag[15]) {
        // block timeline (diag[15] = capacity): start / end in 10-ns ticks (low 32 bits), at diag[16 + 2 b]
        diag[16 + 2 * blockIdx.x] = (int32_t)t_start;
        diag[17 + 2 * blockIdx.x] = (int32_t)(long long)__builtin_amdgcn_s_memrealtime();
        if (kMode == 2 && diag[14] > 0) {          // diag[14] != 0: two more words per block behind the timeline
            diag[16 + 2 * diag[15] + 2 * blockIdx.x] = g_block_info[0];
            diag[17 + 2 * diag[15] + 2 * blockIdx.x] = g_block_info[1];
        }
    }
}

}  // namespace bff

using namespace bff;

extern "C" int bff_row_stats(const uint64_t *rows, int32_t n_rows, int64_t nw, int32_t *area, int32_t *mean_word,
                             uint64_t *chunk_mask, int32_t chunk_mask_given, uint32_t *hist, int64_t *signature,
                             uint16_t *chunk_pop, void *stream)
{
    BFF_REQUIRE(n_rows >= 0 && nw >= 0, "bff_row_stats: bad sizes");
    if (n_rows == 0) return BFF_OK;
    BFF_REQUIRE(rows && area && mean_word && chunk_mask && hist && signature, "bff_row_stats: null pointer");
    const int n_chunks = (int)ceil_div(nw, kCW);
    BFF_LIMIT(n_chunks <= kMaxChunks, "bff_row_stats: more than %d chunks (N > %d points)", kMaxChunks, kMaxChunks * kCW * 64);
    const int mw = (int)ceil_div(n_chunks, 64);
    static_assert(kBins == kWave, "row_stats_sparse_kernel: one histogram bin per lane");
    if (chunk_mask_given) {
        if (chunk_pop) {                            // the sparse pass writes the flagged chunks only
            hipError_t e = zero_async(chunk_pop, sizeof(uint16_t) * (size_t)n_rows * mw * 64, as_stream(stream));
            if (e != hipSuccess) return fail((int)e, "bff_row_stats: memset: %s", hipGetErrorString(e));
        }
        row_stats_sparse_kernel<<<(unsigned)ceil_div(n_rows, 4), 256, 0, as_stream(stream)>>>(
            rows, n_rows, nw, mw, (int)ceil_div(nw > 0 ? nw : 1, kBins), area, mean_word, chunk_mask, hist, signature, chunk_pop);
        return launched("bff_row_stats");
    }
    row_stats_kernel<<<n_rows, 256, mw * sizeof(uint64_t), as_stream(stream)>>>(
        rows, nw, mw, (int)ceil_div(nw > 0 ? nw : 1, kBins), area, mean_word, chunk_mask, hist, signature, chunk_pop);
    return launched("bff_row_stats");
}

extern "C" int bff_merge_adjacency(const uint64_t *rows, int32_t n_rows, int64_t nw, const int32_t *order,
                                   const uint64_t *chunk_mask, uint64_t *tile_mask, const uint32_t *hist,
                                   const int32_t *area,
                                   const int32_t *label_id, float iou_thres, uint64_t *adj, int32_t *inter,
                                   void *stream)
{
    BFF_REQUIRE(n_rows >= 0 && nw >= 0, "bff_merge_adjacency: bad sizes");
    if (n_rows == 0) return BFF_OK;
    BFF_REQUIRE(rows && area && label_id && adj, "bff_merge_adjacency: null pointer");
    BFF_REQUIRE((chunk_mask == nullptr) == (tile_mask == nullptr), "bff_merge_adjacency: chunk_mask and tile_mask go together");
    const int nt = (int)ceil_div(n_rows, kT);
    BFF_LIMIT((int64_t)nt * (nt + 1) / 2 < (1ll << 31), "bff_merge_adjacency: too many rows");
    const int n_chunks = (int)ceil_div(nw, kCW);
    BFF_LIMIT(n_chunks <= kMaxChunks, "bff_merge_adjacency: more than %d chunks (N > %d points)", kMaxChunks, kMaxChunks * kCW * 64);
    const int mw = (int)ceil_div(n_chunks, 64);
    // pairs with an empty intersection have IoU 0 (or NaN): they can only be skipped when 0 > thr is false
    const bool sparse = chunk_mask && !(0.0f > iou_thres);
    if (sparse) tile_masks_kernel<<<nt, 256, 0, as_stream(stream)>>>(chunk_mask, order, n_rows, mw, tile_mask, nullptr, nullptr, 0, nullptr, nullptr, nullptr,
                                                                     nullptr, nullptr, nullptr, nullptr, nullptr);
    const int aw = nt;   // ceil(n_rows/64) words per adjacency row
    merge_adjacency_kernel<<<(unsigned)((int64_t)nt * (nt + 1) / 2), 256, 0, as_stream(stream)>>>(
        rows, n_rows, nw, order, sparse ? tile_mask : nullptr, mw, (sparse && !inter) ? hist : nullptr, area, label_id,
        iou_thres, adj, aw, inter, nt);
    return launched("bff_merge_adjacency");
}

// The second-level (chunk) bound pays when a histogram bin is much coarser than a chunk -- clouds of ~0.5 M points and
// more (config 4: tile pass 8.4 -> 2.7 ms); on smaller clouds the pairs that survive the 64-bin bound are genuine
// near-misses that the chunk bound cannot reject either, and its table look-ups cost more than they save (config 2:
// 0.45 -> 0.52 ms).  BFF_CHUNK_BOUND=0/1 forces it off / on.
extern "C" int32_t bff_merge_uses_chunk_bound(int64_t nw)
{
    static const int forced = [] { const char *e = getenv("BFF_CHUNK_BOUND"); return e ? atoi(e) : -1; }();
    if (forced >= 0) return forced != 0;
    // from 4 chunks per histogram bin (2048 words = 131 k points).  Round 2 had it from 16 (config 4 only): at config 2 its
    // table cost what it saved then; with the shorter chain and four scenes in flight it is 0.23 vs 0.295 ms for the tile
    // pass alone and 1351-1363 vs 1205-1286 scenes/s
    return ceil_div(nw > 0 ? nw : 1, kBins) >= 4 * kCW;
}

// Scratch of bff_merge_components for n rows in the order: the offset of every region and the size of the whole, in
// int32 words from an 8-byte aligned base.  bff_merge_scratch_words and merge_components_streams read it here only.
struct MergeScratch {
    int64_t n_pos, total, cap2;                    // padded rows, tile pairs, capacity of list 2
    int64_t hist_sorted, tile_hmax, tile_amin;     // [kBins / 2][n_pos] packed bins, [nt][kBins] maxima, [nt] smallest areas
    int64_t row_sorted, area_sorted, label_sorted; // [n_pos] each: position-indexed row tables
    int64_t counts, list1, list2;                  // [4] lengths of lists 1, 2 and slots handed out; [total]; [cap2]
    int64_t pass2, part2;                          // per entry of list 2: two 64-bit pass masks (even offset), a part word
    int64_t arrive, partial;                       // [kMaxSlots] and [kMaxSlots][kT * kT], adjacent: cleared by one fill
    int64_t words;                                 // size of the buffer
};

static MergeScratch merge_scratch_layout(int64_t n)
{
    MergeScratch s;
    const int64_t nt = ceil_div(n > 0 ? n : 1, kT);
    s.n_pos = nt * kT;
    s.total = nt * (nt + 1) / 2;
    // list 2: every surviving pair once + the extra parts of the pairs that are split
    s.cap2 = s.total + (int64_t)(kMaxParts - 1) * (s.total < kMaxSlots ? s.total : kMaxSlots);
    int64_t at = 0;
    auto take = [&at](int64_t words) { const int64_t o = at; at += words; return o; };
    s.hist_sorted = take((kBins / 2) * s.n_pos); s.tile_hmax = take(kBins * nt); s.tile_amin = take(nt);
    s.row_sorted = take(s.n_pos); s.area_sorted = take(s.n_pos); s.label_sorted = take(s.n_pos);
    s.counts = take(4); s.list1 = take(s.total); s.list2 = take(s.cap2);
    const int64_t align = at & 1;                  // 0 or 1 word, so that the 64-bit pass masks start at an even offset
    at += align;
    s.pass2 = take(4 * s.cap2); s.part2 = take(s.cap2);
    s.arrive = take(kMaxSlots); s.partial = take((int64_t)kMaxSlots * (kT * kT));
    // 6 - align unused words close the buffer: callers have always been told 6 words more than the regions add up to
    // (2 for the alignment, 4 that belonged to no region); the scene workspace and its one fill are sized from it
    s.words = at + 6 - align;
    return s;
}

extern "C" int64_t bff_merge_scratch_words(int32_t n_rows) { return merge_scratch_layout(n_rows).words; }

extern "C" int bff_merge_components(const uint64_t *rows, int32_t n_rows, int64_t nw, const int32_t *order,
                                    int32_t n_order, const uint64_t *chunk_mask, uint64_t *tile_mask,
                                    const uint32_t *hist, uint32_t *scratch, const int32_t *area,
                                    const int32_t *label_id, float iou_thres, int32_t *parent, int32_t init_parent,
                                    int32_t *comp, int32_t *diag, const uint16_t *chunk_pop, void *stream)
{
    return merge_components_streams(rows, n_rows, nw, order, n_order, chunk_mask, tile_mask, hist, scratch, area, label_id,
                                    iou_thres, parent, init_parent, comp, diag, chunk_pop, stream, stream, nullptr, nullptr);
}

int bff::merge_components_streams(const uint64_t *rows, int32_t n_rows, int64_t nw, const int32_t *order,
                                  int32_t n_order, const uint64_t *chunk_mask, uint64_t *tile_mask,
                                  const uint32_t *hist, uint32_t *scratch, const int32_t *area,
                                  const int32_t *label_id, float iou_thres, int32_t *parent, int32_t init_parent,
                                  int32_t *comp, int32_t *diag, const uint16_t *chunk_pop, void *stream, void *heavy_stream,
                                  void *before_heavy, void *after_heavy)
{
    BFF_REQUIRE(n_rows >= 0 && nw >= 0 && n_order >= 0 && n_order <= n_rows, "bff_merge_components: bad sizes");
    if (n_rows == 0) return BFF_OK;
    BFF_REQUIRE(rows && chunk_mask && tile_mask && hist && scratch && area && label_id && parent &&
                (order || n_order == n_rows), "bff_merge_components: null pointer");
    const int nt = (int)ceil_div(n_order, kT);
    BFF_LIMIT((int64_t)nt * (nt + 1) / 2 < (1ll << 31), "bff_merge_components: too many rows");
    const int n_chunks = (int)ceil_div(nw, kCW);
    BFF_LIMIT(n_chunks <= kMaxChunks, "bff_merge_components: more than %d chunks (N > %d points)", kMaxChunks, kMaxChunks * kCW * 64);
    const int mw = (int)ceil_div(n_chunks, 64);
    hipStream_t st = as_stream(stream);
    if (chunk_pop && !bff_merge_uses_chunk_bound(nw)) chunk_pop = nullptr;
    // every row appears once in `order` when it lists all of them: the tile pre-pass initialises the forest on the way
    const bool init_in_tiles = init_parent && n_order == n_rows && n_order > 0;
    if (init_parent && !init_in_tiles) uf_init_kernel<<<(unsigned)ceil_div(n_rows, 256), 256, 0, st>>>(parent, n_rows);
    if (n_order > 0) {
        // an empty intersection gives IoU 0 (or NaN): such pairs can only be skipped when 0 > thr is false
        const bool sparse = !(0.0f > iou_thres);
        const MergeScratch lay = merge_scratch_layout(n_order);
        const int64_t n_pos = lay.n_pos, total = lay.total, cap2 = lay.cap2;
        BFF_LIMIT(cap2 < (1ll << 31), "bff_merge_components: too many rows");
        BFF_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 7) == 0, "bff_merge_components: scratch must be 8-byte aligned");
        int32_t *const w = reinterpret_cast<int32_t *>(scratch);
        uint32_t *hist_sorted = scratch + lay.hist_sorted, *tile_hmax = scratch + lay.tile_hmax;
        int32_t *tile_amin = w + lay.tile_amin, *row_sorted = w + lay.row_sorted, *area_sorted = w + lay.area_sorted;
        int32_t *label_sorted = w + lay.label_sorted, *counts = w + lay.counts, *list1 = w + lay.list1, *list2 = w + lay.list2;
        uint64_t *pass2 = reinterpret_cast<uint64_t *>(w + lay.pass2);
        int32_t *part2 = w + lay.part2, *arrive = w + lay.arrive, *partial = w + lay.partial;
        // heavy tile pairs are split over several blocks unless switched off (BFF_MERGE_SPLIT=0); thr < 0 visits every
        // chunk of every pair anyway and keeps the simple form
        static const bool split_on = [] { const char *e = getenv("BFF_MERGE_SPLIT"); return !e || atoi(e) != 0; }();
        const bool do_split = split_on && sparse;
        tile_masks_kernel<<<nt, 256, 0, st>>>(chunk_mask, order, n_order, mw, tile_mask, hist, hist_sorted, (int)n_pos, area,
                                             tile_hmax, tile_amin, label_id, row_sorted, area_sorted, label_sorted,
                                             init_in_tiles ? parent : nullptr);
        hipError_t e = zero_async(counts, 4 * sizeof(int32_t), st);
        if (e == hipSuccess && do_split) e = zero_async(arrive, sizeof(int32_t) * (size_t)kMaxSlots * (kT * kT + 1), st);
        if (e != hipSuccess) return fail((int)e, "bff_merge_components: memset: %s", hipGetErrorString(e));
        tile_pair_filter_kernel<<<(unsigned)ceil_div(total, 256), 256, 0, st>>>(tile_hmax, tile_amin, nt, (int)total,
                                                                               iou_thres, list1, counts);
        tile_pair_rows_kernel<<<(unsigned)ceil_div(total, 4), 256, 0, st>>>(hist_sorted, (int)n_pos, area_sorted, tile_hmax,
                                                                           tile_amin, nt, iou_thres, list1, counts,
                                                                           list2, pass2, counts + 1, sparse ? tile_mask : nullptr,
                                                                           mw, do_split ? part2 : nullptr, counts + 2, (int)cap2);
        const hipEvent_t ev0 = g_merge_start, ev1 = g_merge_stop;      // attached to the dispatch itself when set
        g_merge_start = g_merge_stop = nullptr;
        const bool two = heavy_stream && heavy_stream != stream;
        hipStream_t light = st;
        if (two) {                                                     // the tile pass goes to the heavy stream
            BFF_REQUIRE(before_heavy && after_heavy, "bff_merge_components: two streams need their two events");
            hipError_t ee = hipEventRecord(reinterpret_cast<hipEvent_t>(before_heavy), light);
            if (ee == hipSuccess) ee = hipStreamWaitEvent(as_stream(heavy_stream), reinterpret_cast<hipEvent_t>(before_heavy), 0);
            if (ee != hipSuccess) return fail((int)ee, "bff_merge_components: stream hand-over: %s", hipGetErrorString(ee));
            st = as_stream(heavy_stream);
        }
        static const int diag_mode = [] { const char *e = getenv("BFF_MERGE_DIAG"); return e ? atoi(e) : 1; }();
        // BFF_MERGE_LDS_PAD=<bytes> of unused dynamic LDS: fewer blocks of the tile pass per CU (53 KB each: three fill a CU's
        // LDS and keep every other kernel in flight off that CU)
        static const int lds_pad = [] { const char *e = getenv("BFF_MERGE_LDS_PAD"); return e ? atoi(e) : 0; }();
        auto tile_pass = [&](auto kernel, int pad, int32_t *dg) {
            hipExtLaunchKernelGGL(kernel, dim3((unsigned)cap2), dim3(256), (unsigned)pad, st, ev0, ev1, 0,
                rows, n_order, nw, sparse ? tile_mask : nullptr, mw, hist_sorted, (int)n_pos, row_sorted, area_sorted,
                label_sorted, iou_thres, parent, nt, dg, list2, pass2, counts + 1, chunk_pop, do_split ? part2 : nullptr, partial, arrive);
        };
        if (diag && diag_mode == 2)   // block timeline only (BFF_MERGE_DIAG=2): production occupancy
            tile_pass(merge_components_kernel<2>, 0, diag);
        else if (diag)  // counters + phase clocks compiled in (a couple of registers more: one wave less per SIMD)
            tile_pass(merge_components_kernel<1>, 0, diag);
        else
            tile_pass(merge_components_kernel<0>, lds_pad, nullptr);
        if (two) {
            hipError_t ee = hipEventRecord(reinterpret_cast<hipEvent_t>(after_heavy), st);
            if (ee == hipSuccess) ee = hipStreamWaitEvent(light, reinterpret_cast<hipEvent_t>(after_heavy), 0);
            if (ee != hipSuccess) return fail((int)ee, "bff_merge_components: stream hand-over: %s", hipGetErrorString(ee));
            st = light;
        }
    }
    if (comp) uf_flatten_kernel<<<(unsigned)ceil_div(n_rows, 256), 256, 0, st>>>(parent, n_rows, comp);
    return launched("bff_merge_components");
}

// Profiling aid (bench.py): events attached to the next tile-pass dispatch of this host thread.
extern "C" int bff_profile_next_merge(void *start_event, void *stop_event)
{
    g_merge_start = reinterpret_cast<hipEvent_t>(start_event);
    g_merge_stop = reinterpret_cast<hipEvent_t>(stop_event);
    return BFF_OK;
}
