// Bit-row primitives (include/bff_hip.h: a16, a19, a20): popcount, cross-popcount, clearing flagged chunks, bit
// permutation and scatter, AND, gather and row programs.  Built on them: row_codec.hip (dense, ids and RLE <-> rows),
// merge.hip (a9-a12), groups.hip (a13) and resolve.hip (a16).
//
// A boolean row over N points is nw = ceil(N/64) uint64 words.  Set algebra on rows is AND/OR/
// ANDNOT on words, cardinalities are popcounts, the {0,1} matmuls of the reference
// (F @ F.T, projection_2d_to_3d.py:159; mask_1 @ mask_2.T, refinement.py:84) are
// popcount(a & b) accumulated over words -- exact integers, 1/32 of the bytes of the float form.
#include "rows.h"

namespace bff {

// ---- popcount of rows -----------------------------------------------------------------------
__global__ __launch_bounds__(256) void popcount_rows_kernel(const uint64_t *__restrict__ rows,
                                                             const int32_t *__restrict__ idx, int64_t nw,
                                                             int32_t *__restrict__ area)
{
    __shared__ int part[4];
    const int r = blockIdx.x;
    const uint64_t *row = rows + (int64_t)(idx ? idx[r] : r) * nw;
    int s = 0;
    for (int64_t w = threadIdx.x; w < nw; w += blockDim.x) s += popc64(row[w]);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) s += __shfl_down(s, d);
    if (lane_id() == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) area[r] = part[0] + part[1] + part[2] + part[3];
}

// ---- 64x64 tile of popcount(a_i & b_j) -------------------------------------------------------
// LDS images are [word][row] (pitch 65) so that the 4 rows / 4 columns a thread needs for one word
// are 32 contiguous bytes; thread (ti, tj) of the 16 x 16 thread grid owns rows 4ti..4ti+3 and
// columns 4tj..4tj+3.
__device__ __forceinline__ void tile_popcount(const uint64_t *__restrict__ a, const int32_t *__restrict__ ia,
                                              int na, int i0, const uint64_t *__restrict__ b,
                                              const int32_t *__restrict__ ib, int nb, int j0, int64_t nw,
                                              int64_t k_begin, int64_t k_end,
                                              uint64_t (*sa)[kPitch], uint64_t (*sb)[kPitch], int acc[4][4])
{
    const int tid = threadIdx.x;
    const int ti = tid >> 4, tj = tid & 15;
    const int lk = tid & (kKW - 1), lr = tid >> 5;          // loader: word lk of rows lr, lr+8, ...
    const uint64_t *pa[8];
    const uint64_t *pb[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int ra = i0 + lr + 8 * q, rb = j0 + lr + 8 * q;
        pa[q] = ra < na ? a + (int64_t)(ia ? ia[ra] : ra) * nw : nullptr;
        pb[q] = rb < nb ? b + (int64_t)(ib ? ib[rb] : rb) * nw : nullptr;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = 0;
    for (int64_t k0 = k_begin; k0 < k_end; k0 += kKW) {
        const bool kin = k0 + lk < nw;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            sa[lk][lr + 8 * q] = (kin && pa[q]) ? pa[q][k0 + lk] : 0;
            sb[lk][lr + 8 * q] = (kin && pb[q]) ? pb[q][k0 + lk] : 0;
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

__global__ __launch_bounds__(256) void cross_popcount_kernel(const uint64_t *__restrict__ a,
                                                              const int32_t *__restrict__ ia, int na,
                                                              const uint64_t *__restrict__ b,
                                                              const int32_t *__restrict__ ib, int nb, int64_t nw,
                                                              int64_t k_split, int32_t *__restrict__ inter,
                                                              const int32_t *__restrict__ k_dev, int lim_a, int hole_hi)
{
    __shared__ uint64_t sa[kKW][kPitch], sb[kKW][kPitch];
    // k_dev (optional): only the first *k_dev rows of a (when lim_a) resp. of b's leading block [0, hole_hi) hold data,
    // the rest of those ranges is all zero: tiles that lie entirely in the zero part are skipped (the output is
    // zeroed by the host when the words are split over z; callers never read the skipped entries otherwise)
    if (k_dev) {
        const int kd = *k_dev;
        if (lim_a && (int)blockIdx.y * kT >= kd) return;
        if ((int)blockIdx.x * kT >= kd && (int)(blockIdx.x + 1) * kT <= hole_hi) return;
    }
    // blockIdx.z owns the word range [z*k_split, (z+1)*k_split): small row counts still fill the chip.
    // Partial counts are combined with integer atomics (exact, order independent) into a zeroed matrix.
    int acc[4][4];
    const int i0 = blockIdx.y * kT, j0 = blockIdx.x * kT;
    const int64_t k_begin = (int64_t)blockIdx.z * k_split;
    tile_popcount(a, ia, na, i0, b, ib, nb, j0, nw, k_begin, min(nw, k_begin + k_split), sa, sb, acc);
    const int ti = threadIdx.x >> 4, tj = threadIdx.x & 15;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int i = i0 + ti * 4 + r, j = j0 + tj * 4 + c;
            if (i < na && j < nb) {
                if (gridDim.z == 1) inter[(int64_t)i * nb + j] = acc[r][c];
                else if (acc[r][c]) atomicAdd(inter + (int64_t)i * nb + j, acc[r][c]);
            }
        }
}

// Undo what the sweep stored: zero exactly the chunks flagged in the rows' occupancy masks (one wave per row), so
// that a zero-filled row arena is all zero again after a scene without touching its other 99 %.
__global__ __launch_bounds__(256) void clear_flagged_chunks_kernel(uint64_t *__restrict__ rows, int n_rows, int64_t nw,
                                                                    const uint64_t *__restrict__ cmask, int mw,
                                                                    const int32_t *__restrict__ veto)
{
    if (veto && *veto) return;                     // the host still needs the rows (general path)
    const int lane = lane_id();
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n_rows) return;
    uint64_t *row = rows + (int64_t)r * nw;
    for (int i = 0; i < mw; ++i) {
        const uint64_t m = cmask[(int64_t)r * mw + i];
        if ((m >> lane) & 1) {
            const int64_t w0 = ((int64_t)i * 64 + lane) * kCW;
#pragma unroll
            for (int k = 0; k < kCW; ++k)
                if (w0 + k < nw) row[w0 + k] = 0;
        }
    }
}

// out bit o of row r = in bit idx[o] of row r  (bit gather; undoes the spatial point sort)
__global__ void permute_bits_kernel(const uint64_t *__restrict__ in, int64_t nw_in, const int32_t *__restrict__ idx,
                                    int64_t n_out, int64_t nw_out, uint64_t *__restrict__ out)
{
    const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool bit = false;
    if (o < n_out) {
        const int s = idx[o];
        bit = (in[(int64_t)blockIdx.y * nw_in + (s >> 6)] >> (s & 63)) & 1;
    }
    const uint64_t bal = __ballot(bit);
    if (lane_id() == 0 && (o >> 6) < nw_out) out[(int64_t)blockIdx.y * nw_out + (o >> 6)] = bal;
}

// Undo the spatial point sort by SCATTER: out[r] bit perm[s] = in[r] bit s for the set bits only (aggregated rows
// hold a few percent of the points, so this touches ~1/50 of what a bit gather per output point reads).  out must be
// zero; perm[s] = original index of sorted position s.  Rows >= *k_dev (when given) are skipped.
__global__ __launch_bounds__(256) void scatter_bits_kernel(const uint64_t *__restrict__ in, int64_t nw_in,
                                                            const int32_t *__restrict__ perm, int64_t n,
                                                            int64_t nw_out, uint64_t *__restrict__ out,
                                                            const int32_t *__restrict__ k_dev)
{
    const int r = blockIdx.y;
    if (k_dev && r >= *k_dev) return;
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= nw_in) return;
    uint64_t v = in[(int64_t)r * nw_in + w];
    while (v) {
        const int b = __ffsll((unsigned long long)v) - 1;
        v &= v - 1;
        const int64_t s = w * 64 + b;
        if (s < n) {
            const int o = perm[s];
            atomicOr((unsigned long long *)(out + (int64_t)r * nw_out + (o >> 6)), 1ull << (o & 63));
        }
    }
}

__global__ void apply_row_ops_kernel(uint64_t *__restrict__ rows, int64_t nw, const int32_t *__restrict__ ops,
                                     int n_ops)
{
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= nw) return;
    if (n_ops < 0) { n_ops = ops[0]; ops += 1; }          // device-side list: [count, triples...]
    for (int k = 0; k < n_ops; ++k) {
        const int op = ops[3 * k], d = ops[3 * k + 1], s = ops[3 * k + 2];
        const uint64_t sv = rows[(int64_t)s * nw + w];
        uint64_t *dp = rows + (int64_t)d * nw + w;
        *dp = op == 0 ? (*dp & ~sv) : op == 1 ? (*dp | sv) : sv;
    }
}

__global__ void and_rows_kernel(uint64_t *__restrict__ rows, int64_t nw, const uint64_t *__restrict__ keep)
{
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w < nw) rows[(int64_t)blockIdx.y * nw + w] &= keep[w];
}

__global__ void gather_rows_kernel(const uint64_t *__restrict__ rows, const int32_t *__restrict__ idx, int64_t nw,
                                   uint64_t *__restrict__ out)
{
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w < nw) out[(int64_t)blockIdx.y * nw + w] = rows[(int64_t)idx[blockIdx.y] * nw + w];
}

}  // namespace bff

using namespace bff;

extern "C" int bff_popcount_rows(const uint64_t *rows, const int32_t *idx, int32_t n_rows, int64_t nw,
                                 int32_t *area, void *stream)
{
    BFF_REQUIRE(n_rows >= 0 && nw >= 0, "bff_popcount_rows: bad sizes");
    if (n_rows == 0) return BFF_OK;
    BFF_REQUIRE(area && (rows || nw == 0), "bff_popcount_rows: null pointer");
    if (nw == 0) {                                      // zero-width rows (rows may be NULL): every count is 0
        hipError_t e = hipMemsetAsync(area, 0, sizeof(int32_t) * (size_t)n_rows, as_stream(stream));
        if (e != hipSuccess) return fail((int)e, "bff_popcount_rows: memset: %s", hipGetErrorString(e));
        return BFF_OK;
    }
    popcount_rows_kernel<<<n_rows, 256, 0, as_stream(stream)>>>(rows, idx, nw, area);
    return launched("bff_popcount_rows");
}

// The z extent of bff_cross_popcount's launch and the words each slice owns: the one statement of that choice
// (bff_cross_popcount_slices answers with it, the launch is sized by it).  0 slices: nothing to launch.
static int64_t cross_popcount_split(int64_t na, int64_t nb, int64_t nw, int64_t *k_split)
{
    *k_split = nw;                                      // words per block along z
    if (na <= 0 || nb <= 0 || nw <= 0) return 0;
    const int64_t tiles = ceil_div(nb, kT) * ceil_div(na, kT);
    if (tiles < 512) {                                  // few tiles: split the words so >= ~512 blocks run
        *k_split = ceil_div(ceil_div(nw * tiles, 512), kKW) * kKW;
        if (*k_split < 2 * kKW) *k_split = 2 * kKW;
    }
    return ceil_div(nw, *k_split);
}

extern "C" int bff_cross_popcount_slices(int32_t na, int32_t nb, int64_t nw)
{
    int64_t k_split;
    return (int)cross_popcount_split(na, nb, nw, &k_split);
}

extern "C" int bff_cross_popcount(const uint64_t *a, const int32_t *ia, int32_t na, const uint64_t *b,
                                  const int32_t *ib, int32_t nb, int64_t nw, int32_t *inter, void *stream)
{
    BFF_REQUIRE(na >= 0 && nb >= 0 && nw >= 0, "bff_cross_popcount: bad sizes");
    if (na == 0 || nb == 0) return BFF_OK;
    BFF_REQUIRE(inter && ((a && b) || nw == 0), "bff_cross_popcount: null pointer");
    int64_t k_split;
    const int64_t nz = cross_popcount_split(na, nb, nw, &k_split);
    if (nz != 1) {                                      // split words meet through atomics; zero-width rows: all zero
        hipError_t e = hipMemsetAsync(inter, 0, sizeof(int32_t) * (size_t)na * nb, as_stream(stream));
        if (e != hipSuccess) return fail((int)e, "bff_cross_popcount: memset: %s", hipGetErrorString(e));
        if (nz == 0) return BFF_OK;
    }
    dim3 grid((unsigned)ceil_div(nb, kT), (unsigned)ceil_div(na, kT), (unsigned)nz);
    cross_popcount_kernel<<<grid, 256, 0, as_stream(stream)>>>(a, ia, na, b, ib, nb, nw, k_split, inter, nullptr, 0, 0);
    return launched("bff_cross_popcount");
}

// bff_cross_popcount where only the first *k_dev rows of the leading `lead` rows of b (and, with limit_a != 0, of a)
// are non-zero: tiles inside the zero part are skipped.  inter is zeroed first.
extern "C" int bff_cross_popcount_dev(const uint64_t *a, int32_t na, const uint64_t *b, int32_t nb, int64_t nw,
                                      int32_t *inter, const int32_t *k_dev, int32_t limit_a, int32_t lead, void *stream)
{
    BFF_REQUIRE(na >= 0 && nb >= 0 && nw >= 0 && lead >= 0 && lead <= nb, "bff_cross_popcount_dev: bad sizes");
    if (na == 0 || nb == 0) return BFF_OK;
    BFF_REQUIRE(a && b && inter && k_dev, "bff_cross_popcount_dev: null pointer");
    const int64_t tiles = ceil_div(nb, kT) * ceil_div(na, kT);
    int64_t k_split = nw;
    // few tiles (the refinement's S1 x (K + S1) product: a dozen, most of their rows zero): split the words until ~2048
    // blocks run, down to one LDS stage each -- the partial counts meet through atomics on non-zero entries only
    // (config 2, K = 20 / 100: 40 / 44 us with 512 blocks of >= 2 stages, 26 / 35 us with 2048 of >= 1)
    constexpr int64_t target = 2048;
    if (tiles < target) {
        k_split = ceil_div(ceil_div(nw * tiles, target), kKW) * kKW;
        if (k_split < kKW) k_split = kKW;
    }
    const int64_t nz = ceil_div(nw, k_split);
    hipError_t e = zero_async(inter, sizeof(int32_t) * (size_t)na * nb, as_stream(stream));
    if (e != hipSuccess) return fail((int)e, "bff_cross_popcount_dev: memset: %s", hipGetErrorString(e));
    dim3 grid((unsigned)ceil_div(nb, kT), (unsigned)ceil_div(na, kT), (unsigned)(nz > 0 ? nz : 1));
    cross_popcount_kernel<<<grid, 256, 0, as_stream(stream)>>>(a, nullptr, na, b, nullptr, nb, nw, k_split, inter, k_dev,
                                                              limit_a, lead);
    return launched("bff_cross_popcount_dev");
}

extern "C" int bff_chunk_mask_words(int64_t nw) { return (int)ceil_div(ceil_div(nw, kCW), 64); }

extern "C" int bff_clear_flagged_chunks(uint64_t *rows, int32_t n_rows, int64_t nw, const uint64_t *chunk_mask,
                                        void *stream)
{
    BFF_REQUIRE(n_rows >= 0 && nw >= 0, "bff_clear_flagged_chunks: bad sizes");
    if (n_rows == 0 || nw == 0) return BFF_OK;
    BFF_REQUIRE(rows && chunk_mask, "bff_clear_flagged_chunks: null pointer");
    clear_flagged_chunks_kernel<<<(unsigned)ceil_div(n_rows, 4), 256, 0, as_stream(stream)>>>(
        rows, n_rows, nw, chunk_mask, (int)ceil_div(ceil_div(nw, kCW), 64), nullptr);
    return launched("bff_clear_flagged_chunks");
}

extern "C" int bff_clear_flagged_chunks_unless(uint64_t *rows, int32_t n_rows, int64_t nw, const uint64_t *chunk_mask,
                                               const int32_t *veto, void *stream)
{
    BFF_REQUIRE(n_rows >= 0 && nw >= 0, "bff_clear_flagged_chunks_unless: bad sizes");
    if (n_rows == 0 || nw == 0) return BFF_OK;
    BFF_REQUIRE(rows && chunk_mask && veto, "bff_clear_flagged_chunks_unless: null pointer");
    clear_flagged_chunks_kernel<<<(unsigned)ceil_div(n_rows, 4), 256, 0, as_stream(stream)>>>(
        rows, n_rows, nw, chunk_mask, (int)ceil_div(ceil_div(nw, kCW), 64), veto);
    return launched("bff_clear_flagged_chunks_unless");
}

extern "C" int bff_permute_bits(const uint64_t *rows_in, int32_t n_rows, int64_t nw_in, const int32_t *idx,
                                int64_t n_out, int64_t nw_out, uint64_t *rows_out, void *stream)
{
    BFF_REQUIRE(n_rows >= 0 && n_out >= 0 && nw_out == ceil_div(n_out, 64) && nw_in >= 0, "bff_permute_bits: bad sizes");
    if (n_rows == 0 || n_out == 0) return BFF_OK;
    BFF_REQUIRE(rows_in && idx && rows_out, "bff_permute_bits: null pointer");
    BFF_LIMIT(n_rows <= 65535, "bff_permute_bits: too many rows");
    dim3 grid((unsigned)ceil_div(nw_out * 64, 256), (unsigned)n_rows);
    permute_bits_kernel<<<grid, 256, 0, as_stream(stream)>>>(rows_in, nw_in, idx, n_out, nw_out, rows_out);
    return launched("bff_permute_bits");
}

extern "C" int bff_apply_row_ops(uint64_t *rows, int64_t nw, const int32_t *ops, int32_t n_ops, void *stream)
{
    BFF_REQUIRE(nw >= 0, "bff_apply_row_ops: bad sizes");
    if (n_ops == 0 || nw == 0) return BFF_OK;
    BFF_REQUIRE(rows && ops, "bff_apply_row_ops: null pointer");
    apply_row_ops_kernel<<<(unsigned)ceil_div(nw, 256), 256, 0, as_stream(stream)>>>(rows, nw, ops, n_ops);
    return launched("bff_apply_row_ops");
}

extern "C" int bff_and_rows(uint64_t *rows, int32_t n_rows, int64_t nw, const uint64_t *keep, void *stream)
{
    BFF_REQUIRE(n_rows >= 0 && nw >= 0, "bff_and_rows: bad sizes");
    if (n_rows == 0 || nw == 0) return BFF_OK;
    BFF_REQUIRE(rows && keep, "bff_and_rows: null pointer");
    BFF_LIMIT(n_rows <= 65535, "bff_and_rows: too many rows");
    dim3 grid((unsigned)ceil_div(nw, 256), (unsigned)n_rows);
    and_rows_kernel<<<grid, 256, 0, as_stream(stream)>>>(rows, nw, keep);
    return launched("bff_and_rows");
}

extern "C" int bff_gather_rows(const uint64_t *rows, const int32_t *idx, int32_t n_out, int64_t nw, uint64_t *out,
                               void *stream)
{
    BFF_REQUIRE(n_out >= 0 && nw >= 0, "bff_gather_rows: bad sizes");
    if (n_out == 0 || nw == 0) return BFF_OK;
    BFF_REQUIRE(rows && idx && out, "bff_gather_rows: null pointer");
    BFF_LIMIT(n_out <= 65535, "bff_gather_rows: too many rows");
    dim3 grid((unsigned)ceil_div(nw, 256), (unsigned)n_out);
    gather_rows_kernel<<<grid, 256, 0, as_stream(stream)>>>(rows, idx, nw, out);
    return launched("bff_gather_rows");
}

extern "C" int bff_scatter_bits(const uint64_t *rows_in, int32_t n_rows, int64_t nw_in, const int32_t *perm, int64_t n,
                                int64_t nw_out, uint64_t *rows_out, const int32_t *k_dev, void *stream)
{
    BFF_REQUIRE(n_rows >= 0 && n >= 0 && nw_out == ceil_div(n, 64) && nw_in >= 0, "bff_scatter_bits: bad sizes");
    if (n_rows == 0 || n == 0 || nw_in == 0) return BFF_OK;
    BFF_REQUIRE(rows_in && perm && rows_out, "bff_scatter_bits: null pointer");
    BFF_LIMIT(n_rows <= 65535, "bff_scatter_bits: too many rows");
    dim3 grid((unsigned)ceil_div(nw_in, 256), (unsigned)n_rows);
    scatter_bits_kernel<<<grid, 256, 0, as_stream(stream)>>>(rows_in, nw_in, perm, n, nw_out, rows_out, k_dev);
    return launched("bff_scatter_bits");
}
