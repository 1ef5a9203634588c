// Row codecs (include/bff_hip.h): dense bytes, per-point ids and 1-D RLE to bit rows, and bit rows back to dense
// bytes and to 1-D RLE.
#include "common.h"

namespace bff {

// ---- dense <-> bits ---------------------------------------------------------------------------
__global__ void unpack_rows_kernel(const uint64_t *__restrict__ rows, int64_t nw, int64_t n, uint8_t *__restrict__ dense)
{
    // one thread expands 8 points (one byte of the bit row) into 8 bytes
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;     // group of 8 points
    const int64_t p0 = g * 8;
    if (p0 >= n) return;
    const uint32_t byte = (uint32_t)(rows[(int64_t)blockIdx.y * nw + (p0 >> 6)] >> (p0 & 63)) & 0xFFu;
    // 4 bits -> 4 bytes: the partial products land on disjoint bits, so there are no carries
    const uint32_t lo = ((byte & 0xF) * 0x00204081u) & 0x01010101u;
    const uint32_t hi = ((byte >> 4) * 0x00204081u) & 0x01010101u;
    uint8_t *out = dense + (int64_t)blockIdx.y * n + p0;
    if (p0 + 8 <= n && (((uintptr_t)out) & 7) == 0) {
        *reinterpret_cast<uint64_t *>(out) = (uint64_t)lo | ((uint64_t)hi << 32);
    } else {
        for (int k = 0; k < 8 && p0 + k < n; ++k) out[k] = (byte >> k) & 1;
    }
}

__global__ void pack_rows_kernel(const uint8_t *__restrict__ dense, int64_t n, int64_t nw, uint64_t *__restrict__ rows)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool bit = p < n && dense[(int64_t)blockIdx.y * n + p] != 0;
    const uint64_t bal = __ballot(bit);
    if (lane_id() == 0 && (p >> 6) < nw) rows[(int64_t)blockIdx.y * nw + (p >> 6)] = bal;
}

// ---- per-point ids -> bit rows (evaluation consumer, scannetv2_inst_eval.py:334: `gts == instance_id`) ---
__global__ void ids_to_rows_kernel(const int64_t *__restrict__ ids, int64_t n, const int64_t *__restrict__ values,
                                   int64_t nw, uint64_t *__restrict__ rows)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool bit = p < n && ids[p] == values[blockIdx.y];
    const uint64_t bal = __ballot(bit);
    if (lane_id() == 0 && (p >> 6) < nw) rows[(int64_t)blockIdx.y * nw + (p >> 6)] = bal;
}

// ---- 1-D RLE -> bit rows ----------------------------------------------------------------------
__global__ void rle_to_rows_kernel(const int32_t *__restrict__ run_start, const int32_t *__restrict__ run_end,
                                   const int32_t *__restrict__ offs, int64_t n, int64_t nw, uint64_t *__restrict__ rows)
{
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= nw) return;
    const int g = blockIdx.y;
    const int64_t p0 = w * 64, p1 = p0 + 64;
    int lo = offs[g], hi = offs[g + 1], r = hi;
    while (lo < r) {                                  // first run with end > p0
        const int mid = (lo + r) >> 1;
        if ((int64_t)run_end[mid] > p0) r = mid; else lo = mid + 1;
    }
    uint64_t v = 0;
    for (; r < hi; ++r) {
        const int64_t s = run_start[r], e = run_end[r];
        if (s >= p1) break;
        const int a = (int)(max(s, p0) - p0), b = (int)(min(e, p1) - p0);    // [a, b) within the word, b > a
        const uint64_t upto_b = b >= 64 ? ~0ull : ((1ull << b) - 1);
        v |= upto_b & ~((1ull << a) - 1);
    }
    if (p1 > n) v &= (n - p0 >= 64) ? ~0ull : ((1ull << (n - p0)) - 1);
    rows[(int64_t)g * nw + w] = v;
}

// ---- bit rows -> 1-D RLE (rle_encode_batch, rle_encode_decode.py:10-32) ------------------------------
// A run starts at point p iff bit p is set and bit p-1 is not; it ends (exclusive) at e iff bit e-1 is set
// and bit e is not.  Padding bits are zero and one virtual zero word follows the row, so a run reaching the
// last point ends at N like any other.  Starts and ends alternate: the k-th end closes the k-th start.
// Pass 1 counts the starts per row; pass 2 writes counts[2k] = start+1 (1-based) and counts[2k+1] = end,
// rank by rank (block scan of the per-word counts); pass 3 turns the ends into lengths.  rle_word_edges: common.h.
__global__ __launch_bounds__(256) void rle_count_kernel(const uint64_t *__restrict__ rows, int64_t nw,
                                                         int32_t *__restrict__ n_runs)
{
    __shared__ int part[4];
    const uint64_t *row = rows + (int64_t)blockIdx.x * nw;
    int c = 0;
    for (int64_t w = threadIdx.x; w < nw; w += 256) {
        uint64_t st, en;
        rle_word_edges(row, w, nw, st, en);
        c += popc64(st);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) c += __shfl_down(c, d);
    if (lane_id() == 0) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) n_runs[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

__global__ __launch_bounds__(256) void rle_write_kernel(const uint64_t *__restrict__ rows, int64_t nw,
                                                         const int64_t *__restrict__ run_offs,
                                                         int64_t *__restrict__ counts)
{
    __shared__ int wsum[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t *row = rows + (int64_t)blockIdx.x * nw;
    int64_t *out = counts + 2 * run_offs[blockIdx.x];
    int base_st = 0, base_en = 0;
    for (int64_t w0 = 0; w0 <= nw; w0 += 256) {                  // <= : includes the virtual word nw
        const int64_t w = w0 + tid;
        uint64_t st = 0, en = 0;
        if (w <= nw) rle_word_edges(row, w, nw, st, en);
        const int packed = popc64(st) | (popc64(en) << 16);      // <= 32 starts / ends per word, 256 words: no carry
        int incl = packed;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const int up = __shfl_up(incl, d); if (lane >= d) incl += up; }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        int excl = incl - packed;
        for (int q = 0; q < wave; ++q) excl += wsum[q];
        const int total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        int64_t rs = base_st + (excl & 0xFFFF), re = base_en + (excl >> 16);
        while (st) { const int b = __ffsll((unsigned long long)st) - 1; st &= st - 1; out[2 * rs++] = w * 64 + b + 1; }
        while (en) { const int b = __ffsll((unsigned long long)en) - 1; en &= en - 1; out[2 * re++ + 1] = w * 64 + b; }
        base_st += total & 0xFFFF;
        base_en += total >> 16;
        __syncthreads();
    }
}

__global__ void rle_lengths_kernel(int64_t *__restrict__ counts, int64_t n_runs_total)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n_runs_total) counts[2 * k + 1] -= counts[2 * k] - 1;       // end - start(0-based)
}

}  // namespace bff

using namespace bff;

extern "C" int bff_unpack_rows(const uint64_t *rows, int32_t n_rows, int64_t nw, int64_t n_points, uint8_t *dense,
                               void *stream)
{
    BFF_REQUIRE(n_rows >= 0 && n_points >= 0 && nw == ceil_div(n_points, 64), "bff_unpack_rows: bad sizes");
    if (n_rows == 0 || n_points == 0) return BFF_OK;
    BFF_REQUIRE(rows && dense, "bff_unpack_rows: null pointer");
    BFF_LIMIT(n_rows <= 65535, "bff_unpack_rows: too many rows");
    dim3 grid((unsigned)ceil_div(ceil_div(n_points, 8), 256), (unsigned)n_rows);
    unpack_rows_kernel<<<grid, 256, 0, as_stream(stream)>>>(rows, nw, n_points, dense);
    return launched("bff_unpack_rows");
}

extern "C" int bff_pack_rows(const uint8_t *dense, int32_t n_rows, int64_t n_points, int64_t nw, uint64_t *rows,
                             void *stream)
{
    BFF_REQUIRE(n_rows >= 0 && n_points >= 0 && nw == ceil_div(n_points, 64), "bff_pack_rows: bad sizes");
    if (n_rows == 0 || n_points == 0) return BFF_OK;
    BFF_REQUIRE(rows && dense, "bff_pack_rows: null pointer");
    BFF_LIMIT(n_rows <= 65535, "bff_pack_rows: too many rows");
    dim3 grid((unsigned)ceil_div(nw * 64, 256), (unsigned)n_rows);
    pack_rows_kernel<<<grid, 256, 0, as_stream(stream)>>>(dense, n_points, nw, rows);
    return launched("bff_pack_rows");
}

extern "C" int bff_rle_to_rows(const int32_t *run_start, const int32_t *run_end, const int32_t *row_run_offs,
                               int32_t n_rows, int64_t n_points, int64_t nw, uint64_t *rows, void *stream)
{
    BFF_REQUIRE(n_rows >= 0 && n_points >= 0 && nw == ceil_div(n_points, 64), "bff_rle_to_rows: bad sizes");
    if (n_rows == 0 || nw == 0) return BFF_OK;
    BFF_REQUIRE(row_run_offs && rows, "bff_rle_to_rows: null pointer");   // run arrays may be empty (NULL)
    BFF_LIMIT(n_rows <= 65535, "bff_rle_to_rows: too many rows");
    dim3 grid((unsigned)ceil_div(nw, 256), (unsigned)n_rows);
    rle_to_rows_kernel<<<grid, 256, 0, as_stream(stream)>>>(run_start, run_end, row_run_offs, n_points, nw, rows);
    return launched("bff_rle_to_rows");
}

extern "C" int bff_rle_count_runs(const uint64_t *rows, int32_t n_rows, int64_t nw, int32_t *n_runs, void *stream)
{
    BFF_REQUIRE(n_rows >= 0 && nw >= 0, "bff_rle_count_runs: bad sizes");
    if (n_rows == 0) return BFF_OK;
    BFF_REQUIRE(rows && n_runs, "bff_rle_count_runs: null pointer");
    rle_count_kernel<<<n_rows, 256, 0, as_stream(stream)>>>(rows, nw, n_runs);
    return launched("bff_rle_count_runs");
}

extern "C" int bff_rle_encode_rows(const uint64_t *rows, int32_t n_rows, int64_t nw, const int64_t *run_offs,
                                   int64_t n_runs_total, int64_t *counts, void *stream)
{
    BFF_REQUIRE(n_rows >= 0 && nw >= 0 && n_runs_total >= 0, "bff_rle_encode_rows: bad sizes");
    if (n_rows == 0 || n_runs_total == 0) return BFF_OK;
    BFF_REQUIRE(rows && run_offs && counts, "bff_rle_encode_rows: null pointer");
    rle_write_kernel<<<n_rows, 256, 0, as_stream(stream)>>>(rows, nw, run_offs, counts);
    rle_lengths_kernel<<<(unsigned)ceil_div(n_runs_total, 256), 256, 0, as_stream(stream)>>>(counts, n_runs_total);
    return launched("bff_rle_encode_rows");
}

extern "C" int bff_ids_to_rows(const int64_t *ids, int64_t n_points, const int64_t *values, int32_t n_values, int64_t nw,
                               uint64_t *rows, void *stream)
{
    BFF_REQUIRE(n_points >= 0 && n_values >= 0 && nw == ceil_div(n_points, 64), "bff_ids_to_rows: bad sizes");
    if (n_values == 0 || n_points == 0) return BFF_OK;
    BFF_REQUIRE(ids && values && rows, "bff_ids_to_rows: null pointer");
    BFF_LIMIT(n_values <= 65535, "bff_ids_to_rows: too many values");
    dim3 grid((unsigned)ceil_div(nw * 64, 256), (unsigned)n_values);
    ids_to_rows_kernel<<<grid, 256, 0, as_stream(stream)>>>(ids, n_points, values, nw, rows);
    return launched("bff_ids_to_rows");
}
