// Group formation on the device and the OR of every group's member rows with its confidence mean
// (include/bff_hip.h: a13).
#include <hip/hip_fp16.h>

#include <cstdlib>

#include "rows.h"

namespace bff {

constexpr int kFuseMax = BFF_GROUP_CAP_MAX;      // most groups the device forms by itself

// ---- group OR / confidence mean ---------------------------------------------------------------
constexpr int kOrSplit = 32;      // members per block along z

// Sequential mean of one group's confidences by the first wave of the calling block: all its lanes gather
// 1024 confidences into LDS at once (the gathers are the slow part), then lane 0 runs the strictly sequential
// sum the reference defines (P:225) -- one rounding in the confidence dtype per step.
template <typename T>
__device__ __forceinline__ void group_conf_mean_wave(const T *__restrict__ conf, const int32_t *__restrict__ offs,
                                                     const int32_t *__restrict__ members, int g, T *__restrict__ mean,
                                                     T *stage /* LDS [1024] */)
{
    const int lane = threadIdx.x;                  // callers pass threads 0..63 only
    const int lo = offs[g], hi = offs[g + 1];
    T s;
    if constexpr (sizeof(T) == 2) s = __float2half_rn(0.0f); else s = 0.0f;
    for (int base = lo; base < hi; base += 1024) {
        const int cnt = min(1024, hi - base);
        for (int k = lane; k < cnt; k += kWave) stage[k] = conf[members[base + k]];
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");   // one wave: LDS ops complete in issue order
        if (lane == 0) {
#pragma unroll 8
            for (int k = 0; k < cnt; ++k) {
                if constexpr (sizeof(T) == 2) s = __hadd(s, stage[k]);        // one f16 rounding per step
                else s = __fadd_rn(s, stage[k]);
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
    if (lane == 0) {
        if constexpr (sizeof(T) == 2) mean[g] = __float2half_rn(__fdiv_rn(__half2float(s), (float)(hi - lo)));
        else mean[g] = __fdiv_rn(s, (float)(hi - lo));
    }
}

template <typename T>
__global__ __launch_bounds__(256) void or_reduce_groups_kernel(const uint64_t *__restrict__ rows, int64_t nw,
                                                                const int32_t *__restrict__ offs,
                                                                const int32_t *__restrict__ members, int n_groups,
                                                                uint64_t *__restrict__ out, const T *__restrict__ conf,
                                                                T *__restrict__ mean, const uint64_t *__restrict__ cmask, int mw)
{
    __shared__ uint32_t s_occ[kOrSplit];           // cmask given: the members' chunk flags for this block's 256 words
    // blockIdx.z takes members [z*32, z*32+32) of group blockIdx.y; partial ORs meet in the zeroed output.
    // Blocks with blockIdx.y == 0 when conf != NULL (groups then start at y = 1) do not OR anything: their first wave
    // computes the sequential confidence means of groups blockIdx.x, blockIdx.x + gridDim.x, ... so that the
    // longest chain of dependent additions runs beside the OR instead of after it.
    __shared__ T stage[1024];
    const int g = conf ? (int)blockIdx.y - 1 : (int)blockIdx.y;     // slice y = 0 is dispatched first
    if (g < 0) {
        if (blockIdx.z == 0 && threadIdx.x < kWave)
            for (int q = blockIdx.x; q < n_groups; q += gridDim.x) group_conf_mean_wave(conf, offs, members, q, mean, stage);
        return;
    }
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lo = offs[g] + blockIdx.z * kOrSplit, hi = min(offs[g + 1], lo + kOrSplit);
    if (lo >= hi) {                                                // block-uniform
        // one z slice: nothing zeroed the output, so an empty group's row is stored here (with more slices the memset did it)
        if (gridDim.z == 1 && w < nw) out[(int64_t)g * nw + w] = 0;
        return;
    }
    uint64_t v = 0;
    if (cmask) {                                                   // long rows: see or_reduce_grouped_kernel
        if (threadIdx.x < hi - lo) {
            const uint64_t m64 = cmask[(int64_t)members[lo + threadIdx.x] * mw + (blockIdx.x >> 1)];
            s_occ[threadIdx.x] = (uint32_t)(m64 >> (32 * (blockIdx.x & 1)));
        }
        __syncthreads();
        if (w >= nw) return;
        const int c = threadIdx.x >> 3;
        for (int m = lo; m < hi; ++m)
            if ((s_occ[m - lo] >> c) & 1) v |= rows[(int64_t)members[m] * nw + w];
    } else {
        if (w >= nw) return;
#pragma unroll 8
        for (int m = lo; m < hi; ++m) v |= rows[(int64_t)members[m] * nw + w];
    }
    if (gridDim.z == 1) out[(int64_t)g * nw + w] = v;
    else if (v) atomicOr((unsigned long long *)(out + (int64_t)g * nw + w), (unsigned long long)v);
}

template <typename T>
__global__ __launch_bounds__(64) void group_conf_mean_kernel(const T *__restrict__ conf,
                                                             const int32_t *__restrict__ offs,
                                                             const int32_t *__restrict__ members, int n_groups,
                                                             T *__restrict__ mean)
{
    __shared__ T stage[1024];
    group_conf_mean_wave(conf, offs, members, (int)blockIdx.x, mean, stage);
}

// ---- groups on the device -------------------------------------------------------------------------
// Component ids -> the groups merge_masks keeps (P:203-226), without a host round trip: the device twin of
// bff_host_component_csr for at most `cap` groups.  comp[i] = smallest row index of i's component, so group
// order "by smallest member" is the order of the roots, and "members ascending" is the order of the rows.
//   info[0] = K (number of kept groups, may exceed cap), info[1] = flags (1: K > cap, 2: empty components survive
//   the filter, i.e. min_members <= 0 -- both mean "take the general host path"), info[2] = largest kept group,
//   info[3] = number of 32-member slices of the kept groups (work items of bff_or_reduce_grouped).
__global__ void group_count_kernel(int32_t *__restrict__ comp, int n, int32_t *__restrict__ count,
                                   int32_t *__restrict__ parent)
{
    // 64 consecutive rows (two views' masks) belong to a handful of components: one atomic per distinct root of the
    // wave instead of one per row (thousands of rows share a few dozen counters).  parent != NULL: comp is an OUTPUT,
    // the flattened disjoint-set forest (comp[i] = root of i = smallest row of its component; uf_flatten_kernel fused).
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    int root = -1;
    if (i < n) {
        if (parent) { root = uf_find(parent, i); comp[i] = root; }
        else root = comp[i];
    }
    uint64_t todo = __ballot(root >= 0);
    while (todo) {
        const int leader = __ffsll((unsigned long long)todo) - 1;
        const int r = __shfl(root, leader);
        const uint64_t same = __ballot(root == r);
        if (lane_id() == leader) atomicAdd(count + r, __popcll(same));
        todo &= ~same;
    }
}

__global__ __launch_bounds__(1024) void group_scan_kernel(const int32_t *__restrict__ comp, const int32_t *__restrict__ count,
                                                           const int32_t *__restrict__ area, int n, float thr,
                                                           int min_members, int cap, int32_t *__restrict__ info,
                                                           int32_t *__restrict__ sizes, int32_t *__restrict__ first,
                                                           int32_t *__restrict__ offs, int32_t *__restrict__ slices,
                                                           int slice_cap)
{
    __shared__ int wsum[16];
    __shared__ int s_base, s_void, s_max;
    __shared__ int s_off[kFuseMax + 1], s_soff[kFuseMax + 1], s_sz[kFuseMax];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) { s_base = 0; s_void = 0; s_max = 0; }
    __syncthreads();
    const int need = min_members > 1 ? min_members : 1;
    const bool loops = 1.0f > thr;                                  // a non-empty row is adjacent to itself iff 1 > thr
    constexpr int kAhead = 4;                                      // chunks whose loads are in flight together
    __shared__ int wsum2[2][16];
    int base = 0, it = 0;
    for (int d0 = 0; d0 < n; d0 += 1024 * kAhead) {
        int szv[kAhead], arv[kAhead];
#pragma unroll
        for (int u = 0; u < kAhead; ++u) {
            const int c = d0 + u * 1024 + tid;
            const bool root = c < n && comp[c] == c;
            szv[u] = root ? count[c] : -1;                             // -1: not a root
            arv[u] = root ? area[c] : 0;
        }
#pragma unroll
      for (int u = 0; u < kAhead; ++u) {
        const int c0 = d0 + u * 1024;
        if (c0 >= n) break;                                            // block-uniform
        const int c = c0 + tid;
        bool valid = false, is_void = false;
        int sz = 0;
        if (szv[u] >= 0) {
            sz = szv[u];
            is_void = sz == 1 && !(arv[u] > 0 && loops);            // isolated row without a self loop: the reference's []
            valid = !is_void && sz >= need;
        }
        const uint64_t bal = __ballot(valid);
        if (lane == 0) wsum2[it][wave] = __popcll(bal);
        if (is_void) atomicAdd(&s_void, 1);
        __syncthreads();                                   // double-buffered counters: one barrier per chunk
        int g = base + __popcll(bal & ((1ull << lane) - 1)), total = 0;
#pragma unroll
        for (int q = 0; q < 16; ++q) { const int cq = wsum2[it][q]; total += cq; if (q < wave) g += cq; }
        if (valid) {
            if (g < cap) { sizes[g] = sz; first[g] = c; s_sz[g] = sz; }
            atomicMax(&s_max, sz);
        }
        base += total;                                     // every thread keeps the running group count
        it ^= 1;
      }
    }
    if (tid == 0) s_base = base;
    __syncthreads();
    const int k_all = s_base, k = min(k_all, cap);
    {
        // exclusive prefix sums of the groups' sizes and 32-member slice counts over the k <= 512 groups: thread g owns
        // group g (one serial walk by one thread: up to 512 dependent LDS round trips, 20+ us for scenes with many groups)
        const int sz = tid < k ? s_sz[tid] : 0, sl = (sz + kOrSplit - 1) / kOrSplit;
        int io = sz, is = sl;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int uo = __shfl_up(io, d), us = __shfl_up(is, d);
            if (lane >= d) { io += uo; is += us; }
        }
        __syncthreads();                               // wsum was last read two barriers ago; reuse it for both sums
        __shared__ int wsum3[16];
        if (lane == 63) { wsum[wave] = io; wsum3[wave] = is; }
        __syncthreads();
        int bo = 0, bs = 0;
        for (int q = 0; q < wave; ++q) { bo += wsum[q]; bs += wsum3[q]; }
        if (tid < k) { s_off[tid] = bo + io - sz; s_soff[tid] = bs + is - sl; }
        if (tid == k - 1 || (k == 0 && tid == 0)) {
            const int o = k ? bo + io : 0, so = k ? bs + is : 0;
            s_off[k] = o; s_soff[k] = so;
            info[0] = k_all;
            info[1] = (k_all > cap ? 1 : 0) | ((min_members <= 0 && s_void > 0) ? 2 : 0);
            info[2] = s_max;
            info[3] = min(so, slice_cap);
        }
    }
    __syncthreads();
    for (int g = tid; g <= k; g += 1024) offs[g] = s_off[g];
    for (int g = tid + k + 1; g <= cap; g += 1024) offs[g] = s_off[k];
    // slice s of group g covers members [offs[g] + 32 j, min(offs[g+1], ...)): table rows (group, lo, hi)
    const int n_slices = min(s_soff[k], slice_cap);
    for (int sidx = tid; sidx < n_slices; sidx += 1024) {
        int g = 0, hi = k - 1;                       // last group whose first slice is <= sidx
        while (g < hi) { const int mid = (g + hi + 1) >> 1; if (s_soff[mid] <= sidx) g = mid; else hi = mid - 1; }
        const int lo = s_off[g] + (sidx - s_soff[g]) * kOrSplit;
        slices[sidx] = g;
        slices[slice_cap + sidx] = lo;
        slices[2 * slice_cap + sidx] = min(s_off[g + 1], lo + kOrSplit);
    }
}

// members of group g in ascending row order: one block per group walks comp[] 256 rows at a time (ballot per wave,
// the four waves' counts meet in LDS)
__global__ __launch_bounds__(256) void group_members_kernel(const int32_t *__restrict__ comp, int n,
                                                             const int32_t *__restrict__ info, int cap,
                                                             const int32_t *__restrict__ first,
                                                             const int32_t *__restrict__ offs,
                                                             int32_t *__restrict__ members)
{
    __shared__ int wcnt[2][4];
    const int g = blockIdx.x;
    if (g >= min(info[0], cap)) return;
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const int root = first[g];
    int base = offs[g], it = 0;
    constexpr int kAhead = 4;                                  // steps whose loads are in flight together
    for (int j0 = 0; j0 < n; j0 += 256 * kAhead) {
        int cv[kAhead];
#pragma unroll
        for (int u = 0; u < kAhead; ++u) {
            const int i = j0 + u * 256 + (int)threadIdx.x;
            cv[u] = i < n ? comp[i] : -1;
        }
#pragma unroll
        for (int u = 0; u < kAhead; ++u, it ^= 1) {
            const int i = j0 + u * 256 + (int)threadIdx.x;
            if (j0 + u * 256 >= n) break;                      // block-uniform
            const bool m = cv[u] == root;                      // roots are >= 0
            const uint64_t bal = __ballot(m);
            if (lane == 0) wcnt[it][wave] = __popcll(bal);
            __syncthreads();                                   // double-buffered counters: one barrier per step
            int before = 0, total = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) { const int c = wcnt[it][q]; total += c; if (q < wave) before += c; }
            if (m) members[base + before + __popcll(bal & ((1ull << lane) - 1))] = i;
            base += total;
        }
    }
}

// bff_or_reduce_groups for groups formed on the device: the work items are the 32-member slices listed by
// group_scan_kernel (their number is only known on the device: blocks beyond it leave at once); slice y = 0 of the
// grid computes the sequential confidence means, as in or_reduce_groups_kernel.
template <typename T>
__global__ __launch_bounds__(256) void or_reduce_grouped_kernel(const uint64_t *__restrict__ rows, int64_t nw,
                                                                 const int32_t *__restrict__ info, int cap,
                                                                 const int32_t *__restrict__ offs,
                                                                 const int32_t *__restrict__ members,
                                                                 const int32_t *__restrict__ slices, int slice_cap,
                                                                 uint64_t *__restrict__ out, const T *__restrict__ conf,
                                                                 T *__restrict__ mean, const uint64_t *__restrict__ cmask, int mw)
{
    __shared__ T stage[1024];
    __shared__ uint32_t s_occ[kOrSplit];           // cmask given: the 32 chunk flags of every member for this block's 256 words
    if (blockIdx.y == 0) {
        if (conf && threadIdx.x < kWave) {
            const int k = min(info[0], cap);
            for (int q = blockIdx.x; q < k; q += gridDim.x) group_conf_mean_wave(conf, offs, members, q, mean, stage);
        }
        return;
    }
    const int sidx = (int)blockIdx.y - 1;
    if (sidx >= info[3]) return;
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= nw && !cmask) return;
    const int g = slices[sidx], lo = slices[slice_cap + sidx], hi = slices[2 * slice_cap + sidx];
    uint64_t v = 0;
    if (cmask) {
        // long rows (~1 % occupied): a block's 256 words are 32 chunks = one 32-bit piece of a member's chunk flags;
        // a member's word is loaded only where the member has points
        if (threadIdx.x < hi - lo) {
            const uint64_t m64 = cmask[(int64_t)members[lo + threadIdx.x] * mw + (blockIdx.x >> 1)];
            s_occ[threadIdx.x] = (uint32_t)(m64 >> (32 * (blockIdx.x & 1)));
        }
        __syncthreads();
        const int c = threadIdx.x >> 3;                            // chunk of this thread's word within the block
        if (w < nw)
            for (int m = lo; m < hi; ++m)
                if ((s_occ[m - lo] >> c) & 1) v |= rows[(int64_t)members[m] * nw + w];
    } else {
#pragma unroll 8
        for (int m = lo; m < hi; ++m) v |= rows[(int64_t)members[m] * nw + w];
    }
    if (v) atomicOr((unsigned long long *)(out + (int64_t)g * nw + w), (unsigned long long)v);
}

}  // namespace bff

using namespace bff;

// Rows at least this long are OR-ed through their chunk flags (BFF_OR_SPARSE_MIN_NW): config 4 reads 4.8 GB of rows
// that are ~1 % occupied.  Config 2 (3125 words): round 2 measured the dense pass (234 MB) and the flagged one the same end
// to end; with four scenes in flight on the shorter chain the flagged pass is 21 vs 40-45 us and worth ~5 % of the
// throughput (the dense read competed with the other scenes' kernels for HBM), so the limit is 1024 words now.
static int64_t or_sparse_min_words()
{
    static const int64_t v = [] { const char *e = getenv("BFF_OR_SPARSE_MIN_NW"); return e ? atoll(e) : 1024ll; }();
    return v;
}

extern "C" int bff_or_reduce_groups(const uint64_t *rows, int64_t nw, const int32_t *group_offs,
                                    const int32_t *members, int32_t n_groups, int32_t max_group_size,
                                    uint64_t *out, const void *conf, int32_t conf_dtype, void *conf_mean,
                                    const uint64_t *chunk_mask, void *stream)
{
    BFF_REQUIRE(n_groups >= 0 && nw >= 0, "bff_or_reduce_groups: bad sizes");
    if (n_groups == 0) return BFF_OK;
    BFF_REQUIRE(rows && group_offs && members && out, "bff_or_reduce_groups: null pointer");
    BFF_REQUIRE((conf == nullptr) == (conf_mean == nullptr) && (conf_dtype == 0 || conf_dtype == 1),
                "bff_or_reduce_groups: conf and conf_mean go together, dtype 0 (f32) or 1 (f16)");
    if (nw == 0 && !conf) return BFF_OK;
    // z covers the largest group in slices of kOrSplit members; max_group_size is a host-known bound
    const int nz = (int)ceil_div(max_group_size > 0 ? max_group_size : 1, kOrSplit);
    if (nz > 1 && nw > 0) {
        hipError_t e = hipMemsetAsync(out, 0, sizeof(uint64_t) * (size_t)n_groups * nw, as_stream(stream));
        if (e != hipSuccess) return fail((int)e, "bff_or_reduce_groups: memset: %s", hipGetErrorString(e));
    }
    dim3 grid((unsigned)ceil_div(nw > 0 ? nw : 1, 256), (unsigned)(n_groups + (conf ? 1 : 0)), (unsigned)nz);
    const uint64_t *cm = (chunk_mask && nw >= or_sparse_min_words()) ? chunk_mask : nullptr;
    const int mw = (int)ceil_div(ceil_div(nw, kCW), 64);
    if (conf_dtype == 1)
        or_reduce_groups_kernel<__half><<<grid, 256, 0, as_stream(stream)>>>(rows, nw, group_offs, members, n_groups, out,
                                                                            (const __half *)conf, (__half *)conf_mean, cm, mw);
    else
        or_reduce_groups_kernel<float><<<grid, 256, 0, as_stream(stream)>>>(rows, nw, group_offs, members, n_groups, out,
                                                                           (const float *)conf, (float *)conf_mean, cm, mw);
    return launched("bff_or_reduce_groups");
}

extern "C" int bff_group_conf_mean(const void *conf, int32_t dtype, const int32_t *group_offs,
                                   const int32_t *members, int32_t n_groups, void *mean, void *stream)
{
    BFF_REQUIRE(n_groups >= 0 && (dtype == 0 || dtype == 1), "bff_group_conf_mean: bad arguments");
    if (n_groups == 0) return BFF_OK;
    BFF_REQUIRE(conf && group_offs && members && mean, "bff_group_conf_mean: null pointer");
    const unsigned grid = (unsigned)n_groups;
    if (dtype == 1)
        group_conf_mean_kernel<__half><<<grid, 64, 0, as_stream(stream)>>>((const __half *)conf, group_offs, members,
                                                                           n_groups, (__half *)mean);
    else
        group_conf_mean_kernel<float><<<grid, 64, 0, as_stream(stream)>>>((const float *)conf, group_offs, members,
                                                                          n_groups, (float *)mean);
    return launched("bff_group_conf_mean");
}

extern "C" int32_t bff_group_slice_cap(int32_t n_rows, int32_t cap) { return n_rows / kOrSplit + cap + 1; }

extern "C" int bff_group_components(int32_t *comp, int32_t *parent, const int32_t *area, int32_t n_rows, float iou_thres,
                                    int32_t min_members, int32_t cap, int32_t *count, int32_t count_is_zero,
                                    int32_t *info, int32_t *sizes,
                                    int32_t *first, int32_t *offs, int32_t *members, int32_t *slices, void *stream)
{
    BFF_REQUIRE(n_rows >= 0 && cap > 0, "bff_group_components: bad sizes");
    BFF_LIMIT(cap <= kFuseMax, "bff_group_components: at most %d groups on the device", kFuseMax);
    BFF_REQUIRE(info && sizes && first && offs && slices && (n_rows == 0 || (comp && area && count && members)),
                "bff_group_components: null pointer");
    hipStream_t st = as_stream(stream);
    if (n_rows > 0) {
        if (!count_is_zero) {
            hipError_t e = hipMemsetAsync(count, 0, sizeof(int32_t) * (size_t)n_rows, st);
            if (e != hipSuccess) return fail((int)e, "bff_group_components: memset: %s", hipGetErrorString(e));
        }
        group_count_kernel<<<(unsigned)ceil_div(n_rows, 256), 256, 0, st>>>(comp, n_rows, count, parent);
    }
    group_scan_kernel<<<1, 1024, 0, st>>>(comp, count, area, n_rows, iou_thres, min_members, cap, info, sizes, first, offs,
                                         slices, bff_group_slice_cap(n_rows, cap));
    if (n_rows > 0)
        group_members_kernel<<<(unsigned)cap, 256, 0, st>>>(comp, n_rows, info, cap, first, offs, members);
    return launched("bff_group_components");
}

extern "C" int bff_or_reduce_grouped(const uint64_t *rows, int64_t nw, int32_t n_rows, const int32_t *info, int32_t cap,
                                     const int32_t *offs, const int32_t *members, const int32_t *slices, uint64_t *out,
                                     const void *conf, int32_t conf_dtype, void *conf_mean, const uint64_t *chunk_mask,
                                     void *stream)
{
    BFF_REQUIRE(nw >= 0 && n_rows >= 0 && cap > 0, "bff_or_reduce_grouped: bad sizes");
    BFF_REQUIRE(rows && info && offs && members && slices && out, "bff_or_reduce_grouped: null pointer");
    BFF_REQUIRE((conf == nullptr) == (conf_mean == nullptr) && (conf_dtype == 0 || conf_dtype == 1),
                "bff_or_reduce_grouped: conf and conf_mean go together, dtype 0 (f32) or 1 (f16)");
    const int slice_cap = bff_group_slice_cap(n_rows, cap);
    BFF_LIMIT(slice_cap + 1 <= 65535, "bff_or_reduce_grouped: too many member slices");
    hipStream_t st = as_stream(stream);
    if (nw > 0) {
        hipError_t e = zero_async(out, sizeof(uint64_t) * (size_t)cap * nw, st);
        if (e != hipSuccess) return fail((int)e, "bff_or_reduce_grouped: memset: %s", hipGetErrorString(e));
    }
    dim3 grid((unsigned)ceil_div(nw > 0 ? nw : 1, 256), (unsigned)(slice_cap + 1));
    // through the chunk flags only when the rows are long (config 2: the dense pass runs at HBM speed and the flagged
    // form was measured slower; config 4: 4.8 GB of rows, ~1 % occupied)
    const uint64_t *cm = (chunk_mask && nw >= or_sparse_min_words()) ? chunk_mask : nullptr;
    const int mw = (int)ceil_div(ceil_div(nw, kCW), 64);
    if (conf_dtype == 1)
        or_reduce_grouped_kernel<__half><<<grid, 256, 0, st>>>(rows, nw, info, cap, offs, members, slices, slice_cap, out,
                                                              (const __half *)conf, (__half *)conf_mean, cm, mw);
    else
        or_reduce_grouped_kernel<float><<<grid, 256, 0, st>>>(rows, nw, info, cap, offs, members, slices, slice_cap, out,
                                                             (const float *)conf, (float *)conf_mean, cm, mw);
    return launched("bff_or_reduce_grouped");
}
