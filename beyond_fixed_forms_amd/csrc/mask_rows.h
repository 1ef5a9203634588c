// Row directory of the 2-D masks (include/bff_hip.h: bff_mask_row_directory): formats shared by the build
// (mask_rows.hip) and the sweep's look-up mode (project.hip).
//
//   mask table  uint32 [n_masks + 1][4], one 16-byte entry per mask g:
//                 [0] c0 | R0 << 16     smallest column / first image row any run touches
//                 [1] c1 | R1 << 16     largest column / last image row (inclusive)
//                 [2] dir_offs[g]       position of row R0's entry in the directory
//                 [3] mask_run_offs[g]  the mask's first run
//               a mask without runs has the empty box [0] = 0xffffffff, [1] = 0 (no pixel passes the box test);
//               entry n_masks is such an empty box with the directory's total size and the run tables' total
//               length, so that entry g + 1 always ends mask g's runs
//   directory   uint32, one entry per image row R0..R1 of every mask, for the runs that intersect the row:
//                 0                                   none (a direct entry with an empty interval)
//                 cs | ce << 15                       exactly one: its column interval [cs, ce) clipped to the row
//                 1 << 31 | count << 27 | first       more: `first` = index of the first such run relative to the
//                                                     mask, count saturated at kRowCountSat; a saturated count
//                                                     means "binary-search from `first` to the mask's last run"
//                                                     (first = 0 when the index itself does not fit in 27 bits)
#pragma once

#include <cstdint>

namespace bff {

constexpr uint32_t kRowFlag = 1u << 31;
constexpr int kRowCountShift = 27;
constexpr uint32_t kRowCountSat = 15;            // 4 bits
constexpr uint32_t kRowFirstMask = (1u << kRowCountShift) - 1;
constexpr uint32_t kRowLinear = 4;               // counts up to here are scanned run by run
constexpr int kRowsFrames = 8;                   // frames per block of the sweep whose tables go into LDS
constexpr int kRowsMaskSlots = 65;               // <= 64 masks of a frame + the entry that ends the last one

// what the sweep's look-up mode reads (all device pointers)
struct MaskRows {
    const uint4 *tab;
    const uint32_t *dir;
    const int32_t *run_start, *run_end;
    const int32_t *view_mask_offs;
};

// Does one of the runs [lo, hi) of a mask cover pixel p?  `e` is the row's flagged directory entry, first_run / end_run
// the mask's runs.  Sorted, disjoint, non-empty runs: the only candidate is the first run that ends behind p.
__device__ __forceinline__ bool runs_cover(const int32_t *__restrict__ run_start, const int32_t *__restrict__ run_end,
                                           uint32_t e, uint32_t first_run, uint32_t end_run, int p)
{
    const uint32_t count = (e >> kRowCountShift) & kRowCountSat;
    uint32_t lo = first_run + (e & kRowFirstMask);
    uint32_t hi = count == kRowCountSat ? end_run : lo + count;
    if (count <= kRowLinear) {
        bool in = false;
        for (uint32_t i = lo; i < hi; ++i) in |= run_start[i] <= p && p < run_end[i];
        return in;
    }
    while (lo < hi) {                            // first run with end > p
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (run_end[mid] > p) hi = mid; else lo = mid + 1;
    }
    const uint32_t stop = count == kRowCountSat ? end_run : first_run + (e & kRowFirstMask) + count;
    return lo < stop && run_start[lo] <= p;
}

}  // namespace bff
