// Shared by the bit-row units: what more than one of rows.hip, merge.hip, groups.hip, scene.hip and the 3-D stages
// (cells.h) needs.
// Anything a single unit uses stays in that unit.
#pragma once

#include "common.h"

namespace bff {

// rows.hip (cross_popcount_kernel) and merge.hip (the tile pass) stage the same 64 x 64 tiles
constexpr int kT = 64;        // tile of 64 x 64 row pairs per 256-thread block
constexpr int kKW = 32;       // words staged per step
constexpr int kPitch = kT + 1;

// merge.hip builds the forest, groups.hip flattens it (group_count_kernel).
// parent[] is a disjoint-set forest over ROW indices (roots point to themselves, links go to the
// smaller index).  Reads bypass L1 (agent-scope relaxed atomics) so every wave sees links made by
// other CUs; a stale view can only make a tile do work it could have skipped, never change the result:
// once two rows share a root they are connected for good, and links are made with compare-and-swap.
__device__ __forceinline__ int uf_find(int32_t *parent, int x)
{
    int p = __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (p != x) {
        const int g = __hip_atomic_load(parent + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // path halving: point x at its grandparent.  g is an ancestor of x, so the forest stays a forest
        // whatever other waves do meanwhile (links only ever go to smaller indices).
        if (g != p) __hip_atomic_store(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = p;
        p = g;
    }
    return x;
}

// The larger root hangs under the smaller, so the final root of a component is its smallest member whatever the
// interleaving.  merge.hip's tile epilogue, and the element forests of spatial.hip and density.hip (cells.h).
__device__ __forceinline__ void uf_union(int32_t *parent, int a, int b)
{
    for (;;) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }            // a > b: hang the larger root under the smaller
        int expected = a;
        if (__hip_atomic_compare_exchange_strong(parent + a, &expected, b, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT))
            return;
    }
}

// bff_merge_components with the tile pass on a stream of its own (`heavy`; bff_scene_project keeps the chip-filling
// kernels of the scenes in flight on shared heavy streams so that they do not run four at a time): the pre-pass and the
// two tile-pair filters run on `stream`, `before_heavy` is recorded there and awaited by `heavy`, the tile pass runs on
// `heavy`, `after_heavy` is recorded there and awaited by `stream`.  heavy == stream (events unused): one stream.
// Defined in merge.hip, called by scene.hip.
int merge_components_streams(const uint64_t *rows, int32_t n_rows, int64_t nw, const int32_t *order,
                             int32_t n_order, const uint64_t *chunk_mask, uint64_t *tile_mask,
                             const uint32_t *hist, uint32_t *scratch, const int32_t *area,
                             const int32_t *label_id, float iou_thres, int32_t *parent, int32_t init_parent,
                             int32_t *comp, int32_t *diag, const uint16_t *chunk_pop, void *stream, void *heavy_stream,
                             void *before_heavy, void *after_heavy);

}  // namespace bff
