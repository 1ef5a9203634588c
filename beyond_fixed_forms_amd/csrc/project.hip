// Per-frame projection sweep, point-major (include/bff_hip.h: a2-a7, a15).
//
// Data layout in HBM
//   xyz        f64 [3][n_pad]            structure of arrays: a wave reads 3 x 512 B contiguous
//   depth      f32 [n_depth][H*W]        gathered at the projected pixel (4 B / visible point)
//   maskbits   u32|u64 [n_mviews][H*W]   bit b = mask b of that frame covers the pixel (one gather
//                                         returns all masks of the frame)
//   rows       u64 [n_rows][nw]          instance bit rows: a wave's 64 points are exactly one word,
//                                         so __ballot() of "bit b set" IS the output word
// Kernel shape (sweep.h): 256 threads = 4 waves own 1024 consecutive points; pose and intrinsics are wave-uniform (scalar
// loads / kernel arguments).  The frame loop has no block barrier: a wave transposes its ballots through a private LDS
// slice and stores its own sector of every row of the frame.
#include <hip/hip_ext.h>

#include "sweep.h"

namespace bff {

// two uint16 per register (a pixel as column | row << 16): component-wise minimum / maximum
__device__ __forceinline__ uint32_t pk_min_u16(uint32_t a, uint32_t b)
{
    uint32_t r;
    asm("v_pk_min_u16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ uint32_t pk_max_u16(uint32_t a, uint32_t b)
{
    uint32_t r;
    asm("v_pk_max_u16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// component-wise minimum (kMin) or maximum of v over the 64 lanes, in every lane: six DPP steps as wave_xor_scan (mask_decode.hip)
// (lanes a step does not reach take the operation's identity), the total out of lane 63
template <bool kMin>
__device__ __forceinline__ uint32_t wave_reduce_pk_u16(uint32_t v)
{
    constexpr int id = kMin ? -1 : 0;
#define BFF_DPP_PK(ctrl, rows) do { const uint32_t t_ = (uint32_t)__builtin_amdgcn_update_dpp(id, (int)v, ctrl, rows, 0xF, false); \
                                    v = kMin ? pk_min_u16(v, t_) : pk_max_u16(v, t_); } while (0)
    BFF_DPP_PK(0x111, 0xF);     // row_shr:1
    BFF_DPP_PK(0x112, 0xF);     // row_shr:2
    BFF_DPP_PK(0x114, 0xF);     // row_shr:4
    BFF_DPP_PK(0x118, 0xF);     // row_shr:8
    BFF_DPP_PK(0x142, 0xA);     // row_bcast:15 -> rows 1 and 3
    BFF_DPP_PK(0x143, 0xC);     // row_bcast:31 -> rows 2 and 3
#undef BFF_DPP_PK
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

// kRows: the frame's masks are not decoded into `maskbits`; a visible point asks the masks' row directory (mask_rows.h)
// at its pixel instead.  The block's <= kRowsFrames frames keep their mask tables in LDS behind the tap table.
// kVis (with kRows): visibility and pixel of a (point, frame) pair come out of the scene's visibility table; the cloud, the
// poses, the tap table and the depth frames are not touched, and a frame whose four mask words are zero is skipped.
template <typename WordT, bool kLabels, bool kRaw, bool kRows = false, bool kVis = false>
__global__ __launch_bounds__(kBlock) void project_views_kernel(
    const double *__restrict__ xyz, int64_t n_points, int64_t n_pad,
    const double *__restrict__ inv_pose, CameraK K, int n_frames, int frames_per_block,
    const void *__restrict__ depth, RawDepth raw, const int32_t *__restrict__ depth_index, int H, int W, double thresh,
    const WordT *__restrict__ maskbits, const uint8_t *__restrict__ labels, int64_t label_stride,
    const uint32_t *__restrict__ segmap, int64_t seg_words,
    const int32_t *__restrict__ frame_mask,
    const int32_t *__restrict__ frame_rowbase, const int32_t *__restrict__ frame_nmask,
    const int32_t *__restrict__ frame_flags,
    uint64_t *__restrict__ rows, int64_t nw, uint64_t *__restrict__ chunk_mask, int mw,
    int32_t *__restrict__ masked_count, int32_t *__restrict__ viewed_count,
    const double *__restrict__ tile_bounds, MaskRows mr, VisTable vt)
{
    static_assert(!kVis || (kRows && !kRaw && !kLabels), "the cached sweep is the look-up sweep without depth");
    // per wave: [bit][kPPT words] transposition buffer for the wave's sector of the frame's rows
    __shared__ uint64_t stage_all[kBlock / kWave][sizeof(WordT) * 8][kPPT];
    extern __shared__ uint32_t s_taps[];                   // kRaw: the resize's tap table (RawDepth::taps)
    if (kRaw) fill_lds_taps(s_taps, raw);
    const uint4 *s_mtab = nullptr;
    if constexpr (kRows) {
        // mask tables of the block's frames: entry m of frame slot k at [k * kRowsMaskSlots + m], m <= the frame's masks
        uint4 *dst = reinterpret_cast<uint4 *>(s_taps + (kRaw ? (3 * raw.n_taps + 3) / 4 * 4 : 0));
        for (int i = (int)threadIdx.x; i < kRowsFrames * kRowsMaskSlots; i += kBlock) {
            const int fk = i / kRowsMaskSlots, m = i - fk * kRowsMaskSlots;
            const int f = (int)blockIdx.y * frames_per_block + fk;
            if (fk < frames_per_block && f < n_frames) {
                const int mi = frame_mask[f];
                if (mi >= 0 && m <= frame_nmask[f]) dst[i] = mr.tab[mr.view_mask_offs[mi] + m];
            }
        }
        s_mtab = dst;
        __syncthreads();
    }

    // kVis: the wave index as a scalar, so that the table's words come in by scalar loads
    const int tid = threadIdx.x, lane = tid & 63, wave = kVis ? __builtin_amdgcn_readfirstlane(tid >> 6) : tid >> 6;
    // Block -> XCD mapping is the plain round-robin of the dispatch order.  Both XCD-aware mappings were measured on
    // config 2 and lost: an eighth of the (spatially sorted) cloud per XCD makes the work per XCD uneven -- frustum
    // culling empties whole regions of a frame and dispatch is in order -- (0.34 -> 0.8 ms); one frame tile per XCD, so
    // that a depth / mask line is fetched by one L2 only, ran 0.338 -> 0.345 ms alone and 0.44 -> 0.55 ms beside the other
    // scenes' kernels: the lines re-fetched by other XCDs come out of the Infinity Cache, not HBM.
    const int64_t bx = blockIdx.x;
    const int f0 = blockIdx.y * frames_per_block;
    const int64_t word0 = bx * kWordsPerBlock + (int64_t)wave * kPPT;   // the wave's first word
    const int64_t hw = (int64_t)H * W;
    uint64_t (*stage)[kPPT] = stage_all[wave];

    double px[kPPT], py[kPPT], pz[kPPT];
    bool valid[kPPT];
    int mcount[kPPT], vcount[kPPT];
#pragma unroll
    for (int j = 0; j < kPPT; ++j) {
        const int64_t n = (word0 + j) * kWave + lane;
        valid[j] = n < n_points;
        const int64_t m = valid[j] ? n : 0;
        if constexpr (!kVis) {
            px[j] = xyz[m];
            py[j] = xyz[n_pad + m];
            pz[j] = xyz[2 * n_pad + m];
        }
        mcount[j] = 0;
        vcount[j] = 0;
    }
    constexpr int kGeo = kVis ? 0 : kPPT;                   // points whose geometry and depth a frame evaluates (kVis: none)

    const int f1 = min(n_frames, f0 + frames_per_block);
    const double dW = (double)W, dH = (double)H;
    // frustum culling of the wave's 256 points against the <= 8 frames of the tile (geom.h: exact)
    uint64_t culled = 0;                                   // bit 8 k set: frame f0 + k cannot see this wave's points
    if (!kVis && tile_bounds && __ballot(valid[0]))        // the table has one box per tile that holds points (a wave's
                                                           // first point is lane 0's; asking valid[] costs no register)
        culled = cull_frames(tile_bounds + 6 * (word0 / kPPT), inv_pose, K, f0, f1, lane, dW, dH);
    for (int f = f0; f < f1; ++f) {
        if ((culled >> (8 * (f - f0))) & 1) continue;      // wave-uniform
        const double *P = inv_pose + 16 * (int64_t)f;
        const float *dimg = kRaw ? nullptr : reinterpret_cast<const float *>(depth) + (int64_t)depth_index[f] * hw;
        const char *rimg = kRaw ? raw_frame(depth, depth_index[f], raw) : nullptr;
        const int mi = (kRows || maskbits) ? frame_mask[f] : -1;
        const bool has_masks = mi >= 0;
        const WordT *mimg = (!kRows && has_masks) ? maskbits + (int64_t)mi * hw : nullptr;
        const uint8_t *limg = (kLabels && has_masks) ? labels + (int64_t)mi * label_stride : nullptr;   // wave-uniform
        const uint32_t *smap = (segmap && has_masks) ? segmap + (int64_t)mi * seg_words * (kLabels ? 2 : 1) : nullptr;
        const int nm = has_masks ? frame_nmask[f] : 0;
        const bool count_viewed = (frame_flags[f] & 1) != 0;
        // Three phases per frame so that a thread's gathers are all in flight together (the sweep is bound by
        // memory latency x concurrency, not by issue): (1) geometry of the 4 points, (2) depth + segment-bitmap
        // gathers of every in-bounds point, (3) mask-word gathers of every visible point in a masked segment.
        int pix[kPPT];
        int pu[kPPT];                                       // kRaw: the pixel's column (its row is (pix - pu) / W)
        double cz[kPPT];
        bool tvis[kPPT] = {};                               // kVis: the table's answer
        if constexpr (kVis) {
            const int64_t e0 = (int64_t)depth_index[f] * vt.stride + word0;     // wave-uniform
            // the four mask words and their offsets in one round trip, then the visible lanes' pixels in a second one
            uint64_t m[kPPT], any = 0;
            uint32_t at[kPPT];
#pragma unroll
            for (int j = 0; j < kPPT; ++j) {
                m[j] = vt.mask[e0 + j];
                at[j] = vt.off[e0 + j];
                any |= m[j];
            }
            if (!any) continue;                             // nothing of this wave is visible in the frame
#pragma unroll
            for (int j = 0; j < kPPT; ++j) {
                tvis[j] = (m[j] >> lane) & 1;
                at[j] += __builtin_amdgcn_mbcnt_hi((uint32_t)(m[j] >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m[j], 0u));
                pu[j] = 0;
            }
#pragma unroll
            for (int j = 0; j < kPPT; ++j)
                if (tvis[j]) pu[j] = (int)vt.pix[at[j]];
#pragma unroll
            for (int j = 0; j < kPPT; ++j)
                pix[j] = tvis[j] ? (pu[j] >> 16) * W + (pu[j] & 0xffff) : -1;
        }
#pragma unroll
        for (int j = 0; j < kGeo; ++j) {
            double u, v;                                    // bit-identical to the reference's dgemm (header contract)
            camera_pixel(P, K, px[j], py[j], pz[j], cz[j], u, v);
            const bool inb = valid[j] && pixel_in_bounds(u, v, dW, dH);
            pix[j] = inb ? (int)v * W + (int)u : -1;       // H*W < 2^31 (checked by the entry point)
            pu[j] = inb ? (int)u | ((int)v << 16) : 0;     // kRaw: H, W < 2^15 (checked by the entry point)
        }
        float dval[kPPT];
        PixelTexels tex[kPPT];
        uint32_t sbits[kPPT], fbits[kPPT];                 // fbits (kLabels): segments in word form
#pragma unroll
        for (int j = 0; j < kGeo; ++j) {
            dval[j] = 0.0f;
            sbits[j] = 0xffffffffu;
            fbits[j] = 0xffffffffu;
            if (kRaw) tex[j] = PixelTexels{};
            if (pix[j] >= 0) {
                if (kRaw) tex[j] = fetch_texels(s_taps, W, pu[j] & 0xffff, pu[j] >> 16, rimg, raw);   // all in flight together
                else dval[j] = dimg[pix[j]];
                // segments without any mask pixel were never written by the decoder: consult its bitmap
                if (kLabels) {
                    if (smap) {
                        const uint2 sf = reinterpret_cast<const uint2 *>(smap)[pix[j] >> 12];
                        sbits[j] = sf.x;
                        fbits[j] = sf.y;
                    }
                } else if (smap) {
                    sbits[j] = smap[pix[j] >> 12];
                }
            }
        }
        if (kRaw) {
#pragma unroll
            for (int j = 0; j < kPPT; ++j)
                if (pix[j] >= 0) dval[j] = bilinear_depth(tex[j]);
        }
        bool vis[kPPT];
        WordT wv[kPPT];
        if (kLabels) {
            // segment by segment the decoder wrote either a palette block (4-bit index per pixel + the segment's distinct
            // words, one 128-byte line) or the mask words (rle_to_maskbits_kernel<.., true>).  A point gathers its index
            // byte or its word -- both kinds in flight together --, then the palette entry out of the line the index
            // came from.
            // The palette entry's address depends on the index byte: a second, dependent round trip.  The first 16 bytes of
            // the palette (entries 0-3 of 32 bits, 0-1 of 64) are therefore fetched WITH the index byte -- same 128-byte
            // line, no extra line -- and only a pixel of a later piece pays the dependent load.
            // (32-bit words only: with 64-bit words two entries cover too few pixels -- config 4 ran 1.55 -> 1.69 ms with them)
            constexpr int kSpec = sizeof(WordT) == 4 ? 4 : 0;
            uint32_t lb[kPPT];
            uint4 first4[kPPT];
            bool pal_go[kPPT];
#pragma unroll
            for (int j = 0; j < kPPT; ++j) {
                vis[j] = (pix[j] >= 0) && depth_visible(cz[j], dval[j], thresh);
                const int sb = (pix[j] >> 7) & 31;
                const bool go = vis[j] && limg && ((sbits[j] >> sb) & 1);
                const bool words = (fbits[j] >> sb) & 1;
                lb[j] = 0;
                wv[j] = 0;
                first4[j] = make_uint4(0, 0, 0, 0);
                pal_go[j] = go && !words;
                if (go && !words) {
                    lb[j] = limg[(pix[j] & ~127) + ((pix[j] & 127) >> 1)];
                    if (kSpec) first4[j] = *reinterpret_cast<const uint4 *>(limg + (pix[j] & ~127) + 64);
                }
                if (go && words) wv[j] = mimg[pix[j]];
            }
#pragma unroll
            for (int j = 0; j < kPPT; ++j) {
                const uint32_t idx = (lb[j] >> (4 * (pix[j] & 1))) & 15u;
                if (pal_go[j]) {
                    if (idx < (uint32_t)kSpec) {
                        wv[j] = (WordT)(idx == 0 ? first4[j].x : idx == 1 ? first4[j].y : idx == 2 ? first4[j].z : first4[j].w);
                    } else {
                        wv[j] = *reinterpret_cast<const WordT *>(limg + (pix[j] & ~127) + 64 + sizeof(WordT) * idx);
                    }
                }
            }
        } else if constexpr (kRows) {
            uint32_t bmin = 0xffffffffu, bmax = 0;         // bounding box of the wave's visible pixels
#pragma unroll
            for (int j = 0; j < kPPT; ++j) {
                vis[j] = kVis ? tvis[j] : (pix[j] >= 0) && depth_visible(cz[j], dval[j], thresh);
                wv[j] = 0;
                if (vis[j]) {
                    bmin = pk_min_u16(bmin, (uint32_t)pu[j]);
                    bmax = pk_max_u16(bmax, (uint32_t)pu[j]);
                }
            }
            if (has_masks && __ballot(bmax >= bmin)) {     // wave-uniform; some lane has a visible point
                const uint4 *ft = s_mtab + (f - f0) * kRowsMaskSlots;
                bmin = wave_reduce_pk_u16<true>(bmin);
                bmax = wave_reduce_pk_u16<false>(bmax);
                // lane m: can mask m's box hold one of the wave's visible pixels at all?
                bool may = false;
                if (lane < nm) {
                    const uint2 box = *reinterpret_cast<const uint2 *>(ft + lane);
                    may = pk_min_u16(box.x, bmax) == box.x && pk_max_u16(box.y, bmin) == box.y;
                }
                uint64_t cand = __ballot(may);
                // The candidates three at a time: a lane's directory entries of a round (<= 3 masks x 4 points) are all in
                // flight before the first is looked at.  Masks and tables are wave-uniform: LDS broadcast reads.
                constexpr int kRound = 3;                   // 128 VGPRs: four waves per SIMD, as the dense sweep (4: 132, three waves)
                while (cand) {
                    int mk[kRound];
                    uint32_t ent[kRound][kPPT];
#pragma unroll
                    for (int k = 0; k < kRound; ++k) {
                        mk[k] = cand ? __ffsll((unsigned long long)cand) - 1 : -1;
                        cand &= cand - 1;                  // 0 stays 0
                        if (mk[k] < 0) continue;
                        const uint4 t = ft[mk[k]];
#pragma unroll
                        for (int j = 0; j < kPPT; ++j) {
                            ent[k][j] = 0;
                            const uint32_t p = (uint32_t)pu[j];
                            if (vis[j] && pk_min_u16(pk_max_u16(p, t.x), t.y) == p)
                                ent[k][j] = mr.dir[t.z + ((p >> 16) - (t.x >> 16))];
                        }
                    }
#pragma unroll
                    for (int k = 0; k < kRound; ++k) {
                        if (mk[k] < 0) continue;
#pragma unroll
                        for (int j = 0; j < kPPT; ++j) {
                            const uint32_t e = ent[k][j], u = (uint32_t)pu[j] & 0xffffu;
                            bool in = (e & 0x7fffu) <= u && u < ((e >> 15) & 0x7fffu);
                            if (e & kRowFlag)              // several runs on the row: the run table decides
                                in = runs_cover(mr.run_start, mr.run_end, e, ft[mk[k]].w, ft[mk[k] + 1].w, pix[j]);
                            if (in) wv[j] |= (WordT)1 << mk[k];
                        }
                    }
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < kPPT; ++j) {
                vis[j] = (pix[j] >= 0) && depth_visible(cz[j], dval[j], thresh);
                wv[j] = 0;
                if (vis[j] && mimg && ((sbits[j] >> ((pix[j] >> 7) & 31)) & 1)) wv[j] = mimg[pix[j]];
            }
        }
        WordT present = 0;
#pragma unroll
        for (int j = 0; j < kPPT; ++j) {
            if (count_viewed) vcount[j] += vis[j] ? 1 : 0;
            mcount[j] += (sizeof(WordT) == 8) ? __popcll((uint64_t)wv[j]) : __popc((uint32_t)wv[j]);
            present |= wv[j];
        }
#ifdef BFF_DIAG_NO_ROW_STORES
        if (false) {
#else
        if (has_masks) {                                   // wave-uniform
#endif
            // the wave's 32-B sector (kPPT words) of each of the frame's nm rows: lane -> (row lane/4 + 16 i,
            // word lane%4).  Most waves see no mask at all in a given frame: the caller zeroed the rows.
            const int64_t rb = frame_rowbase[f];
            const int wd = lane & (kPPT - 1);
            if (__ballot(present != 0)) {
                // lane b collects the ballots of bit b: OR the words across the wave, visit the set bits only
#pragma unroll
                for (int d = 32; d > 0; d >>= 1) present |= __shfl_xor(present, d);
                uint64_t mine[kPPT] = {};
                while (present) {
                    const int b = (sizeof(WordT) == 8) ? __ffsll((unsigned long long)present) - 1
                                                       : __ffs((unsigned)present) - 1;
                    present &= present - 1;
#pragma unroll
                    for (int j = 0; j < kPPT; ++j) {
                        const uint64_t bal = __ballot((wv[j] >> b) & 1);
                        if (lane == b) mine[j] = bal;
                    }
                }
                if (lane < (int)(sizeof(WordT) * 8)) {
#pragma unroll
                    for (int j = 0; j < kPPT; ++j) stage[lane][j] = mine[j];
                }
                lds_phase_fence();                         // wave-private slice: LDS ops complete in issue order
                // only the rows that received a bit are stored (their 32-B sector), and flagged in the rows'
                // chunk occupancy masks so that later passes visit nothing else
                const int chunk = (int)(word0 / kCW);
                for (int b0 = 0; b0 < nm; b0 += kWave / kPPT) {        // wave-uniform trip count
                    const int b = b0 + lane / kPPT;
                    const uint64_t v = b < nm ? stage[b][wd] : 0;
                    const uint64_t nz = __ballot(v != 0);
                    if ((nz >> (lane & ~(kPPT - 1))) & ((1u << kPPT) - 1)) {
                        if (word0 + wd < nw) rows[(rb + b) * nw + word0 + wd] = v;     // nw need not be a multiple of 4
                        if (chunk_mask && wd == 0)
                            atomicOr((unsigned long long *)(chunk_mask + (rb + b) * mw + (chunk >> 6)), 1ull << (chunk & 63));
                    }
                }
                lds_phase_fence();                         // reads done before the next frame's writes
            }
        }
    }
#pragma unroll
    for (int j = 0; j < kPPT; ++j) {
        const int64_t n = (word0 + j) * kWave + lane;
        if (valid[j]) {
            if (masked_count && mcount[j]) atomicAdd(masked_count + n, mcount[j]);
            if (viewed_count && vcount[j]) atomicAdd(viewed_count + n, vcount[j]);
        }
    }
}

// Bounding boxes of the sweep's point tiles (one wave of project_views_kernel = kPPT words = 256 consecutive points
// of the spatially sorted cloud): bounds[t] = (xmin, ymin, zmin, xmax, ymax, zmax).  NaN coordinates are ignored
// (such a point is never in bounds), an empty tile gives (+inf, -inf) and is never culled.
__global__ __launch_bounds__(kBlock) void point_tile_bounds_kernel(const double *__restrict__ xyz, int64_t n_points,
                                                                    int64_t n_pad, int64_t n_tiles,
                                                                    double *__restrict__ bounds)
{
    const int lane = threadIdx.x & 63;
    const int64_t t = (int64_t)blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6);
    if (t >= n_tiles) return;
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
#pragma unroll
    for (int j = 0; j < kPPT; ++j) {
        const int64_t n = (t * kPPT + j) * kWave + lane;
        if (n < n_points)
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const double v = xyz[a * n_pad + n];
                lo[a] = fmin(lo[a], v);
                hi[a] = fmax(hi[a], v);
            }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            lo[a] = fmin(lo[a], __shfl_xor(lo[a], d));
            hi[a] = fmax(hi[a], __shfl_xor(hi[a], d));
        }
    if (lane < 3) bounds[6 * t + lane] = lane == 0 ? lo[0] : lane == 1 ? lo[1] : lo[2];
    else if (lane < 6) bounds[6 * t + lane] = lane == 3 ? hi[0] : lane == 4 ? hi[1] : hi[2];
}

}  // namespace bff

using namespace bff;

// Profiling aid (bench.py): events attached to the next sweep dispatch of this host thread.
static thread_local hipEvent_t g_sweep_start = nullptr, g_sweep_stop = nullptr;

void bff::take_sweep_events(hipEvent_t *start, hipEvent_t *stop)
{
    *start = g_sweep_start;
    *stop = g_sweep_stop;
    g_sweep_start = g_sweep_stop = nullptr;
}

extern "C" int bff_profile_next_sweep(void *start_event, void *stop_event)
{
    g_sweep_start = reinterpret_cast<hipEvent_t>(start_event);
    g_sweep_stop = reinterpret_cast<hipEvent_t>(stop_event);
    return BFF_OK;
}

extern "C" void *bff_event_create(void)
{
    hipEvent_t e = nullptr;
    return hipEventCreate(&e) == hipSuccess ? e : nullptr;
}

extern "C" int bff_event_destroy(void *event)
{
    hipError_t e = hipEventDestroy(reinterpret_cast<hipEvent_t>(event));
    return e == hipSuccess ? BFF_OK : fail((int)e, "bff_event_destroy: %s", hipGetErrorString(e));
}

extern "C" int bff_event_record(void *event, void *stream)
{
    hipError_t e = hipEventRecord(reinterpret_cast<hipEvent_t>(event), as_stream(stream));
    return e == hipSuccess ? BFF_OK : fail((int)e, "bff_event_record: %s", hipGetErrorString(e));
}

extern "C" int bff_event_synchronize(void *event)
{
    hipError_t e = hipEventSynchronize(reinterpret_cast<hipEvent_t>(event));
    return e == hipSuccess ? BFF_OK : fail((int)e, "bff_event_synchronize: %s", hipGetErrorString(e));
}

extern "C" int bff_event_elapsed_ms(void *start_event, void *stop_event, float *ms)
{
    BFF_REQUIRE(start_event && stop_event && ms, "bff_event_elapsed_ms: null pointer");
    hipError_t e = hipEventSynchronize(reinterpret_cast<hipEvent_t>(stop_event));
    if (e == hipSuccess)
        e = hipEventElapsedTime(ms, reinterpret_cast<hipEvent_t>(start_event), reinterpret_cast<hipEvent_t>(stop_event));
    return e == hipSuccess ? BFF_OK : fail((int)e, "bff_event_elapsed_ms: %s", hipGetErrorString(e));
}

// The frame tile of a block: >= ~4096 blocks in flight, tiles of up to 8 frames (the culling ballot and the LDS mask
// tables hold 8).  The one statement of the choice: the sweep and bff_count_viewed (frames_per_block == 0) ask here.
extern "C" int32_t bff_sweep_frames_per_block(int64_t n_points, int32_t n_frames)
{
    if (n_points <= 0 || n_frames <= 0) return 1;
    const int64_t fpb = (int64_t)n_frames * ceil_div(n_points, (int64_t)kPtsPerBlock) / 4096;
    return fpb < 1 ? 1 : (fpb > 8 ? 8 : (int32_t)fpb);
}

// a raw-depth sweep's RawDepth and the LDS bytes of its tap table
static int sweep_raw_depth(int32_t depth_h, int32_t depth_w, int32_t height, int32_t width, int32_t layout, void *stream,
                           RawDepth *raw, size_t *taps_bytes)
{
    BFF_LIMIT(height < (1 << 15) && width < (1 << 16), "bff_project_views_u16: image too large");
    return raw_depth_launch(depth_h, depth_w, height, width, layout, as_stream(stream), raw, taps_bytes,
                            "bff_project_views_u16: the resize's tap table (12 B per image row and column) exceeds 48 KB of LDS: "
                            "resize in a separate pass (bff_depth_from_u16)");
}

static int project_views_launch(const double *xyz, int64_t n_points, int64_t n_pad,
                                const double *inv_pose, const double *cam_intr_host, int32_t n_frames,
                                const void *depth, const RawDepth *raw, size_t taps_bytes, const int32_t *depth_index,
                                int32_t height, int32_t width, double depth_thresh,
                                const void *maskbits, const uint8_t *labels, const uint32_t *segmap, int32_t word_bits,
                                const int32_t *frame_mask, const int32_t *frame_rowbase, const int32_t *frame_nmask,
                                const int32_t *frame_flags,
                                uint64_t *rows, int64_t n_rows, int64_t nw, uint64_t *chunk_mask,
                                int32_t *masked_count, int32_t *viewed_count, const double *tile_bounds,
                                void *stream, const MaskRows *mask_rows = nullptr, const VisTable *vis = nullptr)
{
    BFF_REQUIRE(n_points >= 0 && n_pad >= n_points && n_frames >= 0, "bff_project_views: bad sizes");
    BFF_REQUIRE(height > 0 && width > 0, "bff_project_views: bad image size");
    BFF_LIMIT((int64_t)height * width < (1ll << 31), "bff_project_views: image larger than 2^31 pixels");
    if (n_points == 0 || n_frames == 0) return BFF_OK;
    BFF_REQUIRE((vis || (xyz && inv_pose && cam_intr_host && depth)) && depth_index && frame_flags, "bff_project_views: null pointer");
    BFF_REQUIRE(!vis || (mask_rows && !raw), "bff_project_views_cached: the cached sweep is a look-up sweep without depth");
    BFF_REQUIRE(nw == ceil_div(n_points, 64), "bff_project_views: nw must be ceil(n_points/64)");
    if (maskbits || mask_rows) {
        BFF_REQUIRE(word_bits == 32 || word_bits == 64, "bff_project_views: word_bits must be 32 or 64");
        BFF_REQUIRE(frame_mask && frame_rowbase && frame_nmask && rows && n_rows >= 0, "bff_project_views: mask frames need row outputs");
    }
    size_t rows_bytes = 0;
    if (mask_rows) {
        BFF_REQUIRE(!maskbits && !labels && !segmap, "bff_project_views_lookup: the row directory replaces the decoded planes");
        BFF_REQUIRE(mask_rows->tab && mask_rows->dir && mask_rows->view_mask_offs, "bff_project_views_lookup: null pointer");
        BFF_LIMIT(height < (1 << 15) && width < (1 << 15), "bff_project_views_lookup: image too large for packed entries");
        rows_bytes = sizeof(uint4) * kRowsFrames * kRowsMaskSlots;
        BFF_LIMIT(taps_bytes + rows_bytes + sizeof(uint64_t) * kBlock * kPPT <= 64 * 1024,
                  "bff_project_views_lookup: tap table and mask tables exceed 64 KB of LDS");
    }
    const int mw = (int)ceil_div(ceil_div(nw, kCW), 64);
    const CameraK K = camera_k(cam_intr_host);
    const int64_t gx = ceil_div(n_points, kPtsPerBlock);
    const int fpb = bff_sweep_frames_per_block(n_points, n_frames);
    dim3 grid((unsigned)gx, (unsigned)ceil_div(n_frames, fpb));
    const int64_t seg_words = ceil_div(ceil_div((int64_t)height * width, 128), 32);
    const int64_t label_stride = bff_label_plane_stride((int64_t)height * width);
    BFF_REQUIRE(!labels || (maskbits && segmap), "bff_project_views: a label plane comes with its word plane and segment bitmap");
    hipEvent_t ev0, ev1;                                        // attached to the dispatch itself when set
    take_sweep_events(&ev0, &ev1);
    const RawDepth rd = raw ? *raw : RawDepth{};
    const MaskRows mr = mask_rows ? *mask_rows : MaskRows{};
    const VisTable vt = vis ? *vis : VisTable{};
    static_assert(kRowsFrames >= 8, "a block's frame tile must fit the LDS mask tables");
#define BFF_SWEEP(WORD, ...)                                                                                             \
    hipExtLaunchKernelGGL((project_views_kernel<WORD, __VA_ARGS__>), grid, dim3(kBlock), (unsigned)(taps_bytes + rows_bytes), \
        as_stream(stream), ev0, ev1, 0,                                                                                  \
        xyz, n_points, n_pad, inv_pose, K, n_frames, fpb, depth, rd, depth_index, height, width, depth_thresh,           \
        (const WORD *)maskbits, labels, label_stride, segmap, seg_words, frame_mask, frame_rowbase, frame_nmask,        \
        frame_flags, rows, nw, chunk_mask, mw, masked_count, viewed_count, tile_bounds, mr, vt)
    // template arguments: labels, raw depth, look-up, cached (the look-up and cached forms come without planes: checked above)
#define BFF_SWEEP_FORM(WORD)                                                                                             \
    do { if (vis) BFF_SWEEP(WORD, false, false, true, true);                                                             \
         else if (mask_rows) { if (raw) BFF_SWEEP(WORD, false, true, true); else BFF_SWEEP(WORD, false, false, true); }  \
         else if (labels) { if (raw) BFF_SWEEP(WORD, true, true); else BFF_SWEEP(WORD, true, false); }                   \
         else { if (raw) BFF_SWEEP(WORD, false, true); else BFF_SWEEP(WORD, false, false); } } while (0)
    if (word_bits == 32 || !(maskbits || mask_rows)) BFF_SWEEP_FORM(uint32_t); else BFF_SWEEP_FORM(uint64_t);
#undef BFF_SWEEP_FORM
#undef BFF_SWEEP
    return launched("bff_project_views");
}

extern "C" int bff_project_views(const double *xyz, int64_t n_points, int64_t n_pad,
                                 const double *inv_pose, const double *cam_intr_host, int32_t n_frames,
                                 const float *depth, const int32_t *depth_index, int32_t height, int32_t width,
                                 double depth_thresh,
                                 const void *maskbits, const uint8_t *labels, const uint32_t *segmap, int32_t word_bits,
                                 const int32_t *frame_mask, const int32_t *frame_rowbase, const int32_t *frame_nmask,
                                 const int32_t *frame_flags,
                                 uint64_t *rows, int64_t n_rows, int64_t nw, uint64_t *chunk_mask,
                                 int32_t *masked_count, int32_t *viewed_count, const double *tile_bounds,
                                 void *stream)
{
    return project_views_launch(xyz, n_points, n_pad, inv_pose, cam_intr_host, n_frames, depth, nullptr, 0, depth_index, height,
                                width, depth_thresh, maskbits, labels, segmap, word_bits, frame_mask, frame_rowbase,
                                frame_nmask, frame_flags, rows, n_rows, nw, chunk_mask, masked_count, viewed_count,
                                tile_bounds, stream);
}

extern "C" int bff_project_views_u16(const double *xyz, int64_t n_points, int64_t n_pad,
                                     const double *inv_pose, const double *cam_intr_host, int32_t n_frames,
                                     const void *depth_raw, int32_t depth_h, int32_t depth_w, int32_t depth_layout,
                                     const int32_t *depth_index, int32_t height, int32_t width, double depth_thresh,
                                     const void *maskbits, const uint8_t *labels, const uint32_t *segmap, int32_t word_bits,
                                     const int32_t *frame_mask, const int32_t *frame_rowbase, const int32_t *frame_nmask,
                                     const int32_t *frame_flags,
                                     uint64_t *rows, int64_t n_rows, int64_t nw, uint64_t *chunk_mask,
                                     int32_t *masked_count, int32_t *viewed_count, const double *tile_bounds,
                                     void *stream)
{
    RawDepth raw;
    size_t taps_bytes = 0;
    if (n_points == 0 || n_frames == 0) return BFF_OK;
    BFF_REQUIRE(height > 0 && width > 0, "bff_project_views_u16: bad image size");
    const int rc = sweep_raw_depth(depth_h, depth_w, height, width, depth_layout, stream, &raw, &taps_bytes);
    if (rc != BFF_OK) return rc;
    return project_views_launch(xyz, n_points, n_pad, inv_pose, cam_intr_host, n_frames, depth_raw, &raw, taps_bytes, depth_index,
                                height, width, depth_thresh, maskbits, labels, segmap, word_bits, frame_mask, frame_rowbase,
                                frame_nmask, frame_flags, rows, n_rows, nw, chunk_mask, masked_count, viewed_count,
                                tile_bounds, stream);
}

extern "C" int bff_project_views_lookup(const double *xyz, int64_t n_points, int64_t n_pad,
                                        const double *inv_pose, const double *cam_intr_host, int32_t n_frames,
                                        const void *depth, int32_t depth_h, int32_t depth_w, int32_t depth_layout,
                                        const int32_t *depth_index, int32_t height, int32_t width, double depth_thresh,
                                        const uint32_t *mask_tab, const uint32_t *mask_dir, const int32_t *run_start,
                                        const int32_t *run_end, const int32_t *view_mask_offs, int32_t word_bits,
                                        const int32_t *frame_mask, const int32_t *frame_rowbase, const int32_t *frame_nmask,
                                        const int32_t *frame_flags,
                                        uint64_t *rows, int64_t n_rows, int64_t nw, uint64_t *chunk_mask,
                                        int32_t *masked_count, int32_t *viewed_count, const double *tile_bounds,
                                        void *stream)
{
    BFF_REQUIRE(depth_layout >= -1 && depth_layout <= 2, "bff_project_views_lookup: depth_layout must be -1, 0, 1 or 2");
    if (n_points == 0 || n_frames == 0) return BFF_OK;
    BFF_REQUIRE(height > 0 && width > 0, "bff_project_views_lookup: bad image size");
    const MaskRows mr{reinterpret_cast<const uint4 *>(mask_tab), mask_dir, run_start, run_end, view_mask_offs};
    RawDepth raw;
    size_t taps_bytes = 0;
    if (depth_layout >= 0) {
        const int rc = sweep_raw_depth(depth_h, depth_w, height, width, depth_layout, stream, &raw, &taps_bytes);
        if (rc != BFF_OK) return rc;
    }
    return project_views_launch(xyz, n_points, n_pad, inv_pose, cam_intr_host, n_frames, depth, depth_layout >= 0 ? &raw : nullptr,
                                taps_bytes, depth_index, height, width, depth_thresh, nullptr, nullptr, nullptr, word_bits, frame_mask,
                                frame_rowbase, frame_nmask, frame_flags, rows, n_rows, nw, chunk_mask, masked_count,
                                viewed_count, tile_bounds, stream, &mr);
}

extern "C" int bff_project_views_cached(int64_t n_points, int32_t n_frames, const int32_t *depth_index, int32_t height,
                                        int32_t width, const uint64_t *vis_mask, const uint32_t *vis_off,
                                        const uint32_t *vis_pix, const uint32_t *mask_tab, const uint32_t *mask_dir,
                                        const int32_t *run_start, const int32_t *run_end, const int32_t *view_mask_offs,
                                        int32_t word_bits, const int32_t *frame_mask, const int32_t *frame_rowbase,
                                        const int32_t *frame_nmask, const int32_t *frame_flags, uint64_t *rows, int64_t n_rows,
                                        int64_t nw, uint64_t *chunk_mask, int32_t *masked_count, int32_t *viewed_count,
                                        void *stream)
{
    if (n_points <= 0 || n_frames <= 0) return BFF_OK;
    BFF_REQUIRE(height > 0 && width > 0, "bff_project_views_cached: bad image size");
    BFF_REQUIRE(vis_mask && vis_off && vis_pix, "bff_project_views_cached: null table");
    const MaskRows mr{reinterpret_cast<const uint4 *>(mask_tab), mask_dir, run_start, run_end, view_mask_offs};
    const VisTable vt{vis_mask, vis_off, vis_pix, bff_visibility_words(n_points)};
    return project_views_launch(nullptr, n_points, n_points, nullptr, nullptr, n_frames, nullptr, nullptr, 0, depth_index, height,
                                width, 0.0, nullptr, nullptr, nullptr, word_bits, frame_mask, frame_rowbase, frame_nmask,
                                frame_flags, rows, n_rows, nw, chunk_mask, masked_count, viewed_count, nullptr, stream, &mr, &vt);
}

extern "C" int bff_point_tile_bounds(const double *xyz, int64_t n_points, int64_t n_pad, double *bounds, void *stream)
{
    BFF_REQUIRE(n_points >= 0 && n_pad >= n_points, "bff_point_tile_bounds: bad sizes");
    if (n_points == 0) return BFF_OK;
    BFF_REQUIRE(xyz && bounds, "bff_point_tile_bounds: null pointer");
    const int64_t n_tiles = ceil_div(n_points, (int64_t)kPPT * kWave);
    point_tile_bounds_kernel<<<(unsigned)ceil_div(n_tiles, kBlock / kWave), kBlock, 0, as_stream(stream)>>>(
        xyz, n_points, n_pad, n_tiles, bounds);
    return launched("bff_point_tile_bounds");
}

extern "C" int bff_point_tile_size(void) { return kPPT * kWave; }
